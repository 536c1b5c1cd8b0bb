"""rainfall_test (src/testModels.jl:387-585) without a GPU: the name, the numpy restatement of the warm-rain thermodynamics
(oracle/oracle_np.py), the reference's zero sedimentation flux, Julia's whole-column min / max of condensation_adjustment, a twin
run that exercises every process, and the host descriptor."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import cases
from tests import rainfall as RF


def test_rainfall_test_has_an_id_and_bf02_test_still_does_not():
    import scythe_jl_amd as S
    lib = S.load()
    assert lib.sx_equation_set_id(b"rainfall_test") == 11
    assert lib.sx_equation_set_id(b"BF02_test") == -1


def test_buck_derivative_and_latent_heat():
    """sat_pressure_liquid_buck_dT is the T derivative of sat_pressure_liquid_buck (centred difference, 1e-7 relative) and
    L_v(T_0) is L_v0."""
    Tk = np.linspace(230.0, 310.0, 41)
    for p in (300.0, 700.0, 1013.0):
        h = 1e-3
        fd = (O.th_sat_pressure_liquid_buck(Tk + h, p) - O.th_sat_pressure_liquid_buck(Tk - h, p)) / (2.0 * h)
        an = O.th_sat_pressure_liquid_buck_dT(Tk, p)
        assert np.abs(fd / an - 1.0).max() < 1e-7
    assert O.th_L_v(O.TH["T_0"]) == O.TH["L_v0"]


def test_sedimentation_flux_is_exactly_zero():
    """Vt = -14.164 rho_r^0.1364 (rho_d0 / rho_d)^0.5 f_ice(Tk) is clamped at 0 from below (src/microphysics.jl:252-261), so the
    flux divergence of src/testModels.jl:524-528 vanishes for every state - the library drops the term on that account.  If the
    reference ever fixes the sign, this is the test that fails."""
    g = cases.oracle_grid(RF.rz_rain(num_cells=4, zDim=12))
    rng = np.random.default_rng(7)
    for scale in (0.0, 1e-9, 1e-5, 1e-3, 2e-2):
        n = 4 * 12 * 6
        q_r = scale * rng.random(n)
        rho_d = rng.uniform(0.3, 1.3, n)
        Tk = rng.uniform(200.0, 310.0, n)
        assert np.all(O.th_sedimentation(q_r, rho_d, Tk) == 0.0)
        assert np.all(O.sedimentation_flux(g, q_r, rho_d, Tk) == 0.0)


def test_column_min_max_are_lexicographic():
    """Without signed zeros or NaN, Julia's isless on vectors orders like Python's list comparison: column_min / column_max equal
    min / max of the rows as lists - one whole row each, decided at the first differing level."""
    rng = np.random.default_rng(11)
    for _ in range(200):
        nz = int(rng.integers(1, 9))
        x = rng.integers(-2, 3, size=(6, nz)).astype(float) * 0.5 + 1.0   # many ties, no zeros
        y = rng.integers(-2, 3, size=(6, nz)).astype(float) * 0.5 + 1.0
        mn, mx = O.column_min(x, y), O.column_max(x, y)
        for r in range(6):
            assert list(mn[r]) == min(list(x[r]), list(y[r]))
            assert list(mx[r]) == max(list(x[r]), list(y[r]))


def test_column_min_max_use_julias_isequal_and_isless():
    """Where Python and Julia differ: -0.0 == 0.0 for Python, but isequal(-0.0, 0.0) is false and isless(-0.0, 0.0) true; NaN
    is isequal to NaN and above every number."""
    x = np.array([[-0.0, 5.0, 1.0]])
    y = np.array([[0.0, 1.0, 1.0]])
    assert min([-0.0, 5.0, 1.0], [0.0, 1.0, 1.0]) == [0.0, 1.0, 1.0]          # Python: ties at level 0, decides at level 1
    assert np.array_equal(O.column_min(x, y), x) and np.signbit(O.column_min(x, y)[0, 0])
    assert np.array_equal(O.column_max(x, y), y) and not np.signbit(O.column_max(x, y)[0, 0])
    a = np.array([[np.nan, 1.0]])
    b = np.array([[np.nan, 2.0]])
    assert np.array_equal(O.column_min(a, b), a, equal_nan=True)             # NaN level is equal: level 1 decides
    c = np.array([[1e300, 0.0]])
    assert np.array_equal(O.column_max(a, c), a, equal_nan=True)             # NaN above every number
    assert np.array_equal(O.column_min(a, c), c)
    same = np.array([[1.0, 2.0]])
    assert not O.column_isless(same, same.copy())[0]                        # equal columns: the first argument stays
    # the scalar min / max of q_condensation stay elementwise, with -0.0 < 0.0 and NaN propagating
    assert np.signbit(O.jl_min(0.0, -0.0)) and not np.signbit(O.jl_max(-0.0, 0.0))
    assert np.isnan(O.jl_min(np.nan, 1.0)) and np.isnan(O.jl_max(1.0, np.nan))
    assert np.array_equal(O.jl_min([1.0, 3.0], [2.0, 2.0]), [1.0, 2.0])


@pytest.mark.parametrize("semi", [True, False])
def test_twin_run_exercises_every_process(monkeypatch, semi):
    """10 steps of the oracle twin stay finite and every microphysical rate of the tendency - condensation, its entropy
    source, rain evaporation, the qss source, autoconversion, collection - is non-zero somewhere, as is the adjustment's
    q_cond; mu + mubar stays positive (q_v = 0 gives NaN in the reference, and no guard is added)."""
    case = RF.rz_rain(semiimplicit=semi)
    m = cases.OracleModel(case, numpy_twin=True)
    seen = {}
    adj = []
    orig = O.condensation_adjustment

    def spy(np1, par, nz, elementwise=False):
        out = orig(np1, par, nz, elementwise)
        adj.append(np.abs(out[:, 5] - np1[:, 5]).max())
        return out
    monkeypatch.setattr("oracle.oracle_np.condensation_adjustment", spy)
    nz = case["grid"]["zDim"]
    for _ in range(10):
        ph = m.physical()
        for k, v in O.rain_rates(m.g, case["par"], ph).items():
            seen[k] = max(seen.get(k, 0.0), np.abs(v).max())
        mubar = case["par"]["ref_state"]["mubar"][np.arange(len(ph)) % nz, 0]
        assert (ph[:, 2, 0] + mubar).min() > 0.0
        m.step()
    assert np.isfinite(m.physical()).all()
    assert seen.pop("Vt_flux") == 0.0
    assert all(v > 0.0 for v in seen.values()), seen
    assert len(adj) == 10 and min(adj) > 0.0


def test_mixed_case_tells_the_column_rule_from_a_pointwise_one():
    """rz_rain_mixed: some columns keep the raw q_cond, some take -q_c, and the run after 3 steps differs by O(1) from one that
    clamps point by point."""
    case = RF.rz_rain_mixed()
    a = cases.OracleModel(case, numpy_twin=True)
    b = cases.OracleModel(case, numpy_twin=True)
    b.m.elementwise = True
    ph = a.physical()
    R = O.ref_levels(case["par"], len(ph), 12)
    T = O.thermo_state(*(ph[:, v, 0] for v in (0, 1, 2, 5, 6)), R["sbar"], R["xibar"], R["mubar"])
    q_cond = ((T["q_v"] - O.th_q_sat_liquid(T["Tk"], T["p"]) - ph[:, 7, 0]) /
              (1.0 + O.th_Q_s_factor(T["Tk"], T["p"], T["q_v"], T["q_l"]))).reshape(-1, 12)
    takes = O.column_isless(q_cond, (-T["q_c"]).reshape(-1, 12))
    assert 0 < takes.sum() < len(takes)
    for _ in range(3):
        a.step()
        b.step()
    assert cases.rel_err_per_var(b.physical(), a.physical()) > 1e-6


def test_model_desc_packs_the_reference_state_and_checks_the_variables():
    import scythe_jl_amd as S
    case = RF.rz_rain(num_cells=4, zDim=12)
    gp, mp = cases.hip_params(case)
    m, keep = S.model.model_desc(mp, gp)
    assert m.equation_set == 11 and m.semiimplicit == 1 and m.w_index == 5 and m.xi_index == 2
    assert np.array_equal(keep["ref"], mp.ref_state.packed())
    assert bool(m.ref_state)
    assert keep["par"][S._lib.PARAM_ORDER.index("Pxi_bar")] == case["par"]["Pxi_bar"]
    bad = dict(RF.VARS)
    bad["mu_c"], bad["mu_r"] = 7, 6
    gp2 = S.GridParameters(**dict(case["grid"], vars=bad))
    mp.grid_params = gp2
    with pytest.raises(ValueError, match="rainfall_test needs grid_params.vars"):
        S.model.model_desc(mp, gp2)
