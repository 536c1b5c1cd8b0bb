"""-m gpu: rainfall_test (src/testModels.jl:387-585 + condensation_adjustment, src/microphysics.jl:139-195) on the HIP path -
against the numpy oracle twin (oracle/oracle_np.py) on one patch and on tiles, the whole-column clamp against a pointwise one, graph
replay, a sounding file, integrate_model and restart, fp32 derivative planes, the refusals of sx_create and a seeded sweep."""
import os

import numpy as np
import pytest

from tests import cases
from tests import rainfall as RF

pytestmark = pytest.mark.gpu
TOL = 1e-10     # fields within 1e-10 relative of the oracle twin (cases.rel_err_per_var: every variable, every slot)
F32_TOL_VAL = 1e-6      # values with fp32-stored derivative planes (the suite's bound, tests/test_gpu_parity.py)


def _advance(model, steps):
    for _ in range(steps):
        model.step()
    return model.physical()


def _twin(case, steps, elementwise=False):
    m = cases.OracleModel(case, numpy_twin=True)
    m.m.elementwise = elementwise
    return _advance(m, steps)


def _parity(case, steps, num_tiles=1, exchange="a2a", impl="torch", oracle=None):
    """rel_err_per_var of the HIP run against the one-patch oracle twin after `steps` steps, and that twin's result; also checks
    that the run changed every variable."""
    hip = cases.HipModel(case, num_tiles=num_tiles, exchange=exchange, impl=impl)
    p0 = hip.physical().copy()
    a = _advance(hip, steps)
    hip.run.close()
    if oracle is None:
        oracle = _twin(case, steps)
    assert np.isfinite(a).all()
    for v in range(a.shape[1]):
        assert np.abs(a[:, v, 0] - p0[:, v, 0]).max() > 1e-4 * np.abs(p0[:, v, 0]).max(), v
    return cases.rel_err_per_var(a, oracle), oracle


@pytest.mark.parametrize("semi,zDim", [(True, 12), (False, 12), (True, 14), (False, 16)])
def test_rainfall_matches_the_oracle_twin(semi, zDim):
    """12 steps (Euler, AB2, then AB3) with and without the semi-implicit adjustment, at 12, 14 and 16 levels (two groups of
    columns per workgroup of k_condensation that are not a power of two)."""
    err, _ = _parity(RF.rz_rain(semiimplicit=semi, zDim=zDim), 12)
    print("\nrainfall_test semi=%s zDim=%d: %.2e" % (semi, zDim, err))
    assert err < TOL


_ORACLE = {}


@pytest.mark.parametrize("num_cells,ntiles", [(20, 2), (30, 3)])
@pytest.mark.parametrize("exchange", ["a2a", "iface", "gather"])
@pytest.mark.parametrize("impl", ["lib", "torch"])
def test_rainfall_on_tiles_matches_the_one_patch_oracle_twin(num_cells, ntiles, exchange, impl):
    """2 and 3 tiles, every exchange protocol through the library's own buffers and through the Python-side stand-in, 12 steps
    against the one-patch twin (computed once per patch)."""
    case = RF.rz_rain(num_cells=num_cells)
    err, _ORACLE[num_cells] = _parity(case, 12, num_tiles=ntiles, exchange=exchange, impl=impl,
                                      oracle=_ORACLE.get(num_cells))
    print("\n%d cells, %d tiles, %s / %s: %.2e" % (num_cells, ntiles, exchange, impl, err))
    assert err < TOL


@pytest.mark.parametrize("semi", [True, False])
def test_condensation_adjustment_clamps_whole_columns(semi):
    """rz_rain_mixed, 3 steps: the twin's whole-column clamp and a pointwise one differ by more than 1e-6, and the GPU follows the
    whole-column one to 1e-10."""
    case = RF.rz_rain_mixed(semiimplicit=semi)
    col, pw = _twin(case, 3), _twin(case, 3, elementwise=True)
    apart = cases.rel_err_per_var(pw, col)
    hip = cases.HipModel(case)
    a = _advance(hip, 3)
    hip.run.close()
    err = cases.rel_err_per_var(a, col)
    print("\nmixed semi=%s: column vs pointwise %.2e, GPU vs column %.2e" % (semi, apart, err))
    assert apart > 1e-6
    assert np.isfinite(a).all() and err < TOL


def test_step_replayed_from_a_hip_graph_is_bit_identical(monkeypatch):
    """sx_step with SX_GRAPH=1: the captured step holds k_phys_rain, the semi-implicit kernel and k_condensation; 14 steps and 4
    more are bit-identical to plain launches."""
    case = RF.rz_rain(num_cells=9, zDim=16)
    plain = cases.HipModel(case)
    monkeypatch.setenv("SX_GRAPH", "1")
    graph = cases.HipModel(case)
    for _ in range(14):
        plain.step()
        graph.step()
    fa, fb = plain.run.tiles[0].var_np1, graph.run.tiles[0].var_np1
    assert np.isfinite(fa).all()
    assert np.array_equal(fa, fb)
    assert np.array_equal(plain.physical(), graph.physical())
    for _ in range(4):
        plain.step()
        graph.step()
    assert np.array_equal(plain.run.tiles[0].var_np1, graph.run.tiles[0].var_np1)
    plain.run.close()
    graph.run.close()


def test_rainfall_with_reference_state_built_from_a_sounding_file(tmp_path):
    """ModelParameters.ref_state_file -> interpolate_reference_file -> ReferenceState on the device (Pxi_bar from the reference
    state), then the same run in the twin fed with the same profiles."""
    import scythe_jl_amd as S
    case = RF.rz_rain(num_cells=6, zDim=16)
    f = tmp_path / "sounding.txt"
    f.write_text("1000.0 300.0 16.0\n" + "".join("%g %g %g\n" % (a, 300.0 + 4.0e-3 * a, 16.0 * np.exp(-a / 2.5e3))
                                                 for a in np.linspace(250.0, 10500.0, 42)))
    gp = S.GridParameters(**dict(case["grid"]))
    mp = S.ModelParameters(ts=case["ts"], equation_set="rainfall_test", grid_params=gp, physical_params={"K": 10.0},
                           options={"semiimplicit": True}, ref_state_file=str(f))
    run = S.ModelRun(mp)
    rs = mp.ref_state
    assert rs is not None and 300.0 ** 2 < rs.Pxi_bar < 360.0 ** 2
    pts = S.getGridpoints(run.tiles[0])
    run.set_initial_conditions([case["ic"](pts.reshape(len(pts), -1))])
    case["par"] = dict(K=10.0, Pxi_bar=rs.Pxi_bar, ref_state=dict(sbar=rs.sbar, xibar=rs.xibar, mubar=rs.mubar))
    ref = _twin(case, 4)
    a = _advance(run, 4)
    assert not run.tiles[0].check_nan()
    run.close()
    assert cases.rel_err_per_var(a, ref) < TOL


def test_integrate_model_output_and_restart(tmp_path):
    """integrate_model on rainfall_test (initial conditions from CSV, 12 steps, output every 6) writes all eight variables, and
    its last file equals a ModelRun's fields; a run saved after 5 steps and restarted in a fresh run continues bit-identically."""
    import scythe_jl_amd as S
    case = RF.rz_rain(num_cells=6)
    gp, mp0 = cases.hip_params(case)
    par = {k: v for k, v in case["par"].items() if k != "ref_state"}
    model = S.ModelParameters(ts=case["ts"], integration_time=12 * case["ts"], output_interval=6 * case["ts"],
                              equation_set="rainfall_test", initial_conditions=str(tmp_path / "ic.csv"),
                              output_dir=str(tmp_path / "out"), grid_params=gp, physical_params=par,
                              options={"semiimplicit": True}, ref_state=mp0.ref_state)
    grid = S.createGrid(gp)
    pts = S.getGridpoints(grid)
    grid.close()
    vals = case["ic"](pts)
    np.savetxt(model.initial_conditions, np.concatenate([pts, vals], axis=1), delimiter=",",
               header="r,z," + ",".join(RF.VARS), comments="", fmt="%.17g")
    assert S.integrate_model(model) is True
    files = sorted(f for f in os.listdir(model.output_dir) if f.startswith("physical_out_"))
    assert files == ["physical_out_0.0.csv", "physical_out_12.0.csv", "physical_out_6.0.csv"], files
    path = os.path.join(model.output_dir, "physical_out_12.0.csv")
    header = open(path).readline().strip().split(",")
    assert header[:10] == ["r", "z"] + list(RF.VARS) and "qss_zz" in header
    final = np.loadtxt(path, delimiter=",", skiprows=1)
    run = cases.HipModel(case)
    ph = _advance(run, 12)
    run.run.close()
    assert np.array_equal(final[:, 2:], np.concatenate([ph[:, :, d] for d in range(ph.shape[2])], axis=1))
    assert np.abs(ph[:, :, 0] - vals).max() > 1e-3

    a = cases.HipModel(case, num_tiles=2)
    whole = _advance(a, 10)
    a.run.close()
    b = cases.HipModel(case, num_tiles=2)
    _advance(b, 5)
    ck = str(tmp_path / "ck.npz")
    b.run.save_checkpoint(ck)
    b.run.close()
    c = cases.HipModel(case, num_tiles=2)
    c.run.load_checkpoint(ck)
    assert c.run.t == 5
    halves = _advance(c, 5)
    c.run.close()
    assert np.array_equal(whole, halves)


def test_fp32_derivative_planes_follow_the_twin():
    """storage="f32": k_phys_rain<float> reads fp32 derivative slots (values, state and arithmetic stay fp64); after 12 steps the
    values are within the suite's fp32 bound of the fp64 twin, and not bit-equal to it (the fp32 path ran)."""
    case = RF.rz_rain(num_cells=8, zDim=16)
    hip = cases.HipModel(case, storage="f32")
    a = _advance(hip, 12)
    hip.run.close()
    b = _twin(case, 12)
    err = cases.rel_err_per_var(a[:, :, :1], b[:, :, :1])
    print("\nrainfall_test f32 planes: values %.2e" % err)
    assert np.isfinite(a).all()
    assert 1e-13 < err < F32_TOL_VAL


def _model_run_with(monkeypatch, grid, semi=True, null_ref=False):
    """ModelRun of rainfall_test on `grid`, past the host-side variable check (so that sx_create's own checks answer)."""
    import scythe_jl_amd as S
    monkeypatch.setattr(S.model, "RAINFALL_VARS", dict(grid["vars"]))
    if null_ref:
        orig = S.model.model_desc

        def no_ref(model, patch):
            m, keep = orig(model, patch)
            m.ref_state = None
            return m, keep
        monkeypatch.setattr(S.model, "model_desc", no_ref)
    case = RF.rz_rain(num_cells=6, semiimplicit=semi)
    case["grid"] = grid
    gp, mp = cases.hip_params(case)
    return S.ModelRun(mp, num_tiles=1, device="cuda")


def test_sx_create_refuses_what_rainfall_test_cannot_run(monkeypatch):
    import scythe_jl_amd as S
    g = RF.rz_rain(num_cells=6)["grid"]
    rl = dict(geometry="RL", xmin=0.0, xmax=10.0, num_cells=8, vars=dict(RF.VARS))
    with pytest.raises(S.ScytheHipError, match="equation set does not match the grid geometry / variable count"):
        _model_run_with(monkeypatch, rl, semi=False)
    seven = {k: v for k, v in RF.VARS.items() if k != "qss"}
    with pytest.raises(S.ScytheHipError, match="equation set does not match the grid geometry / variable count"):
        _model_run_with(monkeypatch, dict(g, vars=seven))
    with pytest.raises(S.ScytheHipError, match="rainfall_test needs sx_model_desc.ref_state"):
        _model_run_with(monkeypatch, g, null_ref=True)
    moved = {"s": 1, "xi": 2, "mu": 3, "u": 4, "mu_c": 5, "w": 6, "mu_r": 7, "qss": 8}
    with pytest.raises(S.ScytheHipError, match="rainfall_test with semiimplicit needs xi = variable 2 and w = variable 5"):
        _model_run_with(monkeypatch, dict(g, vars=moved))
    monkeypatch.undo()
    case = RF.rz_rain(num_cells=6)
    case["grid"] = dict(g, vars=moved)
    gp, mp = cases.hip_params(case)
    with pytest.raises(ValueError, match="rainfall_test needs grid_params.vars"):
        S.ModelRun(mp, num_tiles=1, device="cuda")


# ----------------------------------------------------------------------------- seeded sweep
def draw(rng):
    semi = bool(rng.random() < 0.6)
    tiles = int(rng.choice([1, 1, 2, 3]))
    nc = int(rng.integers(4, 10)) if tiles == 1 else int(rng.integers(9 * tiles, 9 * tiles + 8))
    zDim = int(rng.choice([6, 9, 12, 14, 16, 20]))
    case = RF.rz_rain(num_cells=nc, zDim=zDim, semiimplicit=semi, xmax=float(rng.uniform(1.5e4, 3.0e4)),
                      K=float(rng.uniform(0.0, 20.0)), ts=(float(rng.uniform(0.5, 1.0)) if semi else float(rng.uniform(0.05, 0.1))))
    exchange = str(rng.choice(["a2a", "gather", "iface"])) if tiles > 1 else "a2a"
    impl = str(rng.choice(["torch", "lib"])) if tiles > 1 else "torch"
    return case, tiles, exchange, impl


def test_seeded_random_rainfall_configurations():
    """10 seeded draws (cells, 6 - 20 levels, tiles, exchange, K, time step, semi-implicit or not), 6 steps each, against the
    one-patch oracle twin at 1e-10 in every variable and slot (the d2/dz2 slot at 20 levels: 1e-10 (zDim / 16)^4)."""
    import scythe_jl_amd as S
    rng = np.random.default_rng(20261016)
    bad, compared = [], 0
    for i in range(10):
        case, tiles, exchange, impl = draw(rng)
        g = case["grid"]
        what = "%d: cells=%d zDim=%d semi=%s tiles=%d/%s/%s ts=%.3f K=%.2f" % (
            i, g["num_cells"], g["zDim"], case["semiimplicit"], tiles, exchange, impl, case["ts"], case["par"]["K"])
        try:
            hip = cases.HipModel(case, num_tiles=tiles, exchange=exchange, impl=impl)
        except S.ScytheHipError as e:
            assert "fewer than 6 free" in str(e) or "too few cells" in str(e), what + ": " + str(e)
            print(what, "refused:", e)
            continue
        a = _advance(hip, 6)
        hip.run.close()
        b = _twin(case, 6)
        # d2/dz2 (the last slot) carries the O(zDim^4) norm of the Chebyshev operator: bounded by TOL (zDim / 16)^4 beyond 16
        # levels.  (At 32 levels, not drawn, it measured 5e-10 - 1.8e-9 on the MI355X, every other slot within 7e-11.)
        err = cases.rel_err_per_var(a[:, :, :-1], b[:, :, :-1])
        err_zz = cases.rel_err_per_var(a[:, :, -1:], b[:, :, -1:])
        print(what, "%.2e, d2/dz2 %.2e" % (err, err_zz))
        compared += 1
        if not (np.isfinite(a).all() and err < TOL and err_zz < TOL * max(1.0, (g["zDim"] / 16.0) ** 4)):
            bad.append("%s: %.2e, d2/dz2 %.2e" % (what, err, err_zz))
    assert compared >= 7
    assert not bad, "\n" + "\n".join(bad)
