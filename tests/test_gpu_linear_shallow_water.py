"""-m gpu: LinearShallowWater1D and LinearShallowWaterRL (src/shallowWaterModels.jl:235-298) on the HIP path - against the numpy
oracle twin running the restated tendency (oracle/oracle_np.py), against closed-form gravity waves, through restart and
integrate_model, and the refusals of sx_create.

The linear gravity wave is the suite's one exact, oscillating, multi-variable solution on an RL grid: h drives v through its
d/dlambda slot and v drives h back through its own, so the azimuthal slots of two variables are coupled against an exact answer."""
import os

import numpy as np
import pytest

from tests import cases
from tests import linear_sw as LS

pytestmark = pytest.mark.gpu
TOL = 1e-10     # fields within 1e-10 relative of the oracle twin (cases.rel_err_per_var: every variable, every slot)


def _advance(model, steps):
    for _ in range(steps):
        model.step()
    return model.physical()


def _parity(case, steps, num_tiles=1, exchange="a2a", impl="torch", oracle=None):
    """rel_err_per_var of the HIP run against the one-patch oracle twin after `steps` steps; `oracle` = that twin's result if
    already computed for this case.  Also checks that the run changed every variable (the comparison is not of two idle states)."""
    hip = cases.HipModel(case, num_tiles=num_tiles, exchange=exchange, impl=impl)
    p0 = hip.physical().copy()
    a = _advance(hip, steps)
    hip.run.close()
    if oracle is None:
        oracle = _advance(cases.OracleModel(case, numpy_twin=True), steps)
    assert np.isfinite(a).all()
    for v in range(a.shape[1]):
        assert np.abs(a[:, v, 0] - p0[:, v, 0]).max() > 1e-3 * np.abs(p0[:, v, 0]).max()
    return cases.rel_err_per_var(a, oracle), oracle


@pytest.mark.parametrize("bc", ["PERIODIC", "walls"])
def test_linear_shallow_water_1d_matches_the_oracle_twin(bc):
    """R grid, 40 steps: PERIODIC, and walls (u R1T0, h R1T1 at both ends)."""
    err, _ = _parity(LS.r_case(num_cells=24, bc=bc), 40)
    print("\nLinearShallowWater1D %s: %.2e" % (bc, err))
    assert err < TOL


@pytest.mark.parametrize("ring_L", [None, 16, 32, 24, 12])
def test_linear_shallow_water_rl_matches_the_oracle_twin(ring_L):
    """RL grid, 40 steps: native ragged rings (DFT kernels), uniform power-of-two tables (FFT kernels), uniform tables of a
    multiple of 4 that is not a power of two (DFT kernels on a uniform table); wavenumbers 1-3 in every variable."""
    err, _ = _parity(LS.rl_case(num_cells=10, ring_L=ring_L), 40)
    print("\nLinearShallowWaterRL ring_L=%s: %.2e" % (ring_L, err))
    assert err < TOL


_ORACLE = {}


@pytest.mark.parametrize("num_cells,ntiles", [(20, 2), (30, 3)])
@pytest.mark.parametrize("exchange", ["a2a", "iface", "gather"])
@pytest.mark.parametrize("impl", ["lib", "torch"])
def test_linear_shallow_water_rl_on_tiles_matches_the_one_patch_oracle_twin(num_cells, ntiles, exchange, impl):
    """Native rings split into 2 and 3 tiles (gridpoint-balanced), every exchange protocol through the library's own buffers
    (loopback) and through the Python-side stand-in, 20 steps against the one-patch twin (computed once per patch)."""
    case = LS.rl_case(num_cells=num_cells)
    err, _ORACLE[num_cells] = _parity(case, 20, num_tiles=ntiles, exchange=exchange, impl=impl,
                                      oracle=_ORACLE.get(num_cells))
    print("\n%d cells, %d tiles, %s / %s: %.2e" % (num_cells, ntiles, exchange, impl, err))
    assert err < TOL


# ----------------------------------------------------------------------------- closed forms
def periodic_mode_error(num_cells, ts, steps, K, m=2, g=2.0, H=0.5):
    """LinearShallowWater1D on the PERIODIC line [-6, 6] from h = cos(kap x), u = sqrt(g / H) cos(kap x): max error of h and
    of u / sqrt(g / H) against the matrix-exponential solution of the mode (tests/linear_sw.py::mode_1d), and the change of h."""
    kap = 2.0 * np.pi * m / 12.0
    u0 = np.sqrt(g / H) + 0.0j
    keep = {}

    def ic(p):
        keep["x"] = p[:, 0]
        return np.stack(LS.mode_1d(p[:, 0], 0.0, kap, g, H, K, 1.0, u0), axis=1)
    case = LS.r_case(num_cells=num_cells, K=K, ts=ts, g=g, H=H)
    case["ic"] = ic
    hip = cases.HipModel(case)
    ph = _advance(hip, steps)
    hip.run.close()
    h, u = LS.mode_1d(keep["x"], ts * steps, kap, g, H, K, 1.0, u0)
    h0, _ = LS.mode_1d(keep["x"], 0.0, kap, g, H, K, 1.0, u0)
    return max(np.abs(ph[:, 0, 0] - h).max(), np.abs(ph[:, 1, 0] - u).max() / abs(u0)), np.abs(h - h0).max()


@pytest.mark.parametrize("K", [0.0, 0.05])
def test_periodic_gravity_wave_follows_the_exact_mode(K):
    """K = 0: a gravity wave travelling at c = sqrt(g H) = 1 with u / h = sqrt(g / H) = 2 (g and H enter differently: a swap is
    an O(1) error); K = 0.05: the same wave damped by the K u_rr term.  T = 3 (half a wavelength, h changes by 2.0 / 1.9):
    error 3.2e-3 / 3.3e-3 at 24 cells and 6.2e-5 / 1.35e-4 at 48 (measured on the MI355X; the oracle twin gives the same
    digits, tests/test_linear_shallow_water.py) - the spline's truncation error, falling faster than DX^4 while kap DX = 0.52
    is still coarse.  Bars at about 3 x."""
    a, change = periodic_mode_error(24, 0.02, 150, K)
    b, _ = periodic_mode_error(48, 0.01, 300, K)
    print("\nperiodic mode K = %g: changed by %.2f, error 24 cells %.2e, 48 cells %.2e" % (K, change, a, b))
    assert change > 1.8 and a < 1e-2 and b < 4e-4 and a / b > 16.0


def bessel_mode_errors(ring_L, m, n=5, g=2.0, H=0.5, R=16.0, num_cells=64, ts=0.005):
    """LinearShallowWaterRL with K = 0 from tests/linear_sw.py::bessel_gravity_mode, kap = (n-th zero of J_m') / R so that u = 0
    and h_r = 0 at the outer wall (BCR: u R1T0, h R1T1), run for one period 2 pi / w.  Errors of h, u, v relative to each
    field's maximum on the annulus 0.5 < r < 14 (away from the inner rings that truncate wavenumber m and from the edge), and
    the largest change of h over the period (it has gone through -h)."""
    from scipy.special import jnp_zeros
    kap = jnp_zeros(m, n)[-1] / R
    w = kap * np.sqrt(g * H)
    steps = int(round(2.0 * np.pi / w / ts))
    keep = {}

    def ic(p):
        keep["r"], keep["l"] = p[:, 0], p[:, 1]
        return np.stack(LS.bessel_gravity_mode(p[:, 0], p[:, 1], 0.0, m, kap, g, H), axis=1)
    grid = dict(geometry="RL", xmin=0.0, xmax=R, num_cells=num_cells, vars=LS.VARS_RL, ring_L=ring_L,
                BCR={"h": "R1T1", "u": "R1T0", "v": "R0"})
    hip = cases.HipModel(dict(name="bessel_gw", grid=grid, eq="LinearShallowWaterRL", ts=ts, par=dict(g=g, K=0.0, H=H), ic=ic))
    mid = _advance(hip, steps // 2)[:, 0, 0].copy()
    ph = _advance(hip, steps - steps // 2)
    hip.run.close()
    r = keep["r"]
    inner = (r > 0.5) & (r < 14.0)
    exact = LS.bessel_gravity_mode(r, keep["l"], steps * ts, m, kap, g, H)
    h0 = LS.bessel_gravity_mode(r, keep["l"], 0.0, m, kap, g, H)[0]
    errs = [np.abs(ph[:, v, 0] - exact[v])[inner].max() / np.abs(exact[v][inner]).max() for v in range(3)]
    return errs, np.abs(mid - h0)[inner].max() / np.abs(h0[inner]).max()


# errors of (h, u, v) after one period, measured on the MI355X (native rings and the 64-point table agree to 3 digits):
# m = 1: 2.5e-4, 4.5e-4, 3.4e-4;  m = 2: 8.3e-4, 1.8e-3, 4.7e-3.  Bars at about 3 x.
BESSEL_BOUND = {1: (7.5e-4, 1.4e-3, 1.0e-3), 2: (2.5e-3, 5.4e-3, 1.4e-2)}


@pytest.mark.parametrize("ring_L,m", [(None, 1), (None, 2), (64, 1), (64, 2)])
def test_bessel_gravity_mode_over_one_period(ring_L, m):
    """h = J_m(kap r) cos(m lam - w t) with the u and v that make it an exact rotating gravity wave; one period (1,350 steps of
    0.005 for m = 1, 1,230 for m = 2) on native rings (DFT kernels) and on a 64-point uniform table (FFT kernels).  At half
    the period h has gone through -h, a change of 2.0 times its amplitude; after the full period h, u and v are back within
    2.5e-4 / 4.5e-4 / 3.4e-4 (m = 1) and 8.3e-4 / 1.8e-3 / 4.7e-3 (m = 2) of the closed form, relative to each field's
    maximum (measured on the MI355X) - a wrong sign, a missing 1 / r or a swapped g / H in any of the three tendencies is an
    O(1) error after a period."""
    errs, change = bessel_mode_errors(ring_L, m)
    print("\nBessel gravity mode ring_L=%s m=%d: h changed by %.2f at half period, error h %.2e u %.2e v %.2e"
          % ((ring_L, m, change) + tuple(errs)))
    assert change > 1.9
    assert all(e < b for e, b in zip(errs, BESSEL_BOUND[m])), (errs, BESSEL_BOUND[m])


# ----------------------------------------------------------------------------- restart, end to end, refusals
@pytest.mark.parametrize("make,ntiles", [(lambda: LS.rl_case(num_cells=10), 1), (lambda: LS.rl_case(num_cells=27, ring_L=16), 3),
                                         (lambda: LS.r_case(num_cells=24), 2)])
def test_restart_from_a_checkpoint_is_bit_identical(tmp_path, make, ntiles):
    """Ten steps unbroken against five, save_checkpoint, a fresh run that loads it, five more."""
    case = make()
    a = cases.HipModel(case, num_tiles=ntiles)
    whole = _advance(a, 10)
    a.run.close()
    b = cases.HipModel(case, num_tiles=ntiles)
    _advance(b, 5)
    ck = str(tmp_path / "ck.npz")
    b.run.save_checkpoint(ck)
    b.run.close()
    c = cases.HipModel(case, num_tiles=ntiles)
    c.run.load_checkpoint(ck)
    assert c.run.t == 5
    halves = _advance(c, 5)
    c.run.close()
    assert np.array_equal(whole, halves)


def test_integrate_model_writes_the_rl_gravity_wave(tmp_path):
    """integrate_model on a LinearShallowWaterRL model: initial conditions from CSV, 20 steps with output every 10, the
    physical_out files carry h, u, v (and their slots); the final one equals a ModelRun's fields after 20 steps exactly."""
    import scythe_jl_amd as S
    case = LS.rl_case(num_cells=8)
    gp, _ = cases.hip_params(case)
    model = S.ModelParameters(ts=case["ts"], integration_time=20 * case["ts"], output_interval=10 * case["ts"],
                              equation_set="LinearShallowWaterRL", initial_conditions=str(tmp_path / "ic.csv"),
                              output_dir=str(tmp_path / "out"), grid_params=gp, physical_params=dict(case["par"]))
    grid = S.createGrid(gp)
    pts = S.getGridpoints(grid)
    grid.close()
    vals = case["ic"](pts)
    np.savetxt(model.initial_conditions, np.concatenate([pts, vals], axis=1), delimiter=",", header="r,l,h,u,v", comments="",
               fmt="%.17g")
    assert S.integrate_model(model) is True
    files = sorted(f for f in os.listdir(model.output_dir) if f.startswith("physical_out_"))
    assert files == ["physical_out_0.0.csv", "physical_out_0.05.csv", "physical_out_0.1.csv"], files
    path = os.path.join(model.output_dir, "physical_out_0.1.csv")
    header = open(path).readline().strip().split(",")
    assert header[:5] == ["r", "l", "h", "u", "v"] and "v_ll" in header
    final = np.loadtxt(path, delimiter=",", skiprows=1)
    run = cases.HipModel(case)
    ph = _advance(run, 20)
    run.run.close()
    assert np.array_equal(final[:, :2], pts)
    assert np.array_equal(final[:, 2:], np.concatenate([ph[:, :, d] for d in range(ph.shape[2])], axis=1))
    assert np.abs(ph[:, :, 0] - vals).max() > 1e-3


@pytest.mark.parametrize("eq,geometry,nv", [("LinearShallowWater1D", "RL", LS.VARS_RL), ("LinearShallowWaterRL", "R", LS.VARS_RL),
                                            ("LinearShallowWaterRL", "RL", LS.VARS_1D), ("LinearShallowWater1D", "R", {"h": 1})])
def test_sx_create_refuses_the_wrong_grid_or_too_few_variables(eq, geometry, nv):
    import scythe_jl_amd as S
    gp = S.GridParameters(geometry=geometry, xmin=0.0, xmax=10.0, num_cells=8, vars=nv)
    mp = S.ModelParameters(ts=0.01, equation_set=eq, grid_params=gp, physical_params=dict(g=1.0, H=1.0))
    with pytest.raises(S.ScytheHipError, match="equation set does not match the grid geometry / variable count"):
        S.ModelRun(mp, num_tiles=1, device="cuda")


# ----------------------------------------------------------------------------- seeded sweep
RADIAL = ["R0", "R1T0", "R1T1", "R1T2", "R2T10", "R2T20", "R3"]


def draw(rng):
    """Set, cell count, ring table, tiles and exchange, g / H / K, boundary conditions per variable, time step from the
    gravity-wave speed and the cell size."""
    eq = str(rng.choice(LS.SETS, p=[0.3, 0.7]))
    tiles = int(rng.choice([1, 1, 2, 3]))
    nc = int(rng.integers(4, 16)) if tiles == 1 else int(rng.integers(9 * tiles, 9 * tiles + 8))
    g, H, K = float(rng.uniform(0.5, 3.0)), float(rng.uniform(0.2, 2.0)), float(rng.choice([0.0, rng.uniform(0.0, 0.01)]))
    xmax = float(rng.uniform(0.5, 1.5)) * nc
    DX = xmax / nc
    ts = 0.03 * DX / np.sqrt(g * H)
    if eq == "LinearShallowWater1D":
        case = LS.r_case(num_cells=nc, bc="PERIODIC", g=g, H=H, K=K, ts=ts)
        if rng.random() < 0.6:
            case["grid"].update(xmin=0.0, xmax=xmax, BCL={v: str(rng.choice(RADIAL)) for v in LS.VARS_1D},
                                BCR={v: str(rng.choice(RADIAL)) for v in LS.VARS_1D})
    else:
        ring_L = rng.choice([None, None, None, 16, 32, 24, 12, 20, 8])
        case = LS.rl_case(num_cells=nc, ring_L=None if ring_L is None else int(ring_L), g=g, H=H, K=K, ts=ts, xmax=xmax,
                          bcl={v: str(rng.choice(RADIAL)) for v in LS.VARS_RL}, bcr={v: str(rng.choice(RADIAL)) for v in LS.VARS_RL})
    exchange = str(rng.choice(["a2a", "gather", "iface"])) if tiles > 1 else "a2a"
    impl = str(rng.choice(["torch", "lib"])) if tiles > 1 else "torch"
    return case, tiles, exchange, impl


def test_seeded_random_linear_shallow_water_configurations():
    """12 seeded draws, 10 steps each, against the one-patch oracle twin at 1e-10 in every variable and slot."""
    import scythe_jl_amd as S
    rng = np.random.default_rng(20261016)
    bad, compared = [], 0
    for i in range(12):
        case, tiles, exchange, impl = draw(rng)
        g = case["grid"]
        what = "%d: %s cells=%d ring_L=%s tiles=%d/%s/%s BCL=%s BCR=%s par=%s" % (
            i, case["eq"], g["num_cells"], g.get("ring_L"), tiles, exchange, impl, g.get("BCL"), g.get("BCR"),
            {k: round(v, 4) for k, v in case["par"].items()})
        try:
            hip = cases.HipModel(case, num_tiles=tiles, exchange=exchange, impl=impl)
        except S.ScytheHipError as e:
            # a refusal must be one of the documented ones (too few free coefficients for the interface-only solve)
            assert "fewer than 6 free" in str(e) or "too few cells" in str(e), what + ": " + str(e)
            print(what, "refused:", e)
            continue
        a = _advance(hip, 10)
        hip.run.close()
        b = _advance(cases.OracleModel(case, numpy_twin=True), 10)
        err = cases.rel_err_per_var(a, b)
        print(what, "%.2e" % err)
        compared += 1
        if not (np.isfinite(a).all() and err < TOL):
            bad.append("%s: %.2e" % (what, err))
    assert compared >= 9
    assert not bad, "\n" + "\n".join(bad)
