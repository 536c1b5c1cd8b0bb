"""sx_parcels_* on the GPU against the twins of tests/parcels.py: the longdouble twin is the arbiter, the rounding bound of a
velocity is the one derived there, and positions are held to 8 x the spread the CPU suite measures between the Float64 and the
longdouble twin (tests/test_parcels.py::test_twin_spread -> P.TWIN_SPREAD).  The margin is that large because the device sums in a
different, fixed order (lanes stride over the columns, a butterfly and a wave loop reduce them) and uses its own sincos."""
import numpy as np
import pytest

from tests import cases
from tests import parcels as P
from tests.test_parcels import GEOMS, rotation_bound

pytestmark = pytest.mark.gpu

MARGIN = 8.0


# every geometry on its smallest grid, and RLZ on the grid above 1,024 columns per variable (256 lanes per parcel)
GRIDS = [pytest.param(geom, False, id=geom) for geom in GEOMS] + [pytest.param("RLZ", True, id="RLZ_wide")]


def _tile(geom, A, wide=False):
    import scythe_jl_amd as S
    gp, mp = cases.hip_params(P.grid_case(geom, wide))
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(A)
    return tile


def _tile_from_values(case, ic):
    """a one-tile handle whose A is the transform of the gridpoint values ic(points)"""
    import scythe_jl_amd as S
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp)
    pts = S.getGridpoints(tile)
    tile.set_physical_values(ic(pts.reshape(len(pts), -1)))
    tile.spectralTransform_()
    tile.splineTransform_()
    return tile


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


@pytest.mark.parametrize("geom,wide", GRIDS)
def test_velocity(geom, wide):
    g = cases.oracle_grid(P.grid_case(geom, wide))
    A = P.smooth_state(g, seed=3)
    pts, var = P.special_points(g), P.velocity_vars(g)
    tile = _tile(geom, A, wide)
    tile.set_parcels(pts, P.VELOCITY[geom])
    tile.enable_timers(True)
    tile.advance_parcels(0.0)
    pos, vel, status = tile.parcels()
    # the timers know the kernel, and its A bytes are parcels x velocity variables x 4 rows x b_zDim x (2 kDim + 1) doubles
    assert tile.timers()["k_parcels"][1] == 1
    assert tile.kernel_bytes("k_parcels") == 8.0 * 4 * g.b_zDim * g.K2 * len(var) * len(pts)
    tile.enable_timers(False)
    if g.has_l:                                     # parcel 0 sits at r = 0 with lambda = 0.7: after a step the centre has lambda = 0
        assert pos[0, 0] == 0.0 and pos[0, 1] == 0.0 and pts[0, 1] == 0.7
        assert (pos[:, 1] > -np.pi).all() and (pos[:, 1] <= np.pi).all()
    red = pts.copy()
    if g.has_l:
        red[:, 1] = P.reduce_lambda(pts[:, 1])
    truth, S_abs, bound = P.velocity(g, A, red, var, xp=True, with_bound=True)
    ev = tile.evaluate(pts, all_k=True)
    r_twin = np.abs(vel.astype(P.XP) - truth) / bound
    r_eval = np.stack([np.abs(vel[:, c] - ev[:, v - 1, 0]) for c, v in enumerate(var)], axis=1) / bound
    print("%s: |device - longdouble twin| / bound max %.3f; |device - sx_evaluate ALL_K| / bound max %.3f (allowed 1, 2)"
          % (geom, float(r_twin.max()), float(r_eval.max())))
    assert np.isfinite(vel).all() and np.abs(vel).max() > 0
    assert (r_twin <= 1.0).all(), r_twin.max()
    assert (r_eval <= 2.0).all(), r_eval.max()
    assert vel[8].tobytes() == vel[4].tobytes() and vel[9].tobytes() == vel[2].tobytes()        # duplicates
    tile.close()


def test_solid_body_rotation():
    """v = Omega r, u = 0 held by A (rl_advection's conditions are R0 on both sides: they admit it); 50 steps of theta = 1e-3"""
    omega, theta, n = 0.25, 1.0e-3, 50
    dt = theta / omega
    case = cases.rl_advection(num_cells=6)
    g = cases.oracle_grid(case)
    tile = _tile_from_values(case, lambda p: np.stack([0.0 * p[:, 0], 0.0 * p[:, 0], omega * p[:, 0]], axis=1))
    A = tile.patchSpectral
    pts = np.array([[0.5, 0.3], [3.0, -2.0], [9.0, 3.1], [6.0, 1.0e6], [0.01, 2.0]])
    tile.set_parcels(pts, ("u", "v"))
    tw = P.Parcels(g, pts, (2, 3), xp=False)
    lam0 = tw.pos[:, 1].copy()
    for _ in range(n):
        tile.advance_parcels(dt)
        tw.advance(A, dt)
    pos, vel, status = tile.parcels()
    assert (status == 0).all() and (tw.status == 0).all()
    d = P.distance(g, pos, np.stack([pts[:, 0], lam0 + n * theta], axis=1))
    print("distance from the circle / bound:", d / rotation_bound(pts[:, 0], theta, n))
    assert (d <= rotation_bound(pts[:, 0], theta, n)).all(), d
    unit = dt * P.EPS * tw.S_max
    s = P.distance(g, pos, tw.pos) / unit
    print("device - Float64 twin after %d steps: %.1f dt eps S (allowed %.0f x %.0f)" % (n, s.max(), MARGIN, P.TWIN_SPREAD))
    assert (s <= MARGIN * P.TWIN_SPREAD).all(), s
    tile.close()


def _random_run(geom, pts, steps=6, tile=None, A=None, g=None, dt=None):
    tile.set_parcels(pts, P.VELOCITY[geom])
    path = []
    for _ in range(steps):
        tile.advance_parcels(dt)
        path.append(tile.parcels())
    return path


@pytest.mark.parametrize("geom,wide", GRIDS)
def test_frozen_random_state_and_independence(geom, wide):
    """67 parcels, 6 steps in a state that does not change: positions against the longdouble twin; the same parcels reversed and
    three of them alone take bitwise the same paths; an empty set advances and reads back empty"""
    g = cases.oracle_grid(P.grid_case(geom, wide))
    A = P.smooth_state(g, seed=11)
    pts, var = P.interior_points(g, 67, seed=13), P.velocity_vars(g)
    dt = P.crossing_dt(g, A, pts, var)
    tile = _tile(geom, A, wide)
    path = _random_run(geom, pts, tile=tile, dt=dt)
    hi = P.Parcels(g, pts, var, xp=True)
    for _ in range(6):
        hi.advance(A, dt)
    pos, vel, status = path[-1]
    assert (status == 0).all() and (hi.status == 0).all() and np.isfinite(pos).all()
    s = P.distance(g, pos, hi.pos) / (dt * P.EPS * hi.S_max)
    print("%s: device - longdouble twin after 6 steps: %.1f dt eps S (allowed %.0f x %.0f)" % (geom, s.max(), MARGIN, P.TWIN_SPREAD))
    assert (s <= MARGIN * P.TWIN_SPREAD).all(), s.max()
    rev = _random_run(geom, pts[::-1], tile=tile, dt=dt)
    for a, b in zip(path, rev):
        assert _bits(a[0], a[1], a[2]) == _bits(b[0][::-1], b[1][::-1], b[2][::-1])
    for i in (0, 33, 66):
        alone = _random_run(geom, pts[i:i + 1], tile=tile, dt=dt)
        for a, b in zip(path, alone):
            assert _bits(a[0][i], a[1][i], a[2][i]) == _bits(b[0][0], b[1][0], b[2][0]), (geom, i)
    tile.set_parcels(np.zeros((0, pts.shape[1])), P.VELOCITY[geom])
    tile.advance_parcels(dt)
    pos, vel, status = tile.parcels()
    assert pos.shape == (0, pts.shape[1]) and vel.shape == (0, pts.shape[1]) and status.shape == (0,) and tile.n_parcels == 0
    tile.close()


def test_leaving_and_wrap():
    case = P.grid_case("RZ")
    g = cases.oracle_grid(case)
    L, H = g.xmax - g.xmin, g.zmax - g.zmin
    # u and v constant: v (conditions R0) stands in for the vertical wind, w's own conditions hold it to zero at both ends
    tile = _tile_from_values(case, lambda p: np.stack([0 * p[:, 0], 0.004 * L + 0 * p[:, 0], 0.004 * H + 0 * p[:, 0], 0 * p[:, 0]], axis=1))
    inside = np.array([[g.xmin + 0.5 * L, g.zmin + 0.5 * H], [g.xmin + 0.3 * L, g.zmin + 0.2 * H]])
    start = np.array([[g.xmax - 0.01 * L, g.zmin + 0.5 * H], inside[0], [g.xmin + 0.5 * L, g.zmax - 0.01 * H], inside[1]])

    def run(p):
        tile.set_parcels(p, ("u", "v"))
        out = []
        for _ in range(8):
            tile.advance_parcels(1.0)
            out.append(tile.parcels())
        return out
    both, alone = run(start), run(inside)
    for (pos, vel, status), (pos1, vel1, status1) in zip(both, alone):
        assert _bits(pos[[1, 3]], vel[[1, 3]], status[[1, 3]]) == _bits(pos1, vel1, status1)       # the neighbours' bits
    assert list(both[1][2]) == [0, 0, 0, 0] and list(both[2][2]) == [1, 0, 2, 0] and list(both[7][2]) == [1, 0, 2, 0]
    for k in range(3, 8):                                                  # frozen at the last inside position for 5 further steps
        assert _bits(both[k][0][[0, 2]]) == _bits(both[1][0][[0, 2]]) and np.isfinite(both[k][0]).all() and np.isfinite(both[k][1]).all()
    assert both[7][0][0, 0] <= g.xmax and both[7][0][2, 1] <= g.zmax and both[7][0][1, 0] > inside[0, 0]
    tile.close()

    case = P.grid_case("R")
    g = cases.oracle_grid(case)
    L = g.xmax - g.xmin
    tile = _tile_from_values(case, lambda p: np.ones((len(p), 1)))
    tile.set_parcels(np.array([[g.xmax - 0.01 * L], [g.xmin + 0.5 * L]]), ("u",))
    for _ in range(3):
        tile.advance_parcels(0.02 * L)
    pos, vel, status = tile.parcels()
    assert (status == 0).all() and np.abs(vel - 1.0).max() < 1e-12
    assert np.abs(pos[:, 0] - (g.xmin + np.array([0.05, 0.56]) * L)).max() < 1e-11 * L, pos
    tile.close()


MODEL_POINTS = np.array([[1.0, 0.5], [4.0, -2.5], [7.5, 3.0], [0.2, 1.0], [9.0, 0.0]])


def _model_run(with_parcels, steps=8, manual=False, checkpoint=None, resume=None, case=None, points=MODEL_POINTS, vel=("u", "v"),
               timed=False):
    """timed: every kernel of the steps is timed and the launch counts come back (a run of its own: timers change the schedule)"""
    hip = cases.HipModel(case or cases.rl_advection(num_cells=6))
    run, tile = hip.run, hip.run.tiles[0]
    if resume is not None:
        run.load_checkpoint(resume)
    elif with_parcels and manual:
        tile.set_parcels(points, vel)
    elif with_parcels:
        run.set_parcels(points, vel)
    if timed:
        tile.enable_timers(True)
        for _ in range(steps):
            run.step()
        calls = {k: v[1] for k, v in tile.timers().items()}
        run.close()
        return calls
    path = []
    while run.t < steps:
        if manual:
            tile.advance_parcels(run.model.ts)
        run.step()
        path.append(run.parcels())
        if checkpoint is not None and run.t == 4:
            run.save_checkpoint(checkpoint)
    out = dict(A=run.patch_spectral(), state=tile.get_state(), path=path)
    run.close()
    return out


@pytest.mark.parametrize("overlap", ["0", "1"])
def test_with_the_model(overlap, monkeypatch, tmp_path):
    """LinearAdvectionRL, 8 steps of ModelRun.step() with a parcel set, with SX_OVERLAP unset and set (this equation set keeps one
    stream either way; the second stream is the next test's): the model state is bitwise the state of the run without parcels, the paths are bitwise those of advance_parcels(ts); step by hand, and a run
    resumed from the checkpoint of step 4 ends bitwise where the uninterrupted one does"""
    monkeypatch.setenv("SX_OVERLAP", overlap)
    ck = str(tmp_path / "ck.npz")
    plain = _model_run(False)
    auto = _model_run(True, checkpoint=ck)
    manual = _model_run(True, manual=True)
    assert _bits(plain["A"], plain["state"]) == _bits(auto["A"], auto["state"])
    assert len(plain["path"][-1][2]) == 0 and len(auto["path"][-1][2]) == len(MODEL_POINTS)
    for a, b in zip(auto["path"], manual["path"]):
        assert _bits(*a) == _bits(*b)
    moved = np.abs(auto["path"][-1][0] - auto["path"][0][0]).max()
    assert moved > 0 and np.isfinite(auto["path"][-1][0]).all()
    resumed = _model_run(True, resume=ck)
    assert len(resumed["path"]) == 4
    assert _bits(*resumed["path"][-1]) == _bits(*auto["path"][-1])
    assert _bits(resumed["A"], resumed["state"]) == _bits(auto["A"], auto["state"])


# the shape on which sx_advance's second stream is live (tests/test_gpu_evaluate.py): the node-space inverse needs 32 levels on
# uniform power-of-two rings; its wb is the diagnostic variable SX_DEFER_DIAG defers
HRBL_POINTS = np.array([[2.0e4, 0.5, 300.0], [1.1e5, -2.5, 1500.0], [2.4e5, 3.0, 50.0], [3.0e3, 1.0, 900.0], [2.9e5, 0.0, 1900.0]])


@pytest.mark.parametrize("switch", ["SX_OVERLAP", "SX_DEFER_DIAG"])
def test_with_the_model_second_stream_and_deferred_diagnostic(switch, monkeypatch):
    """The HRBL set on RLZ 8 cells x 32 levels x 32-point rings with parcels on ub, vb, wb.  SX_OVERLAP=1: the inner-ring chain runs on
    the second stream while k_parcels has read A on the first.  SX_DEFER_DIAG=1: wb's coefficients are stale when the parcels want
    them, so the advance brings them up to date first (more launches than the one kernel).  Either way the model state is bitwise
    the state without parcels and the paths are bitwise those of advance_parcels(ts); step by hand."""
    monkeypatch.setenv(switch, "1")
    kw = dict(case=cases.rlz_hrbl(num_cells=8, zDim=32, ring_L=32), points=HRBL_POINTS, vel=("ub", "vb", "wb"))
    plain = _model_run(False, **kw)
    auto = _model_run(True, **kw)
    manual = _model_run(True, manual=True, **kw)
    assert _bits(plain["A"], plain["state"]) == _bits(auto["A"], auto["state"])
    for a, b in zip(auto["path"], manual["path"]):
        assert _bits(*a) == _bits(*b)
    pos, vel, status = auto["path"][-1]
    assert np.isfinite(pos).all() and (status == 0).all() and np.abs(pos - auto["path"][0][0]).max() > 0 and np.abs(vel[:, :2]).max() > 0
    c0, c1 = _model_run(False, steps=3, timed=True, **kw), _model_run(True, steps=3, timed=True, **kw)
    assert c1.pop("k_parcels") == 3 and "k_parcels" not in c0
    if switch == "SX_OVERLAP":
        assert {"k_phys_hrbl_inner", "k_node_fft"} <= set(c0), c0           # the two chains of launch_inverse_and_physics
        assert c1 == c0                                                      # nothing but k_parcels is added
    else:
        # steps 2 and 3 find wb's coefficients deferred: each advance launches the forward transform, the inner products and the
        # solve for that one variable before k_parcels
        assert sum(c1.values()) > sum(c0.values()), (c0, c1)


def test_refusals():
    import scythe_jl_amd as S
    g = cases.oracle_grid(P.grid_case("RZ"))
    tile = _tile("RZ", P.smooth_state(g, seed=3))
    good = P.interior_points(g, 5, seed=1)
    tile.set_parcels(good, ("u", "w"))
    tile.advance_parcels(1.0e-3)
    before = tile.parcels()
    bad = good.copy()
    bad[2, 1] = np.nan
    with pytest.raises(S.ScytheHipError, match="NaN"):
        tile.set_parcels(bad, ("u", "w"))
    bad = good.copy()
    bad[1, 0] = g.xmax + 1.0
    with pytest.raises(S.ScytheHipError, match="outside the tile"):
        tile.set_parcels(bad, ("u", "w"))
    with pytest.raises(S.ScytheHipError, match="var_l"):
        from scythe_jl_amd import _lib as L
        L.check(tile._lib.sx_parcels_set(tile._h, 5, np.asfortranarray(good).ctypes.data_as(L.P_D), 2, 3, 0))
    with pytest.raises(S.ScytheHipError, match="variable index"):
        tile.set_parcels(good, (g.V + 1, "w"))
    with pytest.raises(S.ScytheHipError, match="NaN or Inf"):
        tile.advance_parcels(float("inf"))
    # the restart blob: a wrong magic, a wrong size, a position outside the tile
    blob = tile.get_parcel_state()
    for change, what in ((lambda b: b.__setitem__(0, 1.0), "does not belong"), (lambda b: b.__setitem__(1, 4.0), "does not belong"),
                         (lambda b: b.__setitem__(6, g.xmax + 1.0), "outside the tile")):
        bad = blob.copy()
        change(bad)
        with pytest.raises(S.ScytheHipError, match=what):
            tile.set_parcel_state(bad)
    with pytest.raises(S.ScytheHipError, match="does not belong"):
        tile.set_parcel_state(blob[:-1])
    after = tile.parcels()
    assert _bits(*before) == _bits(*after) and tile.n_parcels == 5
    tile.set_parcel_state(blob)
    assert _bits(*before) == _bits(*tile.parcels()) and _bits(blob) == _bits(tile.get_parcel_state())
    tile.close()
    gp, mp = cases.hip_params(cases.rl_advection(num_cells=8))
    run = S.ModelRun(mp, num_tiles=2, device="cuda")
    with pytest.raises(ValueError, match="one-tile"):
        run.set_parcels(MODEL_POINTS, ("u", "v"))
    run.close()
