"""sx_crossings on the GPU against the twin of tests/crossings.py.

Profiles are held entry by entry to the longdouble twin within 10 x the float64 twin's error on the same input, with the derived
rounding bound of tests/crossings.py as the floor.  Crossings are held to the longdouble twin: counts and directions equal, radii
within 2 tol DX + 10 |float64 twin - longdouble twin| with a floor of 8 eps xmax; the levels are transversal (checked on the twin).
Every test prints its worst figures before it asserts; DESIGN.md 15, "Figures", holds those of one run on the card."""
import numpy as np
import pytest

from tests import cases
from tests import crossings as X
from tests import linear_sw as LS

pytestmark = pytest.mark.gpu

XP = X.XP
EPS = 2.0 ** -52
GRIDS = {"r4": ("r_bcs", dict(num_cells=4)), "rz5x8": ("rz_advection", dict(num_cells=5, zDim=8)),
         "rl6": ("rl_advection", dict(num_cells=6)), "rl12_L16": ("rl_advection", dict(num_cells=12, ring_L=16)),
         "rlz5x6_L8": ("rlz_advection", dict(num_cells=5, zDim=6, ring_L=8))}
RAY_COUNTS = (1, 15, 16, 17, 33)


def _make(name):
    import scythe_jl_amd as S
    maker, kw = GRIDS[name]
    case = getattr(cases, maker)(**kw)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    tile = S.Grid(gp, mp)
    return case, gp, g, tile


def _rays(g, n, seed=3):
    """n seeded rays: lambda in [-2 pi, 4 pi] (so below -2 pi .. above 2 pi are reduced on the host), z with both ends"""
    rng = np.random.default_rng(seed)
    cols = []
    if g.has_l:
        lam = rng.uniform(-2.0 * np.pi, 4.0 * np.pi, n)
        lam[:3] = [0.0, -1.0, 7.0][:min(n, 3)]
        cols.append(lam)
    if g.has_z:
        z = rng.uniform(g.zmin, g.zmax, n)
        z[:2] = [g.zmin, g.zmax][:min(n, 2)]
        cols.append(np.roll(z, 1))
    return np.stack(cols, axis=1) if cols else n


def _sub(rays, sel):
    return rays[sel] if isinstance(rays, np.ndarray) else len(np.arange(rays)[sel])


def _all_slot_program(g):
    """every slot of the geometry on variable 1, and the value of the last variable: every profile kind the geometry has"""
    names = [s if s != "u" else "" for s in g.slots]
    prog = [(0, 1.0 + 0.25 * i, 0, [(1, s)]) for i, s in enumerate(names)]
    if g.V > 1:
        prog.append((0, -0.5, 0, [(g.V, ""), (g.V, "r")]))
    return prog


# ----------------------------------------------------------------------------- 5. profiles, entry by entry
@pytest.mark.parametrize("name", list(GRIDS))
def test_profiles(name):
    import scythe_jl_amd as S
    case, gp, g, tile = _make(name)
    rng = np.random.default_rng(11)
    A = rng.standard_normal((g.S_patch(), g.V))
    tile.set_patch_spectral_a(A)
    prog = _all_slot_program(g)
    packed = S.pack_reduce_program(gp, prog)
    pl = X.plan(g, packed[1])
    rays = _rays(g, 33)
    q = X.reduce_rays(g, rays)
    Px, P64 = X.profiles(g, A, pl, q, xp=True), X.profiles(g, A, pl, q, xp=False)
    bound = X.profile_bound(g, A, pl, q)
    e64 = np.abs(P64.astype(XP) - Px).max(axis=(0, 2))                      # per profile
    full = None
    for n in RAY_COUNTS:
        res = tile.crossings(prog, [0.0], _sub(rays, slice(0, n)), return_profiles=True)
        assert res.profiles.shape == (g.b_rDim, len(pl.keys), n)
        err = np.abs(res.profiles.astype(XP) - Px[:, :, :n])
        lim = np.maximum(10.0 * e64[None, :, None], bound[:, :, :n])
        scale = np.abs(Px).max(axis=(0, 2))
        print("%s n=%d: profile error / largest entry, worst %.3g (float64 twin %.3g, floor %.3g); worst error / bar %.3g"
              % (name, n, float((err.max(axis=(0, 2)) / scale).max()), float((e64 / scale).max()),
                 float((bound.max(axis=(0, 2)) / scale).max()), float((err / lim).max())))
        assert (err <= lim).all()
        if n == 33:
            full = res.profiles
    # the smaller calls are prefixes of the largest, bitwise (the ray count does not enter a ray's sum)
    for n in RAY_COUNTS[:-1]:
        res = tile.crossings(prog, [0.0], _sub(rays, slice(0, n)), return_profiles=True)
        assert res.profiles.tobytes() == np.asfortranarray(full[:, :, :n]).tobytes(), (name, n)
    n = RAY_COUNTS[-2]                                                       # the last call's
    nb = 8.0 * (g.b_rDim * g.b_zDim * g.K2 * (2 if g.V > 1 else 1) + n * q.shape[1] + g.b_rDim * len(pl.keys) * n)
    assert tile.kernel_bytes("k_ray_profiles") == nb
    tile.close()


# ----------------------------------------------------------------------------- smooth fields for the crossings
def _field(g, pts):
    """axisymmetric plus wave 1 and 2 (plus a vertical tilt), in every variable with another amplitude"""
    r = pts[:, 0]
    s = (r - g.xmin) / (g.xmax - g.xmin)
    f = np.exp(-(2.2 * s) ** 2) + 0.15 * s
    if g.has_l:
        l = pts[:, 1]
        f = f * (1.0 + 0.6 * s * np.cos(l - 0.3) + 0.8 * s * s * np.sin(2.0 * l + 0.2))
    if g.has_z:
        zz = (pts[:, -1] - g.zmin) / (g.zmax - g.zmin)
        f = f * (1.0 + 0.3 * zz - 0.2 * zz * zz)
    return np.stack([f * (1.0 + 0.5 * v) for v in range(g.V)], axis=1)


def _filled(name):
    import scythe_jl_amd as S
    case, gp, g, tile = _make(name)
    pts = S.getGridpoints(tile)
    pts = pts.reshape(len(pts), -1)
    tile.set_physical_values(_field(g, pts))
    tile.spectralTransform_()
    tile.splineTransform_()
    return case, gp, g, tile, pts


def _radii(pts):
    r = pts[:, 0]
    return r[np.concatenate([[True], r[1:] != r[:-1]])]


def _check_against_twin(name, g, gp, tile, prog, levels, rays, radii, max_cross=4, tol=None):
    """counts, directions, radii of the device against the longdouble twin with the bar of the module docstring; returns the result"""
    import scythe_jl_amd as S
    packed = S.pack_reduce_program(gp, prog)
    A = tile.patchSpectral
    t = 1e-9 if tol is None else tol
    tx = X.crossings(g, A, packed, levels, rays, tol=t, max_cross=max_cross, xp=True, radii=radii)
    t64 = X.crossings(g, A, packed, levels, rays, tol=t, max_cross=max_cross, xp=False, radii=radii)
    res = tile.crossings(prog, levels, rays, tol=tol, max_cross=max_cross)
    # transversal levels: |g'| DX at every root of the twin is at least 1e-3 of the field's range on the ray's stations
    pl = X.plan(g, packed[1])
    q = X.reduce_rays(g, rays)
    Px = X.profiles(g, A, pl, q, xp=True)
    st = X.stations(g, radii)
    worst_t = np.inf
    for i in range(len(q)):
        fn = lambda r: X.value(g, Px[:, :, i], pl, packed, r, True)
        gv = np.array([fn(r) for r in st])
        rng_ = float(gv.max() - gv.min())
        for j in range(len(levels)):
            for k in range(min(int(tx.count[j, i]), max_cross)):
                r0, h = tx.radius[k, j, i], 1e-4 * g.DX
                lo, hi = max(r0 - h, st[0]), min(r0 + h, st[-1])
                slope = abs(float((fn(hi) - fn(lo)) / XP(hi - lo)))
                worst_t = min(worst_t, slope * g.DX / rng_)
    assert worst_t >= 1e-3, (name, worst_t)
    assert np.array_equal(res.count, tx.count) and np.array_equal(res.dir, tx.dir), (name, res.count, tx.count)
    assert np.array_equal(np.isnan(res.radius), np.isnan(tx.radius))
    with np.errstate(invalid="ignore"):
        err = np.abs(res.radius - tx.radius)
        bar = np.maximum(2.0 * t * g.DX + 10.0 * np.abs(t64.radius - tx.radius), 8.0 * EPS * max(abs(g.xmax), abs(g.xmin)))
    ok = ~np.isnan(tx.radius)
    print("%s: %d crossings, least |g'| DX / range %.3g, worst |r - twin| %.3g DX, worst error / bar %.3g"
          % (name, int(ok.sum()), worst_t, float((err[ok] / g.DX).max()) if ok.any() else 0.0, float((err[ok] / bar[ok]).max()) if ok.any() else 0.0))
    assert ok.any() and (err[ok] <= bar[ok]).all() and (res.status == tx.status).all()
    return res


# ----------------------------------------------------------------------------- 7. crossings against the twin
@pytest.mark.parametrize("name", list(GRIDS))
def test_crossings_against_twin(name):
    case, gp, g, tile, pts = _filled(name)
    rays = _rays(g, 5, seed=5)
    prog = [(0, 1.0, 0, [(1, ""), (1, "")]), (0, 0.3, 0, [(1, "")])]        # h^2 + 0.3 h: monotone in h > 0
    res = _check_against_twin(name, g, gp, tile, prog, [0.2, 0.55, 0.9], rays, _radii(pts))
    assert (res.count >= 1).any()
    tile.close()


# ----------------------------------------------------------------------------- 6. ray and level independence, bitwise
@pytest.mark.parametrize("name", ["rl12_L16", "rlz5x6_L8"])
def test_ray_and_level_independence(name):
    case, gp, g, tile, pts = _filled(name)
    rays = _rays(g, 33, seed=9)
    prog = [(0, 1.0, 0, [(1, ""), (1, "")]), (0, 0.3, 0, [(1, "")]), (0, 0.01 * g.DX, 0, [(1, "r")])]
    levels = [0.2, 0.55, 0.9]
    full = tile.crossings(prog, levels, rays, return_profiles=True)
    assert (full.count >= 1).any()
    for i in (0, 7, 15, 16, 32):
        for sub in (rays[[i]], rays[[i, i]]):
            one = tile.crossings(prog, levels, sub, return_profiles=True)
            for k in range(len(sub)):
                assert one.profiles[:, :, k].tobytes() == full.profiles[:, :, i].tobytes(), (name, i)
                assert one.radius[:, :, k].tobytes() == full.radius[:, :, i].tobytes() and one.dir[:, :, k].tobytes() == full.dir[:, :, i].tobytes()
                assert (one.count[:, k] == full.count[:, i]).all() and one.status[k] == full.status[i]
    for j, c in enumerate(levels):
        one = tile.crossings(prog, [c], rays)
        assert one.radius[:, 0, :].tobytes() == full.radius[:, j, :].tobytes() and (one.count[0] == full.count[j]).all()
        assert one.dir[:, 0, :].tobytes() == full.dir[:, j, :].tobytes()
    tile.close()


# ----------------------------------------------------------------------------- 8. shape edges
R2 = [(0, 1.0, 2, [])]                                                      # the program r^2: no plane, no A


@pytest.mark.parametrize("nc", [21, 22])
def test_station_chunks(nc):
    """21 cells are 65 stations, 22 are 68: a crossing between stations 63 and 64 (across the lane chunks), one inside the second chunk,
    and levels exactly on stations (the last of the first chunk, the first of the second)"""
    import scythe_jl_amd as S
    case = cases.r_bcs(num_cells=nc)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    tile = S.Grid(gp, mp)
    st = X.stations(g, S.getGridpoints(tile))
    assert len(st) == {21: 65, 22: 68}[nc]
    mid = 0.5 * (st[63] + st[64])
    levels = [mid * mid, float(st[63]) ** 2, float(st[64]) ** 2, float(st[30]) ** 2]
    if nc == 22:
        levels.append((0.5 * (st[65] + st[66])) ** 2)
    res = tile.crossings(R2, levels, 1, max_cross=2)
    assert (res.count[:, 0] == 1).all() and (res.dir[0, :, 0] == 1).all() and res.status[0] == 0
    assert np.isnan(res.radius[1]).all() and (res.dir[1] == 0).all()
    assert abs(res.radius[0, 0, 0] - mid) <= 2e-9 * g.DX and st[63] < res.radius[0, 0, 0] < st[64]
    assert res.radius[0, 1, 0] == st[63] and res.radius[0, 2, 0] == st[64] and res.radius[0, 3, 0] == st[30]      # bitwise the stations
    if nc == 22:
        assert abs(res.radius[0, 4, 0] - 0.5 * (st[65] + st[66])) <= 2e-9 * g.DX
    tw = X.crossings(g, np.zeros((g.S_patch(), 1)), S.pack_reduce_program(gp, R2), levels, 1, max_cross=2, xp=False, radii=st[1:-1])
    assert np.array_equal(tw.count, res.count) and np.array_equal(tw.dir, res.dir)
    assert np.nanmax(np.abs(tw.radius - res.radius)) <= 2e-9 * g.DX
    # no crossing: count 0, radii NaN, directions 0
    none = tile.crossings(R2, [1.0e6, -1.0], 1)
    assert (none.count == 0).all() and np.isnan(none.radius).all() and (none.dir == 0).all() and none.status[0] == 0
    assert tile.kernel_bytes("k_ray_profiles") == 0
    tile.close()


def test_more_crossings_than_kept():
    """count reports every crossing, the first max_cross are kept in outward order"""
    import scythe_jl_amd as S
    case = cases.r_bcs(bcl="R0", bcr="R0", num_cells=21)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    tile = S.Grid(gp, mp)
    r = S.getGridpoints(tile)
    tile.set_physical_values(np.cos(2.0 * np.pi * r / 2.4)[:, None])
    tile.spectralTransform_()
    tile.splineTransform_()
    prog = [(0, 1.0, 0, [(1, "")])]
    many = tile.crossings(prog, [0.1], 1, max_cross=16)
    n = int(many.count[0, 0])
    assert 8 <= n <= 16 and (np.diff(many.radius[:n, 0, 0]) > 0).all() and (many.dir[1:n, 0, 0] == -many.dir[:n - 1, 0, 0]).all()
    few = tile.crossings(prog, [0.1], 1, max_cross=3)
    assert few.count[0, 0] == n and few.radius[:, 0, 0].tobytes() == many.radius[:3, 0, 0].tobytes()
    assert few.dir[:, 0, 0].tobytes() == many.dir[:3, 0, 0].tobytes()
    _check_against_twin("r21 cos", g, gp, tile, prog, [0.1], 1, r, max_cross=16)
    tile.close()


def test_nan_coefficient():
    """a NaN in A: every ray's intervals over the cells of that node are NaN (NaN x any weight), status bit 0 is set, no crossing is
    reported there, and every crossing elsewhere comes back bitwise as before"""
    case, gp, g, tile, pts = _filled("rl12_L16")
    rays = _rays(g, 5, seed=5)
    prog = [(0, 1.0, 0, [(1, "")])]
    levels = [0.2, 0.55, 0.9]
    before = tile.crossings(prog, levels, rays, max_cross=4)
    assert (before.status == 0).all() and (before.count >= 1).any()
    A = tile.patchSpectral
    m = 6
    A[(0 * g.K2 + 0) * g.b_rDim + m, 0] = np.nan                           # z-mode 0, block 0, node m of variable 1
    tile.set_patch_spectral_a(A)
    after = tile.crossings(prog, levels, rays, max_cross=4)
    assert (after.status & 1).all()
    lo, hi = g.xmin + (m - 3) * g.DX, g.xmin + (m + 1) * g.DX              # the cells whose 4 nodes include m
    st = X.stations(g, _radii(pts))
    inner = st[np.searchsorted(st, lo, side="right") - 1]                   # stations bounding the NaN intervals
    outer = st[np.searchsorted(st, hi, side="left")]
    kept = 0
    for i in range(len(rays)):
        for j in range(len(levels)):
            b = before.radius[:, j, i]
            b = b[~np.isnan(b)]
            a = after.radius[:, j, i]
            a = a[~np.isnan(a)]
            assert not ((a > inner) & (a < outer)).any()
            want = b[(b <= inner) | (b >= outer)]
            assert a.tobytes() == want.tobytes(), (i, j, a, want)
            assert after.count[j, i] == len(want)
            kept += len(want)
    assert kept > 0
    # another variable's program does not read the NaN
    other = tile.crossings([(0, 1.0, 0, [(2, "")])], [0.3], rays)
    assert (other.status == 0).all()
    tile.close()


# ----------------------------------------------------------------------------- 9. state untouched
def _lsw_case():
    return LS.rl_case(num_cells=12, ring_L=16)


def test_state_untouched():
    case = _lsw_case()
    g = cases.oracle_grid(case)
    rays = _rays(g, 17, seed=2)
    prog = [(0, 1.0, 0, [("u", ""), ("u", "")]), (0, 1.0, 0, [("v", ""), ("v", "")]), (0, 0.1, 0, [("h", "l")])]
    ends = []
    for with_calls in (0, 1):
        hip = cases.HipModel(case)
        tile = hip.run.tiles[0]
        for s in range(6):
            hip.step()
            if with_calls:
                state0, np10, phys0 = tile.get_state(), tile.var_np1, tile.physical
                res = tile.crossings(prog, [0.005, 0.02], rays, return_profiles=True)
                assert tile.get_state().tobytes() == state0.tobytes() and tile.var_np1.tobytes() == np10.tobytes()
                assert tile.physical.tobytes() == phys0.tobytes()
        ends.append((tile.get_state(), tile.var_np1))
        hip.run.close()
    assert res.count.sum() > 0
    assert ends[0][0].tobytes() == ends[1][0].tobytes() and ends[0][1].tobytes() == ends[1][1].tobytes()


# ----------------------------------------------------------------------------- 10. refusals
def _raw(tile, coef, packed, n_rays, rays, levels, tol, max_cross, out, n_levels=None):
    from scythe_jl_amd import _lib as L
    packed = np.ascontiguousarray(packed, dtype=np.int32).reshape(-1, 11)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    rays = None if rays is None else np.asfortranarray(rays, dtype=np.float64)
    lev = np.ascontiguousarray(levels, dtype=np.float64)
    radius, dirs, count, status = out
    return tile._lib.sx_crossings(tile._h, len(coef), coef.ctypes.data_as(L.P_D), packed.ctypes.data_as(L.P_I32), n_rays,
                                  None if rays is None else rays.ctypes.data_as(L.P_D), len(lev) if n_levels is None else n_levels,
                                  lev.ctypes.data_as(L.P_D), tol, 0, max_cross, radius.ctypes.data_as(L.P_D), dirs.ctypes.data_as(L.P_I32),
                                  count.ctypes.data_as(L.P_I32), status.ctypes.data_as(L.P_I32), None)


def _sentinels():
    return (np.full(16 * 9 * 4, -7.25), np.full(16 * 9 * 4, -7, dtype=np.int32), np.full(9 * 4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32))


def _untouched(out):
    return (out[0] == -7.25).all() and all((o == -7).all() for o in out[1:])


def _term(out=0, p=0, factors=()):
    return [out, p, len(factors)] + [f[0] for f in factors] + [0] * (4 - len(factors)) + [f[1] for f in factors] + [0] * (4 - len(factors))


OK_TERM = _term(0, 0, [(1, 0)])
RAYS4 = np.array([0.0, 1.0, 2.0, 3.0])[:, None]
REFUSALS = {
    "n_out = 2": dict(coef=[1.0, 1.0], packed=[OK_TERM, _term(1, 0, [(1, 0)])]),
    "9 levels": dict(levels=np.linspace(0.1, 0.9, 9)),
    "max_cross = 0": dict(max_cross=0),
    "max_cross = 17": dict(max_cross=17),
    "a NaN ray": dict(rays=np.array([0.0, np.nan, 2.0, 3.0])[:, None]),
    "an Inf level": dict(levels=[0.5, np.inf]),
    "a NaN tol": dict(tol=np.nan),
    "p = -1 on a tile with r = 0": dict(packed=[_term(0, -1, [(1, 0)])]),
    "a slot the geometry lacks": dict(packed=[_term(0, 0, [(1, 5)])]),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(what):
    case, gp, g, tile = _make("rl12_L16")
    kw = dict(coef=[1.0], packed=[OK_TERM], rays=RAYS4, levels=[0.5], tol=0.0, max_cross=4)
    out = _sentinels()
    assert _raw(tile, kw["coef"], kw["packed"], 4, kw["rays"], kw["levels"], kw["tol"], kw["max_cross"], out) == 0 and not _untouched(out)
    kw.update(REFUSALS[what])
    out = _sentinels()
    assert _raw(tile, kw["coef"], kw["packed"], 4, kw["rays"], kw["levels"], kw["tol"], kw["max_cross"], out) != 0, what
    assert tile._lib.sx_last_error().decode() and _untouched(out), what
    tile.close()


def test_refusal_z_out_of_range_and_null():
    case, gp, g, tile = _make("rlz5x6_L8")
    rays = np.array([[0.0, 1.0], [1.0, 2.0], [2.0, 3.5], [3.0, 0.0]])                 # zmax = 3
    out = _sentinels()
    assert _raw(tile, [1.0], [OK_TERM], 4, rays, [0.5], 0.0, 4, out) != 0 and b"outside" in tile._lib.sx_last_error() and _untouched(out)
    assert _raw(tile, [1.0], [OK_TERM], 4, None, [0.5], 0.0, 4, out) != 0 and _untouched(out)      # null rays with n_rays > 0
    assert _raw(tile, [1.0], [OK_TERM], 0, None, [0.5], 0.0, 4, out) == 0 and _untouched(out)      # n_rays == 0: nothing written
    rays[2, 1] = 3.0
    assert _raw(tile, [1.0], [OK_TERM], 4, rays, [0.5], 0.0, 4, out) == 0 and not _untouched(out)
    tile.close()


def test_refusal_two_tile_handle():
    import scythe_jl_amd as S
    case = cases.rl_advection(num_cells=8, ring_L=16)
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp, tile_cell0=0, tile_num_cells=4, tile_num=0)
    out = _sentinels()
    assert _raw(tile, [1.0], [OK_TERM], 4, RAYS4, [0.5], 0.0, 4, out) != 0 and b"one-tile" in tile._lib.sx_last_error() and _untouched(out)
    tile.close()


# ----------------------------------------------------------------------------- 11. end to end: wind radii
def test_wind_radii_end_to_end():
    import scythe_jl_amd as S
    case = _lsw_case()
    xmax = case["grid"]["xmax"]
    vm, rm = 40.0, xmax / 6.0

    def ic(p):
        r, l = p[:, 0], p[:, 1]
        x = r / rm
        v = 2.0 * vm * x / (1.0 + x * x) * (1.0 + 0.2 * np.cos(l))
        return np.stack([0.0 * r, 0.0 * r, v], axis=1)
    case = dict(case, ic=ic)
    g = cases.oracle_grid(case)
    hip = cases.HipModel(case)
    tile = hip.run.tiles[0]
    thr = [20.0, 30.0]
    n = 16
    wr = hip.run.wind_radii("u", "v", thr, n_azimuths=n, quadrants=True)
    assert wr.radii.shape == (2, n) and wr.quadrants.shape == (2, 4) and not np.isnan(wr.radii).any()
    A = tile.patchSpectral
    pts = S.getGridpoints(tile)
    prog = S.pack_reduce_program(hip.gp, [(0, 1.0, 0, [("u", ""), ("u", "")]), (0, 1.0, 0, [("v", ""), ("v", "")])])
    lev = np.asarray(thr) ** 2
    tx = X.crossings(g, A, prog, lev, wr.azimuths[:, None], max_cross=16, xp=True, radii=_radii(pts))
    t64 = X.crossings(g, A, prog, lev, wr.azimuths[:, None], max_cross=16, xp=False, radii=_radii(pts))
    for j in range(2):
        want, w64 = X.select(tx, j, "outermost", falling=True), X.select(t64, j, "outermost", falling=True)
        err = np.abs(wr.radii[j] - want)
        bar = np.maximum(2.0e-9 * g.DX + 10.0 * np.abs(w64 - want), 8.0 * EPS * xmax)
        print("wind radii %g: %s\n  worst |r - twin| / bar %.3g" % (thr[j], np.array2string(wr.radii[j], precision=4), float((err / bar).max())))
        assert (err <= bar).all()
        assert np.array_equal(wr.quadrants[j], X.quadrant_max(wr.azimuths, wr.radii[j]))          # exactly the maxima of the rays
        exact = rm * (1.0 + np.sqrt(1.0 - (thr[j] / (vm * (1.0 + 0.2 * np.cos(wr.azimuths)))) ** 2)) / (thr[j] / (vm * (1.0 + 0.2 * np.cos(wr.azimuths))))
        print("  closed form of the analytic wind: worst |r - exact| %.3g DX (the spline is not the function: printed, not asserted)"
              % float(np.abs(wr.radii[j] - exact).max() / g.DX))
    assert (wr.quadrants[:, 0] > wr.quadrants[:, 2]).all()                  # NE beyond SW: the wave-1 factor
    # radius_where: the same crossings through the other entry
    rw = hip.run.radius_where(prog_terms(), lev[0], wr.azimuths, which="outermost")
    assert rw.tobytes() == wr.radii[0].tobytes()
    inner = hip.run.radius_where(prog_terms(), lev[0], wr.azimuths, which="innermost")
    assert (inner < rw).all()
    rad, dr, cnt = hip.run.radius_where(prog_terms(), lev[0], wr.azimuths, which="all")
    assert (cnt == 2).all() and (dr[0] == 1).all() and (dr[1] == -1).all() and rad[0].tobytes() == inner.tobytes()
    # an unreachable threshold: NaN everywhere, quadrants included
    none = hip.run.wind_radii("u", "v", [500.0], n_azimuths=8)
    assert np.isnan(none.radii).all() and np.isnan(none.quadrants).all()
    tile.enable_timers(True)
    tile.reset_timers()
    hip.run.wind_radii("u", "v", thr, n_azimuths=n)
    tm = tile.timers()
    assert tm["k_ray_profiles"][1] == 1 and tm["k_crossings"][1] == 1 and tm["k_ray_profiles"][0] > 0 and tm["k_crossings"][0] > 0
    assert tile.kernel_bytes("k_crossings") == 8.0 * g.b_rDim * 2 * n + 12.0 * 16 * 2 * n + 4.0 * 3 * n
    hip.run.close()


def prog_terms():
    return [(0, 1.0, 0, [("u", ""), ("u", "")]), (0, 1.0, 0, [("v", ""), ("v", "")])]
