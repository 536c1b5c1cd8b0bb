"""sx_isosurface on the GPU against the twin of tests/isosurface.py.

Profiles are held entry by entry to the longdouble twin within the derived rounding bound of tests/isosurface.py.  Crossings are
held to the longdouble twin: counts, directions and status equal, heights within 2 tol (zmax - zmin) + 10 |float64 twin - longdouble
twin| with a floor of 8 eps max(|zmin|, |zmax|), carried values within the derived series bound + |d/dz carried| x that bar.  Every
test prints its worst figures before it asserts; DESIGN.md 21, "Figures", holds those of one run on the card."""
import numpy as np
import pytest

from tests import cases
from tests import isosurface as I
from tests import test_isosurface as TI
from tests.test_gpu_crossings import _term

pytestmark = pytest.mark.gpu

XP = I.XP
EPS = 2.0 ** -52
GRIDS = {"rz5x8": ("rz_advection", dict(num_cells=5, zDim=8), {}),
         "rlz5x6_L8": ("rlz_advection", dict(num_cells=5, zDim=6, ring_L=8), {}),
         "rlz_bz15": ("rlz_advection", dict(num_cells=5, zDim=18, ring_L=8), dict(b_zDim=15)),       # the 16-row tiles of the z-modes
         "rlz_bz16": ("rlz_advection", dict(num_cells=5, zDim=18, ring_L=8), dict(b_zDim=16)),
         "rlz_bz17": ("rlz_advection", dict(num_cells=5, zDim=18, ring_L=8), dict(b_zDim=17)),
         "rz5x64": ("rz_advection", dict(num_cells=5, zDim=64), {}),                                  # one chunk of stations, and one more
         "rz5x65": ("rz_advection", dict(num_cells=5, zDim=65), {})}
COUNTS = (1, 15, 16, 17, 33)


def _case(name):
    maker, kw, over = GRIDS[name]
    case = getattr(cases, maker)(**kw)
    return dict(case, grid=dict(case["grid"], **over))


def _make(name):
    import scythe_jl_amd as S
    case = _case(name)
    gp, mp = cases.hip_params(case)
    return case, gp, cases.oracle_grid(case), S.Grid(gp, mp)


def _columns(g, n, seed=3, one_cell=None):
    """n seeded columns: r over the tile (or inside the cell `one_cell`), with the inner end, the outer end, a cell boundary and a
    duplicate among them; lambda in [-2 pi, 4 pi] (so below -2 pi .. above 2 pi are reduced on the host)"""
    rng = np.random.default_rng(seed)
    if one_cell is None:
        r = rng.uniform(g.xmin, g.xmax, n)
        special = [g.xmin, g.xmax, g.xmin + 2 * g.DX, r[min(4, n - 1)]]
        r[:min(n, 4)] = special[:min(n, 4)]
    else:
        r = g.xmin + g.DX * (one_cell + rng.uniform(0.0, 1.0, n))
    cols = [r]
    if g.has_l:
        lam = rng.uniform(-2.0 * np.pi, 4.0 * np.pi, n)
        lam[:3] = [0.0, -1.0, 7.0][:min(n, 3)]
        cols.append(lam if n < 4 or one_cell is not None else np.concatenate([lam[:3], lam[4:5], lam[4:]]))      # column 3 = column 4: a duplicate
    return np.stack(cols, axis=1)


def _heights(tile, g):
    import scythe_jl_amd as S
    return S.getGridpoints(tile)[:g.zDim, -1].copy()                        # z fastest: the levels of the first column, as printed


def _all_slot_program(g):
    """every slot of the geometry on variable 1, and a product of the last variable: every profile kind the geometry has"""
    names = [s if s != "u" else "" for s in g.slots]
    return [(0, 1.0 + 0.25 * i, 0, [(1, s)]) for i, s in enumerate(names)] + [(0, -0.5, 0, [(g.V, ""), (g.V, "r")])]


def _same(a, b, i, k):
    """column i of result a is bitwise column k of result b"""
    ok = a.height[:, :, i].tobytes() == b.height[:, :, k].tobytes() and a.dir[:, :, i].tobytes() == b.dir[:, :, k].tobytes()
    ok = ok and (a.count[:, i] == b.count[:, k]).all() and a.status[i] == b.status[k]
    for x, y in ((a.carry, b.carry), (a.values, b.values), (a.profiles, b.profiles)):
        if x is not None and y is not None:
            ok = ok and x[..., i].tobytes() == y[..., k].tobytes()
    return bool(ok)


# ----------------------------------------------------------------------------- profiles, entry by entry
@pytest.mark.parametrize("name", ["rz5x8", "rlz5x6_L8", "rlz_bz15", "rlz_bz16", "rlz_bz17"])
def test_profiles(name):
    import scythe_jl_amd as S
    case, gp, g, tile = _make(name)
    rng = np.random.default_rng(11)
    A = rng.standard_normal((g.S_patch(), g.V))
    tile.set_patch_spectral_a(A)
    prog = _all_slot_program(g)
    pl = I.plan(g, S.pack_reduce_program(gp, prog)[1])
    cols = _columns(g, 33)
    q = I.reduce_columns(g, cols)
    Cx, C64 = I.profiles(g, A, pl, q, xp=True), I.profiles(g, A, pl, q, xp=False)
    bound = I.profile_bound(g, A, pl, q)
    res = tile.isosurface(prog, [0.0], cols, return_profiles=True)
    assert res.profiles.shape == (g.b_zDim, len(pl.keys), 33) and S.isosurface_check(gp, prog) == len(pl.keys)
    err = np.abs(res.profiles.astype(XP) - Cx)
    e64 = np.abs(C64.astype(XP) - Cx)
    scale = np.abs(Cx).max(axis=(0, 2))
    print("%s: profile error / largest entry, worst: device %.3g, float64 twin %.3g, bound %.3g; worst error / bound %.3g"
          % (name, float((err.max(axis=(0, 2)) / scale).max()), float((e64.max(axis=(0, 2)) / scale).max()),
             float((bound.max(axis=(0, 2)) / scale).max()), float((err / bound).max())))
    assert (err <= bound).all()
    nv, live = 2, (2 * g.kDim + 1 if g.has_l else 1)
    cells = np.clip(np.floor((cols[:, 0] - g.xmin) / g.DX).astype(int), 0, g.nc - 1)
    units = sum(-(-int((cells == c).sum()) // 16) for c in range(g.nc)) * nv if g.has_l else 33 * len(pl.keys)
    assert tile.kernel_bytes("k_column_profiles") == 8.0 * (4.0 * g.b_zDim * live * units + q.shape[1] * 33 + g.b_zDim * len(pl.keys) * 33)
    tile.close()


# ----------------------------------------------------------------------------- smooth fields for the crossings
def _field(g, pts):
    """rises with height through most of (0.3, 1.1), with a radial trend and waves 1 and 2; every variable another amplitude"""
    r, z = pts[:, 0], pts[:, -1]
    s, zz = (r - g.xmin) / (g.xmax - g.xmin), (z - g.zmin) / (g.zmax - g.zmin)
    f = 0.3 + 0.6 * zz + 0.05 * np.sin(2.0 * np.pi * zz) + 0.1 * s
    if g.has_l:
        l = pts[:, 1]
        f = f * (1.0 + 0.2 * s * np.cos(l - 0.3) + 0.15 * s * s * np.sin(2.0 * l + 0.2))
    return np.stack([f * (1.0 + 0.5 * v) for v in range(g.V)], axis=1)


def _filled(name, field=_field):
    import scythe_jl_amd as S
    case, gp, g, tile = _make(name)
    pts = S.getGridpoints(tile)
    tile.set_physical_values(field(g, pts))
    tile.spectralTransform_()
    tile.splineTransform_()
    return case, gp, g, tile


PROG = [(0, 1.0, 0, [(1, ""), (1, "")]), (0, 0.3, 0, [(1, "")]), (1, 1.0, 0, [(2, "z")]), (2, 1.0, 0, [(1, "r")])]      # f^2 + 0.3 f; carried: d/dz of variable 2, d/dr of variable 1
LEVELS = [0.3, 0.6, 0.9]


def _carry_bound(g, A, pl, q, packed, out):
    """the derived bound of carried output `out` (one term, one factor: coef x a plane) at any height, per column: the series bound
    with the coefficient errors that the profile's rounding bound, CA C and the Dc applications leave; and the plane's series in
    longdouble for its z derivative"""
    t = [k for k in range(len(packed[0])) if packed[1][k, 0] == out]
    assert len(t) == 1 and packed[1][t[0], 2] == 1
    coef = abs(float(packed[0][t[0]]))
    j = pl.planes.index((int(packed[1][t[0], 3]), int(packed[1][t[0], 7])))
    CA, Dc = I.operators(g, g.names[pl.planes[j][0] - 1], xp=False)
    C64, dC = np.abs(I.profiles(g, A, pl, q, xp=False)[:, pl.pprof[j], :]), I.profile_bound(g, A, pl, q)[:, pl.pprof[j], :]
    out_b = np.zeros(len(q))
    for i in range(len(q)):
        a_abs = np.abs(CA) @ (C64[:, i] + dC[:, i])
        da = np.abs(CA) @ dC[:, i] + I.EPS * (g.b_zDim + 2.0) * (np.abs(CA) @ C64[:, i])
        for _ in range(pl.pz[j]):
            a_abs, da = I.coeff_bound(np.abs(Dc), a_abs, da)
        out_b[i] = coef * I.series_bound(g.zmin, g.zmax, a_abs, da)
    return out_b, j


def _check_carried(name, g, A, packed, cols, carry, tx, ok, bar):
    """carried outputs (each one term, one factor): within the series bound + |d/dz carried| x the bar of the height"""
    pl = I.plan(g, packed[1])
    q = I.reduce_columns(g, cols)
    Cx = I.profiles(g, A, pl, q, xp=True)
    for o in range(1, carry.shape[0] + 1):
        bnd, j = _carry_bound(g, A, pl, q, packed, o)
        CAx, Dcx = I.operators(g, g.names[pl.planes[j][0] - 1], xp=True)
        worst = 0.0
        for i in range(len(q)):
            a = CAx @ Cx[:, pl.pprof[j], i]
            for _ in range(pl.pz[j] + 1):
                a = Dcx @ a                                                 # the z derivative of the carried plane
            for k, lev in zip(*np.nonzero(ok[:, :, i])):
                slope = abs(float(packed[0][[t for t in range(len(packed[0])) if packed[1][t, 0] == o][0]])) * abs(float(I.series(g.zmin, g.zmax, a, tx.height[k, lev, i], xp=True)))
                lim = bnd[i] + slope * bar[k, lev, i]
                e = abs(float(XP(carry[o - 1, k, lev, i]) - tx.carry[o - 1, k, lev, i]))
                worst = max(worst, e / lim)
                assert e <= lim, (name, o, i, lev, k, e, lim)
        print("  %s carried output %d: worst error / (series bound + slope x bar) %.3g" % (name, o, worst))


@pytest.mark.parametrize("name", ["rz5x8", "rlz5x6_L8", "rz5x64", "rz5x65"])
def test_crossings_against_twin(name):
    import scythe_jl_amd as S
    case, gp, g, tile = _filled(name)
    cols = _columns(g, 6, seed=5)
    packed = S.pack_reduce_program(gp, PROG)
    A, hts = tile.patchSpectral, _heights(tile, g)
    tx = I.isosurface(g, A, packed, LEVELS, cols, n_carry=2, max_cross=4, xp=True, heights=hts)
    t64 = I.isosurface(g, A, packed, LEVELS, cols, n_carry=2, max_cross=4, xp=False, heights=hts)
    res = tile.isosurface(PROG, LEVELS, cols, carry=2, max_cross=4, return_values=True)
    assert np.array_equal(res.count, tx.count) and np.array_equal(res.dir, tx.dir) and np.array_equal(res.status, tx.status), (res.count, tx.count)
    assert np.array_equal(np.isnan(res.height), np.isnan(tx.height)) and np.array_equal(np.isnan(res.carry), np.isnan(tx.carry.astype(np.float64)))
    ok = ~np.isnan(tx.height)
    assert ok.sum() >= 6
    with np.errstate(invalid="ignore"):
        err = np.abs(res.height - tx.height)
        bar = np.maximum(2.0e-9 * (g.zmax - g.zmin) + 10.0 * np.abs(t64.height - tx.height), 8.0 * EPS * max(abs(g.zmin), abs(g.zmax)))
    print("%s: %d crossings, worst |z - twin| %.3g (zmax - zmin), worst error / bar %.3g"
          % (name, int(ok.sum()), float(err[ok].max() / (g.zmax - g.zmin)), float((err[ok] / bar[ok]).max())))
    assert (err[ok] <= bar[ok]).all()
    # the station values as the kernel formed them: within 10 x the float64 twin's error, with a floor for the recurrence's growth
    # (4.5 n^2 u per coefficient, tests/isosurface.py) through the program (|dg / df| <= 2.5) and the coefficients' sum: 64 zDim^2 u max |g|
    verr = np.abs(res.values.astype(XP) - tx.values)
    vbar = 10.0 * np.abs(t64.values.astype(XP) - tx.values) + 64.0 * g.zDim ** 2 * I.EPS * np.abs(tx.values).max()
    assert (verr <= vbar).all()
    _check_carried(name, g, A, packed, cols, res.carry, tx, ok, bar)
    tile.close()


# ----------------------------------------------------------------------------- batch edges, order, independence: bitwise
@pytest.mark.parametrize("name", ["rz5x8", "rlz5x6_L8"])
def test_batch_edges(name):
    case, gp, g, tile = _filled(name)
    kw = dict(carry=2, max_cross=4, return_values=True, return_profiles=True)
    cols = _columns(g, 33, seed=9, one_cell=2)                              # 33 columns of ONE radial cell: batches of 16, 16, 1
    full = tile.isosurface(PROG, LEVELS, cols, **kw)
    assert (full.count >= 1).any()
    for n in COUNTS[:-1]:
        part = tile.isosurface(PROG, LEVELS, cols[:n], **kw)
        assert all(_same(part, full, i, i) for i in range(n)), (name, n)
    spread = _columns(g, 33, seed=9)                                        # every cell, both ends, a cell boundary, a duplicate
    fwd, rev = tile.isosurface(PROG, LEVELS, spread, **kw), tile.isosurface(PROG, LEVELS, spread[::-1], **kw)
    assert all(_same(rev, fwd, 32 - i, i) for i in range(33))
    assert _same(fwd, fwd, 3, 4) and (fwd.status == 0).all()                # the duplicate
    mixed = tile.isosurface(PROG, LEVELS, np.concatenate([spread[:5], cols[:20], spread[5:]]), **kw)     # other batch neighbours
    assert all(_same(mixed, fwd, i, i) for i in range(5)) and all(_same(mixed, full, 5 + i, i) for i in range(20))
    tile.close()


@pytest.mark.parametrize("name", ["rz5x8", "rlz5x6_L8"])
def test_independence(name):
    case, gp, g, tile = _filled(name)
    cols = _columns(g, 33, seed=9)
    full = tile.isosurface(PROG, LEVELS, cols, carry=2, return_values=True, return_profiles=True)
    assert (full.count >= 1).any()
    for i in (0, 7, 16, 32):
        one = tile.isosurface(PROG, LEVELS, cols[[i]], carry=2)             # alone, and without values / profiles
        assert _same(one, full, 0, i) and one.values is None and one.profiles is None
    for j, c in enumerate(LEVELS):
        one = tile.isosurface(PROG, [c], cols, carry=2)
        assert one.height[:, 0, :].tobytes() == full.height[:, j, :].tobytes() and one.dir[:, 0, :].tobytes() == full.dir[:, j, :].tobytes()
        assert (one.count[0] == full.count[j]).all() and one.carry[:, :, 0, :].tobytes() == full.carry[:, :, j, :].tobytes()
    bare = tile.isosurface(PROG[:2], LEVELS, cols, carry=0, return_values=True)      # n_carry = 0: the surface itself has the same bits
    assert bare.carry is None and bare.height.tobytes() == full.height.tobytes() and bare.dir.tobytes() == full.dir.tobytes()
    assert bare.values.tobytes() == full.values.tobytes() and (bare.count == full.count).all() and (bare.status == full.status).all()
    tile.close()


# ----------------------------------------------------------------------------- shape edges of the scan
@pytest.mark.parametrize("name", ["rlz5x6_L8", "rz5x65"])
def test_root_exactly_on_a_station(name):
    """the value the kernel formed at station k, passed back as the level: d is exactly 0 there, the sign rule counts the root once
    in the two intervals around it, and the height is bitwise the station"""
    case, gp, g, tile = _filled(name)
    cols = _columns(g, 5, seed=5)
    hts = _heights(tile, g)
    vals = tile.isosurface(PROG[:2], [0.0], cols, return_values=True).values
    for k in sorted({1, g.zDim // 2, g.zDim - 2, g.zDim - 1} | ({63, 64} if g.zDim > 64 else set())):      # 63 | 64: across the lane chunks
        for c in range(len(cols)):
            res = tile.isosurface(PROG[:2], [vals[k, c]], cols[[c]], max_cross=16)
            kept = res.height[:, 0, 0][~np.isnan(res.height[:, 0, 0])]
            near = kept[(kept >= hts[k - 1]) & (kept <= hts[min(k + 1, g.zDim - 1)])]
            assert res.status[0] == 0 and len(near) == 1 and near[0].tobytes() == hts[k].tobytes(), (name, k, c, near, hts[k])
    tile.close()


def test_field_equal_to_the_level_and_no_crossing():
    case, gp, g, tile = _filled("rz5x8")
    cols = _columns(g, 5, seed=5)
    const = [(0, 2.5, 0, [])]                                               # no plane: identically 2.5
    res = tile.isosurface(const, [2.5, 7.0], cols, max_cross=3)
    assert (res.count == 0).all() and (res.status == 0).all() and np.isnan(res.height).all() and (res.dir == 0).all()
    assert tile.kernel_bytes("k_column_profiles") == 0
    tile.close()


def test_more_crossings_than_kept():
    """count reports every crossing, the first max_cross are kept upward"""
    wave = lambda g, pts: np.stack([np.cos(5.0 * np.pi * (pts[:, -1] - g.zmin) / (g.zmax - g.zmin)) * (1.0 + 0.1 * v) for v in range(g.V)], axis=1)
    case, gp, g, tile = _filled("rz5x64", wave)
    cols = _columns(g, 3, seed=5)
    prog = [(0, 1.0, 0, [(1, "")]), (1, 1.0, 0, [(1, "z")])]
    many = tile.isosurface(prog, [0.1], cols, carry=1, max_cross=16)
    assert (many.count[0] == 5).all() and (np.diff(many.height[:5, 0, :], axis=0) > 0).all() and (many.dir[:5, 0, 0] == [-1, 1, -1, 1, -1]).all()
    assert (np.sign(many.carry[0, :5, 0, :]) == many.dir[:5, 0, :]).all()   # d/dz has the sign of the direction
    few = tile.isosurface(prog, [0.1], cols, carry=1, max_cross=2)
    assert (few.count[0] == 5).all() and few.height.tobytes() == np.asfortranarray(many.height[:2]).tobytes()
    assert few.carry.tobytes() == np.asfortranarray(many.carry[:, :2]).tobytes() and few.dir.tobytes() == np.asfortranarray(many.dir[:2]).tobytes()
    tile.close()


def test_nan_coefficient():
    """a NaN in A: the columns whose four node rows hold it have NaN station values (NaN x any weight), status bit 0 and no crossing;
    every other column comes back bitwise as before"""
    case, gp, g, tile = _filled("rlz5x6_L8")
    cols = _columns(g, 17, seed=7)
    before = tile.isosurface(PROG, LEVELS, cols, carry=2, return_values=True)
    assert (before.status == 0).all() and (before.count >= 1).any()
    A = tile.patchSpectral
    m = 4
    A[(0 * g.K2 + 0) * g.b_rDim + m, 0] = np.nan                            # z-mode 0, block 0, node m of variable 1
    tile.set_patch_spectral_a(A)
    after = tile.isosurface(PROG, LEVELS, cols, carry=2, return_values=True)
    cells = np.clip(np.floor((cols[:, 0] - g.xmin) / g.DX).astype(int), 0, g.nc - 1)
    hit = (cells <= m) & (m <= cells + 3)
    assert hit.any() and (~hit).any()
    assert ((after.status[hit] & 1) == 1).all() and (after.count[:, hit] == 0).all() and np.isnan(after.values[:, hit]).all()
    assert all(_same(after, before, i, i) for i in np.nonzero(~hit)[0])
    tile.close()


# ----------------------------------------------------------------------------- state untouched
def test_state_untouched():
    case = _case("rlz5x6_L8")
    g = cases.oracle_grid(case)
    cols = _columns(g, 17, seed=2)
    prog = [(0, 1.0, 0, [("h", "")]), (1, 1.0, 0, [("u", "z")]), (2, 1.0, 0, [("v", "r")])]
    ends = []
    for with_calls in (0, 1):
        hip = cases.HipModel(case)
        tile = hip.run.tiles[0]
        for s in range(5):
            hip.step()
            if with_calls:
                state0, np10, phys0, A0 = tile.get_state(), tile.var_np1, tile.physical, tile.patchSpectral
                res = tile.isosurface(prog, [0.05, 0.2], cols, carry=2, return_values=True, return_profiles=True)
                assert tile.get_state().tobytes() == state0.tobytes() and tile.var_np1.tobytes() == np10.tobytes()
                assert tile.physical.tobytes() == phys0.tobytes() and tile.patchSpectral.tobytes() == A0.tobytes()
        ends.append((tile.get_state(), tile.var_np1))
        hip.run.close()
    assert res.status.shape == (17,)
    assert ends[0][0].tobytes() == ends[1][0].tobytes() and ends[0][1].tobytes() == ends[1][1].tobytes()


# ----------------------------------------------------------------------------- refusals
def _raw(tile, coef, packed, n_carry, n_cols, cols, levels, tol, max_cross, out, carry="auto"):
    from scythe_jl_amd import _lib as L
    packed = np.ascontiguousarray(packed, dtype=np.int32).reshape(-1, 11)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    cols = None if cols is None else np.asfortranarray(cols, dtype=np.float64)
    lev = np.ascontiguousarray(levels, dtype=np.float64)
    height, dirs, count, status, car = out
    pc = (car.ctypes.data_as(L.P_D) if n_carry > 0 else None) if carry == "auto" else carry
    return tile._lib.sx_isosurface(tile._h, len(coef), coef.ctypes.data_as(L.P_D), packed.ctypes.data_as(L.P_I32), n_carry, n_cols,
                                   None if cols is None else cols.ctypes.data_as(L.P_D), len(lev), lev.ctypes.data_as(L.P_D), tol, 0, max_cross,
                                   height.ctypes.data_as(L.P_D), dirs.ctypes.data_as(L.P_I32), count.ctypes.data_as(L.P_I32),
                                   status.ctypes.data_as(L.P_I32), pc, None, None)


def _sentinels():
    return (np.full(16 * 9 * 4, -7.25), np.full(16 * 9 * 4, -7, dtype=np.int32), np.full(9 * 4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32),
            np.full(9 * 16 * 9 * 4, -7.25))


def _untouched(out):
    return (out[0] == -7.25).all() and (out[4] == -7.25).all() and all((o == -7).all() for o in out[1:4])


OK_TERM = _term(0, 0, [(1, 0)])
COLS4 = np.array([[1.0, 0.0], [3.0, 1.0], [0.0, 2.0], [10.0, 3.0]])          # rlz_advection: r in [0, 10]
REFUSALS = {
    "a term whose out is above n_carry": dict(coef=[1.0, 1.0], packed=[OK_TERM, _term(1, 0, [(1, 0)])]),
    "n_carry = 9": dict(n_carry=9),
    "n_carry = -1": dict(n_carry=-1),
    "9 levels": dict(levels=np.linspace(0.1, 0.9, 9)),
    "no level": dict(levels=[]),
    "max_cross = 0": dict(max_cross=0),
    "max_cross = 17": dict(max_cross=17),
    "a NaN lambda": dict(cols=np.array([[1.0, 0.0], [3.0, np.nan], [0.0, 2.0], [10.0, 3.0]])),
    "an Inf r": dict(cols=np.array([[1.0, 0.0], [np.inf, 1.0], [0.0, 2.0], [10.0, 3.0]])),
    "an r beyond the outer end": dict(cols=np.array([[1.0, 0.0], [10.5, 1.0], [0.0, 2.0], [10.0, 3.0]])),
    "an r below the inner end": dict(cols=np.array([[1.0, 0.0], [-0.5, 1.0], [0.0, 2.0], [10.0, 3.0]])),
    "an Inf level": dict(levels=[0.5, np.inf]),
    "a NaN tol": dict(tol=np.nan),
    "p = -1 with a column at r = 0": dict(packed=[_term(0, -1, [(1, 0)])]),
    "a slot the geometry lacks": dict(packed=[_term(0, 0, [(1, 7)])]),
    "null columns": dict(cols=None),
    "null carry with n_carry = 1": dict(coef=[1.0, 1.0], packed=[OK_TERM, _term(1, 0, [(1, 0)])], n_carry=1, carry=None),
    "more than 2^20 columns": dict(n_cols=(1 << 20) + 1),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(what):
    case, gp, g, tile = _make("rlz5x6_L8")
    kw = dict(coef=[1.0], packed=[OK_TERM], n_carry=0, n_cols=4, cols=COLS4, levels=[0.5], tol=0.0, max_cross=4, carry="auto")
    out = _sentinels()
    assert _raw(tile, out=out, **kw) == 0 and not _untouched(out)
    kw.update(REFUSALS[what])
    out = _sentinels()
    assert _raw(tile, out=out, **kw) != 0, what
    assert tile._lib.sx_last_error().decode() and _untouched(out), what
    if what == "p = -1 with a column at r = 0":                             # without that column the program is accepted
        kw["cols"] = COLS4[[0, 1, 3, 3]]
        assert _raw(tile, out=out, **kw) == 0 and not _untouched(out)
    tile.close()


def test_refusals_of_the_handle():
    import scythe_jl_amd as S
    out = _sentinels()
    case = cases.rl_advection(num_cells=8, ring_L=16)                       # no vertical
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp)
    assert _raw(tile, [1.0], [OK_TERM], 0, 4, COLS4[:, :1], [0.5], 0.0, 4, out) != 0 and b"no vertical" in tile._lib.sx_last_error() and _untouched(out)
    tile.close()
    case = _case("rlz5x6_L8")                                               # a two-tile handle
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp, tile_cell0=0, tile_num_cells=3, tile_num=0)
    cols = np.array([[1.0, 0.0], [3.0, 1.0], [0.0, 2.0], [5.0, 3.0]])
    assert _raw(tile, [1.0], [OK_TERM], 0, 4, cols, [0.5], 0.0, 4, out) != 0 and b"one-tile" in tile._lib.sx_last_error() and _untouched(out)
    tile.close()
    case, gp, g, tile = _make("rlz5x6_L8")
    assert _raw(tile, [1.0], [OK_TERM], 0, 0, None, [0.5], 0.0, 4, out) == 0 and _untouched(out)      # n_cols == 0: nothing written
    tile.close()


# ----------------------------------------------------------------------------- end to end
def test_on_surface_end_to_end():
    """the closed form of tests/test_isosurface.py through ModelRun.on_surface on an RLZ model handle: against the longdouble twin
    on the handle's own A (the bar of the module docstring) and against the formula (the spline's error: DESIGN.md 21 holds the
    10-cell figure of the twin, 1.5e-4; 1e-3 is asserted)"""
    import scythe_jl_amd as S
    base = cases.rlz_advection(num_cells=10, zDim=8, ring_L=16)

    def ic(p):
        f = TI.GAMMA * p[:, 2] + TI._b(p[:, 0]) * (1.0 + TI.EPS2 * np.cos(2.0 * p[:, 1]))
        return np.stack([f, 0.3 + 0.0 * f, 0.2 * p[:, 0]], axis=1)
    case = dict(base, ic=ic, grid={k: v for k, v in base["grid"].items() if k != "BCB"})
    g = cases.oracle_grid(case)
    hip = cases.HipModel(case)
    tile = hip.run.tiles[0]
    cols = TI.closed_form_columns()
    surf = [(0, 1.0, 0, [("h", "")])]
    hgt, vals = hip.run.on_surface(surf, TI.LEVEL, ["v", [(0, 1.0, 0, [("h", "z")])]], cols)
    assert hgt.shape == (24,) and vals.shape == (2, 24) and not np.isnan(hgt).any()
    prog = S.pack_reduce_program(hip.gp, surf + [(1, 1.0, 0, [("v", "")]), (2, 1.0, 0, [("h", "z")])])
    A, hts = tile.patchSpectral, _heights(tile, g)
    tx = I.isosurface(g, A, prog, [TI.LEVEL], cols, n_carry=2, max_cross=16, xp=True, heights=hts)
    t64 = I.isosurface(g, A, prog, [TI.LEVEL], cols, n_carry=2, max_cross=16, xp=False, heights=hts)
    want, w64 = I.select(tx, 0, "lowest"), I.select(t64, 0, "lowest")
    bar = np.maximum(2.0e-9 * (g.zmax - g.zmin) + 10.0 * np.abs(w64 - want), 8.0 * EPS * g.zmax)
    exact = TI.closed_form_height(cols)
    print("on_surface: worst |z - twin| / bar %.3g; worst |z - formula| %.3e; carried v: worst |v - 0.2 r| %.3e, h_z: worst |h_z - Gamma| %.3e"
          % (float((np.abs(hgt - want) / bar).max()), float(np.abs(hgt - exact).max()), float(np.abs(vals[0] - 0.2 * cols[:, 0]).max()),
             float(np.abs(vals[1] - TI.GAMMA).max())))
    assert (np.abs(hgt - want) <= bar).all() and np.abs(hgt - exact).max() < 1.0e-3
    res = tile.isosurface(surf + [(1, 1.0, 0, [("v", "")]), (2, 1.0, 0, [("h", "z")])], [TI.LEVEL], cols, carry=2, max_cross=16)
    assert (res.count == 1).all() and vals.tobytes() == np.ascontiguousarray(res.carry[:, 0, 0, :]).tobytes() and hgt.tobytes() == res.height[0, 0].tobytes()
    with np.errstate(invalid="ignore"):
        bar3 = np.maximum(2.0e-9 * (g.zmax - g.zmin) + 10.0 * np.abs(t64.height - tx.height), 8.0 * EPS * g.zmax)
    _check_carried("on_surface", g, A, prog, cols, res.carry, tx, ~np.isnan(tx.height), bar3)
    # height_where: the same surface through the other entry; nothing falls through the level
    hw = hip.run.height_where(surf, TI.LEVEL, cols, which="highest", rising=True)
    assert hw.tobytes() == hgt.tobytes() and np.isnan(hip.run.height_where(surf, TI.LEVEL, cols, rising=False)).all()
    assert np.isnan(hip.run.height_where(surf, 500.0, cols)).all()          # an unreachable level
    tile.enable_timers(True)
    tile.reset_timers()
    hip.run.on_surface(surf, TI.LEVEL, ["v"], cols)
    tm = tile.timers()
    assert tm["k_column_profiles"][1] == 1 and tm["k_isosurface"][1] == 1 and tm["k_column_profiles"][0] > 0 and tm["k_isosurface"][0] > 0
    n = 24
    assert tile.kernel_bytes("k_isosurface") == 8.0 * g.b_zDim * 2 * n + (12.0 + 8.0) * 16 * n + 4.0 * 2 * n + 8.0 * g.zDim * n
    hip.run.close()
