"""sx_distribution on the GPU against the twin of tests/distribution.py.

Counts are held to the twin EXACTLY (the binned quantity is plain fp64 on both sides); every sum is held to its longdouble
counterpart within tests/reduce.py::BOUND applied to the slot's S_abs - the roundings of a slot's sum are sx_reduce's, derived there.
Shapes are those of tests/test_gpu_reduce.py: the smallest with every index path."""
import ctypes as C

import numpy as np
import pytest

from tests import cases
from tests import distribution as D
from tests import reduce as R

pytestmark = pytest.mark.gpu

XP = D.XP
GEOMS = [("R", None), ("RZ", None), ("RL", None), ("RL", 16), ("RLZ", None), ("RLZ", 16)]


def _case(geom, ring_L=None):
    if geom == "R":
        return cases.r_bcs(num_cells=12)
    if geom == "RZ":
        return cases.rz_advection(num_cells=9, zDim=12)
    if geom == "RL":
        return cases.rl_slab(num_cells=9, ring_L=ring_L)
    return cases.rlz_hrbl(num_cells=9, zDim=10, ring_L=ring_L)


def _points(tile):
    import scythe_jl_amd as S
    pts = S.getGridpoints(tile)
    return pts.reshape(len(pts), -1)


def _quantile_edges(q, n_bins):
    """edges ON evenly spread sorted distinct values of q, the smallest excluded (a program of r alone takes one value per ring, and
    neighbours may be one ulp apart): underflow holds the smallest value, every bin its own lower edge, overflow the last edge"""
    d = np.unique(q[np.isfinite(q)])
    assert len(d) >= n_bins + 2
    e = d[np.round(np.linspace(1, len(d) - 1, n_bins + 1)).astype(int)]
    assert len(np.unique(e)) == n_bins + 1 and d[0] < e[0]
    return e


def _held(tile, g, data, pts, gp, prog, edges, kind, source, c0, n, what, populated=True):
    """one call against the twin: counts exact, sums within the bound, a second call the same bytes"""
    import scythe_jl_amd as S
    packed = S.pack_reduce_program(gp, prog)
    got = tile.distribution(prog, edges, kind, source)
    count, sums, sabs, _ = D.distribution(g, data, pts, packed, edges, kind, c0, n)
    assert got.count.shape == count.shape and got.count.dtype == np.int64 and got.sums.shape == sums.shape
    assert np.array_equal(got.count, count), what
    if populated:
        tot = count.sum(axis=1)
        assert tot[0] > 0 and tot[-2] > 0 and (tot[1:-2] > 0).sum() >= (len(edges) - 1 + 1) // 2, (what, tot)
    D.check(got.sums, sums, sabs, what)
    assert np.array_equal(got.measure, got.sums[:, 0, :])
    empty = count == 0
    assert (got.sums[empty[:, None, :].repeat(sums.shape[1], axis=1)] == 0).all() and not np.signbit(got.sums[empty[:, None, :].repeat(sums.shape[1], axis=1)]).any()
    again = tile.distribution(prog, edges, kind, source)
    assert again.count.tobytes() == got.count.tobytes() and again.sums.tobytes() == got.sums.tobytes(), what
    return got, count, sums, sabs


@pytest.mark.parametrize("tiles", [1, 3])
@pytest.mark.parametrize("geom,ring_L", GEOMS)
def test_against_twin(geom, ring_L, tiles):
    import scythe_jl_amd as S
    case = _case(geom, ring_L)
    hip = cases.HipModel(case, num_tiles=tiles, exchange="gather", impl="lib" if tiles > 1 else "torch")
    for _ in range(3):
        hip.step()
    g = cases.oracle_grid(case)
    for t, tile in zip(hip.run.tile_ids, hip.run.tiles):
        c0, n = hip.run.layout.cell0[t], hip.run.layout.ncells[t]
        pts = _points(tile)
        tile.tileTransform_()
        phys, np1 = tile.physical, tile.var_np1
        for n_int in (1, 3):
            for source, data in (("physical", phys), ("state", np1)):
                prog = R.random_program(g, 11 + n_int, n_out=n_int + 1, source=source)
                q = D.program_values64(data, pts[:, 0], S.pack_reduce_program(hip.gp, prog))
                edges = _quantile_edges(q, 5)
                for kind in ("domain", "level"):
                    _held(tile, g, data, pts, hip.gp, prog, edges, kind, source, c0, n,
                          "%s ring_L=%s tiles=%d tile %d %s %s %d integrands" % (geom, ring_L, tiles, t, kind, source, n_int))
    hip.run.close()


def _tile(geom, ring_L=None, storage="f64", **kw):
    import scythe_jl_amd as S
    case = _case(geom, ring_L) if not kw else getattr(cases, kw.pop("maker"))(**kw)
    gp, mp = cases.hip_params(case, storage)
    g = cases.oracle_grid(case)
    tile = S.Grid(gp, mp)
    return case, gp, g, tile, _points(tile)


@pytest.mark.parametrize("geom,ring_L", [("RL", None), ("RLZ", 16), ("RZ", None)])
def test_edge_exactness(geom, ring_L):
    """values exactly on edges and one ulp below, -0.0 against an edge of 0.0, +-inf, and one NaN at a known point"""
    case, gp, g, tile, pts = _tile(geom, ring_L)
    edges = np.array([-1.0, 0.0, 0.5, 2.0])
    pool = np.concatenate([edges, np.nextafter(edges, -np.inf), [-0.0, np.inf, -np.inf, 0.25, 1.0, 3.0, -2.0]])
    rng = np.random.default_rng(23)
    vals = rng.standard_normal((tile.N, g.V))
    vals[:, 0] = pool[rng.integers(0, len(pool), tile.N)]
    vals[:len(pool), 0] = pool                                       # every special value at least once
    P = tile.N // 2 + 3
    prog = [(0, 1.0, 0, [(1, 0)]), (1, 1.0, 0, [(2, 0)])]
    res = {}
    for name, at_p in (("nan", np.nan), ("over", np.inf), ("under", -np.inf)):
        vals[P, 0] = at_p
        tile.set_physical_values(vals)
        for kind in ("domain", "level"):
            got, count, _, _ = _held(tile, g, vals, pts, gp, prog, edges, kind, "state", 0, g.nc, "%s edges %s %s" % (geom, name, kind), populated=False)
            assert (count.sum(axis=1)[:-1] > 0).all()
            assert got.count[-1].sum() == (1 if name == "nan" else 0)
            res[name, kind] = got
    nz = g.zDim
    for kind in ("domain", "level"):
        a, over, under = res["nan", kind], res["over", kind], res["under", kind]
        assert a.count[-1, P % nz if kind == "level" else 0] == 1
        # every slot but the NaN slot is bitwise what it is when the point's contribution lies elsewhere: in the overflow slot (all
        # but that one compared) and in the underflow slot (all but that one)
        assert a.sums[:-2].tobytes() == over.sums[:-2].tobytes() and a.count[:-2].tobytes() == over.count[:-2].tobytes()
        assert a.sums[1:-1].tobytes() == under.sums[1:-1].tobytes() and a.count[1:-1].tobytes() == under.count[1:-1].tobytes()
    tile.close()


@pytest.mark.parametrize("n_bins", [1, 5, 64])
@pytest.mark.parametrize("geom,ring_L", [("RL", None), ("RLZ", 16)])
def test_bin_loop_extremes(geom, ring_L, n_bins):
    """a constant field: every lane in one slot; consecutive points in different bins across all of them: as many distinct slots per
    wave as there are"""
    case, gp, g, tile, pts = _tile(geom, ring_L)
    edges = np.arange(n_bins + 1.0)
    rng = np.random.default_rng(29)
    vals = rng.standard_normal((tile.N, g.V))
    prog = [(0, 1.0, 0, [(1, 0)]), (1, 0.5, 1, [(2, 0), (2, 0)])]
    for name, field in (("constant", np.full(tile.N, 0.5)), ("cycling", (np.arange(tile.N) % n_bins) + 0.5)):
        vals[:, 0] = field
        tile.set_physical_values(vals)
        for kind in ("domain", "level"):
            got, count, _, _ = _held(tile, g, vals, pts, gp, prog, edges, kind, "state", 0, g.nc, "%s %s %d bins %s" % (geom, name, n_bins, kind),
                                     populated=False)
            tot = count.sum(axis=1)
            assert tot[0] == 0 and tot[-1] == 0 and tot[-2] == 0
            assert (tot[1] == tile.N) if name == "constant" else (tot[1:-2] >= tile.N // n_bins).all()
    tile.close()


@pytest.mark.parametrize("geom,ring_L", [("RZ", None), ("RL", None), ("RLZ", None), ("RLZ", 16)])
def test_consistency(geom, ring_L):
    """per group the counts add to the group's points; the slot sums add to tile.reduce of the integrand (domain) or to the twin's
    per-level area integral (level), within the sum of the two bounds; the measure adds to the nf = 0 integral"""
    import scythe_jl_amd as S
    case = _case(geom, ring_L)
    hip = cases.HipModel(case)
    for _ in range(2):
        hip.step()
    tile, g = hip.run.tiles[0], cases.oracle_grid(case)
    tile.tileTransform_()
    pts, phys = _points(tile), tile.physical
    prog = R.random_program(g, 31, n_out=3)
    packed = S.pack_reduce_program(hip.gp, prog)
    edges = _quantile_edges(D.program_values64(phys, pts[:, 0], packed), 7)
    nz = g.zDim
    bound = XP(R.BOUND)
    dom = tile.distribution(prog, edges, "domain")
    count, sums, sabs, _ = D.distribution(g, phys, pts, packed, edges, "domain")
    assert dom.count.sum() == tile.N
    prog_r = [(0, 1.0, 0, [])] + [t for t in prog if t[0] > 0]
    red = tile.reduce(prog_r)
    _, rabs = R.reduce(g, phys, pts, S.pack_reduce_program(hip.gp, prog_r))
    err = np.abs(dom.sums[:, :, 0].astype(XP).sum(axis=0) - red.astype(XP))
    lim = bound * sabs[:, :, 0].sum(axis=0) + bound * rabs
    print("%s ring_L=%s: sum of the slots against reduce, error / allowance %s" % (geom, ring_L, (err / lim).astype(float)))
    assert (err <= lim).all() and (np.abs(red) > 0).all()
    lev = tile.distribution(prog, edges, "level")
    cl, sl, al, _ = D.distribution(g, phys, pts, packed, edges, "level")
    assert (lev.count.sum(axis=0) == tile.N // nz).all() and np.array_equal(lev.count.sum(axis=1), dom.count[:, 0])
    err = np.abs(lev.sums.astype(XP).sum(axis=0) - sl.sum(axis=0))
    assert (err <= 2 * bound * al.sum(axis=0)).all()
    hip.run.close()


def test_fp32_storage():
    """a program naming derivative slots with storage="f32": the twin reads the rounded planes; zDim = 32: two lanes of a wave per level"""
    import scythe_jl_amd as S
    case, gp, g, tile, pts = _tile(None, storage="f32", maker="rlz_hrbl", num_cells=6, zDim=32, ring_L=32)
    tile.set_physical_values(np.array(case["ic"](pts), dtype=np.float64))
    tile.spectralTransform_()
    tile.splineTransform_()
    tile.tileTransform_()
    phys = tile.physical
    assert (phys[:, :, 1:] == phys[:, :, 1:].astype(np.float32)).all() and np.abs(phys[:, :, 1:]).max() > 0
    prog = R.random_program(g, 37, n_out=2)
    assert {s for _, s in S.reduce_planes(gp, prog)} - {0}
    edges = _quantile_edges(D.program_values64(phys, pts[:, 0], S.pack_reduce_program(gp, prog)), 32)
    for kind in ("domain", "level"):
        _held(tile, g, phys, pts, gp, prog, edges, kind, "physical", 0, g.nc, "f32 storage %s" % kind)
    planes = S.reduce_planes(gp, prog)
    assert tile.kernel_bytes("k_distribution") == tile.N * sum(8 if s == 0 else 4 for _, s in planes)
    tile.close()


def _raw(tile, kind, source, coef, packed, n_out, n_bins, edges, count, sums, n_terms=None):
    from scythe_jl_amd import _lib as L
    packed = np.ascontiguousarray(packed, dtype=np.int32).reshape(-1, 11) if packed is not None else None
    coef = np.ascontiguousarray(coef, dtype=np.float64) if coef is not None else None
    edges = np.ascontiguousarray(edges, dtype=np.float64) if edges is not None else None
    n = n_terms if n_terms is not None else len(packed)
    return tile._lib.sx_distribution(tile._h, kind, source, n, coef.ctypes.data_as(L.P_D) if coef is not None else None,
                                     packed.ctypes.data_as(L.P_I32) if packed is not None else None, n_out, n_bins,
                                     edges.ctypes.data_as(L.P_D) if edges is not None else None,
                                     count.ctypes.data_as(L.P_I64) if count is not None else None,
                                     sums.ctypes.data_as(L.P_D) if sums is not None else None)


def _term(out=0, p=0, factors=()):
    return [out, p, len(factors)] + [f[0] for f in factors] + [0] * (4 - len(factors)) + [f[1] for f in factors] + [0] * (4 - len(factors))


def test_side_effects_and_refusals():
    """tests/test_gpu_extrema.py::test_scan_side_effects_and_refusals' pattern"""
    case = cases.rl_slab(num_cells=8)
    hip = cases.HipModel(case)
    for _ in range(2):
        hip.step()
    tile = hip.run.tiles[0]
    tile.tileTransform_()
    state0, phys0, A0 = tile.get_state(), tile.physical, tile.patchSpectral.copy()
    tile.enable_timers(True)
    tile.reset_timers()
    e3 = [0.0, 1.0, 2.0, 3.0]
    tile.distribution([(0, 0.5, 0, [("ub", ""), ("ub", "")]), (1, 0.5, 0, [("vb", ""), ("vb", "r")])], e3, "level")
    tm = tile.timers()
    assert tm["k_distribution"][1] == 1 and tm["k_distribution"][0] > 0 and tm["k_distribution_final"][1] == 1
    assert tile.kernel_bytes("k_distribution") == 3 * tile.N * 8 > 0
    tile.distribution([(0, 1.0, 0, [("h", "")])], e3, "domain", "state")
    assert tile.kernel_bytes("k_distribution") == tile.N * 8
    assert tile.get_state().tobytes() == state0.tobytes() and tile.physical.tobytes() == phys0.tobytes()
    assert tile.patchSpectral.tobytes() == A0.tobytes()
    lib = tile._lib
    ok = _term(0, -1, [(1, 0), (6, 4)])
    nf5, nfm = _term(0, 0, [(1, 0)]), _term(0, 0, [])
    nf5[2], nfm[2] = 5, -1
    bad = [("out below", 0, 0, [1.0], [_term(-1, 0, [(1, 0)])], 1, 3, e3), ("out at n_out", 0, 0, [1.0], [_term(1, 0, [(1, 0)])], 1, 3, e3),
           ("p above", 0, 0, [1.0], [_term(0, 3, [(1, 0)])], 1, 3, e3), ("p below", 0, 0, [1.0], [_term(0, -3, [(1, 0)])], 1, 3, e3),
           ("var 0", 0, 0, [1.0], [_term(0, 0, [(0, 0)])], 1, 3, e3), ("var above", 0, 0, [1.0], [_term(0, 0, [(7, 0)])], 1, 3, e3),
           ("slot below", 0, 0, [1.0], [_term(0, 0, [(1, -1)])], 1, 3, e3), ("slot above", 0, 0, [1.0], [_term(0, 0, [(1, 5)])], 1, 3, e3),
           ("n_factors above", 0, 0, [1.0], [nf5], 1, 3, e3), ("n_factors below", 0, 0, [1.0], [nfm], 1, 3, e3),
           ("state slot", 0, 1, [1.0], [_term(0, 0, [(1, 1)])], 1, 3, e3), ("n_terms above", 0, 0, [1.0] * 65, [ok] * 65, 1, 3, e3),
           ("source", 0, 2, [1.0], [ok], 1, 3, e3), ("kind", 2, 0, [1.0], [ok], 1, 3, e3),
           ("17 planes", 0, 0, [1.0] * 5, [_term(0, 0, [(v, s) for v, s in [(1 + i // 5, i % 5) for i in range(4 * k, min(4 * k + 4, 17))]])
                                           for k in range(5)], 1, 3, e3),
           ("n_out 0", 0, 0, [], [], 0, 3, e3), ("n_out 5", 0, 0, [1.0], [ok], 5, 3, e3),
           ("n_bins 0", 0, 0, [1.0], [ok], 1, 0, e3), ("n_bins 65", 0, 0, [1.0], [ok], 1, 65, np.arange(66.0)),
           ("edge nan", 0, 0, [1.0], [ok], 1, 3, [0.0, np.nan, 2.0, 3.0]), ("edge inf", 0, 0, [1.0], [ok], 1, 3, [0.0, 1.0, 2.0, np.inf]),
           ("edges equal", 0, 0, [1.0], [ok], 1, 3, [0.0, 1.0, 1.0, 3.0]), ("edges falling", 0, 0, [1.0], [ok], 1, 3, [0.0, 2.0, 1.0, 3.0]),
           ("null edges", 0, 0, [1.0], [ok], 1, 3, None)]
    big = 68 * 5
    for what, kind, source, coef, packed, n_out, n_bins, edges in bad:
        for k in ((kind,) if what == "kind" else (0, 1)):
            count, sums = np.full(big, -7, dtype=np.int64), np.full(big, -7.25)
            assert _raw(tile, k, source, coef, packed, n_out, n_bins, edges, count, sums) != 0, what
            assert lib.sx_last_error().decode(), what
            assert (count == -7).all() and (sums == -7.25).all(), what
    count, sums = np.full(big, -7, dtype=np.int64), np.full(big, -7.25)
    assert _raw(tile, 0, 0, None, [ok], 1, 3, e3, count, sums) != 0 and (count == -7).all() and (sums == -7.25).all()            # null coef
    assert _raw(tile, 0, 0, [1.0], None, 1, 3, e3, count, sums, n_terms=1) != 0 and (count == -7).all() and (sums == -7.25).all()
    assert _raw(tile, 0, 0, [1.0], [ok], 1, 3, e3, None, sums) != 0 and (sums == -7.25).all()
    assert _raw(tile, 0, 0, [1.0], [ok], 1, 3, e3, count, None) != 0 and (count == -7).all()
    assert _raw(tile, 0, 0, [1.0], [ok], 1, 3, e3, count, sums) == 0 and count[:6].sum() == tile.N and sums[0] != -7.25
    assert (count[6:] == -7).all() and (sums[6:] == -7.25).all()
    hip.run.close()


def test_lds_limit_on_the_device():
    """64 levels: 64 bins with three integrands are refused with the limit's message and nothing written; 40 bins with the measure only
    (55 KB of LDS) and 32 bins with one integrand (80 KB: above the 64 KB a launch gets unasked) run and agree with the twin"""
    import scythe_jl_amd as S
    case, gp, g, tile, pts = _tile(None, maker="rlz_hrbl", num_cells=6, zDim=64, ring_L=16)
    vals = np.random.default_rng(43).standard_normal((tile.N, g.V))
    tile.set_physical_values(vals)
    q = [(0, 1.0, 0, [("u", "")])]
    three = q + [(j, 1.0, 0, [("v", "")]) for j in (1, 2, 3)]
    coef, packed, n_out = S.pack_reduce_program(gp, three)
    count, sums = np.full(67 * 64, -7, dtype=np.int64), np.full(67 * 4 * 64, -7.25)
    assert _raw(tile, 1, 1, coef, packed, 4, 64, np.linspace(-2, 2, 65), count, sums) != 0
    assert "163840" in tile._lib.sx_last_error().decode() and "LDS" in tile._lib.sx_last_error().decode()
    assert (count == -7).all() and (sums == -7.25).all()
    _held(tile, g, vals, pts, gp, three, np.linspace(-2, 2, 65), "domain", "state", 0, g.nc, "64 levels domain 64 bins 3 integrands")
    _held(tile, g, vals, pts, gp, q, np.linspace(-2, 2, 41), "level", "state", 0, g.nc, "64 levels x 40 bins", populated=False)
    _held(tile, g, vals, pts, gp, q + [(1, 0.5, 0, [("v", ""), ("v", "")])], np.linspace(-2, 2, 33), "level", "state", 0, g.nc,
          "64 levels x 32 bins, one integrand", populated=False)
    tile.close()


@pytest.mark.parametrize("geom,ring_L", [("RLZ", 16), ("RL", None)])
def test_order_of_first_use(geom, ring_L):
    """distribution then reduce on one handle, reduce then distribution on another: the same bytes and kernel_bytes (the property
    tests/test_gpu_diagnostics_shared.py checks for the others)"""
    import scythe_jl_amd as S
    case = _case(geom, ring_L)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    prog = [(0, 1.0, 1, [("h", ""), ("h", "")]), (1, -0.5, 0, [("u", ""), ("v", "")])]
    edges = np.linspace(-1.0, 1.0, 9)

    def handle():
        tile = S.Grid(gp, mp)
        tile.set_physical_values(np.random.default_rng(11).standard_normal((tile.N, g.V)))
        return tile

    def dist(t):
        d = [t.distribution(prog, edges, k, "state") for k in ("domain", "level")]
        return b"".join(x.count.tobytes() + x.sums.tobytes() for x in d), t.kernel_bytes("k_distribution")

    def red(t):
        return t.reduce(prog, "domain", "state").tobytes() + t.reduce(prog, "azimuth", "state").tobytes(), t.kernel_bytes("k_reduce")
    first, second = handle(), handle()
    d1, r1 = dist(first), red(first)
    r2, d2 = red(second), dist(second)
    assert d1 == d2 and r1 == r2 and d1[1] > 0 and r1[1] > 0 and any(d1[0])
    first.close()
    second.close()
    third = handle()                      # a handle that closes with the distribution state alone
    assert dist(third) == d1
    third.close()


def test_host_conveniences():
    """cfad columns sum to 1 with the outside fractions; exceedance, integrated_kinetic_energy and quantile against the twin on rl_slab"""
    import scythe_jl_amd as S
    case = cases.rlz_hrbl(num_cells=6, zDim=10, ring_L=16)
    hip = cases.HipModel(case)
    for _ in range(2):
        hip.step()
    tile = hip.run.tiles[0]
    tile.tileTransform_()
    u = tile.physical[:, hip.gp.vars["u"] - 1, 0]
    cf = hip.run.cfad("u", np.quantile(u, [0.2, 0.4, 0.6, 0.8]))
    assert cf.frac.shape == (3, 10) and cf.under.shape == (10,) and (cf.frac > 0).any() and (cf.nan == 0).all()
    assert np.abs(cf.frac.sum(axis=0) + cf.under + cf.over + cf.nan - 1.0).max() <= 16 * 2.0 ** -53
    raw = hip.run.cfad([(0, 1.0, 0, [("u", "")])], np.quantile(u, [0.2, 0.4, 0.6, 0.8]), normalize=False)
    assert np.abs((raw.frac.sum(axis=0) + raw.under + raw.over) / raw.area - 1.0).max() <= 16 * 2.0 ** -53
    hip.run.close()

    case = cases.rl_slab(num_cells=9)
    hip = cases.HipModel(case, num_tiles=3, exchange="gather", impl="lib")
    for _ in range(3):
        hip.step()
    g = cases.oracle_grid(case)
    iu, iv = hip.gp.vars["u"] - 1, hip.gp.vars["v"] - 1
    rho = 1.15
    q_all, w_all, ke_all = [], [], []
    for t, tile in zip(hip.run.tile_ids, hip.run.tiles):
        tile.tileTransform_()
        phys, pts = tile.physical, _points(tile)
        w, _, _ = D.point_weights(g, pts, "domain", hip.run.layout.cell0[t], hip.run.layout.ncells[t])
        uu, vv = phys[:, iu, 0], phys[:, iv, 0]
        q_all.append(uu * uu + vv * vv)                                     # plain float64, term order: 0.0 + u u + v v
        w_all.append(w)
        ke_all.append((XP(0.5 * rho) * uu.astype(XP) * uu.astype(XP) + XP(0.5 * rho) * vv.astype(XP) * vv.astype(XP)) * w)
    q, w, ke = np.concatenate(q_all), np.concatenate(w_all), np.concatenate(ke_all)
    speed = np.sqrt(q)
    thr = np.quantile(speed, [0.3, 0.6, 0.9])
    bound = XP(R.BOUND)
    ike = hip.run.integrated_kinetic_energy("u", "v", thr, density=rho)
    exc = hip.run.exceedance([(0, 1.0, 0, [("u", ""), ("u", "")]), (0, 1.0, 0, [("v", ""), ("v", "")])], thr ** 2)
    assert exc.integral is None and exc.measure.tobytes() == ike.measure.tobytes() and np.array_equal(ike.thresholds, thr)
    for i, c in enumerate(thr ** 2):
        sel = q >= c
        assert 0 < sel.sum() < len(q)
        # the bound of every slot and tile that enters, and the host's few additions of positive numbers
        assert abs(XP(ike.measure[i]) - w[sel].sum()) <= 2 * bound * w[sel].sum()
        assert abs(XP(ike.integral[i]) - ke[sel].sum()) <= 2 * bound * ke[sel].sum()
    one = hip.run.exceedance([(0, 1.0, 0, [("u", ""), ("u", "")]), (0, 1.0, 0, [("v", ""), ("v", "")])], [thr[1] ** 2])
    assert abs(XP(one.measure[0]) - w[q >= thr[1] ** 2].sum()) <= 2 * bound * w.sum() and one.measure.shape == (1,)

    prog = [(0, 1.0, 0, [("u", ""), ("u", "")]), (0, 1.0, 0, [("v", ""), ("v", "")])]
    for p in (0.5, 0.9, 0.99):
        Q, cum, M = D.weighted_quantile(q, w, p)
        assert np.abs(cum - XP(p) * M).min() >= XP(1e-9) * M               # on the twin alone: a rounding of the measure cannot flip the slot
        res = hip.run.quantile(prog, p, tol=1e-6)
        inside = int(((q >= res.lo) & (q < res.hi)).sum())
        print("quantile p = %g: twin %.17g, bracket [%.17g, %.17g) after %d passes, %d point(s) inside" % (p, Q, res.lo, res.hi, res.passes, inside))
        assert res.lo <= Q < res.hi and res.nan_count == 0 and 1 <= res.passes <= 8
        assert res.hi - res.lo <= 1e-6 * (q.max() - q.min()) or inside == 1
        assert abs(XP(res.measure) - M) <= 2 * bound * M
    hip.run.close()
