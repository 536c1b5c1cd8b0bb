"""sx_distribution_slot and sx_distribution_check (pure host helpers) and the twin of tests/distribution.py, without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import cases
from tests import distribution as D
from tests import reduce as R

XP = D.XP


def _case(geom):
    if geom == "R":
        return cases.r_bcs(num_cells=12)
    if geom == "RZ":
        return cases.rz_advection(num_cells=9, zDim=12)
    if geom == "RL":
        return cases.rl_slab(num_cells=9)
    return cases.rlz_hrbl(num_cells=9, zDim=10, ring_L=16)


@pytest.mark.parametrize("n_bins", [1, 5, 64])
def test_slot_against_searchsorted(n_bins):
    import scythe_jl_amd as S
    rng = np.random.default_rng(3 + n_bins)
    edges = np.sort(rng.uniform(-3.0, 5.0, n_bins + 1))
    edges[n_bins // 2] = 0.0                                   # an edge at zero: -0.0 belongs to the bin that starts there
    edges = np.unique(edges)
    assert len(edges) == n_bins + 1 and (np.diff(edges) > 0).all()
    probes = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), 0.5 * (edges[1:] + edges[:-1]),
                             [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1.7e308, -1.7e308]])
    want = D.slots(edges, probes)
    got = np.array([S.distribution_slot(edges, q) for q in probes])
    assert np.array_equal(got, want)
    at0 = int(np.nonzero(edges == 0.0)[0][0])
    assert S.distribution_slot(edges, -0.0) == S.distribution_slot(edges, 0.0) == at0 + 1
    assert S.distribution_slot(edges, -np.inf) == 0 and S.distribution_slot(edges, np.inf) == n_bins + 1
    assert S.distribution_slot(edges, np.nan) == n_bins + 2
    assert S.distribution_slot(edges, edges[0]) == 1 and S.distribution_slot(edges, np.nextafter(edges[0], -np.inf)) == 0
    assert S.distribution_slot(edges, edges[-1]) == n_bins + 1 and S.distribution_slot(edges, np.nextafter(edges[-1], -np.inf)) == n_bins


def test_slot_refusals():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = L.load()
    e = np.array([0.0, 1.0, 2.0])
    s = C.c_int32(-9)
    assert lib.sx_distribution_slot(2, None, 0.5, C.byref(s)) != 0 and lib.sx_last_error().decode() and s.value == -9
    assert lib.sx_distribution_slot(2, e.ctypes.data_as(L.P_D), 0.5, None) != 0
    assert lib.sx_distribution_slot(0, e.ctypes.data_as(L.P_D), 0.5, C.byref(s)) != 0 and s.value == -9
    assert lib.sx_distribution_slot(65, np.arange(66.0).ctypes.data_as(L.P_D), 0.5, C.byref(s)) != 0 and s.value == -9
    for bad in ([0.0, 0.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, 1.0, np.inf], [-np.inf, 1.0, 2.0]):
        with pytest.raises(S.ScytheHipError):
            S.distribution_slot(bad, 0.5)
        assert s.value == -9
    assert lib.sx_distribution_slot(2, e.ctypes.data_as(L.P_D), 0.5, C.byref(s)) == 0 and s.value == 1


def _term(out=0, p=0, factors=()):
    return [out, p, len(factors)] + [f[0] for f in factors] + [0] * (4 - len(factors)) + [f[1] for f in factors] + [0] * (4 - len(factors))


def test_check_refusals():
    """everything sx_distribution refuses of a call that needs no device"""
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    from scythe_jl_amd.model import grid_desc
    lib = L.load()
    gp, _ = cases.hip_params(cases.rl_slab(num_cells=9))              # 6 variables, 5 slots
    desc, keep = grid_desc(gp)
    e3 = [0.0, 1.0, 2.0, 3.0]

    def raw(d, kind, source, packed, n_out, n_bins, edges, n_terms=None):
        pk = np.ascontiguousarray(packed, dtype=np.int32).reshape(-1, 11) if packed is not None else None
        ed = np.ascontiguousarray(edges, dtype=np.float64) if edges is not None else None
        return lib.sx_distribution_check(C.byref(d) if d is not None else None, kind, source, n_terms if n_terms is not None else len(pk),
                                         pk.ctypes.data_as(L.P_I32) if pk is not None else None, n_out, n_bins,
                                         ed.ctypes.data_as(L.P_D) if ed is not None else None)

    ok = _term(0, -1, [(1, 0), (6, 4)])
    assert raw(desc, 0, 0, [ok], 1, 3, e3) == 0 and raw(desc, 1, 0, [ok, _term(3, 0, [(2, 1)])], 4, 3, e3) == 0
    nf5, nfm = _term(0, 0, [(1, 0)]), _term(0, 0, [])
    nf5[2], nfm[2] = 5, -1
    bad = [("out below", 0, 0, [_term(-1, 0, [(1, 0)])], 1, 3, e3), ("out at n_out", 0, 0, [_term(1, 0, [(1, 0)])], 1, 3, e3),
           ("p above", 0, 0, [_term(0, 3, [(1, 0)])], 1, 3, e3), ("p below", 0, 0, [_term(0, -3, [(1, 0)])], 1, 3, e3),
           ("var 0", 0, 0, [_term(0, 0, [(0, 0)])], 1, 3, e3), ("var above", 0, 0, [_term(0, 0, [(7, 0)])], 1, 3, e3),
           ("slot below", 0, 0, [_term(0, 0, [(1, -1)])], 1, 3, e3), ("slot above", 0, 0, [_term(0, 0, [(1, 5)])], 1, 3, e3),
           ("n_factors above", 0, 0, [nf5], 1, 3, e3), ("n_factors below", 0, 0, [nfm], 1, 3, e3),
           ("state slot", 0, 1, [_term(0, 0, [(1, 1)])], 1, 3, e3), ("n_terms above", 0, 0, [ok] * 65, 1, 3, e3),
           ("source", 0, 2, [ok], 1, 3, e3),
           ("17 planes", 0, 0, [_term(0, 0, [(v, s) for v, s in [(1 + i // 5, i % 5) for i in range(4 * k, min(4 * k + 4, 17))]])
                                for k in range(5)], 1, 3, e3),
           ("n_out 0", 0, 0, [], 0, 3, e3), ("n_out 5", 0, 0, [ok], 5, 3, e3),
           ("n_bins 0", 0, 0, [ok], 1, 0, [0.0]), ("n_bins 65", 0, 0, [ok], 1, 65, np.arange(66.0)), ("n_bins negative", 0, 0, [ok], 1, -1, e3),
           ("edge nan", 0, 0, [ok], 1, 3, [0.0, np.nan, 2.0, 3.0]), ("edge inf", 0, 0, [ok], 1, 3, [0.0, 1.0, 2.0, np.inf]),
           ("edge -inf", 0, 0, [ok], 1, 3, [-np.inf, 1.0, 2.0, 3.0]), ("edges equal", 0, 0, [ok], 1, 3, [0.0, 1.0, 1.0, 3.0]),
           ("edges falling", 0, 0, [ok], 1, 3, [0.0, 2.0, 1.0, 3.0]), ("null edges", 0, 0, [ok], 1, 3, None),
           ("kind 2", 2, 0, [ok], 1, 3, e3), ("kind -1", -1, 0, [ok], 1, 3, e3)]
    for what, kind, source, packed, n_out, n_bins, edges in bad:
        assert raw(desc, kind, source, packed, n_out, n_bins, edges) != 0, what
        assert lib.sx_last_error().decode(), what
    assert raw(desc, 0, 0, None, 1, 3, e3, n_terms=1) != 0 and lib.sx_last_error().decode()            # null terms
    assert raw(None, 0, 0, [ok], 1, 3, e3) != 0 and lib.sx_last_error().decode()
    desc.abi_version = 1
    assert raw(desc, 0, 0, [ok], 1, 3, e3) != 0
    # a negative r power on a tile with a gridpoint at r == 0 (sx_reduce_planes' own refusal)
    g0 = S.GridParameters(geometry="R", xmin=-4.5, xmax=4.5, num_cells=9, vars={"u": 1})
    with pytest.raises(S.ScytheHipError, match="r == 0"):
        S.distribution_check(g0, [(0, 1.0, -1, [("u", "")])], e3)
    S.distribution_check(g0, [(0, 1.0, 2, [("u", "")])], e3, "level")


def test_lds_limit():
    """SX_DIST_LEVEL keeps every level's bins in the LDS of one workgroup: zDim (n_bins + 3) (16 n_out + 4) + 8 (n_bins + 1) <= 163840"""
    import scythe_jl_amd as S

    def gp(zDim):
        return cases.hip_params(cases.rlz_hrbl(num_cells=6, zDim=zDim, ring_L=16))[0]
    q = [(0, 1.0, 0, [("u", "")])]
    one, three = q + [(1, 1.0, 0, [("v", "")])], q + [(j, 1.0, 0, [("v", "")]) for j in (1, 2, 3)]
    S.distribution_check(gp(64), q, np.arange(41.0), "level")                 # 64 levels x 40 bins, the measure only
    S.distribution_check(gp(32), one, np.arange(33.0), "level")               # 32 levels x 32 bins, one integrand
    S.distribution_check(gp(64), three, np.arange(65.0), "domain")            # the domain kind has no such limit
    S.distribution_check(gp(64), one, np.arange(33.0), "level")               # the bench grid's levels, 32 bins, one integrand
    S.distribution_check(gp(64), one, np.arange(65.0), "level")               # 154888 bytes
    for zDim, terms, nb in ((64, three, 64), (64, three, 40), (128, q, 64)):
        n_out = max(t[0] for t in terms) + 1
        need = zDim * (nb + 3) * (16 * n_out + 4) + 8 * (nb + 1)
        assert need > 163840
        with pytest.raises(S.ScytheHipError, match="163840") as ei:
            S.distribution_check(gp(zDim), terms, np.arange(nb + 1.0), "level")
        assert str(need) in str(ei.value)
    # a grid without a vertical: the level kind is the domain kind
    gl, _ = cases.hip_params(cases.rl_slab(num_cells=9))
    S.distribution_check(gl, [(0, 1.0, 0, [("u", "")])] + [(j, 1.0, 0, [("v", "")]) for j in (1, 2, 3)], np.arange(65.0), "level")


def test_packing(monkeypatch):
    """Grid.distribution hands its term list to pack_reduce_program exactly as Grid.reduce does (tests/test_extrema.py's recorder)"""
    import scythe_jl_amd as S
    from scythe_jl_amd import model as M
    gp, _ = cases.hip_params(_case("RLZ"))
    terms = [(0, 1.0, 0, [("ub", ""), ("ub", "")]), (0, 1.0, 0, [("vb", ""), ("vb", "")]), (1, 2.0, -1, [("h", "l")])]

    class Stop(Exception):
        pass
    seen = []

    def recorder(patch, t):
        seen.append((patch, t))
        raise Stop()
    tile = S.Grid.__new__(S.Grid)
    tile.patch_params = gp
    with monkeypatch.context() as mp:
        mp.setattr(M, "pack_reduce_program", recorder)
        for call in (lambda: S.Grid.reduce(tile, terms, "domain", "state"), lambda: S.Grid.distribution(tile, terms, [0.0, 1.0], "level", "state")):
            with pytest.raises(Stop):
                call()
    assert len(seen) == 2 and seen[1][0] is gp and seen[1][1] is terms
    with pytest.raises(ValueError):
        S.Grid.distribution(tile, terms, [0.0, 1.0], "azimuth")
    assert S.Distribution._fields == ("count", "measure", "sums", "edges")


@pytest.mark.parametrize("geom", ["R", "RZ", "RL", "RLZ"])
def test_twin_rules(geom):
    """the twin's own rules: the counts of a group sum to its points, the slot sums add up to tests/reduce.py's integral, the measure
    to the nf = 0 integral, and the float64 q agrees with the longdouble evaluation within the scan bound"""
    import scythe_jl_amd as S
    from tests import extrema as X
    case = _case(geom)
    gp, _ = cases.hip_params(case)
    g = cases.oracle_grid(case)
    pts = g.gridpoints()
    pts = pts.reshape(len(pts), -1)
    N = len(pts)
    rng = np.random.default_rng(5)
    data = rng.standard_normal((N, g.V, g.D))
    prog = R.random_program(g, 17, n_out=4)
    packed = S.pack_reduce_program(gp, prog)
    q = D.program_values64(data, pts[:, 0], packed)
    qx, sabs_q, nt = X.integrand(data, pts[:, 0], packed)
    assert (np.abs(q.astype(XP) - qx[0]) <= X.scan_bound(sabs_q, nt)[0]).all() and np.abs(q).max() > 0
    lo, hi = np.quantile(q, [0.1, 0.9])
    edges = np.linspace(lo, hi, 6)
    data[7, :, :] = np.nan                                        # one NaN point
    nz = g.zDim
    for kind, groups in (("domain", 1), ("level", nz)):
        count, sums, sabs, sl = D.distribution(g, data, pts, packed, edges, kind)
        assert count.shape == (8, groups) and sums.shape == (8, 4, groups)
        assert (count.sum(axis=0) == N // groups).all() and count[-1].sum() == 1 and count[0].sum() > 0 and count[-2].sum() > 0
        assert (count[1:-2].sum(axis=1) > 0).sum() >= 3                 # at least half the bins hold points
        assert sl[7] == 7 and np.isnan(sums[7, 1:]).any()
    data[7, :, :] = 0.25
    count, sums, sabs, sl = D.distribution(g, data, pts, packed, edges, "domain")
    prog_m = [(0, 1.0, 0, [])] + [(o, c, p, f) for o, c, p, f in prog if o > 0]
    truth, tabs = R.reduce(g, data, pts, S.pack_reduce_program(gp, prog_m))
    tot = sums[:, :, 0].sum(axis=0)
    assert (np.abs(tot - truth) <= XP(2.0 ** -60) * tabs).all() and tot[0] > 0
    cl, sl_, _, _ = D.distribution(g, data, pts, packed, edges, "level")
    assert np.array_equal(cl.sum(axis=1), count[:, 0])
    # the weighted quantile by sorting
    w, _, _ = D.point_weights(g, pts)
    Q, cum, M = D.weighted_quantile(q, w, 0.5)
    assert (w[q < Q].sum() <= XP(0.5) * M * (1 + XP(2.0 ** -60))) and (w[q <= Q].sum() >= XP(0.5) * M * (1 - XP(2.0 ** -60)))
