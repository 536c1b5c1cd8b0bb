"""CPU-only: the host side of sx_reduce - the quadrature weights (sx_reduce_weights) against the twin of tests/reduce.py and against
closed forms, the program validator (sx_reduce_planes) and the invariants() programs."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import cases, linear_sw
from tests import reduce as R

XP = R.XP


def _ulps(a, b):
    """|a - b| in units of the spacing of b (b longdouble, rounded to double for the spacing)"""
    b64 = np.asarray(b, dtype=np.float64)
    return np.max(np.abs(np.asarray(a).astype(XP) - b) / np.spacing(np.abs(b64)).astype(XP))


SHAPES = [("R", cases.r_bcs(num_cells=12), None), ("RZ", cases.rz_advection(num_cells=9, zDim=12), None),
          ("RL native", cases.rl_slab(num_cells=9), None), ("RL uniform 16", cases.rl_slab(num_cells=9, ring_L=16), None),
          ("RLZ", cases.rlz_hrbl(num_cells=9, zDim=10), None), ("RLZ tile 2 of 3", cases.rlz_hrbl(num_cells=9, zDim=10), 1),
          ("R tile 2 of 3", cases.r_bcs(num_cells=12), 1)]


@pytest.mark.parametrize("name,case,tile", SHAPES, ids=[s[0] for s in SHAPES])
def test_weights_against_twin(name, case, tile):
    import scythe_jl_amd as S
    gp, _ = cases.hip_params(case)
    g = cases.oracle_grid(case)
    c0, n = (0, g.nc) if tile is None else cases.even_tiles(g.nc, 3)[tile]
    w_r, w_l, w_z = S.reduce_weights(gp, c0, n)
    t_r, t_l, t_z = R.weights(g, c0, n)
    assert w_r.shape == t_r.shape and w_l.shape == t_l.shape
    assert _ulps(w_r, t_r) <= 2 and _ulps(w_l, t_l) <= 2
    if g.has_z:
        assert w_z.shape == t_z.shape and _ulps(w_z, t_z) <= 2
    else:
        assert w_z is None
    if not g.has_l:
        assert (w_l == 1.0).all()


def _within(got, truth, sabs):
    assert abs(got - truth) <= XP(R.BOUND) * sabs, (float(got), float(truth), float(abs(got - truth) / (XP(R.BOUND) * sabs)))


@pytest.mark.parametrize("geometry,pmax", [("R", 5), ("RL", 4)])
def test_radial_weights_are_gauss_legendre(geometry, pmax):
    """sum w_r r^p over a tile = the integral of r^p J(r) over its cells: 3-point Gauss-Legendre is exact to degree 5 per cell, so
    only the rounding of the weights and of the printed radii (p ulp) is left"""
    import scythe_jl_amd as S
    gp = S.GridParameters(geometry=geometry, xmin=0.5, xmax=6.5, num_cells=12, vars={"u": 1})
    c0, n = 4, 5
    w_r, _, _ = S.reduce_weights(gp, c0, n)
    r = O.mish_points(0.5, 0.5, c0, n).astype(XP)
    a, b = XP(0.5) + XP(c0) * XP(0.5), XP(0.5) + XP(c0 + n) * XP(0.5)
    j = 1 if geometry == "RL" else 0
    for p in range(pmax + 1):
        got = (w_r.astype(XP) * r ** p).sum()
        q = p + j + 1
        _within(got, (b ** q - a ** q) / XP(q), (np.abs(w_r).astype(XP) * r ** p).sum())


@pytest.mark.parametrize("zDim", [9, 10, 32])
def test_vertical_weights_are_clenshaw_curtis(zDim):
    """sum w_z z^p = (zmax^(p+1) - zmin^(p+1)) / (p + 1) for p <= zDim - 1, at the grid's own Float64 levels"""
    import scythe_jl_amd as S
    zmin, zmax = 0.25, 2.0
    gp = S.GridParameters(geometry="RZ", xmin=0.0, xmax=1.0, num_cells=4, zmin=zmin, zmax=zmax, zDim=zDim, vars={"u": 1})
    _, _, w_z = S.reduce_weights(gp)
    z = O.Cheb(zmin, zmax, zDim).z.astype(XP)
    for p in range(zDim):
        got = (w_z.astype(XP) * z ** p).sum()
        _within(got, (XP(zmax) ** (p + 1) - XP(zmin) ** (p + 1)) / XP(p + 1), (np.abs(w_z).astype(XP) * np.abs(z) ** p).sum())


@pytest.mark.parametrize("ring_L", [None, 16])
def test_azimuthal_weights_sum_to_two_pi(ring_L):
    import scythe_jl_amd as S
    case = cases.rl_slab(num_cells=9, ring_L=ring_L)
    gp, _ = cases.hip_params(case)
    g = cases.oracle_grid(case)
    _, w_l, _ = S.reduce_weights(gp)
    for i in range(g.rDim):
        _within(XP(int(g.L[i])) * XP(w_l[i]), XP(2) * R.PI_X, XP(int(g.L[i])) * XP(w_l[i]))


# ----------------------------------------------------------------------------- sx_reduce_planes
def _raw_planes(gp, source, packed, n_out, n_terms=None, null_terms=False, c0=0, n=None):
    """(rc, planes, n_planes, message) of a raw sx_reduce_planes call; planes / n_planes start as -7"""
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    from scythe_jl_amd.model import grid_desc
    d, keep = grid_desc(gp, c0, n)
    packed = np.ascontiguousarray(packed, dtype=np.int32).reshape(-1, 11)
    planes = np.full((16, 2), -7, dtype=np.int32)
    cnt = C.c_int32(-7)
    lib = S.load()
    rc = lib.sx_reduce_planes(C.byref(d), source, len(packed) if n_terms is None else n_terms,
                              None if null_terms else packed.ctypes.data_as(L.P_I32), n_out, planes.ctypes.data_as(L.P_I32), C.byref(cnt))
    return rc, planes, cnt.value, lib.sx_last_error().decode()


def _term(out=0, p=0, factors=()):
    row = [out, p, len(factors)] + [f[0] for f in factors] + [0] * (4 - len(factors)) + [f[1] for f in factors] + [0] * (4 - len(factors))
    return row


def test_planes_order_and_deduplication():
    import scythe_jl_amd as S
    gp, _ = cases.hip_params(cases.rlz_hrbl(num_cells=9, zDim=10))
    terms = [(0, 1.0, 0, [("ub", ""), ("vb", "r")]), (1, 2.0, 1, [("vb", "r"), ("h", "zz"), ("ub", "")]), (1, 1.0, -1, []),
             (2, 1.0, 0, [(6, 3), ("h", "zz")])]
    planes = S.reduce_planes(gp, terms)
    assert planes.tolist() == [[4, 0], [5, 1], [1, 6], [6, 3]]
    assert S.reduce_planes(gp, [(0, 1.0, 2, []), (3, -1.0, 0, [])]).shape == (0, 2)          # n_factors = 0 names no plane
    assert S.reduce_planes(gp, []).shape == (0, 2)
    # factor entries past n_factors are ignored, whatever they hold
    row = _term(0, 0, [(1, 0)])
    row[4], row[8] = 99, 99
    rc, pl, n, msg = _raw_planes(gp, 0, [row], 1)
    assert rc == 0 and n == 1 and pl[0].tolist() == [1, 0]


def test_planes_limit():
    gp, _ = cases.hip_params(cases.rlz_hrbl(num_cells=9, zDim=10))
    all_planes = [(v, s) for v in (1, 2, 3) for s in range(7)]

    def prog(k):
        return [_term(i // 4 % 16, 0, all_planes[i:min(i + 4, k)]) for i in range(0, k, 4)]
    rc, pl, n, msg = _raw_planes(gp, 0, prog(16), 16)
    assert rc == 0 and n == 16 and pl.tolist() == [list(p) for p in all_planes[:16]]
    rc, pl, n, msg = _raw_planes(gp, 0, prog(17), 16)
    assert rc != 0 and "16" in msg and n == -7 and (pl == -7).all()


def test_planes_refusals():
    import scythe_jl_amd as S
    gp, _ = cases.hip_params(cases.rl_slab(num_cells=9))           # 6 variables, 5 slots
    ok = _term(0, 0, [(1, 0), (6, 4)])
    assert _raw_planes(gp, 0, [ok], 1)[0] == 0
    bad = {"out below": _term(-1, 0, [(1, 0)]), "out at n_out": _term(1, 0, [(1, 0)]), "p above": _term(0, 3, [(1, 0)]),
           "p below": _term(0, -3, [(1, 0)]), "var 0": _term(0, 0, [(0, 0)]), "var above": _term(0, 0, [(1, 0), (7, 0)]),
           "slot below": _term(0, 0, [(1, -1)]), "slot above": _term(0, 0, [(1, 5)])}
    nf5 = _term(0, 0, [(1, 0)])
    nf5[2] = 5
    bad["n_factors above"] = nf5
    nfm = _term(0, 0, [])
    nfm[2] = -1
    bad["n_factors below"] = nfm
    for what, row in bad.items():
        rc, pl, n, msg = _raw_planes(gp, 0, [ok, row], 1)
        assert rc != 0 and msg and n == -7 and (pl == -7).all(), what
    # counts over the limits, a null pointer with a non-zero count, an unknown source
    assert _raw_planes(gp, 0, [ok] * 64, 1)[0] == 0
    assert _raw_planes(gp, 0, [ok] * 65, 1)[0] != 0
    assert _raw_planes(gp, 0, [_term(15, 0, [(1, 0)])], 16)[0] == 0
    assert _raw_planes(gp, 0, [ok], 17)[0] != 0
    assert _raw_planes(gp, 0, [ok], 1, null_terms=True)[0] != 0
    assert _raw_planes(gp, 0, [], 0, n_terms=0, null_terms=True)[0] == 0
    assert _raw_planes(gp, 2, [ok], 1)[0] != 0
    # SX_REDUCE_STATE holds the values only
    assert _raw_planes(gp, 1, [_term(0, 0, [(1, 0), (2, 0)])], 1)[0] == 0
    rc, pl, n, msg = _raw_planes(gp, 1, [_term(0, 0, [(1, 0), (2, 1)])], 1)
    assert rc != 0 and "slot 0" in msg
    with pytest.raises(S.ScytheHipError):
        S.reduce_planes(gp, [(0, 1.0, 0, [("h", "r")])], source="state")
    with pytest.raises(ValueError):
        S.reduce_planes(gp, [(0, 1.0, 0, [("h", "z")])])           # an RL grid has no z slot
    # p < 0 where a gridpoint sits at r == 0: an R grid with an odd cell count centred on 0 - its middle tile only
    g0 = S.GridParameters(geometry="R", xmin=-1.5, xmax=1.5, num_cells=3, vars={"u": 1})
    assert 0.0 in O.mish_points(-1.5, 1.0, 0, 3)
    neg, pos = _term(0, -1, [(1, 0)]), _term(0, 1, [(1, 0)])
    assert _raw_planes(g0, 0, [neg], 1)[0] != 0 and _raw_planes(g0, 0, [pos], 1)[0] == 0
    assert _raw_planes(g0, 0, [neg], 1, c0=1, n=1)[0] != 0
    assert _raw_planes(g0, 0, [neg], 1, c0=0, n=1)[0] == 0 and _raw_planes(g0, 0, [neg], 1, c0=2, n=1)[0] == 0
    assert _raw_planes(gp, 0, [_term(0, -2, [(1, 0)])], 1)[0] == 0           # polar: the first ring lies inside the first cell


# ----------------------------------------------------------------------------- invariants()
def _twin_on(case, fields):
    import scythe_jl_amd as S
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    pts = g.gridpoints()
    pts = pts.reshape(len(pts), -1)
    prog = S.invariants(mp)
    res, _ = R.reduce(g, fields(pts), pts, S.pack_reduce_program(gp, prog))
    return prog, res, g


def _close(a, b):
    assert abs(a - b) <= XP(1e-15) * abs(b), (float(a), float(b))


def test_invariants_linear_shallow_water_1d():
    case = linear_sw.r_case(num_cells=6, bc="walls", g=2.0, H=0.5)
    prog, res, g = _twin_on(case, lambda p: np.stack([1.0 + 0.125 * p[:, 0], 0.25 * p[:, 0] - 1.0], axis=1))
    assert prog.names == ["mass", "energy"]
    X = XP(12)
    _close(res[0], X + XP(0.125) * X ** 2 / 2)
    h2 = X + XP(0.125) * X ** 2 + XP(0.125) ** 2 * X ** 3 / 3
    u2 = XP(0.0625) * X ** 3 / 3 - XP(0.25) * X ** 2 + X
    _close(res[1], (XP(2) * h2 + XP(0.5) * u2) / 2)


def test_invariants_linear_shallow_water_rl():
    case = linear_sw.rl_case(num_cells=4, g=2.0, H=0.5, xmax=8.0)

    def fields(p):
        r, l = p[:, 0], p[:, 1]
        return np.stack([1.0 + 0.25 * r * np.cos(l), 0.125 * r, 0.5 + 0.125 * r * np.sin(l)], axis=1)
    prog, res, g = _twin_on(case, fields)
    Rm, pi = XP(8), R.PI_X
    # the Float64 cos / sin of the fields leave 1e-16 of the wavenumber-1 terms behind: compare to 1e-14
    mass = pi * Rm ** 2
    h2 = pi * Rm ** 2 + XP(0.0625) * pi * Rm ** 4 / 4
    u2 = XP(0.015625) * 2 * pi * Rm ** 4 / 4
    v2 = XP(0.25) * pi * Rm ** 2 + XP(0.015625) * pi * Rm ** 4 / 4
    assert abs(res[0] - mass) <= XP(1e-14) * mass
    en = (XP(2) * h2 + XP(0.5) * (u2 + v2)) / 2
    assert abs(res[1] - en) <= XP(1e-14) * en


def test_invariants_linear_advection_and_others():
    import scythe_jl_amd as S
    prog, res, g = _twin_on(cases.r_bcs(num_cells=6), lambda p: (1.0 + 0.5 * p[:, 0])[:, None])
    assert len(prog.names) == 2
    X = XP(12)
    _close(res[0], X + X ** 2 / 4)
    _close(res[1], X + X ** 2 / 2 + X ** 3 / 12)
    for maker in (cases.rz_advection, cases.rl_advection, cases.rlz_advection):
        gp, mp = cases.hip_params(maker())
        assert [t[3] for t in S.invariants(mp)] == [[("h", "")], [("h", ""), ("h", "")]]
    gp, mp = cases.hip_params(cases.rl_slab(num_cells=9))
    with pytest.raises(ValueError):
        S.invariants(mp)
