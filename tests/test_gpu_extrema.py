"""sx_extrema and sx_extremum_refine on the GPU against the twin of tests/extrema.py.

The scan of one-factor programs is held to numpy EXACTLY (values and rows); programs with arithmetic are held to the longdouble twin
within tests/extrema.py's derived rounding bound of a scanned value.  The refinement is held to the longdouble twin's Newton on the same
A: the position within (gradient rounding bound) / (smallest Hessian eigenvalue) + tol DX, in coordinates scaled by (DX, DX, zmax - zmin).

test_refine_accuracy prints, per case, the steps taken, the position error against the twin, the bound it was held to (scaled units) and
the distance to the closed-form centre of the Gaussian in DX (which the spline is not: printed, not asserted); DESIGN.md 14, "Figures",
holds the numbers of one run on the card."""
import ctypes as C

import numpy as np
import pytest

from tests import cases
from tests import extrema as X

pytestmark = pytest.mark.gpu

XP = X.XP
EPS = X.EPS
CASES = {"rl8": ("rl_slab", dict(num_cells=8)), "rl8_L16": ("rl_slab", dict(num_cells=8, ring_L=16)),
         "rlz6_L16": ("rlz_hrbl", dict(num_cells=6, zDim=10, ring_L=16)), "rlz6": ("rlz_hrbl", dict(num_cells=6, zDim=10)),
         "rz10": ("rz_advection", dict(num_cells=10, zDim=14)), "r24": ("r_bcs", dict(num_cells=24))}
# for the refinement only: 16 x 73 = 1,168 columns per variable, above the 1,024 at which k_refine goes from one wave to four
WIDE = {"rlz12_wide": ("rlz_hrbl", dict(num_cells=12, zDim=24))}


def _make(name, storage="f64"):
    import scythe_jl_amd as S
    maker, kw = CASES[name] if name in CASES else WIDE[name]
    case = getattr(cases, maker)(**kw)
    gp, mp = cases.hip_params(case, storage)
    g = cases.oracle_grid(case)
    tile = S.Grid(gp, mp)
    pts = S.getGridpoints(tile)
    pts = pts.reshape(len(pts), -1)
    return case, gp, g, tile, pts


def _wind(case, g, pts):
    """the case's fields; on the slab / HRBL cases the wind is the _vortex profile with a wave-2 and a smaller wave-1 perturbation, so
    that the speed has ONE largest gridpoint"""
    vals = np.array(case["ic"](pts), dtype=np.float64)
    if g.has_l and g.V == 6:
        r, l = pts[:, 0], pts[:, 1]
        vals[:, 2] = cases._vortex(r) * (1 + 0.05 * np.cos(2 * l - 0.6) + 0.03 * np.cos(l - 0.4))
        if g.has_z:            # and one largest level: 700 is no level and not the middle of the (symmetric) levels
            vals[:, 2] *= 1 - ((pts[:, 2] - 700.0) / 2000.0) ** 2
    return vals


def _filled(name, storage="f64"):
    case, gp, g, tile, pts = _make(name, storage)
    tile.set_physical_values(_wind(case, g, pts))
    tile.spectralTransform_()
    tile.splineTransform_()
    tile.tileTransform_()
    return case, gp, g, tile, pts


def _nz(g):
    return g.zDim if g.has_z else 1


# ----------------------------------------------------------------------------- the scan
@pytest.mark.parametrize("name", list(CASES))
def test_scan_exact(name):
    case, gp, g, tile, pts = _filled(name)
    phys, np1 = tile.physical, tile.var_np1
    prog = [(v, 1.0, 0, [(v + 1, 0)]) for v in range(g.V)]                 # output v = variable v + 1, value slot
    for source, data in (("physical", phys[:, :, 0]), ("state", np1)):
        for kind in ("domain", "azimuth"):
            val, idx = tile.extrema(prog, kind, source)
            tv, ti = X.scan(np.ascontiguousarray(data.T), g.L, _nz(g), kind)
            assert val.shape == tv.shape and idx.dtype == np.int64
            assert np.array_equal(idx, ti), (name, source, kind)
            assert np.array_equal(val, tv), (name, source, kind)
            assert np.array_equal(val, data[idx, np.arange(g.V)]), (name, source, kind)        # val is the value AT idx
            v2, i2 = tile.extrema(prog, kind, source)
            assert v2.tobytes() == val.tobytes() and i2.tobytes() == idx.tobytes()
    # a derivative slot, exactly
    val, idx = tile.extrema([(0, 1.0, 0, [(1, 1)])], "domain")
    tv, ti = X.scan(phys[:, 0, 1][None, :], g.L, _nz(g))
    assert np.array_equal(idx, ti) and np.array_equal(val, tv)
    tile.close()


def _programs(g):
    if not g.has_l:        # R: u; RZ: h u v w - the thread = point branch: several terms per output, r powers, derivative slots, 16 outputs
        a, b = g.names[0], g.names[-1]
        prog = [(0, 1.0, 0, [(a, ""), (a, "")]), (0, 1.0, 0, [(b, ""), (b, "")]), (1, 1.0, -1, [(b, "")]), (2, 1.0, 0, [(a, "r")]),
                (2, -0.5, 1, [(b, "zz" if g.has_z else "rr"), (a, "")])]
        for o in range(3, 16):
            prog.append((o, 0.25 * o, o % 3 - 1 if o % 3 else 0, [(a, ""), (b, "r")][:1 + o % 2]))
            prog.append((o, -1.5, 0, [(b, ""), (a, "")]))
        return prog
    prog = [(0, 1.0, 0, [("u", ""), ("u", "")]), (0, 1.0, 0, [("v", ""), ("v", "")]),     # speed^2
            (1, 1.0, -1, [("v", "")]),                                                  # v / r
            (2, 1.0, 0, [("h", "r")]),                                                  # a derivative slot
            (2, -0.5, 1, [("u", "l"), ("h", "")])]
    for o in range(3, 16):                                                              # 16 outputs at once
        prog.append((o, 0.25 * o, o % 3 - 1 if o % 3 else 0, [("vb", ""), ("h", "")][:1 + o % 2]))
        prog.append((o, -1.5, 0, [("ub", ""), ("u", "")]))
    return prog


@pytest.mark.parametrize("name", ["rl8", "rl8_L16", "rlz6_L16", "rlz6", "rz10", "r24"])
def test_scan_programs(name):
    import scythe_jl_amd as S
    case, gp, g, tile, pts = _filled(name)
    prog = _programs(g)
    packed = S.pack_reduce_program(gp, prog)
    assert packed[2] == 16
    phys = tile.physical
    q, sabs, nt = X.integrand(phys, pts[:, 0], packed)
    bound = X.scan_bound(sabs, nt)
    # the index check is sharp where it matters: the two largest speeds differ by far more than the bound
    top = np.sort(np.asarray(q[0], dtype=np.float64))
    print("%s: speed^2 largest %.6e, runner-up %.6e, bound %.3e" % (name, top[-1], top[-2], bound[0].max()))
    assert top[-1] - top[-2] > 1e3 * bound[0].max()
    if name == "rz10":
        assert tile.N > 256                                              # more than one workgroup of the flat branch
    for kind in ("domain", "azimuth"):
        val, idx = tile.extrema(prog, kind)
        tv, ti = X.scan(q, g.L, _nz(g), kind)
        o_ix = np.arange(16) if kind == "domain" else np.arange(16)[None, None, :]
        for w in (0, 1):
            b_at = bound[o_ix, idx[w]]
            worst = float(np.max(np.abs(val[w].astype(XP) - q[o_ix, idx[w]]) / b_at))
            print("%s %s %s: worst |val - twin at idx| / bound = %.3g" % (name, kind, "min max".split()[w], worst))
            assert (np.abs(val[w].astype(XP) - q[o_ix, idx[w]]) <= b_at).all()          # val within the bound of the twin's value there
            assert (np.abs(q[o_ix, idx[w]] - tv[w]) <= b_at + bound[o_ix, ti[w]]).all()  # and that point is an extremum up to the bound
            assert (np.abs(val[w].astype(XP) - tv[w]) <= b_at + bound[o_ix, ti[w]]).all()
        if kind == "domain":
            assert idx[1, 0] == ti[1, 0]
    tile.close()


@pytest.mark.parametrize("name", ["rl8", "rlz6_L16"])
def test_scan_ties_nan_zero(name):
    case, gp, g, tile, pts = _make(name)
    nz = _nz(g)
    vals = _wind(case, g, pts)
    start = np.concatenate([[0], np.cumsum(np.asarray(g.L) * nz)])
    ring_a, ring_b = 4, len(g.L) - 2
    lev = nz // 2
    pa1, pa2 = start[ring_a] + 1 * nz + lev, start[ring_a] + (g.L[ring_a] - 1) * nz + lev        # one ring, one level, two lambdas
    pb = start[ring_b] + 2 * nz + lev
    vals[[pa1, pa2, pb], 0] = 1.0e6                                       # three equal maxima of h
    vals[:, 5] = 0.0
    vals[3::2, 5] = -0.0                                                  # wb: +0.0 and -0.0 mixed
    tile.set_physical_values(vals)
    prog = [(0, 1.0, 0, [("h", "")]), (1, 1.0, 0, [("wb", "")]), (2, 1.0, 0, [("u", "")])]
    val, idx = tile.extrema(prog, "domain", "state")
    assert idx[1, 0] == pa1 and val[1, 0] == 1.0e6
    assert idx[0, 1] == 0 and idx[1, 1] == 0 and not np.signbit(val[0, 1]) and not np.signbit(val[1, 1])      # a tie: the lowest row, whose value is +0.0
    va, ia = tile.extrema(prog, "azimuth", "state")
    assert ia[1, ring_a, lev, 0] == pa1 and ia[1, ring_b, lev, 0] == pb
    assert (ia[:, :, :, 1] == (start[:-1, None] + np.arange(nz)[None, :])[None]).all()                        # every set of wb: its first lambda
    tv, ti = X.scan(np.ascontiguousarray(vals[:, [0, 5, 1]].T), g.L, nz, "azimuth")
    assert np.array_equal(ia, ti) and np.array_equal(va, tv)
    # a NaN in an outer ring
    pn1, pn2 = start[ring_b] + 3 * nz + lev, start[ring_b] + 1 * nz + lev
    vals[[pn1, pn2], 1] = np.nan
    tile.set_physical_values(vals)
    val2, idx2 = tile.extrema(prog, "domain", "state")
    assert np.isnan(val2[:, 2]).all() and (idx2[:, 2] == pn2).all()
    assert val2[:, :2].tobytes() == val[:, :2].tobytes() and idx2[:, :2].tobytes() == idx[:, :2].tobytes()
    va2, ia2 = tile.extrema(prog, "azimuth", "state")
    assert np.isnan(va2[:, ring_b, lev, 2]).all() and (ia2[:, ring_b, lev, 2] == pn2).all()
    keep = np.ones(va.shape, dtype=bool)
    keep[:, ring_b, lev, 2] = False
    assert np.array_equal(va2[keep], va[keep]) and np.array_equal(ia2[keep], ia[keep]) and not np.isnan(va2[keep]).any()
    tile.close()


def test_scan_fp32_storage():
    import scythe_jl_amd as S
    case = cases.rlz_hrbl(num_cells=6, zDim=32, ring_L=32)
    gp, mp = cases.hip_params(case, "f32")
    g = cases.oracle_grid(case)
    tile = S.Grid(gp, mp)
    pts = S.getGridpoints(tile)
    tile.set_physical_values(_wind(case, g, pts))
    tile.spectralTransform_()
    tile.splineTransform_()
    tile.tileTransform_()
    phys = tile.physical
    assert (phys[:, :, 1:] == phys[:, :, 1:].astype(np.float32)).all()
    val, idx = tile.extrema([(0, 1.0, 0, [("h", "r")]), (1, 1.0, 0, [("v", "")])])        # read in the stored types: exact
    tv, ti = X.scan(np.stack([phys[:, 0, 1], phys[:, 2, 0]]), g.L, g.zDim)
    assert np.array_equal(idx, ti) and np.array_equal(val, tv)
    prog = _programs(g)
    packed = S.pack_reduce_program(gp, prog)
    q, sabs, nt = X.integrand(phys, pts[:, 0], packed)
    bound = X.scan_bound(sabs, nt)
    val, idx = tile.extrema(prog)
    tv, ti = X.scan(q, g.L, g.zDim)
    o = np.arange(16)
    for w in (0, 1):
        assert (np.abs(val[w].astype(XP) - q[o, idx[w]]) <= bound[o, idx[w]]).all()
        assert (np.abs(q[o, idx[w]] - tv[w]) <= bound[o, idx[w]] + bound[o, ti[w]]).all()
    assert tile.kernel_bytes("k_extrema") == tile.N * (3 * 8 + 2 * 4 + 2 * 8)       # h u v ub vb values, h_r u_l as fp32
    tile.close()


def _raw_scan(tile, kind, source, coef, packed, n_out, val, idx, n_terms=None):
    from scythe_jl_amd import _lib as L
    packed = np.ascontiguousarray(packed, dtype=np.int32).reshape(-1, 11) if packed is not None else None
    coef = np.ascontiguousarray(coef, dtype=np.float64) if coef is not None else None
    n = n_terms if n_terms is not None else len(packed)
    return tile._lib.sx_extrema(tile._h, kind, source, n, coef.ctypes.data_as(L.P_D) if coef is not None else None,
                                packed.ctypes.data_as(L.P_I32) if packed is not None else None, n_out,
                                val.ctypes.data_as(L.P_D) if val is not None else None, idx.ctypes.data_as(L.P_I64) if idx is not None else None)


def _term(out=0, p=0, factors=()):
    return [out, p, len(factors)] + [f[0] for f in factors] + [0] * (4 - len(factors)) + [f[1] for f in factors] + [0] * (4 - len(factors))


def test_scan_side_effects_and_refusals():
    case, gp, g, tile, pts = _filled("rl8")
    state0, phys0 = tile.get_state(), tile.physical
    tile.enable_timers(True)
    tile.reset_timers()
    tile.extrema([(0, 0.5, 0, [("ub", ""), ("ub", "")]), (0, 0.5, 0, [("vb", ""), ("vb", "r")])], "azimuth")
    tm = tile.timers()
    assert tm["k_extrema"][1] == 1 and tm["k_extrema"][0] > 0 and tm["k_extrema_final"][1] == 1
    assert tile.kernel_bytes("k_extrema") == 3 * tile.N * 8 > 0
    tile.extrema([(0, 1.0, 0, [("h", "")])], "domain", "state")
    assert tile.kernel_bytes("k_extrema") == tile.N * 8
    assert tile.get_state().tobytes() == state0.tobytes() and tile.physical.tobytes() == phys0.tobytes()
    # every refusal of sx_reduce (tests/test_gpu_reduce.py::test_refusals' list), with val / idx untouched
    lib = tile._lib
    ok = _term(0, -1, [(1, 0), (6, 4)])
    nf5, nfm = _term(0, 0, [(1, 0)]), _term(0, 0, [])
    nf5[2], nfm[2] = 5, -1
    bad = [("out below", 0, 0, [1.0], [_term(-1, 0, [(1, 0)])], 1), ("out at n_out", 0, 0, [1.0], [_term(1, 0, [(1, 0)])], 1),
           ("p above", 0, 0, [1.0], [_term(0, 3, [(1, 0)])], 1), ("p below", 0, 0, [1.0], [_term(0, -3, [(1, 0)])], 1),
           ("var 0", 0, 0, [1.0], [_term(0, 0, [(0, 0)])], 1), ("var above", 0, 0, [1.0], [_term(0, 0, [(7, 0)])], 1),
           ("slot below", 0, 0, [1.0], [_term(0, 0, [(1, -1)])], 1), ("slot above", 0, 0, [1.0], [_term(0, 0, [(1, 5)])], 1),
           ("n_factors above", 0, 0, [1.0], [nf5], 1), ("n_factors below", 0, 0, [1.0], [nfm], 1),
           ("state slot", 0, 1, [1.0], [_term(0, 0, [(1, 1)])], 1), ("n_terms above", 0, 0, [1.0] * 65, [ok] * 65, 1),
           ("n_out above", 0, 0, [1.0], [ok], 17), ("kind", 2, 0, [1.0], [ok], 1), ("source", 0, 2, [1.0], [ok], 1),
           ("17 planes", 0, 0, [1.0] * 5, [_term(0, 0, [(v, s) for v, s in [(1 + i // 5, i % 5) for i in range(4 * k, min(4 * k + 4, 17))]])
                                           for k in range(5)], 1)]
    n_big = 2 * 24 * 17
    for kind in (0, 1):
        for what, k, source, coef, packed, n_out in bad:
            val, idx = np.full(n_big, -7.25), np.full(n_big, -7, dtype=np.int64)
            assert _raw_scan(tile, k if what == "kind" else kind, source, coef, packed, n_out, val, idx) != 0, what
            assert lib.sx_last_error().decode(), what
            assert (val == -7.25).all() and (idx == -7).all(), what
        val, idx = np.full(n_big, -7.25), np.full(n_big, -7, dtype=np.int64)
        assert _raw_scan(tile, kind, 0, None, [ok], 1, val, idx) != 0 and (val == -7.25).all() and (idx == -7).all()        # null coef
        assert _raw_scan(tile, kind, 0, [1.0], None, 1, val, idx, n_terms=1) != 0 and (val == -7.25).all()
        assert _raw_scan(tile, kind, 0, [1.0], [ok], 1, None, idx) != 0 and (idx == -7).all()
        assert _raw_scan(tile, kind, 0, [1.0], [ok], 1, val, None) != 0 and (val == -7.25).all()
        assert _raw_scan(tile, kind, 0, None, None, 0, None, None, n_terms=0) == 0                                          # nothing asked
        assert _raw_scan(tile, kind, 0, [1.0], [ok], 1, val, idx) == 0 and val[0] != -7.25 and idx[0] >= 0
    tile.close()


def test_scan_tiles_and_model_run():
    """three tiles: every tile's rows are its own gridpoints; ModelRun.extrema folds them into rows of ModelRun.gridpoints()"""
    case = cases.rl_slab(num_cells=9)
    hip = cases.HipModel(case, num_tiles=3, exchange="gather", impl="lib")
    for _ in range(2):
        hip.step()
    prog = [(0, 1.0, 0, [("u", ""), ("u", "")]), (0, 1.0, 0, [("v", ""), ("v", "")]), (1, 1.0, 0, [("h", "")])]
    val, idx = hip.run.extrema(prog, "domain", "state")
    allv = np.concatenate([t.var_np1 for t in hip.run._tiles_in_order()], axis=0)
    q = np.stack([allv[:, 1] * allv[:, 1] + allv[:, 2] * allv[:, 2], 0.0 + allv[:, 0]])
    assert len(hip.run.gridpoints()) == len(allv)
    for o in range(2):
        assert val[0, o] == q[o].min() and val[1, o] == q[o].max()
        assert idx[0, o] == int(np.argmin(q[o])) and idx[1, o] == int(np.argmax(q[o]))
    va, ia = hip.run.extrema(prog, "azimuth", "state")
    assert va.shape == (2, 27, 1, 2) and np.array_equal(va[:, :, 0, 1], q[1][ia[:, :, 0, 1]])
    hip.run.close()


# ----------------------------------------------------------------------------- the refinement
def _bump(name, var, centre, width, zc=None, zw=None, sign=1.0, maker_kw=None, pole_bc=False):
    """the tile with A = the transform of a Gaussian bump in variable var: centre = r (R / RZ) or (r, lambda) (RL / RLZ).
    pole_bc: h with the conditions of a scalar that is smooth at the pole - zero slope for k = 0, zero value for k >= 1 (the slab
    case gives h zero slope for every k, which leaves its k >= 1 parts finite at r = 0: a function with no Hessian there)"""
    import scythe_jl_amd as S
    if pole_bc:
        case = getattr(cases, CASES[name][0])(**CASES[name][1])
        case["grid"] = dict(case["grid"], BCL=dict(case["grid"]["BCL"], h="R1T0"), BCL_k0={"h": "R1T1"})
        maker_kw = {}
    elif maker_kw is not None:
        case = cases.r_bcs(**maker_kw)
    if maker_kw is not None:
        gp, mp = cases.hip_params(case)
        g = cases.oracle_grid(case)
        tile = S.Grid(gp, mp)
        pts = S.getGridpoints(tile)
        pts = pts.reshape(len(pts), -1)
    else:
        case, gp, g, tile, pts = _make(name)
    if g.has_l:
        X0, Y0 = centre[0] * np.cos(centre[1]), centre[0] * np.sin(centre[1])
        d2 = (pts[:, 0] * np.cos(pts[:, 1]) - X0) ** 2 + (pts[:, 0] * np.sin(pts[:, 1]) - Y0) ** 2
    else:
        d2 = (pts[:, 0] - centre) ** 2
    b = np.exp(-d2 / width ** 2)
    if zc is not None:
        b = b * np.exp(-((pts[:, -1] - zc) / zw) ** 2)
    vals = np.zeros((tile.N, tile.V))
    vals[:, var - 1] = sign * b
    tile.set_physical_values(vals)
    tile.spectralTransform_()
    tile.splineTransform_()
    return gp, g, tile, pts, np.array(tile.patchSpectral)


def _scaled(g, p):
    """a position as scaled Cartesian coordinates: (X, Y, z) / (DX, DX, zmax - zmin)"""
    p = np.asarray(p, dtype=XP)
    out = [p[0] * np.cos(p[1]) / XP(g.DX), p[0] * np.sin(p[1]) / XP(g.DX)] if g.has_l else [p[0] / XP(g.DX)]
    if g.has_z:
        out.append(p[-1] / XP(g.zmax - g.zmin))
    return np.array(out, dtype=XP)


def _position_bound(g, A, var, twin, free, tol):
    """(gradient rounding bound) / (smallest |eigenvalue| of the reduced Hessian) + tol, both from the twin, in the scaled coordinates"""
    d, S_, B = X.derivatives(g, A, var, twin.pos, xp=True, with_bound=True)
    r = float(twin.pos[0])
    Lz = (g.zmax - g.zmin) if g.has_z else 1.0
    if g.has_l and "r" in free and "l" in free:
        gr, H = X.cartesian(d, r, twin.pos[1], XP)
        gb = np.array([B[1] + B[2] / r, B[1] + B[2] / r, B[3]])
        sc = np.array([g.DX, g.DX, Lz])
    else:
        H = np.array([[d[4], d[5], d[6]], [d[5], d[7], d[8]], [d[6], d[8], d[9]]], dtype=XP)
        gb = np.array([B[1], B[2], B[3]])
        sc = np.array([g.DX, g.DX / max(r, 1e-300) if g.has_l else 1.0, Lz])
    act = [i for i, c in enumerate("rlz") if c in free]
    Hs = np.asarray(H, dtype=np.float64)[np.ix_(act, act)] * np.outer(sc[act], sc[act])
    lam_min = np.abs(np.linalg.eigvalsh(Hs)).min()
    return float(np.linalg.norm(gb[act] * sc[act]) / lam_min + tol)


REFINE = {
    "R off a node": dict(name="r24", var=1, centre=5.3 * 0.5 + 0.11, width=1.4, free="r"),
    "RL 0.3 DX from the pole": dict(name="rl8", var=1, centre=(0.3 * 3.75e4, 0.8), width=1.1e5, free="rl", pole_bc=True),
    "RL at 3.4 DX": dict(name="rl8", var=1, centre=(3.4 * 3.75e4, -2.2), width=9.0e4, free="rl"),
    "RLZ interior": dict(name="rlz6_L16", var=1, centre=(2.3 * 5.0e4, 1.1), width=1.2e5, zc=900.0, zw=700.0, free="rlz"),
    "RLZ lowest level": dict(name="rlz6", var=1, centre=(2.3 * 5.0e4, 1.1), width=1.2e5, zc=0.0, zw=900.0, free="rl"),
    "RZ interior": dict(name="rz10", var=1, centre=4.37e3, width=2.5e3, zc=4.2e3, zw=3.0e3, free="rz"),
    "RLZ interior, 256 lanes": dict(name="rlz12_wide", var=1, centre=(2.3 * 5.0e4, 1.1), width=1.2e5, zc=900.0, zw=700.0, free="rlz"),
}


@pytest.mark.parametrize("what", list(REFINE))
def test_refine_accuracy(what):
    c = dict(REFINE[what])
    free, name, var = c.pop("free"), c.pop("name"), c["var"]
    gp, g, tile, pts, A = _bump(name, **c)
    tol = 1e-9
    val, idx = tile.extrema([(0, 1.0, 0, [(var, "")])], "domain", "state")
    start = pts[idx[1, 0]]
    nz = _nz(g)
    on_end = g.has_z and idx[1, 0] % nz in (0, nz - 1)
    assert on_end == ("lowest" in what)
    res = tile.refine_extremum(var, start[None, :], "max", free, tol)
    import scythe_jl_amd as S
    twin = X.refine(g, A, var, start, 1, S.free_mask(gp, free), tol, 20, xp=True)
    assert res.status[0] == 0 and twin.status == 0, (res.status, twin.status)
    bound = _position_bound(g, A, var, twin, free, tol)
    err = float(np.linalg.norm(_scaled(g, res.pos[0]) - _scaled(g, twin.pos)))
    centre = c["centre"] if g.has_l else (c["centre"],)
    true = list(centre) + ([c["zc"] if "z" in free else res.pos[0, -1]] if g.has_z else [])
    dist = float(np.linalg.norm(_scaled(g, res.pos[0]) - _scaled(g, true)))
    print("%s: %d steps (twin %d), |pos - twin| = %.3e, bound %.3e (scaled units); distance to the Gaussian's centre %.3e DX"
          % (what, res.iters[0], twin.iters, err, bound, dist))
    assert err <= bound
    for cname, col in zip("rlz" if g.has_l and g.has_z else "rl" if g.has_l else "rz" if g.has_z else "r", range(pts.shape[1])):
        if cname not in free:
            assert res.pos[0, col] == start[col]                           # a frozen coordinate keeps its start value
    # value and gradient are those of evaluate at pos, each within the evaluation's own bound
    ev = tile.evaluate(res.pos, all_k=True)[0, var - 1]
    d, S_, B = X.derivatives(g, A, var, res.pos[0], xp=True, with_bound=True)
    sl = {s: i for i, s in enumerate(g.slots)}
    assert abs(res.value[0] - ev[sl["u"]]) <= 2 * B[0] and abs(XP(res.value[0]) - d[0]) <= B[0]
    for col, (s, m) in enumerate([("r", 1)] + ([("l", 2)] if g.has_l else []) + ([("z", 3)] if g.has_z else [])):
        assert abs(res.grad[0, col] - ev[sl[s]]) <= 2 * B[m], (what, s)
        assert abs(XP(res.grad[0, col]) - d[m]) <= B[m], (what, s)
    assert tile.kernel_bytes("k_refine") == 8 * 4 * g.b_zDim * (2 * g.kDim + 1 if g.has_l else 1) * (res.iters[0] + 1)
    tile.close()


def test_refine_statuses():
    import scythe_jl_amd as S
    # 3: an exactly axisymmetric bump on the pole
    gp, g, tile, pts, A = _bump("rl8", 1, (0.0, 0.0), 1.1e5)
    val, idx = tile.extrema([(0, 1.0, 0, [(1, "")])], "domain", "state")
    res = tile.refine_extremum(1, pts[idx[1, 0]][None, :], "max")
    assert res.status[0] == 3 and res.pos[0, 0] < 1e-6 * g.DX, (res.status, res.pos)
    res0 = tile.refine_extremum(1, [[0.0, 0.3]], "max")
    assert res0.status[0] == 3 and res0.iters[0] == 0 and res0.pos[0, 0] == 0.0
    # 5: one step, far from the root
    far = np.array([[1.6 * g.DX, 0.5]])
    res = tile.refine_extremum(1, far, "max", max_iter=1)
    assert res.status[0] == 5 and res.iters[0] == 1 and res.pos[0, 0] != far[0, 0]
    # free = "": value and gradient of evaluate, no step
    res = tile.refine_extremum(1, far, "max", free="")
    ev = tile.evaluate(far, all_k=True)[0, 0]
    d, S_, B = X.derivatives(g, A, 1, far[0], xp=True, with_bound=True)
    assert res.status[0] == 0 and res.iters[0] == 0 and res.pos.tobytes() == far.tobytes()
    assert abs(res.value[0] - ev[0]) <= 2 * B[0] and abs(res.grad[0, 0] - ev[1]) <= 2 * B[1] and abs(res.grad[0, 1] - ev[3]) <= 2 * B[2]
    tile.close()
    # 4: want = "max" at a minimum
    gp, g, tile, pts, A = _bump("rl8", 1, (3.4 * 3.75e4, -2.2), 9.0e4, sign=-1.0)
    val, idx = tile.extrema([(0, 1.0, 0, [(1, "")])], "domain", "state")
    start = pts[idx[0, 0]][None, :]
    res = tile.refine_extremum(1, start, "max")
    assert res.status[0] == 4 and res.iters[0] == 0 and res.pos.tobytes() == start.tobytes()
    assert tile.refine_extremum(1, start, "min").status[0] == 0 and tile.refine_extremum(1, start, "any").status[0] == 0
    tile.close()
    # 1: in the convex tail of a bump Newton (want = "any") walks outwards, a cell at a time, and crosses xmax
    gp, g, tile, pts, A = _bump(None, 1, 6.0, 3.0, maker_kw=dict(bcr="R0", num_cells=24))
    start = np.array([[g.xmax - 2.2 * g.DX]])
    res = tile.refine_extremum(1, start, "any")
    twin = X.refine(g, A, 1, start[0], 0, 1, 1e-9, 20, xp=True)
    print("leaving: status %d after %d steps at r = %.6f (twin: %d, %d, %.6f)" % (res.status[0], res.iters[0], res.pos[0, 0], twin.status, twin.iters, twin.pos[0]))
    assert twin.status == 1 and res.status[0] == 1 and res.iters[0] == twin.iters
    assert g.xmax - g.DX <= res.pos[0, 0] <= g.xmax and abs(res.pos[0, 0] - twin.pos[0]) <= 1e-9 * g.DX
    tile.close()


def test_refine_independence_and_side_effects():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    case = cases.rlz_hrbl(num_cells=6, zDim=10, ring_L=16)
    hip = cases.HipModel(case)
    for _ in range(3):
        hip.step()
    tile = hip.run.tiles[0]
    g = cases.oracle_grid(case)
    rng = np.random.default_rng(4)
    p = np.stack([rng.uniform(0.2, 5.5, 6) * g.DX, rng.uniform(-3, 3, 6), rng.uniform(100.0, 1900.0, 6)], axis=1)
    tile.set_parcels(p[:3], ("u", "v", None))
    tile.advance_parcels(2.0)
    par0 = [x.tobytes() for x in tile.parcels()] + [tile.get_parcel_state().tobytes()]
    state0 = tile.get_state()
    one = tile.refine_extremum("h", p[:1], "any")
    many = tile.refine_extremum("h", p[[4, 2, 0, 5, 1, 3]], "any")
    for a, b in zip(one, many):
        assert np.asarray(a)[0].tobytes() == np.asarray(b)[2].tobytes()
    again = tile.refine_extremum("h", p[:1], "any")
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(one, again))
    assert tile.get_state().tobytes() == state0.tobytes()
    assert [x.tobytes() for x in tile.parcels()] + [tile.get_parcel_state().tobytes()] == par0
    # refusals leave the outputs untouched
    lib = tile._lib

    def raw(var=1, want=1, mask=7, tol=1e-9, n=1, start=p[:1], null=None):
        s = np.asfortranarray(start)
        out = dict(pos=np.full(3 * max(n, 1), -7.25), value=np.full(max(n, 1), -7.25), grad=np.full(3 * max(n, 1), -7.25),
                   status=np.full(max(n, 1), -7, dtype=np.int32), iters=np.full(max(n, 1), -7, dtype=np.int32))
        ptr = {k: (None if k == null else v.ctypes.data_as(L.P_I32 if v.dtype == np.int32 else L.P_D)) for k, v in out.items()}
        rc = lib.sx_extremum_refine(tile._h, var, want, mask, tol, 0, n, None if null == "start" else s.ctypes.data_as(L.P_D), ptr["pos"],
                                    ptr["value"], ptr["grad"], ptr["status"], ptr["iters"])
        clean = all((v == (-7 if v.dtype == np.int32 else -7.25)).all() for v in out.values())
        return rc, clean
    assert raw() == (0, False)
    bad = [dict(var=0), dict(var=7), dict(want=2), dict(want=-2), dict(mask=8), dict(tol=float("nan")), dict(tol=float("inf")),
           dict(start=np.array([[float("nan"), 0.0, 500.0]])), dict(start=np.array([[3.1e5, 0.0, 500.0]])),
           dict(start=np.array([[1e5, 0.0, 2500.0]])), dict(start=np.array([[1e5, float("inf"), 500.0]])), dict(n=-1),
           dict(null="start"), dict(null="pos"), dict(null="value"), dict(null="grad"), dict(null="status"), dict(null="iters")]
    for kw in bad:
        rc, clean = raw(**kw)
        assert rc != 0 and clean and lib.sx_last_error().decode(), kw
    assert raw(n=0, null="start")[0] == 0
    hip.run.close()
    # a coordinate the geometry lacks; a two-tile handle
    case = cases.rl_slab(num_cells=8)
    hip2 = cases.HipModel(case, num_tiles=2, exchange="gather", impl="lib")
    hip2.step()
    with pytest.raises(S.ScytheHipError, match="one-tile"):
        hip2.run.tiles[0].refine_extremum("h", [[1.0e4, 0.0]], "max")
    with pytest.raises(S.ScytheHipError, match="vertical"):
        hip2.run.tiles[0].refine_extremum("h", [[1.0e4, 0.0]], "max", free=4)
    with pytest.raises(ValueError):
        hip2.run.locate("h")
    hip2.run.close()


def test_locate_and_radius_of_maximum():
    import scythe_jl_amd as S
    case = cases.rl_slab(num_cells=8)
    hip = cases.HipModel(case)
    for _ in range(3):
        hip.step()
    run, tile = hip.run, hip.run.tiles[0]
    pts = S.getGridpoints(tile)
    assert np.array_equal(run.gridpoints(), pts)
    # locate by hand: one domain scan of the state, then the refinement of that gridpoint
    for want, row in (("max", 1), ("min", 0)):
        val, idx = tile.extrema([(0, 1.0, 0, [("h", "")])], "domain", "state")
        hand = tile.refine_extremum("h", pts[idx[row, 0]][None, :], want, "rl")
        got = run.locate("h", want)
        assert got.pos.tobytes() == hand.pos[0].tobytes() and got.value == hand.value[0] and got.status == hand.status[0]
        grid = run.locate("h", want, refine=False)
        assert grid.pos.tobytes() == pts[idx[row, 0]].tobytes() and grid.value == val[row, 0] and grid.status == 0
        print("locate(h, %s): gridpoint %s -> %s, status %d" % (want, grid.pos, got.pos, got.status))
    # radius of maximum wind by hand
    val, idx = tile.extrema([(0, 1.0, 0, [("v", "")])], "azimuth", "state")
    ring = int(np.argmax(val[1, :, 0, 0]))
    start = pts[idx[1, ring, 0, 0]]
    hand = tile.refine_extremum("v", start[None, :], "max", "r")
    got = run.radius_of_maximum("v")
    assert got.pos.tobytes() == hand.pos[0].tobytes() and got.value == hand.value[0] and got.status == hand.status[0]
    assert got.pos[1] == start[1] and abs(got.pos[0] - start[0]) <= run.patch.xmax / run.patch.num_cells
    assert run.radius_of_maximum("v", level=0).pos.tobytes() == got.pos.tobytes()
    print("radius of maximum v: ring radius %.1f -> %.1f (status %d, value %.6f)" % (start[0], got.pos[0], got.status, got.value))
    hip.run.close()
