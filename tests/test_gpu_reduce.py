"""sx_reduce on the GPU against the longdouble twin of tests/reduce.py and against closed forms.

Every device number is held to its longdouble counterpart within tests/reduce.py::BOUND (32 ulp of S_abs = sum |w term|), a bound
derived from the count of roundings a term passes through, not from what the kernel gives.  The SX_GRAPH case of the read-only test
runs in a child process started with the switch in its environment (tests/reduce.py::read_only_in_child)."""
import ctypes as C

import numpy as np
import pytest

from tests import cases, linear_sw
from tests import evaluate as E
from tests import reduce as R

pytestmark = pytest.mark.gpu

XP = R.XP
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


@pytest.mark.parametrize("tiles", [1, 3])
@pytest.mark.parametrize("geom,ring_L", GEOMS)
def test_against_twin(geom, ring_L, tiles):
    import scythe_jl_amd as S
    case = _case(geom, ring_L)
    hip = cases.HipModel(case, num_tiles=tiles, exchange="gather", impl="lib" if tiles > 1 else "torch")
    for _ in range(3):
        hip.step()
    g = cases.oracle_grid(case)
    prog, prog_s = R.random_program(g, 11), R.random_program(g, 13, source="state")
    packed, packed_s = S.pack_reduce_program(hip.gp, prog), S.pack_reduce_program(hip.gp, prog_s)
    assert packed[2] == 5 and len(prog) == 12 and sorted(set(packed[1][:, 1])) == [-2, -1, 0, 1, 2]
    used = {(v, s) for v, s in S.reduce_planes(hip.gp, prog)}
    assert {s for _, s in used} == set(range(g.D))                   # every slot of the geometry
    for t, tile in zip(hip.run.tile_ids, hip.run.tiles):
        c0, n = hip.run.layout.cell0[t], hip.run.layout.ncells[t]
        pts = _points(tile)
        tile.tileTransform_()
        phys, np1 = tile.physical, tile.var_np1
        for kind in ("domain", "azimuth"):
            got = tile.reduce(prog, kind)
            truth, sabs = R.reduce(g, phys, pts, packed, kind, c0, n)
            assert got.shape == truth.shape and np.isfinite(got).all() and np.abs(got).max() > 0
            R.check(got, truth, sabs, "%s ring_L=%s tiles=%d tile %d %s physical" % (geom, ring_L, tiles, t, kind))
            assert tile.reduce(prog, kind).tobytes() == got.tobytes()
            got = tile.reduce(prog_s, kind, "state")
            truth, sabs = R.reduce(g, np1, pts, packed_s, kind, c0, n)
            R.check(got, truth, sabs, "%s ring_L=%s tiles=%d tile %d %s state" % (geom, ring_L, tiles, t, kind))
            assert tile.reduce(prog_s, kind, "state").tobytes() == got.tobytes()
    hip.run.close()


def _poly_integral(coefs, a, b, shift=0):
    """integral over [a, b] of x^shift sum_k coefs[k] x^k, in longdouble"""
    return sum(XP(c) * (XP(b) ** (k + shift + 1) - XP(a) ** (k + shift + 1)) / XP(k + shift + 1) for k, c in enumerate(coefs))


def _analytic(geom, zpow):
    """the tile, its points and u = (1 + (r / R)^2) (1 + z / H)^zpow in variable 1, formed in longdouble and rounded once"""
    import scythe_jl_amd as S
    case = _case(geom)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    assert g.xmin == 0.0 and g.zmin == 0.0
    tile = S.Grid(gp, mp)
    pts = _points(tile)
    s, t = pts[:, 0].astype(XP) / XP(g.xmax), pts[:, -1].astype(XP) / XP(g.zmax)
    u = ((1 + s * s) * (1 + t) ** zpow).astype(np.float64)
    vals = np.zeros((tile.N, tile.V))
    vals[:, 0] = u
    tile.set_physical_values(vals)
    return tile, gp, g, pts, vals


def _closed_forms(g, zpow):
    """(int u, int u^2, int u_r) over the patch: radial and vertical factors in s = r / R, t = z / H"""
    j = 1 if g.has_l else 0
    Rm, H = XP(g.xmax), XP(g.zmax)
    az = XP(2) * R.PI_X if g.has_l else XP(1)
    rad1 = _poly_integral([1, 0, 1], 0, 1, j) * Rm ** (j + 1)                     # (1 + s^2) J
    rad2 = _poly_integral([1, 0, 2, 0, 1], 0, 1, j) * Rm ** (j + 1)               # (1 + s^2)^2 J
    radr = _poly_integral([0, 2], 0, 1, j) * Rm ** j                              # d/dr (1 + s^2) = 2 s / R
    ver1 = (XP(2) ** (zpow + 1) - 1) / XP(zpow + 1) * H
    ver2 = (XP(2) ** (2 * zpow + 1) - 1) / XP(2 * zpow + 1) * H
    return az * rad1 * ver1, az * rad2 * ver2, az * radr * ver1


@pytest.mark.parametrize("geom", ["RLZ", "RZ"])
def test_analytic_state(geom):
    """degree 5 in r with the area element and 4 in z: inside both exactness limits, only rounding is left"""
    import scythe_jl_amd as S
    tile, gp, g, pts, vals = _analytic(geom, 2)
    prog = [(0, 1.0, 0, [(1, "")]), (1, 1.0, 0, [(1, ""), (1, "")])]
    got = tile.reduce(prog, "domain", "state")
    _, sabs = R.reduce(g, vals, pts, S.pack_reduce_program(gp, prog))
    i1, i2, _ = _closed_forms(g, 2)
    R.check(got, np.array([i1, i2]), sabs, "%s analytic state" % geom)
    tile.close()


@pytest.mark.parametrize("geom", ["RLZ", "RZ"])
def test_analytic_physical(geom):
    """quadratic in r, linear in z, axisymmetric: in the spline / Chebyshev space, and the l_q filter does not touch it; the
    transforms' rounding enters as well as the reduction's: the project's 1e-10 field bar, relative"""
    tile, gp, g, pts, vals = _analytic(geom, 1)
    tile.spectralTransform_()
    tile.splineTransform_()
    tile.tileTransform_()
    got = tile.reduce([(0, 1.0, 0, [(1, "")]), (1, 1.0, 0, [(1, ""), (1, "")]), (2, 1.0, 0, [(1, "r")])])
    want = _closed_forms(g, 1)
    rel = [float(abs(XP(a) - b) / abs(b)) for a, b in zip(got, want)]
    print("%s analytic physical: relative errors of int u, int u^2, int u_r: %s" % (geom, rel))
    assert max(rel) <= 1e-10, rel
    tile.close()


def test_azimuthal_mean_is_wavenumber_zero():
    import scythe_jl_amd as S
    case = cases.rl_slab(num_cells=9)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    A = np.random.default_rng(19).standard_normal((g.S_patch(), g.V))
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(A)
    tile.tileTransform_()
    mean = tile.reduce([(0, 1.0, 0, [("h", "")])], "azimuth")
    assert mean.shape == (g.rDim, 1, 1)
    A0 = A.copy()
    a0 = A0.reshape(g.b_zDim, g.K2, g.b_rDim, g.V)       # [zm, blk, node, v]: the reference layout, the node fastest
    a0[:, 1:] = 0.0
    rings = np.unique(_points(tile)[:, 0])
    assert len(rings) == g.rDim
    truth = E.evaluate(g, A0, np.stack([rings, np.zeros(g.rDim)], axis=1), xp=True)[:, 0, 0]
    hmax = np.abs(tile.physical[:, 0, 0]).max()
    err = float(np.abs(mean[:, 0, 0].astype(XP) - truth).max() / hmax)
    print("azimuthal mean against the k = 0 block: %.3e of max|h|" % err)
    assert np.abs(truth).max() > 0 and err <= 1e-10
    tile.close()


def test_storage_modes():
    """A value-slot-only program.  From var_np1 (always fp64): identical bytes in all three modes.  From `physical`: storage "f32"
    keeps the value slot and the whole A -> values path fp64, so its value slot and the results are bytewise those of "f64" - which
    shows that the fp32-typed kernel reads slot 0 as fp64; storage "f32x" rounds the transform intermediates to fp32, so its value
    slot is another array: there the results are held to the twin on that mode's own tile.physical.  A program with derivative slots:
    each mode against the twin on its own array."""
    import scythe_jl_amd as S
    case = cases.rlz_hrbl(num_cells=6, zDim=32, ring_L=32)
    g = cases.oracle_grid(case)
    A = np.random.default_rng(41).standard_normal((g.S_patch(), g.V))
    values = np.random.default_rng(42).standard_normal((g.tile_npoints(0, g.nc), g.V))
    val_prog = [(0, 1.0, 1, [("h", ""), ("ub", "")]), (1, -0.5, 0, [("vb", ""), ("vb", ""), ("u", "")]), (2, 1.0, 2, [])]
    der_prog = R.random_program(g, 29)
    res_state, res_phys, planes = [], [], []
    for storage in ("f64", "f32", "f32x"):
        gp, mp = cases.hip_params(case, storage)
        tile = S.Grid(gp, mp)
        tile.set_physical_values(values)
        tile.set_patch_spectral_a(A)
        tile.tileTransform_()
        pts, phys = _points(tile), tile.physical
        res_state.append(tile.reduce(val_prog, "domain", "state").tobytes() + tile.reduce(val_prog, "azimuth", "state").tobytes())
        res_phys.append(tile.reduce(val_prog, "domain").tobytes() + tile.reduce(val_prog, "azimuth").tobytes())
        planes.append(phys[:, :, 0].tobytes())
        if storage != "f64":
            assert (phys[:, :, 1:] == phys[:, :, 1:].astype(np.float32)).all()        # the derivative slots are fp32 numbers
        for kind in ("domain", "azimuth"):
            for name, prog in (("value slots", val_prog), ("derivative slots", der_prog)):
                got = tile.reduce(prog, kind)
                truth, sabs = R.reduce(g, phys, pts, S.pack_reduce_program(gp, prog), kind)
                assert np.abs(got).max() > 0
                R.check(got, truth, sabs, "storage %s %s %s" % (storage, kind, name))
        tile.close()
    assert res_state[0] == res_state[1] == res_state[2]
    assert planes[0] == planes[1]
    assert res_phys[0] == res_phys[1]


@pytest.mark.parametrize("switch,maker,kw", [("plain", "rlz_hrbl", {"num_cells": 6, "zDim": 10, "ring_L": 16}),
                                             ("SX_GRAPH", "rl_slab", {"num_cells": 8})])
def test_read_only(switch, maker, kw, tmp_path):
    r = R.read_only_job(maker, kw) if switch == "plain" else R.read_only_in_child(tmp_path, maker, kw, {switch: "1"})
    assert np.isfinite(r["dom"]).all() and np.abs(r["dom"]).max() > 0 and np.isfinite(r["azi"]).all()
    assert r["state0"].tobytes() == r["state1"].tobytes()
    assert r["np10"].tobytes() == r["np11"].tobytes()
    assert r["phys0"].tobytes() == r["phys1"].tobytes()
    assert r["end0"].tobytes() == r["end1"].tobytes() and np.abs(r["end0"]).max() > 0


def _raw(tile, kind, source, coef, packed, n_out, out, n_terms=None):
    from scythe_jl_amd import _lib as L
    packed = np.ascontiguousarray(packed, dtype=np.int32).reshape(-1, 11) if packed is not None else None
    coef = np.ascontiguousarray(coef, dtype=np.float64) if coef is not None else None
    n = n_terms if n_terms is not None else len(packed)
    return tile._lib.sx_reduce(tile._h, kind, source, n, coef.ctypes.data_as(L.P_D) if coef is not None else None,
                               packed.ctypes.data_as(L.P_I32) if packed is not None else None, n_out,
                               out.ctypes.data_as(L.P_D) if out is not None else None)


def _term(out=0, p=0, factors=()):
    return [out, p, len(factors)] + [f[0] for f in factors] + [0] * (4 - len(factors)) + [f[1] for f in factors] + [0] * (4 - len(factors))


def test_refusals():
    import scythe_jl_amd as S
    case = cases.rl_slab(num_cells=9)                      # 6 variables, 5 slots
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp)
    tile.tileTransform_()
    lib = tile._lib
    ok = _term(0, -1, [(1, 0), (6, 4)])                    # p = -1 is accepted on a polar grid
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
    for kind in (0, 1):
        for what, k, source, coef, packed, n_out in bad:
            out = np.full(27 * 16, -7.25)
            assert _raw(tile, k if what == "kind" else kind, source, coef, packed, n_out, out) != 0, what
            assert lib.sx_last_error().decode(), what
            assert (out == -7.25).all(), what
        out = np.full(27 * 16, -7.25)
        assert _raw(tile, kind, 0, None, [ok], 1, out) != 0 and lib.sx_last_error().decode() and (out == -7.25).all()       # null coef
        assert _raw(tile, kind, 0, [1.0], None, 1, out, n_terms=1) != 0 and lib.sx_last_error().decode() and (out == -7.25).all()
        assert _raw(tile, kind, 0, [1.0], [ok], 1, None) != 0 and lib.sx_last_error().decode()                              # null out
        assert _raw(tile, kind, 0, None, None, 0, None, n_terms=0) == 0                                                      # nothing asked
        assert _raw(tile, kind, 0, [1.0], [ok], 1, out) == 0 and np.isfinite(out[0]) and out[0] != -7.25
    tile.close()
    # p < 0 with a gridpoint at r == 0: an R grid with an odd cell count centred on 0
    g0 = S.GridParameters(geometry="R", xmin=-4.5, xmax=4.5, num_cells=9, vars={"u": 1})
    t0 = S.Grid(g0)
    assert 0.0 in S.getGridpoints(t0)
    t0.set_physical_values(np.ones((t0.N, 1)))
    out = np.full(27, -7.25)
    for source in (0, 1):
        assert _raw(t0, 0, source, [1.0], [_term(0, -1, [(1, 0)])], 1, out) != 0 and "r == 0" in t0._lib.sx_last_error().decode()
        assert (out == -7.25).all()
    assert _raw(t0, 0, 1, [1.0], [_term(0, 2, [(1, 0)])], 1, out) == 0
    _within = abs(XP(out[0]) - XP(2) * XP(4.5) ** 3 / 3)
    assert _within <= XP(R.BOUND) * XP(out[0])              # int r^2 over [-4.5, 4.5]; S_abs is the integral itself (r^2 >= 0)
    t0.close()


def test_model_run():
    import scythe_jl_amd as S
    case = linear_sw.rl_case(num_cells=9)
    hip = cases.HipModel(case, num_tiles=3, exchange="gather", impl="lib")
    for _ in range(3):
        hip.step()
    g = cases.oracle_grid(case)
    prog = S.invariants(hip.mp)
    got = hip.run.integrate(prog)
    truth, sabs = np.zeros(2, dtype=XP), np.zeros(2, dtype=XP)
    for t, tile in zip(hip.run.tile_ids, hip.run.tiles):
        a, b = R.reduce(g, tile.physical, _points(tile), S.pack_reduce_program(hip.gp, prog), "domain", hip.run.layout.cell0[t],
                        hip.run.layout.ncells[t])
        truth, sabs = truth + a, sabs + b
    assert got.shape == (2,) and (got > 0).all()
    R.check(got, truth, sabs, "ModelRun.integrate(invariants)")
    state = hip.run.integrate([(0, 1.0, 0, [("h", "")])], source="state")
    assert abs(state[0] - got[0]) <= 1e-2 * abs(got[0])            # sanity: var_np1 holds the h that physical[:, :, 0] holds after the spline filter
    r, z, mean = hip.run.azimuthal_mean([(0, 1.0, 0, [("u", ""), ("v", "")]), (1, 1.0, 0, [("h", "")])])
    assert r.shape == (3 * g.nc,) and (np.diff(r) > 0).all() and z.shape == (1,) and mean.shape == (3 * g.nc, 1, 2)
    assert np.isfinite(mean).all() and np.abs(mean).max() > 0
    hip.run.close()


def test_timer_and_bytes():
    import scythe_jl_amd as S
    case = cases.rlz_hrbl(num_cells=6, zDim=10, ring_L=16)
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp)
    tile.tileTransform_()
    tile.enable_timers(True)
    tile.reset_timers()
    tile.reduce([(0, 0.5, 0, [("ub", ""), ("ub", "")]), (0, 0.5, 0, [("vb", ""), ("vb", "r")])])
    tm = tile.timers()
    assert tm["k_reduce"][1] == 1 and tm["k_reduce"][0] > 0 and tm["k_reduce_final"][1] == 1
    assert tile.kernel_bytes("k_reduce") == 3 * tile.N * 8
    tile.close()
