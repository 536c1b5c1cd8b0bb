"""sx_evaluate on the GPU against the twin of tests/evaluate.py (longdouble: the arbiter) and against tileTransform!.

The SX_GRAPH, SX_OVERLAP and SX_DEFER_DIAG cases of the read-only test run in a child process started with the switch in its
environment (tests/evaluate.py::read_only_in_child, the pattern of tests/child_run.py)."""
import os

import numpy as np
import pytest

from tests import cases
from tests import evaluate as E

pytestmark = pytest.mark.gpu

GEOMS = [("R", None), ("RZ", None), ("RL", None), ("RL", 16), ("RLZ", None), ("RLZ", 16)]


def _case(geom, ring_L=None, big=False):
    if geom == "R":
        return cases.r_bcs(num_cells=12)
    if geom == "RZ":
        return cases.rz_advection(num_cells=9, zDim=12)
    if geom == "RL":
        return cases.rl_slab(num_cells=9, ring_L=ring_L)
    return cases.rlz_hrbl(num_cells=9, zDim=10, ring_L=ring_L)


def _bounds(new, ref, floor=1e-13):
    """slot d passes when new[d] <= max(10 ref[d], floor): 10 x the measured error of the comparison path (cases.check_full's rule)"""
    return np.maximum(10.0 * np.asarray(ref), floor)


@pytest.mark.parametrize("tiles", [1, 3])
@pytest.mark.parametrize("geom,ring_L", GEOMS)
def test_own_gridpoints(geom, ring_L, tiles):
    import scythe_jl_amd as S
    case = _case(geom, ring_L)
    hip = cases.HipModel(case, num_tiles=tiles, exchange="gather", impl="lib" if tiles > 1 else "torch")
    for _ in range(3):
        hip.step()
    g = cases.oracle_grid(case)
    for t, tile in zip(hip.run.tile_ids, hip.run.tiles):
        pts = S.getGridpoints(tile)
        pts = pts.reshape(len(pts), -1)
        new = tile.evaluate(pts)
        tile.tileTransform_()
        old = tile.physical
        A = tile.patchSpectral
        c0, n = hip.run.layout.cell0[t], hip.run.layout.ncells[t]
        val = max(np.abs(new[:, v, 0] - old[:, v, 0]).max() / max(np.abs(old[:, v, 0]).max(), 1e-300) for v in range(g.V))
        truth = E.evaluate(g, A, pts, cell0=c0, ncells=n, xp=True)           # every gridpoint of the tile
        e_new, e_old = E.slot_errors(new, truth), E.slot_errors(old, truth)
        print("%s ring_L=%s tiles=%d tile %d: value new vs old %.2e; err new %s; err old %s; ratio %s"
              % (geom, ring_L, tiles, t, val, e_new, e_old, e_new / np.maximum(e_old, 1e-300)))
        assert val <= 1e-10, val
        assert (e_new <= _bounds(e_new, e_old)).all(), (e_new, e_old)
    hip.run.close()


@pytest.mark.parametrize("geom,ring_L", GEOMS)
def test_scattered_points_random_coefficients(geom, ring_L):
    import scythe_jl_amd as S
    case = _case(geom, ring_L)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    A = np.random.default_rng(17).standard_normal((g.S_patch(), g.V))
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(A)
    pts = E.scattered_points(g, 2000, seed=23)
    for all_k in (False, True):
        new = tile.evaluate(pts, all_k)
        assert new.shape == (2000, g.V, g.D) and np.isfinite(new).all()
        truth = E.evaluate(g, A, pts, all_k, xp=True)
        f64 = E.evaluate(g, A, pts, all_k, xp=False)
        e_new, e_f64 = E.slot_errors(new, truth), E.slot_errors(f64, truth)
        print("%s ring_L=%s all_k=%s: err new %s; err float64 twin %s" % (geom, ring_L, all_k, e_new, e_f64))
        assert e_new[0] <= 1e-10
        assert (e_new[1:] <= _bounds(e_new[1:], e_f64[1:])).all(), (e_new, e_f64)
    tile.close()


def test_truncation():
    import scythe_jl_amd as S
    case = cases.rl_advection(num_cells=8)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    A = np.zeros((g.S_patch(), g.V))
    a = A.reshape(1, g.K2, g.b_rDim, g.V)
    a[0, 2 * 12 - 1:2 * 12 + 1] = np.random.default_rng(5).standard_normal((2, g.b_rDim, g.V))       # Re and Im of k = 12 only
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(A)
    rad = g.gridpoints()[:, 0]
    r5 = 0.5 * (np.unique(rad)[4] + np.unique(rad)[5])            # between rings 5 and 6: kcap = 5
    assert E.kcap_of(g, r5) == 5
    lam = np.linspace(-3.0, 9.0, 40)
    p5 = np.stack([np.full(40, r5), lam], axis=1)
    ring = tile.evaluate(p5)
    allk = tile.evaluate(p5, all_k=True)
    assert (ring == 0.0).all()
    truth = E.evaluate(g, A, p5, True, xp=True)
    e = E.slot_errors(allk, truth)
    assert np.abs(allk[:, :, 0]).max() > 0 and e[0] <= 1e-10, e
    f64 = E.slot_errors(E.evaluate(g, A, p5, True, xp=False), truth)
    assert (e[1:] <= _bounds(e[1:], f64[1:])).all(), (e, f64)
    r20 = 0.5 * (np.unique(rad)[19] + np.unique(rad)[20])
    assert E.kcap_of(g, r20) >= 12
    p20 = np.stack([np.full(40, r20), lam], axis=1)
    assert tile.evaluate(p20).tobytes() == tile.evaluate(p20, all_k=True).tobytes()
    assert np.abs(tile.evaluate(p20)).max() > 0
    tile.close()


# the shape on which sx_advance's second stream is live: the node-space inverse needs 32 / 64 / 128 levels on uniform power-of-two rings
HRBL_MFMA = ("rlz_hrbl", {"num_cells": 8, "zDim": 32, "ring_L": 32})


@pytest.mark.parametrize("switch,maker,kw", [("plain", "rlz_hrbl", {"num_cells": 6, "zDim": 10, "ring_L": 16}),
                                             ("SX_GRAPH", "rl_slab", {"num_cells": 8}), ("SX_OVERLAP",) + HRBL_MFMA,
                                             ("SX_DEFER_DIAG",) + HRBL_MFMA])
def test_read_only(switch, maker, kw, tmp_path):
    r = E.read_only_job(maker, kw) if switch == "plain" else E.read_only_in_child(tmp_path, maker, kw, {switch: "1"})
    assert np.isfinite(r["got"]).all() and np.abs(r["got"]).max() > 0
    assert r["state0"].tobytes() == r["state1"].tobytes()
    assert r["np10"].tobytes() == r["np11"].tobytes()
    kernels = set(r["kernels"].tolist())
    if switch == "SX_OVERLAP":
        # the handle splits the tile into the ring-wise inner chain and the node-space outer chain (node_mode, R_in > 0): with
        # SX_OVERLAP=1 that is the condition under which launch_inverse_and_physics puts the inner chain on the second stream
        assert {"k_phys_hrbl_inner", "k_node_fft"} <= kernels, kernels
    if switch == "SX_DEFER_DIAG":
        assert r["w_max"] > 0 and r["w_err"] <= 1e-10, (r["w_max"], r["w_err"])


def test_storage_modes():
    import scythe_jl_amd as S
    case = cases.rlz_hrbl(num_cells=6, zDim=32, ring_L=32)
    g = cases.oracle_grid(case)
    A = np.random.default_rng(41).standard_normal((g.S_patch(), g.V))
    pts = E.scattered_points(g, 500, seed=43)
    res = []
    for storage in ("f64", "f32", "f32x"):
        gp, mp = cases.hip_params(case, storage)
        tile = S.Grid(gp, mp)
        tile.set_patch_spectral_a(A)
        res.append(tile.evaluate(pts))
        tile.close()
    assert np.abs(res[0]).max() > 0
    assert res[0].tobytes() == res[1].tobytes() == res[2].tobytes()


def test_chunking():
    import scythe_jl_amd as S
    case = cases.rlz_advection(num_cells=4, zDim=9, ring_L=8)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(np.random.default_rng(7).standard_normal((g.S_patch(), g.V)))
    rng = np.random.default_rng(9)
    n = 150000
    lev = g.cheb(g.names[0]).z
    pts = np.stack([rng.uniform(g.xmin, g.xmax, n), rng.uniform(-7.0, 13.0, n),
                    np.concatenate([lev, np.linspace(g.zmin, g.zmax, 40)])[rng.integers(0, len(lev) + 40, n)]], axis=1)
    whole = tile.evaluate(pts)
    parts = np.concatenate([tile.evaluate(pts[i:i + 1000]) for i in range(0, n, 1000)], axis=0)
    assert np.isfinite(whole).all() and np.abs(whole).max() > 0
    assert whole.tobytes() == np.asfortranarray(parts).tobytes()
    assert tile.evaluate(np.zeros((0, 3))).shape == (0, g.V, g.D)        # n_points == 0 succeeds
    tile.close()


def test_refusals():
    import ctypes as C
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    case = cases.rlz_advection(num_cells=9, zDim=9, ring_L=8)
    hip = cases.HipModel(case, num_tiles=3, exchange="gather", impl="lib")
    hip.step()
    g = cases.oracle_grid(case)
    tile = hip.run.tiles[1]
    lo, hi = E.tile_range(g, hip.run.layout.cell0[1], hip.run.layout.ncells[1])
    good = np.asfortranarray([[lo, 0.3, 1.0], [0.5 * (lo + hi), -2.0, g.zmax], [hi, 8.0, g.zmin]])
    lib = S.load()

    def call(points, out):
        p = np.asfortranarray(points)
        return lib.sx_evaluate(tile._h, p.ctypes.data_as(L.P_D), len(p), 0, out.ctypes.data_as(L.P_D) if out is not None else None)

    bads = []
    for row, col, val in ((0, 0, lo - 1e-6), (2, 0, hi + 1e-6), (1, 2, g.zmax + 1e-6), (1, 2, g.zmin - 1e-6), (1, 0, np.nan),
                          (2, 1, np.inf), (0, 2, np.nan)):
        b = good.copy()
        b[row, col] = val
        bads.append(b)
    for b in bads:
        out = np.full((3, g.V, g.D), -7.25, order="F")
        assert call(b, out) != 0
        assert lib.sx_last_error().decode()
        assert (out == -7.25).all()
        ok = np.full((3, g.V, g.D), -7.25, order="F")
        assert call(good, ok) == 0 and (ok != -7.25).all() and np.isfinite(ok).all()
    assert call(good, None) != 0 and lib.sx_last_error().decode()
    assert lib.sx_evaluate(tile._h, None, 3, 0, np.zeros(1).ctypes.data_as(L.P_D)) != 0
    assert lib.sx_evaluate(tile._h, None, 0, 0, None) == 0
    # ModelRun.evaluate routes by radius: every point of the patch is held by exactly one local tile, the edge by the lower one
    pts = E.scattered_points(g, 200, seed=3)
    pts[0, 0] = hi
    vals, held = hip.run.evaluate(pts)
    assert held.all()
    assert (vals[0] == tile.evaluate(pts[:1])[0]).all()
    hip.run.close()


def test_writer(tmp_path):
    import scythe_jl_amd as S
    from scythe_jl_amd import io
    case = cases.rl_slab(num_cells=9)
    hip = cases.HipModel(case, num_tiles=3, exchange="gather", impl="lib")
    for _ in range(2):
        hip.step()
    hip.mp.output_dir = str(tmp_path)
    pts, idx = S.cartesian_gridpoints(hip.gp, 24, 24)
    t = 6.0
    path = S.write_gridded_output(hip.run, hip.mp, t, pts)
    phys = io.write_output(hip.run, hip.mp, t, spectral=False)
    assert os.path.basename(path).replace("gridded_out_", "") == os.path.basename(phys).replace("physical_out_", "")
    names = hip.gp.var_names()
    with open(path) as f:
        header = f.readline().strip().split(",")
    assert header == ["r", "l"] + [n + s for s in ("", "_r", "_rr", "_l", "_ll") for n in names]
    data = np.loadtxt(path, delimiter=",", skiprows=1, ndmin=2)
    vals, held = hip.run.evaluate(pts)
    assert held.all() and data.shape == (len(idx), 2 + 5 * len(names))
    assert (data[:, :2] == pts).all()
    for d in range(5):
        assert (data[:, 2 + d * len(names):2 + (d + 1) * len(names)] == vals[:, :, d]).all()
    hip.run.close()


def test_timer_and_bytes():
    """k_evaluate is registered with the timers, and sx_kernel_bytes counts batches x 4 rows x live columns of the last call"""
    import scythe_jl_amd as S
    case = cases.rlz_advection(num_cells=4, zDim=9, ring_L=8)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(np.random.default_rng(7).standard_normal((g.S_patch(), g.V)))
    tile.enable_timers(True)
    r = g.xmin + 2.5 * g.DX                      # 5 points of one cell with kcap 3 (uniform L = 8: kmax = min(ri, 3)): one batch
    tile.evaluate(np.array([[r, 0.1 * i, 1.0] for i in range(5)]))
    tm = tile.timers()
    assert tm["k_evaluate"][1] == 1 and tm["k_evaluate"][0] > 0
    assert tile.kernel_bytes("k_evaluate") == 8 * 4 * g.b_zDim * (2 * 3 + 1) * g.V
    tile.close()
