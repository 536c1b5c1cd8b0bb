"""sx_harmonics and sx_evaluate_band on the GPU against the twin of tests/harmonics.py (longdouble: the arbiter) and against the route
a user has without them: tileTransform!, `physical` to the host and a discrete Fourier transform ring by ring.

The SX_GRAPH, SX_OVERLAP and SX_DEFER_DIAG cases of the read-only test run in a child process started with the switch in its
environment (tests/harmonics.py::read_only_in_child, the pattern of tests/child_run.py).

Shapes: the smallest at which the kernel can still go wrong - a block count that is no multiple of 16 or of the wave (K2 56), b_zDim no
multiple of 4 (7, 8 and 22), radii that cross cells and tile edges, and height counts of 5 (one padded tile of 16), 37 (three tiles, the
last one padded) and the 32 levels of a grid with 32 blocks (two full tiles).  RZ80 has b_zDim above 48: the instantiation that holds
32 K steps in registers.  test_launch_cut passes more radii than one launch takes."""
import functools

import numpy as np
import pytest

from tests import cases
from tests import evaluate as E
from tests import harmonics as H
from tests.test_gpu_evaluate import _bounds

pytestmark = pytest.mark.gpu

CASES = {
    "R": lambda: cases.r_bcs(num_cells=12),
    "RZ": lambda: cases.rz_advection(num_cells=9, zDim=12),
    "RL": lambda: cases.rl_slab(num_cells=9),
    "RL16": lambda: cases.rl_slab(num_cells=9, ring_L=16),
    "RLZ": lambda: cases.rlz_hrbl(num_cells=9, zDim=10),
    "RLZ16": lambda: cases.rlz_hrbl(num_cells=9, zDim=10, ring_L=16),
    "RLZ32": lambda: cases.rlz_hrbl(num_cells=6, zDim=32, ring_L=32),
    "RZ80": lambda: cases.rz_advection(num_cells=5, zDim=80),
}


def _heights(g):
    if not g.has_z:
        return None
    lev = g.cheb(g.names[0]).z
    return np.array([g.zmin, lev[2], 0.37 * (g.zmax - g.zmin) + g.zmin, g.zmax, lev[len(lev) // 2]])


def _slot_errors(a, t):
    """per slot: max |a - t| / max |t[..., s]| against the longdouble truth"""
    return np.array([H.rel_err(a[..., s], t[..., s]) for s in range(t.shape[-1])])


@functools.lru_cache(maxsize=None)
def _random_case(name):
    """grid, A, radii, heights and the two twins per truncation flag: computed once, shared, left unchanged"""
    case = CASES[name]()
    g = cases.oracle_grid(case)
    A = np.random.default_rng(17).standard_normal((g.S_patch(), g.V))
    radii, heights, slots = H.sample_radii(g, 37, seed=23), _heights(g), H.grid_slots(g)
    twins = {all_k: (H.harmonics(g, A, radii, heights, all_k, slots, xp=True), H.harmonics(g, A, radii, heights, all_k, slots, xp=False))
             for all_k in (False, True)}
    return case, g, A, radii, heights, slots, twins


@pytest.mark.parametrize("name", list(CASES))
def test_random_coefficients(name):
    import scythe_jl_amd as S
    case, g, A, radii, heights, slots, twins = _random_case(name)
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(A)
    for all_k in (False, True):
        got = tile.harmonics(radii, heights, all_k, slots)
        truth, f64 = twins[all_k]
        assert got.shape == truth.shape and got.dtype == np.complex128 and np.isfinite(got).all()
        e_new, e_f64 = _slot_errors(got, truth), _slot_errors(f64, truth)
        bound = np.concatenate([[1e-10], _bounds(e_new[1:], e_f64[1:])])
        print("%s all_k=%s: err %s; float64 twin %s; ratio to the bound %s" % (name, all_k, e_new, e_f64, e_new / bound))
        assert e_new[0] <= 1e-10
        assert (e_new[1:] <= bound[1:]).all(), (e_new, e_f64)
        assert (got[..., 0, :, :].imag == 0).all()                                  # Im c_0
        assert (got[(truth == 0).astype(bool)] == 0).all()                          # above the cap: exact zeros
    tile.close()


def _many_heights(g, kind):
    lev = g.cheb(g.names[0]).z
    if kind == "levels":
        return np.array(lev)
    rng = np.random.default_rng(41)                   # 37: the two ends, every level, random ones; unsorted
    z = np.concatenate([[g.zmin, g.zmax], lev, rng.uniform(g.zmin, g.zmax, 37 - 2 - len(lev))])
    return rng.permutation(z)


@pytest.mark.parametrize("name,kind", [("RLZ16", "37"), ("RLZ32", "levels")])
def test_more_than_one_height_tile(name, kind):
    """37 heights are three tiles of 16, the last one padded; the 32 levels of RLZ32 are two full ones.  Bounds as above."""
    import scythe_jl_amd as S
    case, g, A, radii, _, slots, _ = _random_case(name)
    heights = _many_heights(g, kind)
    assert len(heights) == (37 if kind == "37" else 32)
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(A)
    for all_k in (False, True):
        truth = H.harmonics(g, A, radii, heights, all_k, slots, xp=True)
        f64 = H.harmonics(g, A, radii, heights, all_k, slots, xp=False)
        got = tile.harmonics(radii, heights, all_k, slots)
        assert got.shape == truth.shape and np.isfinite(got).all()
        e_new, e_f64 = _slot_errors(got, truth), _slot_errors(f64, truth)
        bound = np.concatenate([[1e-10], _bounds(e_new[1:], e_f64[1:])])
        print("%s %d heights all_k=%s: err %s; float64 twin %s; ratio to the bound %s" % (name, len(heights), all_k, e_new, e_f64, e_new / bound))
        assert e_new[0] <= 1e-10
        assert (e_new[1:] <= bound[1:]).all(), (e_new, e_f64)
        assert (got[(truth == 0).astype(bool)] == 0).all()
        # a height's result does not depend on its tile or its place in it: the first 5 alone, bytewise
        few = tile.harmonics(radii, heights[:5], all_k, slots)
        assert np.ascontiguousarray(few).tobytes() == np.ascontiguousarray(got[:, :5]).tobytes()
    tile.close()


@pytest.mark.parametrize("tiles", [1, 3])
@pytest.mark.parametrize("name", ["RL", "RLZ16"])
def test_stepped_model_against_the_host_dft(name, tiles):
    """what a user does today: tileTransform!, `physical` to the host, the DFT of every ring with the gridpoints' own lambda"""
    import scythe_jl_amd as S
    case = CASES[name]()
    hip = cases.HipModel(case, num_tiles=tiles, exchange="gather", impl="lib" if tiles > 1 else "torch")
    for _ in range(3):
        hip.step()
    g = cases.oracle_grid(case)
    for t, tile in zip(hip.run.tile_ids, hip.run.tiles):
        pts = S.getGridpoints(tile)
        pts = pts.reshape(len(pts), -1)
        c0, n = hip.run.layout.cell0[t], hip.run.layout.ncells[t]
        rings = np.arange(3 * c0, 3 * (c0 + n))
        start = np.concatenate([[0], np.cumsum(g.L[rings] * g.zDim)])
        radii = pts[start[:-1], 0]
        lev = pts[:g.zDim, -1] if g.has_z else None
        got = tile.harmonics(radii, lev)[..., 0]                                    # [ir, iz, k, v]
        tile.tileTransform_()
        val = tile.physical[:, :, 0]
        scale = np.maximum(np.abs(got).max(axis=(0, 1, 2)), 1e-300)                 # per variable
        worst = 0.0
        for i, ring in enumerate(rings):
            L, km = int(g.L[ring]), int(g.kmax[ring])
            p = pts[start[i]:start[i + 1]].reshape(L, g.zDim, -1)
            u = val[start[i]:start[i + 1]].reshape(L, g.zDim, g.V)
            d = H.ring_dft(u, p[:, 0, 1])                                           # [k, z, v]
            diff = np.abs(got[i, :, :km + 1].transpose(1, 0, 2) - d[:km + 1]).max(axis=(0, 1)) / scale
            worst = max(worst, float(diff.max()))
        print("%s tiles=%d tile %d: harmonics vs host DFT of physical, worst relative difference %.3e" % (name, tiles, t, worst))
        assert np.abs(got).max() > 0 and worst <= 1e-10, worst
    hip.run.close()


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
    rad = np.unique(g.gridpoints()[:, 0])
    r5, r20 = 0.5 * (rad[4] + rad[5]), 0.5 * (rad[19] + rad[20])
    assert E.kcap_of(g, r5) == 5 and E.kcap_of(g, r20) >= 12
    slots = H.grid_slots(g)
    ring = tile.harmonics([r5], slots=slots)
    assert ring.tobytes() == np.zeros_like(ring).tobytes()
    allk = tile.harmonics([r5], all_k=True, slots=slots)
    only = np.zeros(g.kDim + 1, dtype=bool)
    only[12] = True
    assert (allk[:, :, ~only] == 0).all() and np.abs(allk[:, :, 12]).min() > 0
    truth = H.harmonics(g, A, [r5], None, True, slots, xp=True)
    f64 = H.harmonics(g, A, [r5], None, True, slots, xp=False)
    e, ef = _slot_errors(allk, truth), _slot_errors(f64, truth)
    assert e[0] <= 1e-10 and (e[1:] <= _bounds(e[1:], ef[1:])).all(), (e, ef)
    assert tile.harmonics([r20], slots=slots).tobytes() == tile.harmonics([r20], all_k=True, slots=slots).tobytes()
    assert np.abs(tile.harmonics([r20])).max() > 0
    tile.close()


def _small_rlz():
    import scythe_jl_amd as S
    case = cases.rlz_advection(num_cells=4, zDim=9, ring_L=8)
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(np.random.default_rng(7).standard_normal((g.S_patch(), g.V)))
    return g, tile


def test_chunking_and_order():
    g, tile = _small_rlz()
    rng = np.random.default_rng(9)
    radii = rng.uniform(g.xmin, g.xmax, 3000)
    heights = np.concatenate([[g.zmin, g.zmax], rng.uniform(g.zmin, g.zmax, 5)])
    whole = tile.harmonics(radii, heights, slots=H.SLOTS)
    assert np.isfinite(whole).all() and np.abs(whole).max() > 0
    parts = np.concatenate([tile.harmonics(radii[i:i + 100], heights, slots=H.SLOTS) for i in range(0, 3000, 100)], axis=0)
    assert np.ascontiguousarray(whole).tobytes() == np.ascontiguousarray(parts).tobytes()
    perm = rng.permutation(3000)
    shuffled = tile.harmonics(radii[perm], heights, slots=H.SLOTS)
    back = np.empty_like(np.ascontiguousarray(shuffled))
    back[perm] = shuffled
    assert np.ascontiguousarray(whole).tobytes() == back.tobytes()
    tile.close()


def test_launch_cut():
    """A launch takes at most 32,768 radii (the y extent of a grid): 40,000 in one call are two launches, the second one shorter, and
    equal the calls of 10,000 (one launch each; the cut at 32,768 falls inside the fourth) bytewise."""
    g, tile = _small_rlz()
    rng = np.random.default_rng(13)
    radii = rng.uniform(g.xmin, g.xmax, 40000)
    heights = np.array([g.zmin, 0.3 * (g.zmax - g.zmin) + g.zmin, g.zmax])
    slots = ("u", "rr", "z")
    whole = np.ascontiguousarray(tile.harmonics(radii, heights, slots=slots))
    assert np.isfinite(whole).all() and np.abs(whole[32768:]).max() > 0
    parts = np.concatenate([tile.harmonics(radii[i:i + 10000], heights, slots=slots) for i in range(0, 40000, 10000)], axis=0)
    assert whole.tobytes() == np.ascontiguousarray(parts).tobytes()
    assert whole[32768:].tobytes() == np.ascontiguousarray(tile.harmonics(radii[32768:], heights, slots=slots)).tobytes()
    tile.close()


def test_slot_mask():
    g, tile = _small_rlz()
    radii = H.sample_radii(g, 20, seed=3)
    heights = np.linspace(g.zmin, g.zmax, 7)
    for all_k in (False, True):
        every = tile.harmonics(radii, heights, all_k, H.SLOTS)
        for si, s in enumerate(H.SLOTS):
            one = tile.harmonics(radii, heights, all_k, (s,))
            assert one.shape[-1] == 1
            assert np.ascontiguousarray(one[..., 0]).tobytes() == np.ascontiguousarray(every[..., si]).tobytes(), s
        two = tile.harmonics(radii, heights, all_k, ("rr", "z"))
        assert np.ascontiguousarray(two).tobytes() == np.ascontiguousarray(every[..., [2, 3]]).tobytes()
    tile.close()


HRBL_MFMA = ("rlz_hrbl", {"num_cells": 8, "zDim": 32, "ring_L": 32})


@pytest.mark.parametrize("switch,maker,kw", [("plain", "rlz_hrbl", {"num_cells": 6, "zDim": 10, "ring_L": 16}),
                                             ("SX_GRAPH", "rl_slab", {"num_cells": 8}), ("SX_OVERLAP",) + HRBL_MFMA,
                                             ("SX_DEFER_DIAG",) + HRBL_MFMA])
def test_read_only(switch, maker, kw, tmp_path):
    r = H.read_only_job(maker, kw) if switch == "plain" else H.read_only_in_child(tmp_path, maker, kw, {switch: "1"})
    assert np.isfinite(r["got"]).all() and np.abs(r["got"]).max() > 0 and np.abs(r["band"]).max() > 0
    assert bool(r["same_state"]) and bool(r["same_np1"])                      # around each pair of calls
    assert r["state0"].tobytes() == r["state1"].tobytes()                     # and the steps after them match a run without
    assert r["np10"].tobytes() == r["np11"].tobytes()


def test_refusals():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    case = cases.rlz_advection(num_cells=9, zDim=9, ring_L=8)
    hip = cases.HipModel(case, num_tiles=3, exchange="gather", impl="lib")
    hip.step()
    g = cases.oracle_grid(case)
    tile = hip.run.tiles[1]
    lo, hi = E.tile_range(g, hip.run.layout.cell0[1], hip.run.layout.ncells[1])
    lib = S.load()
    K2 = 2 * (g.kDim + 1)

    def call(h, radii, heights, flags, mask, out, n_r=None, n_z=None):
        r = None if radii is None else np.ascontiguousarray(radii, dtype=np.float64)
        z = None if heights is None else np.ascontiguousarray(heights, dtype=np.float64)
        return lib.sx_harmonics(h, None if r is None else r.ctypes.data_as(L.P_D), len(r) if n_r is None else n_r,
                                None if z is None else z.ctypes.data_as(L.P_D), (0 if z is None else len(z)) if n_z is None else n_z,
                                flags, mask, None if out is None else out.ctypes.data_as(L.P_D))

    good_r, good_z = [lo, 0.5 * (lo + hi), hi], [g.zmin, 1.0, g.zmax]
    fresh = lambda: np.full((K2, 3, 3, g.V, 5), -7.25, order="F")
    bads = [([lo - 1e-6, good_r[1], hi], good_z, 0, 31), (good_r[:2] + [hi + 1e-6], good_z, 0, 31), ([lo, np.nan, hi], good_z, 0, 31),
            (good_r, [g.zmin, g.zmax + 1e-6, 1.0], 0, 31), (good_r, [g.zmin - 1e-6, 1.0, 2.0], 0, 31), (good_r, good_z, 0, 0),
            (good_r, good_z, 0, 32), (good_r, good_z, 2, 31), (good_r, good_z, -1, 31)]
    for radii, heights, flags, mask in bads:
        out = fresh()
        assert call(tile._h, radii, heights, flags, mask, out) != 0
        assert lib.sx_last_error().decode()
        assert (out == -7.25).all()
        ok = fresh()
        assert call(tile._h, good_r, good_z, 0, 31, ok) == 0 and (ok != -7.25).all() and np.isfinite(ok).all()
    assert call(tile._h, good_r, good_z, 0, 31, None) != 0 and lib.sx_last_error().decode()          # null out
    assert call(tile._h, None, good_z, 0, 31, fresh(), n_r=3) != 0                                    # null radii with a count
    assert call(tile._h, good_r, None, 0, 31, fresh(), n_z=3) != 0                                    # null heights with a count
    assert call(tile._h, good_r, good_z, 0, 31, fresh(), n_r=-1) != 0
    assert call(tile._h, None, good_z, 0, 31, None, n_r=0) == 0                                       # n_r = 0 succeeds
    # a grid without a vertical: no z / zz bit, no heights
    rl_case = cases.rl_slab(num_cells=9, ring_L=16)
    gp, mp = cases.hip_params(rl_case)
    grl = cases.oracle_grid(rl_case)
    rl = S.Grid(gp, mp)
    rl.set_patch_spectral_a(np.random.default_rng(2).standard_normal((grl.S_patch(), grl.V)))
    rr = [grl.xmin, 0.5 * (grl.xmin + grl.xmax)]
    fresh_rl = lambda: np.full((2 * (grl.kDim + 1), 1, 2, grl.V, 3), -7.25, order="F")
    for heights, mask in ((None, 8), (None, 1 | 16), ([0.0], 1)):
        out = fresh_rl()
        assert call(rl._h, rr, heights, 0, mask, out) != 0 and lib.sx_last_error().decode()
        assert (out == -7.25).all()
        ok = fresh_rl()
        assert call(rl._h, rr, None, 0, 7, ok) == 0 and (ok != -7.25).all()
    rl.close()
    # ModelRun.harmonics routes by radius: every radius of the patch is held exactly once, a shared edge by the lower tile
    radii = H.sample_radii(g, 60, seed=3)
    radii[0] = hi
    heights = np.array([g.zmin, 1.0])
    vals, held = hip.run.harmonics(radii, heights)
    assert held.all() and vals.shape == (60, 2, g.kDim + 1, g.V, 1)
    assert (vals[0] == tile.harmonics(radii[:1], heights)[0]).all()
    truth = H.harmonics(g, tile.patchSpectral, radii, heights, xp=True)
    assert H.rel_err(vals, truth) <= 1e-10
    hip.run.close()


@pytest.mark.parametrize("name", ["RL", "RLZ16"])
def test_band_evaluation(name):
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    case, g, A, _, _, slots, _ = _random_case(name)
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(A)
    pts = E.scattered_points(g, 2000, seed=23)
    full = tile.evaluate(pts)
    assert tile.evaluate(pts, k_band=(0, g.kDim)).tobytes() == full.tobytes()
    assert tile.evaluate(pts, k_band=(0, g.kDim + 50)).tobytes() == full.tobytes()       # kmax above kDim is clamped
    # the wave-2 part from the harmonics at the same (r, z), one call per distinct height
    wave2 = tile.evaluate(pts, k_band=(2, 2))
    c = np.zeros((len(pts), g.V, len(slots)), dtype=np.complex128)
    if g.has_z:
        for z in np.unique(pts[:, -1]):
            sel = np.nonzero(pts[:, -1] == z)[0]
            c[sel] = tile.harmonics(pts[sel, 0], [z], slots=slots)[:, 0, 2]
    else:
        c = tile.harmonics(pts[:, 0], slots=slots)[:, 0, 2]
    rec = H.from_harmonic(g, c, 2, pts[:, 1], xp=True)
    truth = H.evaluate_band(g, A, pts, 2, 2, xp=True)
    f64 = H.evaluate_band(g, A, pts, 2, 2, xp=False)
    e_new, e_rec, e_f64 = E.slot_errors(wave2, truth), E.slot_errors(rec, truth), E.slot_errors(f64, truth)
    e_pair = E.slot_errors(wave2, rec)
    bound = np.concatenate([[1e-10], _bounds(e_new[1:], e_f64[1:])])
    print("%s band (2, 2): err evaluate %s; from harmonics %s; float64 twin %s; evaluate vs harmonics %s; ratios %s %s"
          % (name, e_new, e_rec, e_f64, e_pair, e_new / bound, e_rec / bound))
    assert np.abs(wave2[:, :, 0]).max() > 0
    assert e_pair[0] <= 1e-10 and e_new[0] <= 1e-10 and e_rec[0] <= 1e-10
    assert (e_new[1:] <= bound[1:]).all() and (e_rec[1:] <= bound[1:]).all(), (e_new, e_rec, e_f64)
    parts = [tile.evaluate(pts, k_band=b) for b in ((0, 1), (2, 2), (3, g.kDim))]
    resid = np.abs(parts[0] + parts[1] + parts[2] - full)
    room = 1e-12 * (np.abs(parts[0]) + np.abs(parts[1]) + np.abs(parts[2]))
    print("%s bands (0,1) + (2,2) + (3,kDim) - full: worst residual / (1e-12 sum |parts|) %.3e" % (name, float((resid / np.maximum(room, 1e-300)).max())))
    assert (resid <= room).all()
    lib = S.load()
    p = np.asfortranarray(pts)
    out = np.full(full.shape, -7.25, order="F")
    for kmin, kmax in ((3, 2), (-1, 2), (0, -1)):
        assert lib.sx_evaluate_band(tile._h, p.ctypes.data_as(L.P_D), len(p), 0, kmin, kmax, out.ctypes.data_as(L.P_D)) != 0
        assert lib.sx_last_error().decode() and (out == -7.25).all()
    with pytest.raises(L.ScytheHipError):
        tile.evaluate(pts, k_band=(3, 2))
    tile.close()


def test_timer_and_bytes():
    """k_harmonics is registered with the timers, and sx_kernel_bytes counts 4 rows x b_zDim x (2 kcap + 1) x 8 per radius and variable"""
    g, tile = _small_rlz()
    tile.enable_timers(True)
    r = g.xmin + 2.5 * g.DX                      # kcap 3 (uniform L = 8: kmax = min(ri, 3))
    assert E.kcap_of(g, r) == 3
    tile.harmonics([r], [1.0, 2.0], slots=("u", "z"))
    tm = tile.timers()
    assert tm["k_harmonics"][1] == 1 and tm["k_harmonics"][0] > 0
    assert tile.kernel_bytes("k_harmonics") == 8 * 4 * g.b_zDim * (2 * 3 + 1) * g.V
    tile.harmonics([r, r, g.xmin], [1.0])
    assert tile.timers()["k_harmonics"][1] == 2
    assert tile.kernel_bytes("k_harmonics") == 8 * 4 * g.b_zDim * (2 * (2 * 3 + 1) + (2 * E.kcap_of(g, g.xmin) + 1)) * g.V
    tile.close()
