"""sx_spectrum on the GPU against the twin of tests/spectrum.py (longdouble: the arbiter; pinned to the oracle by
tests/test_spectrum.py) and, by Parseval, against sx_reduce on the device.

The SX_GRAPH, SX_OVERLAP and SX_DEFER_DIAG cases of the read-only test run in a child process started with the switch in its
environment (tests/spectrum.py::read_only_in_child, the pattern of tests/harmonics.py).

Shapes: those of tests/test_gpu_harmonics.py::CASES, the smallest at which the kernel can still go wrong - block counts that are no
multiple of 16 or 64, b_zDim no multiple of 4, level counts of 10 and 12 (one padded height tile), 32 (two full tiles) and 80 (five
tiles, b_zDim above 48: the instantiation that holds 32 K steps in registers), rings with kmax below kDim."""
import functools

import numpy as np
import pytest

from tests import cases
from tests import harmonics as H
from tests import reduce as R
from tests import spectrum as SP
from tests.test_gpu_evaluate import _bounds

pytestmark = pytest.mark.gpu
XP = SP.XP

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


@functools.lru_cache(maxsize=None)
def _random_case(name):
    """grid, A, the 16 pairs and the two twins: computed once, shared, left unchanged"""
    case = CASES[name]()
    g = cases.oracle_grid(case)
    A = np.random.default_rng(17).standard_normal((g.S_patch(), g.V))
    pairs = SP.sixteen_pairs(g)
    return case, g, A, pairs, SP.spectrum(g, A, pairs, xp=True), SP.spectrum(g, A, pairs, xp=False)


def _tile(case, A):
    import scythe_jl_amd as S
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(A)
    return tile


def _pair_errors(a, t):
    """per pair: max |a - t| / max |t[..., p]| against the longdouble truth"""
    return np.array([H.rel_err(a[..., p], t[..., p]) for p in range(t.shape[-1])])


@pytest.mark.parametrize("name", list(CASES))
def test_random_coefficients(name):
    """Value-slot pairs within 1e-10 max|truth| of the longdouble twin; pairs with a derivative slot within the bound of
    tests/test_gpu_evaluate.py::_bounds from the float64 twin's own error; exact zeros above kmax[ring]."""
    case, g, A, pairs, xp, f64 = _random_case(name)
    q = SP.resolve(g, pairs)
    value = (q[:, 1] == 0) & (q[:, 3] == 0)
    assert len(pairs) == 16 and value.any() and (~value).any()
    tile = _tile(case, A)
    for kind, truth, twin in (("ring", xp[0], f64[0]), ("domain", xp[2], f64[2])):
        got = tile.spectrum(pairs, kind)
        assert got.shape == truth.shape and got.dtype == np.float64 and np.isfinite(got).all()
        e_new, e_f64 = _pair_errors(got, truth), _pair_errors(twin, truth)
        bound = np.where(value, 1e-10, _bounds(e_new, e_f64))
        print("%s %s: largest ratio to the bound, value pairs %.3g, derivative pairs %.3g (float64 twin's own error up to %.3g)"
              % (name, kind, (e_new / bound)[value].max(), (e_new / bound)[~value].max(), e_f64.max()))
        assert (e_new <= bound).all(), (e_new, e_f64)
        assert (got[(truth == 0).astype(bool)] == 0).all()                          # above kmax[ring]: exact zeros
        if kind == "ring" and g.has_l:
            low = np.nonzero(np.asarray(g.kmax) < g.kDim)[0]
            assert len(low) and all((got[int(g.kmax[i]) + 1:, i] == 0).all() and np.abs(got[int(g.kmax[i]), i]).max() > 0 for i in low)
    tile.close()


def _value_pairs(g):
    """power and cross pairs of the value slot over the variables of the grid, 16 at the most"""
    V = g.V
    pairs = [((v, 0), (v, 0)) for v in range(1, V + 1)] + [((v, 0), (v % V + 1, 0)) for v in range(1, V + 1)]
    pairs += [((v, 0), ((v + 1) % V + 1, 0)) for v in range(1, V + 1)]
    return pairs[:16]


@pytest.mark.parametrize("maker,kw", [("rl_slab", {"num_cells": 9}), ("rlz_hrbl", {"num_cells": 6, "zDim": 10, "ring_L": 16})])
def test_parseval_against_reduce_on_the_device(maker, kw):
    """After 5 steps: sum_k spectrum = Grid.reduce of the product programs (domain kind, and azimuth kind summed over the levels with
    w_z), within 32 2^-53 S_abs (tests/reduce.py::BOUND; S_abs from the twin on the model's A) plus the value-slot parity 1e-10
    max|truth|; and the 2-tile patch results equal the 1-tile ones within the same bound."""
    import scythe_jl_amd as S
    case = getattr(cases, maker)(**kw)
    g = cases.oracle_grid(case)
    gp, _ = cases.hip_params(case)
    pairs = _value_pairs(g)
    terms = SP.product_terms(g, pairs)
    w_z = S.reduce_weights(gp)[2] if g.has_z else np.ones(1)
    kept = {}
    for tiles in (1, 2):
        hip = cases.HipModel(case, num_tiles=tiles, exchange="gather", impl="lib" if tiles > 1 else "torch")
        for _ in range(5):
            hip.step()
        run = hip.run
        ring, dom = run.spectrum(pairs, "ring"), run.spectrum(pairs, "domain")
        assert ring.shape == (g.kDim + 1, g.rDim, len(pairs)) and dom.shape == (g.kDim + 1, len(pairs))
        truth_ring, ring_abs, truth_dom, dom_abs = SP.spectrum(g, run.tiles[0].patchSpectral, pairs, xp=True)
        lim_dom = R.BOUND * dom_abs.sum(axis=0).astype(np.float64) + 1e-10 * np.abs(truth_dom).max(axis=0).astype(np.float64)
        lim_ring = R.BOUND * ring_abs.sum(axis=0).astype(np.float64) + 1e-10 * np.abs(truth_ring).max(axis=(0, 1)).astype(np.float64)[None, :]
        integral = run.integrate(terms)
        _, _, mean = run.azimuthal_mean(terms)
        level_sum = np.einsum("z,rzp->rp", w_z, mean)
        e_dom, e_ring = np.abs(dom.sum(axis=0) - integral), np.abs(ring.sum(axis=0) - level_sum)
        print("%s tiles=%d: sum_k spectrum vs reduce, worst ratio to the bound: domain %.3g, ring %.3g"
              % (maker, tiles, (e_dom / lim_dom).max(), (e_ring / lim_ring).max()))
        assert np.abs(integral).max() > 0 and (e_dom <= lim_dom).all() and (e_ring <= lim_ring).all()
        if tiles == 1:
            kept = {"ring": ring, "dom": dom}
        else:
            d_dom, d_ring = np.abs(dom - kept["dom"]).sum(axis=0), np.abs(ring - kept["ring"]).sum(axis=0)
            print("%s: 2 tiles vs 1 tile, worst ratio to the bound: domain %.3g, ring %.3g"
                  % (maker, (d_dom / lim_dom).max(), (d_ring / lim_ring).max()))
            assert (d_dom <= lim_dom).all() and (d_ring <= lim_ring).all()
        run.close()


@pytest.mark.parametrize("name", ["RL16", "RLZ16"])
def test_one_wavenumber_in_one_out(name):
    """A of variable 1 holds the k = 3 cosine block alone, of variable 2 the k = 3 sine block alone: every other k is exactly 0.0 in
    both kinds, and so is the whole cross spectrum of the two."""
    case = CASES[name]()
    g = cases.oracle_grid(case)
    assert g.V >= 2 and g.kDim > 3
    A = np.zeros((g.S_patch(), g.V))
    a = A.reshape(g.b_zDim, g.K2, g.b_rDim, g.V)
    rng = np.random.default_rng(5)
    a[:, 2 * 3 - 1, :, 0] = rng.standard_normal((g.b_zDim, g.b_rDim))            # Re of k = 3
    a[:, 2 * 3, :, 1] = rng.standard_normal((g.b_zDim, g.b_rDim))                # Im of k = 3
    ns = len(H.grid_slots(g))
    powers = [((v, s), (v, s)) for v in (1, 2) for s in range(ns)]
    cross = [((1, s), (2, t)) for s in range(ns) for t in range(ns)][:16 - len(powers)]
    tile = _tile(case, A)
    other = np.arange(g.kDim + 1) != 3
    for kind in ("ring", "domain"):
        got = tile.spectrum(powers + cross, kind)
        assert (got[other] == 0.0).all()
        assert (got[:, ..., len(powers):] == 0.0).all()
        if kind == "ring":
            live = np.asarray(g.kmax) >= 3
            assert (got[3][live][:, :len(powers)] > 0).all() and (got[3][~live] == 0.0).all()
        else:
            assert (got[3, :len(powers)] > 0).all()
    tile.close()


def test_bitwise_properties():
    case, g, A, pairs, _, _ = _random_case("RLZ16")
    tile = _tile(case, A)
    perm = np.random.default_rng(3).permutation(16)
    for kind in ("ring", "domain"):
        first = tile.spectrum(pairs, kind)
        assert tile.spectrum(pairs, kind).tobytes() == first.tobytes()                       # two calls
        shuffled = tile.spectrum([pairs[i] for i in perm], kind)
        assert np.ascontiguousarray(shuffled).tobytes() == np.ascontiguousarray(first[..., perm]).tobytes()
        for p in (0, 4, 7, 15):                                                                # a power pair (a == b once), cross pairs
            alone = tile.spectrum([pairs[p]], kind)
            assert np.ascontiguousarray(alone[..., 0]).tobytes() == np.ascontiguousarray(first[..., p]).tobytes(), p
        assert pairs[0][0] == pairs[0][1] and pairs[7][0] != pairs[7][1]
        swapped = tile.spectrum([(b, a) for a, b in pairs], kind)
        assert swapped.tobytes() == first.tobytes()                                            # (a, b) = (b, a)
    tile.close()


HRBL_MFMA = ("rlz_hrbl", {"num_cells": 8, "zDim": 32, "ring_L": 32})


@pytest.mark.parametrize("switch,maker,kw", [("plain", "rlz_hrbl", {"num_cells": 6, "zDim": 10, "ring_L": 16}),
                                             ("SX_GRAPH", "rl_slab", {"num_cells": 8}), ("SX_OVERLAP",) + HRBL_MFMA,
                                             ("SX_DEFER_DIAG",) + HRBL_MFMA])
def test_read_only(switch, maker, kw, tmp_path):
    r = SP.read_only_job(maker, kw) if switch == "plain" else SP.read_only_in_child(tmp_path, maker, kw, {switch: "1"})
    assert np.isfinite(r["ring"]).all() and np.abs(r["ring"]).max() > 0 and np.abs(r["dom"]).max() > 0
    assert bool(r["same_state"]) and bool(r["same_np1"])                      # around each pair of calls
    assert r["state0"].tobytes() == r["state1"].tobytes()                     # and the steps after them match a run without
    assert r["np10"].tobytes() == r["np11"].tobytes()


def test_refusals():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    case, g, A, _, _, _ = _random_case("RLZ16")
    tile = _tile(case, A)
    lib = S.load()
    K = g.kDim + 1

    def call(h, kind, pairs, out, n=None):
        q = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
        return lib.sx_spectrum(h, kind, (0 if q is None else len(q)) if n is None else n, None if q is None else q.ctypes.data_as(L.P_I32),
                               None if out is None else out.ctypes.data_as(L.P_D))

    good = [[1, 0, 2, 4], [2, 1, 2, 1]]
    fresh = lambda: np.full((K, g.rDim, 17), -7.25, order="F")
    bads = [(2, good, None), (-1, good, None), (0, good, -1), (0, [[1, 0, 1, 0]] * 17, None), (0, None, 2), (0, [[0, 0, 1, 0]], None),
            (1, [[1, 0, g.V + 1, 0]], None), (0, [[1, 5, 1, 0]], None), (1, [[1, 0, 1, -1]], None)]
    for kind, pairs, n in bads:
        out = fresh()
        assert call(tile._h, kind, pairs, out, n) != 0 and lib.sx_last_error().decode(), (kind, pairs, n)
        assert (out == -7.25).all()
        ok = fresh()
        assert call(tile._h, 0, good, ok) == 0 and (ok[:, :, :2] != -7.25).all() and (ok[:, :, 2:] == -7.25).all()
    assert call(tile._h, 0, good, None) != 0 and lib.sx_last_error().decode()          # null out
    out = fresh()
    assert call(tile._h, 0, None, out, 0) == 0 and call(tile._h, 1, None, None, 0) == 0 and (out == -7.25).all()      # n_pairs = 0
    with pytest.raises(ValueError):
        tile.spectrum([((1, "u"), (1, "u"))], kind="level")
    tile.close()
    # a grid without a vertical: no z / zz slot
    case_rl, g_rl, A_rl, _, _, _ = _random_case("RL16")
    rl = _tile(case_rl, A_rl)
    for pairs in ([[1, 3, 1, 0]], [[1, 0, 2, 4]]):
        out = np.full((g_rl.kDim + 1, g_rl.rDim, 1), -7.25, order="F")
        assert call(rl._h, 0, pairs, out) != 0 and lib.sx_last_error().decode() and (out == -7.25).all()
    with pytest.raises(L.ScytheHipError):
        rl.spectrum([((1, "u"), (1, "zz"))])
    assert np.abs(rl.spectrum([((1, "u"), (2, "rr"))])).max() > 0
    rl.close()


def test_timer_and_bytes():
    """k_spectrum is registered with the timers, k_spectrum_final by the domain kind only, and sx_kernel_bytes counts
    4 rows x b_zDim x (2 kmax + 1) x 8 per ring and distinct (var, slot) plane - a plane two pairs share once"""
    case, g, A, _, _, _ = _random_case("RLZ16")
    tile = _tile(case, A)
    tile.enable_timers(True)
    per_plane = sum(8 * 4 * g.b_zDim * (2 * int(k) + 1) for k in g.kmax)
    tile.spectrum([((1, "u"), (1, "u"))], "ring")
    tm = tile.timers()
    assert tm["k_spectrum"][1] == 1 and tm["k_spectrum"][0] > 0 and "k_spectrum_final" not in tm
    assert tile.kernel_bytes("k_spectrum") == per_plane
    tile.spectrum([((1, "u"), (2, "z")), ((2, "z"), (1, "r")), ((1, "u"), (1, "u"))], "domain")
    tm = tile.timers()
    assert tm["k_spectrum"][1] == 2 and tm["k_spectrum_final"][1] == 1 and tm["k_spectrum_final"][0] > 0
    assert tile.kernel_bytes("k_spectrum") == 3 * per_plane                  # (1, u), (2, z), (1, r)
    tile.close()
