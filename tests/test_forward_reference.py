"""The references of tests/test_gpu_forward.py, checked without a GPU: oracle_np.forward_xp (spectralTransform! in extended
precision with its condition scale) and the library's launch plans for launch_sb / launch_zinv (sx_launch_plan through
cases.sb_launch_geometry / zinv_launch_geometry), pinned on shapes worked out by hand from the launcher code."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import cases

# the oracle's Grid.forward evaluates the basis at the Float64 mish points of the tile (delta = (x - x_node) / DX with x rounded):
# a basis value near the end of its support (3e-4 of the largest) then carries the rounding of x / DX relative to itself, up to
# (x / DX) ulp of it.  Measured at most 58 (RL, 8 cells) on these cases; forward_xp uses the exact offsets, as the HIP tables do.
C_ORACLE = 128

XP_CASES = [
    ("rlz_hrbl", lambda: cases.rlz_hrbl(num_cells=5, zDim=10, ring_L=16), None),
    ("rlz_adv-native", lambda: cases.rlz_advection(), None),
    ("rlz_adv-z64-tile", lambda: cases.rlz_advection(num_cells=9, zDim=64, ring_L=32), (3, 4)),
    ("rlz_adv-native-tile", lambda: cases.rlz_advection(num_cells=8, zDim=9), (5, 3)),
    ("rz_adv", lambda: cases.rz_advection(), None),
    ("rl_adv-native", lambda: cases.rl_advection(), None),
    ("r_bcs", lambda: cases.r_bcs(), None),
]


def _tile_values(g, tile, seed):
    c0, n = tile if tile else (0, g.nc)
    return c0, n, np.random.default_rng(seed).standard_normal((g.tile_npoints(c0, n), g.V))


@pytest.mark.parametrize("make,tile", [(m, t) for _, m, t in XP_CASES], ids=[n for n, _, _ in XP_CASES])
def test_forward_xp_is_the_oracle_forward_with_a_scale_that_bounds_b(make, tile):
    """forward_xp agrees with Grid.forward within C_ORACLE 2^-53 of its per-entry scale, the scale bounds |B| (it is the sum of
    the same terms' magnitudes), and entries of zero scale (blocks above a ring's kmax) are zero in both."""
    g = cases.oracle_grid(make())
    c0, n, vals = _tile_values(g, tile, 7)
    B, S = O.forward_xp(g, vals, c0, n)
    f = g.forward(vals, c0, n)
    assert B.dtype == O.XP and B.shape == f.shape == S.shape
    assert (S >= np.abs(B)).all()
    zero = S == 0
    assert not np.any(f[zero]) and not np.any(B[zero])
    c = float((np.abs(f.astype(O.XP) - B)[~zero] / S[~zero]).max() / O.XP(2.0 ** -53))
    assert c <= C_ORACLE, c
    # and the scale is not loose: random values leave |B| within ~sqrt(terms) of it, never 1e-3 below it everywhere
    assert float(np.median(np.abs(B[~zero]) / S[~zero])) > 1e-3


def test_forward_xp_tiles_sum_to_the_patch():
    """The reference's shared-array protocol: tile B arrays added into the patch array are the patch B (forward_xp per tile)."""
    g = cases.oracle_grid(cases.rlz_advection(num_cells=9, zDim=12, ring_L=32))
    _, _, vals = _tile_values(g, None, 8)
    B, S = O.forward_xp(g, vals)
    shared = np.zeros_like(B)
    base = 0
    for c0, n in cases.even_tiles(g.nc, 3):
        N = g.tile_npoints(c0, n)
        Bt, _ = O.forward_xp(g, vals[base:base + N], c0, n)
        g.add_tile_to_shared(shared, Bt, c0, n, False)
        base += N
    assert (np.abs(shared - B) <= O.XP(2.0 ** -53) * S).all()           # far below an fp64 rounding of B


@pytest.mark.parametrize("make", [lambda: cases.rl_advection(num_cells=6, ring_L=16), lambda: cases.rz_advection(),
                                  lambda: cases.rlz_advection(num_cells=5, zDim=12, ring_L=16)], ids=["RL", "RZ", "RLZ"])
def test_spline_solve_of_forward_xp_is_the_c_oracle_a(make):
    """The B of forward_xp (rounded to fp64) through the oracle's spline solve gives the A the C oracle computes from the same
    (random) initial values with its own forward + solve, per spectral column."""
    case = make()
    orc = cases.OracleModel(case)
    g = orc.g
    vals = np.random.default_rng(9).standard_normal((len(orc.pts), g.V))
    orc.m.set_initial(vals)
    B, _ = O.forward_xp(g, vals)
    A = cases.dense_spline_transform(case, np.asarray(B, dtype=np.float64))
    e = cases.rel_err_per_column(A, np.asarray(orc.A), g.b_rDim)
    assert e.max() < 1e-12, e.max()


# ----------------------------------------------------------------------------- launcher mirrors, worked by hand
def _sb(case, env=None, **kw):
    return cases.sb_launch_geometry(case, env, **kw)


def test_sb_mirror_on_the_bench_grid():
    """rlz_hrbl 171 cells x 256 x 64, b_zDim 43: K2 = 2 (127 + 1) = 256; matrix cores (43 <= 64) at 256 threads, bw 32;
    groups = 8 x 6 = 48, nseg = 512 // 48 = 10, cps = max(6, ceil(171 / 10)) = 18, segs 10, last 171 - 9 x 18 = 9;
    MT 3, mhalf 2, waves (mt0, mt1) = (0, 2) (0, 2) (1, 3) (1, 3): two row tiles, two, one, one."""
    case = cases.rlz_hrbl(num_cells=171, zDim=64, ring_L=256)
    assert _sb(case) == dict(kernel="k_sbw_mfma<64, 32, 256>", threads=256, bw=32, groups=48, nseg=10, cps=18, segs=10, last=9,
                             tail=0, ncells=171, K2=256, MT=3, mhalf=2, nmt=(2, 2, 1, 1))
    # SX_DEFER_DIAG's step window (5 variables): groups 40, nseg 12, cps max(6, 15) = 15, segs 12, last 6
    geo = _sb(case, v_cnt=5)
    assert (geo["groups"], geo["nseg"], geo["cps"], geo["segs"], geo["last"]) == (40, 12, 15, 12, 6)
    # SX_SBW_T256=0: k_sbw_mfma<64> at 512 threads, bw 64: groups 24, nseg 256 // 24 = 10 (the 512 budget is only for bw 32),
    # cps 18, segs 10, last 9; waves 0-3 own mhalf = 2 row tiles, waves 4-7 the third
    geo = _sb(case, {"SX_SBW_T256": "0"})
    assert (geo["kernel"], geo["threads"], geo["bw"], geo["nseg"], geo["cps"], geo["segs"], geo["last"]) == \
        ("k_sbw_mfma<64>", 512, 64, 10, 18, 10, 9)
    assert geo["nmt"] == (2, 2, 2, 2, 1, 1, 1, 1)
    assert cases.zinv_launch_geometry(case) == dict(kernel="k_colmat_mfma<4, double, 1>", MT=4, CT=1, OT="double", grid_x=4,
                                                    tail=0, K2=256)


def test_sb_mirror_at_128_levels():
    """rlz_hrbl 4 cells x 16 x 128, b_zDim 86: K2 16, k_sbw_mfma<128, 32> (86 <= 96), bw 32, groups 6, nseg 512 // 6 = 85,
    cps max(2, 1) = 2, segs 2; MT 6, mhalf 3, waves w: mt0 = w >> 1, mt1 = mt0 + 4 -> 2 2 2 2 1 1 1 1 tiles.
    b_zDim 97: k_sbw<128, false>, bw 64, groups 6, nseg 256 // 6 = 42.  zinv: CT 2 (default), 1 / 4 on request, else 2."""
    geo = _sb(cases.rlz_hrbl(num_cells=4, zDim=128, ring_L=16))
    assert (geo["kernel"], geo["threads"], geo["bw"], geo["groups"], geo["nseg"], geo["cps"], geo["segs"], geo["tail"]) == \
        ("k_sbw_mfma<128, 32>", 512, 32, 6, 85, 2, 2, 16)
    assert (geo["MT"], geo["mhalf"], geo["nmt"]) == (6, 3, (2, 2, 2, 2, 1, 1, 1, 1))
    case = cases.rlz_hrbl(num_cells=4, zDim=128, ring_L=16)
    case["grid"]["b_zDim"] = 97
    geo = _sb(case)
    assert (geo["kernel"], geo["bw"], geo["nseg"], "MT" in geo) == ("k_sbw<128, false>", 64, 42, False)
    assert _sb(case, storage="f32x")["kernel"] is None                         # sx_create refuses this shape
    for ct, want in ((None, 2), ("1", 1), ("2", 2), ("3", 2), ("4", 4)):
        z = cases.zinv_launch_geometry(case, {"SX_ZINV_CT": ct} if ct else None)
        assert (z["kernel"], z["grid_x"], z["tail"]) == ("k_colmat_mfma<8, double, %d>" % want, 1, 16)
    assert cases.zinv_launch_geometry(case, storage="f32x")["kernel"] == "k_colmat_mfma<8, float, 2>"


def test_sb_mirror_segments_and_switches():
    """rlz_advection on 16-point rings (K2 16, 3 variables) at zDim 32, b_zDim 22: k_sbw_mfma<32>, groups 3, nseg 85:
    7 cells -> cps 2, segs 4, last 1; 65 cells -> cps max(6, 1) = 6, segs 11, last 5.  SX_SBW_MFMA=0: k_sbw<32, false>,
    nseg 384 // 3 = 128; with SX_SBW_PF=1 k_sbw<32, true>, nseg 85.  SX_SBW_SEG=4 at 10 cells: cps 3, segs 4, last 1."""
    def c(n, nz=32, b=22, L=16):
        case = cases.rlz_advection(num_cells=n, zDim=nz, ring_L=L)
        case["grid"]["b_zDim"] = b
        return case
    g7 = _sb(c(7))
    assert (g7["kernel"], g7["groups"], g7["nseg"], g7["cps"], g7["segs"], g7["last"]) == ("k_sbw_mfma<32>", 3, 85, 2, 4, 1)
    g65 = _sb(c(65))
    assert (g65["cps"], g65["segs"], g65["last"]) == (6, 11, 5)
    assert (_sb(c(7), {"SX_SBW_MFMA": "0"})["kernel"], _sb(c(7), {"SX_SBW_MFMA": "0"})["nseg"]) == ("k_sbw<32, false>", 128)
    pf = _sb(c(7), {"SX_SBW_MFMA": "0", "SX_SBW_PF": "1"})
    assert (pf["kernel"], pf["nseg"]) == ("k_sbw<32, true>", 85)
    s4 = _sb(c(10), {"SX_SBW_SEG": "4"})
    assert (s4["nseg"], s4["cps"], s4["segs"], s4["last"]) == (4, 3, 4, 1)
    # 3 cells of 64-point rings: kmax 9, K2 20 < bw 32; 11 cells of 512-point rings: K2 68, tail 4 at bw 64
    assert (_sb(c(3, 64, 43, 64))["K2"], _sb(c(3, 64, 43, 64))["tail"]) == (20, 20)
    assert (_sb(c(11, 32, 22, 512))["K2"], _sb(c(11, 32, 22, 512))["tail"], _sb(c(11, 32, 22, 512))["groups"]) == (68, 4, 6)
    # zDim 64 with SX_SBW_MFMA=0: k_sbw<64, false>; with SX_SBW_PF=1 k_sbw<64, true>
    off = {"SX_SBW_MFMA": "0"}
    assert _sb(c(4, 64, 43), off)["kernel"] == "k_sbw<64, false>" and _sb(c(4, 64, 64), off | {"SX_SBW_PF": "1"})["kernel"] == "k_sbw<64, true>"
    # zDim 20: k_sbz; zinv k_colmat
    assert _sb(c(4, 20, 13))["kernel"] == "k_sbz" and cases.zinv_launch_geometry(c(4, 20, 13))["kernel"] == "k_colmat"
    # zDim 64 zinv: CT 2 only on request; SX_ZINV_CT=4 takes the default
    assert cases.zinv_launch_geometry(c(4, 64, 43), {"SX_ZINV_CT": "2"})["CT"] == 2
    assert cases.zinv_launch_geometry(c(4, 64, 43), {"SX_ZINV_CT": "4"})["CT"] == 1


def test_sb_mirror_other_geometries():
    assert _sb(cases.rl_advection(num_cells=6, ring_L=16))["kernel"] == "k_sb"
    assert _sb(cases.rz_advection(num_cells=7, zDim=20))["kernel"] == "k_rz_forward"
    assert cases.zinv_launch_geometry(cases.rz_advection(num_cells=7, zDim=20)) is None
    geo = _sb(cases.rz_advection(num_cells=7, zDim=32), {"SX_RZ_FUSED": "0"})
    assert (geo["kernel"], geo["K2"], geo["tail"]) == ("k_sbw_mfma<32>", 1, 1)
