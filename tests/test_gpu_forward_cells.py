"""spectralTransform! as k_fl_forward_cells + k_nodes_z (the forward FFT kernel sums its ring spectra into the spline nodes itself)
against the pair it replaces (SX_SBW_MFMA=2: ring spectra through d_Fl into k_sbw_mfma), from the same var_np1.

The two paths differ only in where the sum over a node's rings is split at the forward segments' edges, so they are two correct fp64
evaluations of B.  The rule is check_full's (tests/cases.py, PARITY_CLAIM): per variable
    max|B_cells - B_rings| / max|B| <= 10 x the spread between the numpy oracle and the C oracle for the same input and shape, and
    max|B_cells - B_numpy| <= 2 x max|B_rings - B_numpy|.
Every case prints its figures.  The segment length S is asked of the library (sx_launch_plan, SX_PLAN_FORWARD_CELLS).  By default the
library takes the pair only on launches of the measured kind (the bench grid); the small grids here take it with SX_SBW_MFMA=3.

One case passes exactly on the second bound: "cells 10 (S 3)" variable 1 and "3 tiles, tile 0" variable 3 measure 2 ulp of the largest
entry against the ring-spectra pair's 1 ulp (ratio 2.00); every other case measures <= 1.5.  A change of summation order in either
path can move those two by an ulp."""
import numpy as np
import pytest

from oracle import oracle_c as OC
from tests import cases

PLAN_FORWARD_CELLS = 3      # include/scythe_hip.h
FORCE = {"SX_SBW_MFMA": "3"}  # the pair wherever its kernels apply; "2": ring spectra everywhere


def _case(L, nc, nz, nvars=6, bz=None):
    """HRBL grid (6 variables, the mixed radial boundary conditions of bench.py) or a one-variable grid without an equation set."""
    if nvars == 6:
        case = cases.rlz_hrbl(num_cells=nc, zDim=nz, ring_L=L)
    else:
        case = dict(name="rlz_one", grid=dict(geometry="RLZ", xmin=0.0, xmax=3.0e5, num_cells=nc, vars={"h": 1}, BCL={"h": "R1T1"},
                                              BCR={"h": "R0"}, zmin=0.0, zmax=2000.0, zDim=nz, ring_L=L),
                    eq="None", ts=1.0, par={},
                    ic=lambda p: (100.0 * np.exp(-(p[:, 0] / 1.0e5) ** 2) * (1 + 0.1 * np.cos(2 * p[:, 1])) * (1 + p[:, 2] / 2000.0))[:, None])
    if bz is not None:
        case["grid"]["b_zDim"] = bz
    return case


def _plan(case, ncells=None):
    g, K2, nc = cases._handle_dims(case, None if ncells is None else (0, ncells))
    kernel, out = cases.launch_plan(PLAN_FORWARD_CELLS, cases.GEOM["RLZ"], g.zDim, g.b_zDim, K2, g.V, nc, 0, case["grid"]["ring_L"], env=FORCE)
    return kernel, dict(on=out[0], S=out[1], segs=out[2], threads=out[3], nps=out[4], zsegs=out[5])


def _S(L=16, nz=32, nc=12):
    return _plan(_case(L, nc, nz))[1]["S"]


def _values(g, case, seed):
    """The vortex initial condition plus a seeded random field of each variable's own magnitude."""
    import scythe_jl_amd as S
    pts = S.getGridpoints(g)
    ic = np.asarray(case["ic"](pts.reshape(len(pts), -1)), dtype=np.float64)
    amp = np.maximum(np.abs(ic).max(axis=0), 1.0)
    return ic + 0.25 * amp * np.random.default_rng(seed).standard_normal(ic.shape)


def _b(monkeypatch, case, cells, vals=None, seed=5):
    import scythe_jl_amd as S
    monkeypatch.setenv("SX_SBW_MFMA", "3" if cells else "2")
    g = S.Grid(*cases.hip_params(case))
    if vals is None:
        vals = _values(g, case, seed)
    g.set_physical_values(vals)
    g.spectralTransform_()
    B = g.spectral
    alloc = (g.kernel_bytes("alloc.d_Fl"), g.kernel_bytes("alloc.d_Fn"))
    g.close()
    return vals, B, alloc


def _check(label, og, vals, Bn, Bo, cell0=0, ncells=None):
    """The rule of the module docstring, per variable; returns the largest two ratios."""
    Bnp = og.forward(vals, cell0, og.nc if ncells is None else ncells)
    Bc = OC.TileOracle(og, cell0, ncells).forward(vals)
    assert Bn.shape == Bo.shape == Bnp.shape == Bc.shape, (Bn.shape, Bo.shape, Bnp.shape, Bc.shape)
    assert np.isfinite(Bn).all()
    worst = [0.0, 0.0]
    for v in range(Bn.shape[1]):
        sc = np.abs(Bnp[:, v]).max()
        spread = np.abs(Bnp[:, v] - Bc[:, v]).max() / sc
        d = np.abs(Bn[:, v] - Bo[:, v]).max() / np.abs(Bo[:, v]).max()
        en, eo = np.abs(Bn[:, v] - Bnp[:, v]).max() / sc, np.abs(Bo[:, v] - Bnp[:, v]).max() / sc
        print("%s var %d: |cells - rings| %.2e, oracle spread %.2e (ratio %.2f); vs numpy: cells %.2e, rings %.2e (ratio %.2f)"
              % (label, v, d, spread, d / spread if spread > 0 else np.inf if d > 0 else 0.0, en, eo, en / eo if eo > 0 else np.inf if en > 0 else 0.0))
        worst[0] = max(worst[0], d / spread if spread > 0 else (np.inf if d > 0 else 0.0))
        worst[1] = max(worst[1], en / eo if eo > 0 else (np.inf if en > 0 else 0.0))
        assert d <= 10.0 * spread, (label, v, d, spread)
        assert en <= 2.0 * eo, (label, v, en, eo)
    return worst


def _ab(monkeypatch, case, label):
    vals, Bn, alloc_n = _b(monkeypatch, case, True)
    _, Bo, alloc_o = _b(monkeypatch, case, False, vals)
    assert alloc_n[0] == 0 and alloc_n[1] > 0 and alloc_o[0] > 0 and alloc_o[1] == 0, (alloc_n, alloc_o)
    return _check(label, cases.oracle_grid(case), vals, Bn, Bo)


def _cell_counts():
    S = _S()
    return sorted({3, S, S + 1, 2 * S + 3, 3 * S + 1})


def test_the_plan_takes_the_pair_where_both_kernels_are_taken_today():
    """Host only: taken on uniform power-of-two rings up to 256 points with 32 / 64 / 128 levels, never with SX_SBW_MFMA=2, on native
    rings, at 512 points, at other level counts or for fp32 spectra; S >= 3, and the counts below leave a last segment of one cell."""
    for L in (16, 64, 256):
        for nz in (32, 64):
            kernel, p = _plan(_case(L, 24, nz))
            assert p["on"] == 1 and p["S"] >= 3 and p["segs"] == -(-24 // p["S"]) and kernel == "k_fl_forward_cells<%d>" % (L.bit_length() - 1)
    case = _case(16, 12, 32)
    g, K2, nc = cases._handle_dims(case)
    args = (cases.GEOM["RLZ"], g.zDim, g.b_zDim, K2, g.V, nc, 0)
    assert cases.launch_plan(PLAN_FORWARD_CELLS, *args, 16, env={"SX_SBW_MFMA": "2"})[1][0] == 0
    assert cases.launch_plan(PLAN_FORWARD_CELLS, *args, 0, env=FORCE)[1][0] == 0
    assert cases.launch_plan(PLAN_FORWARD_CELLS, *args, 512, env=FORCE)[1][0] == 0
    assert cases.launch_plan(PLAN_FORWARD_CELLS, cases.GEOM["RLZ"], g.zDim, g.b_zDim, K2, g.V, nc, 1, 16, env=FORCE)[1][0] == 0
    assert cases.launch_plan(PLAN_FORWARD_CELLS, cases.GEOM["RLZ"], 48, 32, K2, g.V, nc, 0, 16, env=FORCE)[1][0] == 0
    assert cases.launch_plan(PLAN_FORWARD_CELLS, cases.GEOM["RL"], 1, 1, K2, g.V, nc, 0, 16, env=FORCE)[1][0] == 0
    S = _S()
    assert any(n % S == 1 and n > S for n in _cell_counts())
    # by default only launches of the measured kind: not this small grid, not a tile of an 8-way split of the bench grid (21 cells)
    assert cases.launch_plan(PLAN_FORWARD_CELLS, *args, 16, env=None)[1][0] == 0
    assert cases.launch_plan(PLAN_FORWARD_CELLS, cases.GEOM["RLZ"], 64, 43, 256, 6, 21, 0, 256, env=None)[1][0] == 0
    assert cases.launch_plan(PLAN_FORWARD_CELLS, cases.GEOM["RLZ"], 64, 43, 256, 6, 21, 0, 256, env=FORCE)[1][:3] == [1, 3, 7]
    # a longer segment with a last segment of one cell (the GPU case below): 41 cells, 64 levels -> S = 5, 9 segments
    assert _plan(_case(16, 41, 64))[1]["S"] == 5 and _plan(_case(16, 41, 64))[1]["segs"] == 9
    # the bench grid: one workgroup per (chunk, variable, segment), 10 segments of 18 cells = 240 workgroups, one per CU
    assert cases.launch_plan(PLAN_FORWARD_CELLS, cases.GEOM["RLZ"], 64, 43, 256, 6, 171, 0, 256, env=None)[1][:3] == [1, 18, 10]


@pytest.mark.gpu
@pytest.mark.parametrize("nc", _cell_counts())
def test_cell_counts_around_the_segment_length(monkeypatch, nc):
    """3, S, S + 1, 2 S + 3 cells and a count that leaves one cell in the last segment (16-point rings, 32 levels, 6 variables)."""
    _ab(monkeypatch, _case(16, nc, 32), "cells %d (S %d)" % (nc, _S()))


@pytest.mark.gpu
def test_segments_of_five_cells_with_a_last_segment_of_one(monkeypatch):
    """41 cells, 64 levels, 6 variables: S = 5, so nodes with no edge partial are closed and k_nodes_z reads interior nodes (j >= 3);
    the ninth segment holds one cell."""
    assert _S(16, 64, 41) == 5
    _ab(monkeypatch, _case(16, 41, 64), "cells 41 (S 5)")


@pytest.mark.gpu
@pytest.mark.parametrize("full_bz", [False, True], ids=["bz-default", "bz-zDim"])
@pytest.mark.parametrize("nz", [32, 64])
@pytest.mark.parametrize("L", [16, 64, 256])
def test_ring_lengths_levels_and_truncation(monkeypatch, L, nz, full_bz):
    """L 16 / 64 / 256, 32 / 64 levels, b_zDim default and = zDim; the inner rings are truncated at kmax(ri) = ri (71 of them at
    256 points and 24 cells); one variable at 256 points (the six-variable grids are the other lengths)."""
    nc = 24 if L == 256 else 7
    case = _case(L, nc, nz, nvars=1 if L == 256 else 6, bz=nz if full_bz else None)
    og = cases.oracle_grid(case)
    trunc = int((og.kmax[:og.rDim] < og.kDim).sum())
    assert trunc == 71 if L == 256 else trunc > 0, trunc
    _ab(monkeypatch, case, "L %d zDim %d b_zDim %d" % (L, nz, og.b_zDim))


@pytest.mark.gpu
@pytest.mark.parametrize("ntiles", [2, 3])
def test_every_tile_of_a_split_patch(monkeypatch, ntiles):
    """2 and 3 tiles of one process's multi-tile ModelRun: every tile's B rows; the outer tiles' rings are all at full kmax."""
    case = _case(16, 21, 32)
    og = cases.oracle_grid(case)
    got = {}
    for cells in (True, False):
        monkeypatch.setenv("SX_SBW_MFMA", "3" if cells else "2")
        hip = cases.HipModel(case, num_tiles=ntiles)
        for t, g in enumerate(hip.run.tiles):
            vals = got[(t, "vals")] if (t, "vals") in got else _values(g, case, 40 + t)
            g.set_physical_values(vals)
            g.spectralTransform_()
            got[(t, "vals")], got[(t, cells)], got[(t, "tile")] = vals, g.spectral, (g.cell0, g.ncells)
            assert (g.kernel_bytes("alloc.d_Fl") == 0) == cells
        hip.run.close()
    full = 0
    for t in range(ntiles):
        c0, n = got[(t, "tile")]
        full += int(og.kmax[3 * c0:3 * (c0 + n)].min() == og.kDim)
        _check("%d tiles, tile %d (cells %d..%d)" % (ntiles, t, c0, c0 + n - 1), og, got[(t, "vals")], got[(t, True)], got[(t, False)], c0, n)
    assert full >= 1, "no tile with every ring at full kmax"


@pytest.mark.gpu
def test_the_deferred_diagnostic_window(monkeypatch):
    """SX_DEFER_DIAG=1: a step sends 5 variables through the pair, reading B the sixth alone (v_lo = 5, v_cnt = 1); against the ring-spectra
    pair's transform of the same var_np1."""
    import scythe_jl_amd as S
    case = _case(32, 7, 64)
    monkeypatch.setenv("SX_DEFER_DIAG", "1")
    monkeypatch.setenv("SX_SBW_MFMA", "3")
    hip = cases.HipModel(case)
    hip.step()
    t = hip.run.tiles[0]
    vals, Bn = t.var_np1, t.spectral
    assert t.kernel_bytes("alloc.d_Fl") == 0
    hip.run.close()
    monkeypatch.delenv("SX_DEFER_DIAG")
    _, Bo, _ = _b(monkeypatch, case, False, vals)
    _check("SX_DEFER_DIAG=1", cases.oracle_grid(case), vals, Bn, Bo)


@pytest.mark.gpu
def test_graph_replay_is_bitwise_the_plain_launches(monkeypatch):
    """SX_GRAPH=1, 3 steps with the pair: the fields equal those of plain launches bit for bit."""
    case = _case(32, 7, 32)
    monkeypatch.setenv("SX_SBW_MFMA", "3")
    out = []
    for graph in ("0", "1"):
        monkeypatch.setenv("SX_GRAPH", graph)
        hip = cases.HipModel(case)
        for _ in range(3):
            hip.step()
        out.append(hip.physical())
        assert hip.run.tiles[0].kernel_bytes("alloc.d_Fl") == 0
        hip.run.close()
    assert np.isfinite(out[0]).all() and np.array_equal(out[0], out[1])


@pytest.mark.gpu
def test_the_ring_spectra_are_not_allocated(monkeypatch):
    """With the pair the handle holds node spectra and edge partials, [nbt + 3 segments] rows, and no ring spectra, [3 cells] rows."""
    import scythe_jl_amd as S
    case = _case(64, 12, 64)
    _, p = _plan(case)
    sizes = {}
    for cells in (True, False):
        monkeypatch.setenv("SX_SBW_MFMA", "3" if cells else "2")
        g = S.Grid(*cases.hip_params(case))
        row = 8.0 * g.V * 64 * 2 * (cases.oracle_grid(case).kDim + 1)
        sizes[cells] = (g.kernel_bytes("alloc.d_Fl") / row, g.kernel_bytes("alloc.d_Fn") / row, g.kernel_bytes("alloc.total"))
        g.close()
    assert sizes[True][:2] == (0.0, 12 + 3 + 3 * (p["segs"] - 1)) and sizes[False][:2] == (36.0, 0.0), sizes
    assert sizes[True][2] < sizes[False][2]
