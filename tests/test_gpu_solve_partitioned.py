"""-m gpu: the partitioned one-tile B -> A solve (k_solve_part, csrc/sx_iface.hip: 4 waves of a workgroup each own a block of rows of
the same 64 columns, the forward-sweep vector stays in registers) against k_solve (SX_SOLVE_PCR=0) and the dense definition of the
solve, per spectral column, every column.

Shapes: RLZ, 16-point rings, 8 levels, the bench's six variables and boundary-condition sets (cases.rlz_hrbl), so every class of the
headline occurs.  Cells: 9 P = 36 (the smallest partitions the plan admits), 37 and 39 (uneven partitions), 171 (the headline's
174 rows: 44 unknowns in a partition, the register array's size).  The launches are small, so the kernel is asked for by
SX_SOLVE_PCR=2 (wherever its tables exist); which kernel ran is read from the library: sx_launch_plan for the shape, and the bytes
sx_kernel_bytes accounts for the last k_solve launch (2 x S_patch x 8: B in, A out; 4 x: the round trip of y that k_solve makes).

Bars: those of tests/test_gpu_solve.py - 1e-13 between the two device kernels, 1e-12 against the dense solve (condition numbers and the
dense solve's own noise: there)."""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu
P = 4
PLAN_SOLVE = 4      # include/scythe_hip.h


def _case(cells):
    return cases.rlz_hrbl(num_cells=cells, zDim=8, ring_L=16)


def _grids(monkeypatch, case):
    """(handle under SX_SOLVE_PCR=2, handle under SX_SOLVE_PCR=0)"""
    import scythe_jl_amd as S
    gp, mp = cases.hip_params(case)
    monkeypatch.setenv("SX_SOLVE_PCR", "2")
    g2 = S.Grid(gp, mp)
    monkeypatch.setenv("SX_SOLVE_PCR", "0")
    g0 = S.Grid(gp, mp)
    monkeypatch.delenv("SX_SOLVE_PCR")
    return g2, g0


def _solve(g, shared):
    g.set_patch_spectral_b(shared)
    g.splineTransform_()
    return g.patchSpectral, g.kernel_bytes("k_solve") / (8.0 * g.dims.b_rDim * g.dims.n_cols)


def _solve_both(monkeypatch, case, shared=None):
    g2, g0 = _grids(monkeypatch, case)
    if shared is None:
        shared = np.random.default_rng(5).standard_normal((int(g2.dims.s_patch), g2.V))
    (a2, passes2), (a0, passes0) = _solve(g2, shared), _solve(g0, shared)
    g2.close()
    g0.close()
    return shared, a2, a0, passes2, passes0


def _plan(case, env):
    g, K2, _ = cases._handle_dims(case)
    periodic = any(b == "PERIODIC" for b in list(g.BCL.values()) + list(g.BCR.values()))
    ncols = g.V * g.b_zDim * (K2 - 1 if K2 > 1 else 1)
    return cases.launch_plan(PLAN_SOLVE, g.b_rDim, int(periodic) + 1, 2, ncols, env=env)


def _check_columns(case, shared, part, lane):
    nb = case["grid"]["num_cells"] + 3
    assert np.isfinite(part).all() and np.abs(part).max() > 0
    ref = cases.dense_spline_transform(case, shared)
    e_pl = cases.rel_err_per_column(part, lane, nb)
    e_pr, e_lr = cases.rel_err_per_column(part, ref, nb), cases.rel_err_per_column(lane, ref, nb)
    print("%d cells, %d columns: partitioned vs k_solve %.2e, partitioned vs dense %.2e, k_solve vs dense %.2e"
          % (nb - 3, e_pl.size, e_pl.max(), e_pr.max(), e_lr.max()))
    assert e_pl.max() <= 1e-13, ("partitioned vs k_solve", int(e_pl.argmax()), e_pl.max())
    assert e_pr.max() <= 1e-12, ("partitioned vs dense", int(e_pr.argmax()), e_pr.max())


@pytest.mark.parametrize("cells", [9 * P, 9 * P + 1, 9 * P + P - 1, 171])
def test_partitioned_solve_per_column(monkeypatch, cells):
    case = _case(cells)
    assert _plan(case, {"SX_SOLVE_PCR": "2"}) == ("k_solve_part", [P, 64 * P, 0, 0, 0, 0])
    shared, part, lane, passes2, passes0 = _solve_both(monkeypatch, case)
    assert (passes2, passes0) == (2.0, 4.0)              # k_solve_part ran under SX_SOLVE_PCR=2, k_solve under 0
    _check_columns(case, shared, part, lane)


def test_one_cell_below_the_smallest_partition_keeps_k_solve(monkeypatch):
    case = _case(9 * P - 1)
    assert _plan(case, {"SX_SOLVE_PCR": "2"})[0] == "k_solve"
    shared, part, lane, passes2, passes0 = _solve_both(monkeypatch, case)
    assert (passes2, passes0) == (4.0, 4.0)
    assert np.array_equal(part, lane)


def test_the_default_plan_takes_it_where_the_launch_fills_the_chip():
    """Without the switch: the bench grid (65,790 columns) takes the partitioned kernel, the small shapes of this file keep PCR /
    k_solve, and SX_SOLVE_PCR=0 / 1 never take it."""
    full = cases.rlz_hrbl(num_cells=171, zDim=64, ring_L=256)
    assert _plan(full, None)[0] == "k_solve_part"
    assert _plan(full, {"SX_SOLVE_PCR": "0"})[1][0] == 0 and _plan(full, {"SX_SOLVE_PCR": "1"})[1][0] == 0
    assert _plan(_case(171), None)[1][0] == 0
    assert _plan(cases.rlz_hrbl(num_cells=174, zDim=64, ring_L=256), None)[1][0] == 0      # 177 rows: beyond 4 x 44 registers


@pytest.mark.parametrize("cells", [9 * P + 1])
def test_unit_right_hand_sides_at_every_partition_edge(monkeypatch, cells):
    """One solve whose columns are unit vectors: column j (in the library's column order) holds a 1 in one patch row, the rows cycling
    through the first and last three rows of every partition of both classes of every variable (and the boundary rows), so that
    each coupling block meets a right-hand side a smooth field would hide it from."""
    case = _case(cells)
    g = cases.oracle_grid(case)
    nb = g.b_rDim
    cols = g.b_zDim * g.K2
    shared = np.zeros((nb * cols, g.V))
    edge_rows = set(range(4)) | set(range(nb - 4, nb))
    for n in range(nb - 3, nb + 1):                       # unknown counts 3 - rl - rr below nb: every class's partition bounds
        for p in range(1, P):
            u = n * p // P
            edge_rows |= {r for r in range(u - 3, u + 7) if 0 <= r < nb}
    rows = sorted(edge_rows)
    for v in range(g.V):
        x = shared[:, v].reshape(cols, nb)
        for j in range(cols):
            x[j, rows[(j + 5 * v) % len(rows)]] = 1.0
    assert len(rows) <= cols                              # every row occurs in every variable (k = 0 and k >= 1 columns alike below)
    shared, part, lane, passes2, _ = _solve_both(monkeypatch, case, shared)
    assert passes2 == 2.0
    _check_columns(case, shared, part, lane)
    # and the k = 0 columns (their own class: one per z-mode) with every edge row in turn
    for shift in range(0, len(rows), g.b_zDim):
        sh = np.zeros_like(shared)
        for v in range(g.V):
            x = sh[:, v].reshape(g.b_zDim, g.K2, nb)
            for z in range(g.b_zDim):
                x[z, :, rows[(shift + z) % len(rows)]] = 1.0
        _, part, lane, _, _ = _solve_both(monkeypatch, case, sh)
        e = cases.rel_err_per_column(part, lane, nb)
        assert e.max() <= 1e-13, (shift, int(e.argmax()), e.max())


@pytest.mark.parametrize("make", [lambda: cases.kat_r(num_cells=100), lambda: cases.kat_in_geometry("RLZ")], ids=["periodic-R", "periodic-RLZ"])
def test_periodic_grids_keep_k_solve(monkeypatch, make):
    """PERIODIC classes (an R grid's one column, an RLZ grid): the fallback is taken, the fields are those of SX_SOLVE_PCR=0 bit for bit."""
    case = make()
    assert _plan(case, {"SX_SOLVE_PCR": "2"}) == ("k_solve", [0, 64, 0, 0, 0, 0])
    shared, part, lane, passes2, passes0 = _solve_both(monkeypatch, case)
    assert (passes2, passes0) == (4.0, 4.0)
    assert np.array_equal(part, lane)


def _steps(case, n, env, monkeypatch):
    for k in ("SX_SOLVE_PCR", "SX_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = cases.HipModel(case)
    for _ in range(n):
        m.step()
    tile = m.run.tiles[0]
    out = tile.var_np1, np.asarray(m.A), tile.kernel_bytes("k_solve") / (8.0 * tile.dims.b_rDim * tile.dims.n_cols)
    m.run.close()
    return out


def test_twenty_model_steps_against_k_solve(monkeypatch):
    case = _case(9 * P + 1)
    np1_p, A_p, passes_p = _steps(case, 20, {"SX_SOLVE_PCR": "2"}, monkeypatch)
    np1_0, A_0, passes_0 = _steps(case, 20, {"SX_SOLVE_PCR": "0"}, monkeypatch)
    assert (passes_p, passes_0) == (2.0, 4.0)
    assert np.isfinite(np1_p).all()
    e_np1 = max(cases.rel_err(np1_p[:, v], np1_0[:, v]) for v in range(np1_0.shape[1]) if np.abs(np1_0[:, v]).max() > 0)
    e_A = max(cases.rel_err(A_p[:, v], A_0[:, v]) for v in range(A_0.shape[1]) if np.abs(A_0[:, v]).max() > 0)
    print("20 steps, partitioned vs k_solve: var_np1 %.2e, spectral_a %.2e" % (e_np1, e_A))
    assert e_np1 <= 1e-10 and e_A <= 1e-10


def test_graph_replay_with_the_partitioned_kernel_is_bit_identical(monkeypatch):
    case = _case(9 * P + 1)
    np1_g, A_g, passes_g = _steps(case, 6, {"SX_SOLVE_PCR": "2", "SX_GRAPH": "1"}, monkeypatch)
    np1_p, A_p, passes_p = _steps(case, 6, {"SX_SOLVE_PCR": "2"}, monkeypatch)
    assert (passes_g, passes_p) == (2.0, 2.0)
    assert np.array_equal(np1_g, np1_p) and np.array_equal(A_g, A_p)
