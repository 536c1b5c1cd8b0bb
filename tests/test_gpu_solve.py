"""splineTransform! (B -> A, src/semiimplicit.jl:237, 285) at every launch geometry of the parallel-cyclic-reduction solve.

launch_solve_pcr (csrc/sx_pcr.hip) puts R = 4 / 8 / 16 columns of one boundary-condition class in a workgroup (4 up to 4,096
launch columns, 8 up to 16,384, 16 above), halves R while nblk_max * R > 1024 (nblk = ceil(unknowns / 3)), and runs
roundup64(max(nblk_max * R, b_rDim * R / 4)) threads; with nblk_max > 1024 there are no tables and the launch takes k_solve.
Every case below names that geometry in its id (R, threads, and the column count of the last, partial workgroup of a
variable's k = 0 run / of a group's k >= 1 run); test_the_ids_name_the_launch_geometry checks the ids against the launcher's
arithmetic (cases.pcr_launch_geometry) on the host.

Errors are measured per spectral column (cases.rel_err_per_column): a wrong tail column of a partial workgroup shows whatever
the magnitude of the other columns.  The reference is the oracle's dense definition of the solve, Gamma^T (Gamma (P + eps_q Q)
Gamma^T)^-1 Gamma b by a dense Cholesky factor in fp64.  Its matrices are well conditioned: 2-norm condition number 7.2 for a
PERIODIC class and 3.3e2 for the R0 class (l_q = 2, any cell count), so the dense fp64 solve is good to ~1e-13 of a column's
scale and the bars below (1e-13 between the two device kernels, 1e-12 against the dense solve) are not the reference's noise."""
import numpy as np
import pytest

from tests import cases

TOL = 1e-10


def _kat_rlz(n):
    """The notebook's PERIODIC KAT on an RLZ grid (cases.kat_in_geometry) with n cells, 256-point rings and 128 levels with
    b_zDim = 128: 3 x 128 groups x (2 kmax + 1) columns > 16,384 for n >= 7, so the launch takes R = 16 (at zDim 32 the
    few rings of 7-13 cells give kmax <= 39 and only R = 4)."""
    case = cases.kat_in_geometry("RLZ", ring_L=256, zDim=128)
    case["grid"].update(num_cells=n, b_zDim=128)
    return case


# (id, case maker): id = geometry as launch_solve_pcr computes it
SOLVE_CASES = [
    # R = 16, non-periodic classes (R0 / R1T0 / R1T1: 23-25 unknowns, nblk 8), both runs end in a partial workgroup
    ("rlz_hrbl22x256x32-R16-t128-tail6-tail4", lambda: cases.rlz_hrbl(num_cells=22, zDim=32, ring_L=256)),
    ("rlz_hrbl23x256x32-R16-t192-tail6-tail10", lambda: cases.rlz_hrbl(num_cells=23, zDim=32, ring_L=256)),
    # R = 16, PERIODIC classes of 7-13 unknowns: 64 threads < 6 R = 96 corner-correction entries up to 12 cells, 128 at 13
    ("katRLZ7-periodic-R16-t64-tail16-tail10", lambda: _kat_rlz(7)),
    ("katRLZ8-periodic-R16-t64-tail16-tail16", lambda: _kat_rlz(8)),
    ("katRLZ9-periodic-R16-t64-tail16-tail6", lambda: _kat_rlz(9)),
    ("katRLZ10-periodic-R16-t64-tail16-tail12", lambda: _kat_rlz(10)),
    ("katRLZ11-periodic-R16-t64-tail16-tail2", lambda: _kat_rlz(11)),
    ("katRLZ12-periodic-R16-t64-tail16-tail8", lambda: _kat_rlz(12)),
    ("katRLZ13-periodic-R16-t128-tail16-tail14", lambda: _kat_rlz(13)),
    # R grid (one column): nblk * 4 > 1024 halves R
    ("r_R0_R0-1000-R2-t704-tail1", lambda: cases.r_bcs("R0", "R0", num_cells=1000)),
    ("kat_r-1000-periodic-R2-t704-tail1", lambda: cases.kat_r(num_cells=1000)),
    ("r_R0_R0-2000-R1-t704-tail1", lambda: cases.r_bcs("R0", "R0", num_cells=2000)),
    ("kat_r-2000-periodic-R1-t704-tail1", lambda: cases.kat_r(num_cells=2000)),
    # the largest table (3,072 unknowns, nblk 1024): R = 1 at the 1024-thread limit
    ("r_R0_R0-3069-R1-t1024-tail1", lambda: cases.r_bcs("R0", "R0", num_cells=3069)),
]

# tables too big (3,073 unknowns, nblk 1025): no PCR tables, the launch falls back to k_solve
NO_TABLES = ("r_R0_R0-3070-no-tables-k_solve", lambda: cases.r_bcs("R0", "R0", num_cells=3070))

# transposed multi-tile solve: 2 tiles of 11 cells, 258 groups split 129 / 129 -> 129 x 133 = 17,157 columns per tile
A2A_CASE = lambda: cases.rlz_hrbl(num_cells=22, zDim=64, ring_L=256)
A2A_ID = "rlz_hrbl22x256x64-2tiles-a2a-R16-t128-tail11-tail4"

# the bench grid: 6 x 43 groups x 255 = 65,790 columns, nblk 58
FULL_CASE = lambda: cases.rlz_hrbl(num_cells=171, zDim=64, ring_L=256)
FULL_ID = "rlz_hrbl171x256x64-R16-t960-tail11-tail14"


def _geometry_of_id(name):
    parts = name.split("-")
    R = next(int(p[1:]) for p in parts if p[0] == "R" and p[1:].isdigit())
    threads = next(int(p[1:]) for p in parts if p[0] == "t" and p[1:].isdigit())
    tails = [int(p[4:]) for p in parts if p.startswith("tail")]
    return R, threads, tails


def test_the_ids_name_the_launch_geometry():
    """The geometry in every id is what launch_solve_pcr computes (its plan, through cases.pcr_launch_geometry)."""
    for name, make in SOLVE_CASES + [(FULL_ID, FULL_CASE)]:
        geo = cases.pcr_launch_geometry(make())
        R, threads, tails = _geometry_of_id(name)
        assert geo["tables"] and (geo["R"], geo["threads"]) == (R, threads), (name, geo)
        assert [geo["tail_k0"]] + ([geo["tail_k"]] if geo["tail_k"] is not None else []) == tails, (name, geo)
    assert not cases.pcr_launch_geometry(NO_TABLES[1]())["tables"]
    geo = cases.pcr_launch_geometry(A2A_CASE(), ngroups=129)
    R, threads, tails = _geometry_of_id(A2A_ID)
    assert (geo["R"], geo["threads"], geo["tail_k0"], geo["tail_k"]) == (R, threads, *tails), geo
    assert geo["columns"] > 16384


def test_dense_reference_is_the_oracle_spline_transform():
    """cases.dense_spline_transform (one factor per class, all columns at once) is oracle_np.Grid.spline_transform."""
    for case in (cases.rlz_hrbl(num_cells=5, zDim=10, ring_L=16), cases.kat_in_geometry("RLZ"), cases.rz_semiimplicit()):
        g = cases.oracle_grid(case)
        shared = np.random.default_rng(3).standard_normal((g.b_rDim * g.K2 * g.b_zDim, g.V))
        ref = g.spline_transform(np.asfortranarray(shared))
        assert cases.rel_err_per_column(cases.dense_spline_transform(case, shared), ref, g.b_rDim).max() < 1e-14


def test_per_column_error_sees_a_single_wrong_column():
    a = np.random.default_rng(4).standard_normal((10 * 6, 2))
    b = a.copy()
    b[10 * 5 + 3, 1] += 1e-9 * np.abs(a[10 * 5:10 * 6, 1]).max()        # one node of the last column of variable 1
    e = cases.rel_err_per_column(b, a, 10)
    assert e.shape == (12,) and np.count_nonzero(e) == 1 and abs(e[11] - 1e-9) < 1e-15


def _solve_both(monkeypatch, case, seed=5):
    """splineTransform! on the same random B by a PCR handle (SX_SOLVE_PCR=1) and a lane-per-column handle (SX_SOLVE_PCR=0)."""
    import scythe_jl_amd as S
    gp, mp = cases.hip_params(case)
    monkeypatch.setenv("SX_SOLVE_PCR", "1")
    g1 = S.Grid(gp, mp)
    monkeypatch.setenv("SX_SOLVE_PCR", "0")
    g0 = S.Grid(gp, mp)
    monkeypatch.delenv("SX_SOLVE_PCR")
    shared = np.random.default_rng(seed).standard_normal((int(g1.dims.s_patch), g1.V))
    out = []
    for g in (g1, g0):
        g.set_patch_spectral_b(shared)
        g.splineTransform_()
        out.append(g.patchSpectral)
        g.close()
    return shared, out[0], out[1]


def _check_columns(case, shared, pcr, lane):
    nb = case["grid"]["num_cells"] + 3
    assert np.isfinite(pcr).all() and np.abs(pcr).max() > 0
    ref = cases.dense_spline_transform(case, shared)
    e_pl = cases.rel_err_per_column(pcr, lane, nb)
    e_pr, e_lr = cases.rel_err_per_column(pcr, ref, nb), cases.rel_err_per_column(lane, ref, nb)
    assert e_pl.max() <= 1e-13, ("PCR vs k_solve", int(e_pl.argmax()), e_pl.max())
    assert e_pr.max() <= 1e-12, ("PCR vs dense", int(e_pr.argmax()), e_pr.max())
    assert e_lr.max() <= 1e-12, ("k_solve vs dense", int(e_lr.argmax()), e_lr.max())


@pytest.mark.gpu
@pytest.mark.parametrize("make", [m for _, m in SOLVE_CASES], ids=[n for n, _ in SOLVE_CASES])
def test_pcr_solve_per_column_at_every_launch_geometry(monkeypatch, make):
    """PCR handle vs lane-per-column handle vs the dense solve, per spectral column (geometry in the id)."""
    case = make()
    shared, pcr, lane = _solve_both(monkeypatch, case)
    _check_columns(case, shared, pcr, lane)


@pytest.mark.gpu
def test_pcr_solve_without_tables_falls_back_to_the_lane_per_column_kernel(monkeypatch):
    """3,073 unknowns: nblk_max = 1025 > 1024, pcr_state()->ok is false, and a SX_SOLVE_PCR=1 handle's launch is k_solve's -
    bit-identical to the SX_SOLVE_PCR=0 handle, and the dense solve per column."""
    case = NO_TABLES[1]()
    shared, pcr, lane = _solve_both(monkeypatch, case)
    assert np.array_equal(pcr, lane)
    _check_columns(case, shared, pcr, lane)


@pytest.mark.gpu
def test_transposed_two_tile_solve_at_r16_equals_one_tile_and_oracle(monkeypatch):
    """LINEAR = false launch of k_solve_pcr (rows shared by two tiles summed on input, written to both on output) at R = 16:
    rlz_hrbl 22 cells x 256 x 64 on 2 tiles with exchange="a2a" and SX_SOLVE_PCR=1, 129 groups x 133 = 17,157 columns per tile,
    128 threads, partial workgroups of 11 (k = 0) and 4 (k >= 1) columns.  Model fields after 3 steps against a one-tile
    SX_SOLVE_PCR=0 run (k_solve) and the C oracle."""
    case = A2A_CASE()
    monkeypatch.setenv("SX_SOLVE_PCR", "1")
    multi = cases.HipModel(case, num_tiles=2, exchange="a2a")
    monkeypatch.setenv("SX_SOLVE_PCR", "0")
    one = cases.HipModel(case)
    monkeypatch.delenv("SX_SOLVE_PCR")
    orc = cases.OracleModel(case)
    for _ in range(3):
        multi.step()
        one.step()
        orc.step()
    a, b, c = multi.physical(), one.physical(), orc.physical()
    assert np.isfinite(a).all()
    assert cases.rel_err_per_var(a, b) < TOL
    assert cases.rel_err_per_var(a, c) < TOL
    multi.run.close()
    one.run.close()


@pytest.mark.gpu
def test_pcr_solve_at_full_size_per_column(monkeypatch):
    """The bench grid (rlz_hrbl 171 cells x 256 x 64: 65,790 launch columns, R = 16, 960 threads, partial workgroups of 11 and
    14 columns) with SX_SOLVE_PCR=1 against SX_SOLVE_PCR=0 on random B, per column, and both against the dense solve factored
    once per boundary-condition class."""
    case = FULL_CASE()
    shared, pcr, lane = _solve_both(monkeypatch, case)
    _check_columns(case, shared, pcr, lane)
