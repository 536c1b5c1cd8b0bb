"""-m gpu: the kernel variants behind SX_PCR_R, SX_RZ_INV, SX_SBW_T256 and SX_DFT_HALF.

The library reads every switch once per handle, at sx_create (csrc/sx_api.cpp: read_switches), so a handle created after a
monkeypatch.setenv runs the variant: test_two_handles_of_one_process_take_their_own_columns_per_workgroup holds that.  The older
cases start a child process (tests/child_run.py) with the variable set from its first instruction on, which is how a user sets
one; each runs on a shape where the switch changes the launch and is compared with the default in this process and with the
oracle."""
import numpy as np
import pytest

from tests import cases
from tests.child_run import make_case, run_in_child, run_job

pytestmark = pytest.mark.gpu
TOL = 1e-10

# R grid shapes of the PCR solve: one column, so every R > 1 leaves a partial workgroup of 1 column.
# threads = roundup64(max(nblk * R, b_rDim * R / 4)): 64 everywhere except kat_r 13 cells at R = 16 (nblk 5 -> 80 -> 128);
# the PERIODIC corner correction fills 6 R entries, 96 > 64 threads at R = 16 for 7 and 12 cells
PCR_SHAPES = [["kat_r", {"num_cells": 7}, {}], ["kat_r", {"num_cells": 12}, {}], ["kat_r", {"num_cells": 13}, {}],
              ["r_bcs", {"bcl": "R1T2", "bcr": "R2T10", "num_cells": 4}, {}]]      # 4 cells: the minimum, 4 unknowns (nblk 2)


@pytest.mark.parametrize("r", [1, 2, 4, 8, 16], ids=["SX_PCR_R=%d" % r for r in [1, 2, 4, 8, 16]])
def test_pcr_solve_with_forced_columns_per_workgroup(monkeypatch, tmp_path, r):
    """SX_PCR_R=r with SX_SOLVE_PCR=1 (launch_solve_pcr: R = r unless nblk * r > 1024, which none of these reach) on the PERIODIC
    KAT at 7, 12 and 13 cells and on R1T2 / R2T10 at 4 cells: per column against the lane-per-column solve (1e-13) and the
    dense solve (1e-12), the bars of tests/test_gpu_solve.py."""
    job = {"kind": "spline", "cases": PCR_SHAPES}
    for spec in PCR_SHAPES:
        assert cases.pcr_launch_geometry(make_case(spec), r_force=r)["R"] == r
    got = run_in_child(tmp_path, job, {"SX_SOLVE_PCR": "1", "SX_PCR_R": str(r)})
    monkeypatch.setenv("SX_SOLVE_PCR", "0")
    lane = run_job(job)
    bad = []
    for i, spec in enumerate(PCR_SHAPES):
        case = make_case(spec)
        g = cases.oracle_grid(case)
        shared = np.random.default_rng(5).standard_normal((g.b_rDim * g.K2 * g.b_zDim, g.V))
        ref = cases.dense_spline_transform(case, shared)
        a, b = got["a%d" % i], lane["a%d" % i]
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        e_ab = cases.rel_err_per_column(a, b, g.b_rDim).max()
        e_ar = cases.rel_err_per_column(a, ref, g.b_rDim).max()
        e_br = cases.rel_err_per_column(b, ref, g.b_rDim).max()
        if not (e_ab <= 1e-13 and e_ar <= 1e-12 and e_br <= 1e-12):
            bad.append((spec, e_ab, e_ar, e_br))
    assert not bad, "per-column error (PCR vs k_solve, PCR vs dense, k_solve vs dense): %s" % bad


def test_ring_tile_rz_inverse_equals_the_node_form_and_the_general_kernels(monkeypatch, tmp_path):
    """SX_RZ_INV=0: the fused RZ inverse as ring tiles (k_rz_inverse) instead of node tiles (k_rz_inverse_nodes, the default
    while its LDS - 8 (16 roundup32(b_zDim) + 3,588) bytes - fits 64 KB, i.e. b_zDim <= 287).  Two shapes of
    test_rz_fused_matrix_core_transforms_equal_the_general_kernels (b_zDim 20 and 100), that test's bars: every derivative slot
    within 1e-12 of the general kernels (SX_RZ_FUSED=0) and of the node form, B coefficients within 1e-13."""
    job = {"kind": "rz_transforms", "cases": [["rz_advection", {"num_cells": 21, "zDim": 33}, {"b_zDim": 20}],
                                              ["rz_advection", {"num_cells": 33, "zDim": 250}, {"b_zDim": 100}]]}
    got = run_in_child(tmp_path, job, {"SX_RZ_INV": "0"})
    nodes = run_job(job)
    monkeypatch.setenv("SX_RZ_FUSED", "0")
    general = run_job(job)
    for i in range(len(job["cases"])):
        ph = got["phys%d" % i]
        assert np.abs(ph).max() > 0
        for d in range(ph.shape[2]):
            assert cases.rel_err(ph[:, :, d], general["phys%d" % i][:, :, d]) < 1e-12, (i, d)
            assert cases.rel_err(ph[:, :, d], nodes["phys%d" % i][:, :, d]) < 1e-12, (i, d)
        assert cases.rel_err(got["spec%d" % i], general["spec%d" % i]) < 1e-13, i


def _model_variant(tmp_path, spec, steps, overrides):
    job = {"kind": "model", "cases": [spec], "steps": steps}
    got = run_in_child(tmp_path, job, overrides)
    dflt = run_job(job)
    orc = cases.OracleModel(make_case(spec))
    for _ in range(steps):
        orc.step()
    fa, fb = got["var0"], dflt["var0"]
    assert np.isfinite(fa).all()
    for v in range(fa.shape[1]):
        assert np.abs(fa[:, v] - fb[:, v]).max() <= 1e-13 * max(np.abs(fb[:, v]).max(), 1e-300), v
    assert cases.rel_err_per_var(got["phys0"], orc.physical()) < TOL


def test_512_thread_sbw_at_64_levels(tmp_path):
    """SX_SBW_T256=0: at zDim 64 the matrix-core B kernel runs as 512-thread workgroups of 64 wavenumber blocks
    (k_sbw_mfma<64>) instead of the default 256-thread ones of 32 (k_sbw_mfma<64, 32, 256>; both need b_zDim <= 64, here 43).
    rlz_hrbl 8 cells x 32 x 64, 4 steps: every variable within 1e-13 of the default, fields within 1e-10 of the oracle."""
    _model_variant(tmp_path, ["rlz_hrbl", {"num_cells": 8, "zDim": 64, "ring_L": 32}, {}], 4, {"SX_SBW_T256": "0"})


def test_half_ring_forward_dft_on_native_rings(tmp_path):
    """SX_DFT_HALF=1: the forward DFT of native rings (L = 4 + 4 i: not the FFT path; zDim 10 >= 8: the matrix-core DFT) as the
    half-ring kernel (k_fl_forward_dft over ring classes) instead of the quarter-wave work list (k_fl_forward_dft_q).
    rlz_hrbl 9 cells x native x 10, 4 steps: every variable within 1e-13 of the default, fields within 1e-10 of the oracle."""
    _model_variant(tmp_path, ["rlz_hrbl", {"num_cells": 9, "zDim": 10}, {}], 4, {"SX_DFT_HALF": "1"})


def test_two_handles_of_one_process_take_their_own_columns_per_workgroup(monkeypatch):
    """One process, two handles of the PERIODIC KAT at 12 cells with SX_SOLVE_PCR=1: the first created under SX_PCR_R=1, the
    second under SX_PCR_R=4.  The library's plan reports R = 1 and R = 4 under the two environments (the solution does not show
    which R ran: a second handle that kept the first one's R would pass the comparison, not the plan), and each handle's
    solution is within 1e-13 per column of the lane-per-column solve."""
    import scythe_jl_amd as S
    spec = PCR_SHAPES[1]
    case = make_case(spec)
    og = cases.oracle_grid(case)
    geo = cases.pcr_launch_geometry(case)
    job = {"kind": "spline", "cases": [spec]}
    monkeypatch.setenv("SX_SOLVE_PCR", "1")
    grids, sols = [], []
    for r in (1, 4):
        monkeypatch.setenv("SX_PCR_R", str(r))
        _, (R, logR, _, *_) = cases.launch_plan(cases.PLAN_PCR, geo["nblk"], og.b_rDim, cases._handle_dims(case)[1], og.V * og.b_zDim)
        assert (R, 1 << logR) == (r, r)
        g = S.Grid(*cases.hip_params(case))          # both handles alive at once: nothing of the first is shared with the second
        grids.append(g)
    for g in grids:
        g.set_patch_spectral_b(np.random.default_rng(5).standard_normal((int(g.dims.s_patch), g.V)))
        g.splineTransform_()
        sols.append(g.patchSpectral)
        g.close()
    monkeypatch.delenv("SX_PCR_R")
    monkeypatch.setenv("SX_SOLVE_PCR", "0")
    lane = run_job(job)["a0"]
    for r, a in zip((1, 4), sols):
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        e = cases.rel_err_per_column(a, lane, og.b_rDim).max()
        print("SX_PCR_R=%d vs the lane-per-column solve: %.2e" % (r, e))
        assert e <= 1e-13, (r, e)
