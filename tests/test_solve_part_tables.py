"""CPU-only: the tables of the partitioned one-tile B -> A spline solve (csrc/sx_iface.hip::part_tables_host, applied on the device by
k_solve_part) through the host helper sx_solve_part_check, which applies them in double in the kernel's order: P row blocks balanced
in unknowns, each with its own banded Cholesky factor, coupled through the 6 edge values of every block.  Against the oracle's dense
definition of the solve, Gamma^T (Gamma (P + eps_q Q) Gamma^T)^-1 Gamma b (oracle_np.Spline1D.SA), and against the banded Cholesky
statement k_solve applies, for every non-periodic boundary-condition pair at P = 2, 3, 4 partitions.

The bar is 1e-13 of the column's scale: the matrices are well conditioned (2-norm condition number 3.3e2 for the R0 class, l_q = 2, any
cell count: tests/test_gpu_solve.py), the factors are worked out in extended precision and rounded once, and the dense fp64 solve itself
is good to about cond x 2^-53 = 4e-14."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_np as O

BCS = ["R0", "R1T0", "R1T1", "R1T2", "R2T10", "R2T20", "R3"]


def _solve(nc, bcl, bcr, parts, b, xmax=12.0, l_q=2.0):
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    a1, a2 = np.zeros(nc + 3), np.zeros(nc + 3)
    rng = (C.c_int32 * (2 * parts))()
    L.check(lib.sx_solve_part_check(nc, 0.0, xmax, l_q, L.BC[bcl], L.BC[bcr], parts, np.ascontiguousarray(b).ctypes.data_as(L.P_D),
                                    a1.ctypes.data_as(L.P_D), a2.ctypes.data_as(L.P_D), rng))
    return a1, a2, [(rng[2 * p], rng[2 * p + 1]) for p in range(parts)]


@pytest.mark.parametrize("parts", [2, 3, 4])
def test_partitioned_tables_equal_the_dense_solve_for_every_boundary_condition_pair(parts):
    """Random right-hand sides at the smallest partition (9 cells each), uneven partitions (9 P + 1, 9 P + P - 1) and the bench
    grid's 171 cells."""
    rng = np.random.default_rng(parts)
    worst = 0.0
    for nc in (9 * parts, 9 * parts + 1, 9 * parts + parts - 1, 171):
        for bcl in BCS:
            for bcr in BCS:
                sp = O.Spline1D(0.0, 12.0, nc, bcl=bcl, bcr=bcr)
                b = rng.standard_normal(nc + 3)
                a1, a2, _ = _solve(nc, bcl, bcr, parts, b)
                ref = sp.SA(b)
                e, e2 = np.abs(a1 - ref).max() / np.abs(ref).max(), np.abs(a1 - a2).max() / np.abs(a2).max()
                worst = max(worst, e, e2)
                assert e <= 1e-13, ("partitioned vs dense", nc, bcl, bcr, e)
                assert e2 <= 1e-13, ("partitioned vs Cholesky", nc, bcl, bcr, e2)
    print("P = %d: worst of the 4 x 49 cases %.1e" % (parts, worst))


@pytest.mark.parametrize("parts", [2, 3, 4])
def test_unit_right_hand_sides_at_every_partition_edge(parts):
    """A unit vector in each patch row in turn (so in particular in the first and last three rows of every partition, where a wrong
    coupling block shows) at 9 P + 1 cells: column by column the inverse the dense definition gives."""
    nc = 9 * parts + 1
    for bcl, bcr in (("R0", "R0"), ("R1T0", "R1T1"), ("R1T1", "R0"), ("R3", "R2T10"), ("R2T20", "R3")):
        sp = O.Spline1D(0.0, 12.0, nc, bcl=bcl, bcr=bcr)
        ref = sp.SA(np.eye(nc + 3))
        scale = np.abs(ref).max()
        for m in range(nc + 3):
            a1, _, _ = _solve(nc, bcl, bcr, parts, np.eye(nc + 3)[m])
            assert np.abs(a1 - ref[:, m]).max() <= 1e-13 * scale, (bcl, bcr, m)


def test_coupling_ranges_at_the_bench_grid():
    """171 cells in 4 partitions of 43-44 unknowns: the reduced matrix decays with the distance between partitions, and a block below
    2^-70 of its largest entry is not applied - every partition reads its neighbours' edge values at least, never outside [0, P)."""
    _, _, ranges = _solve(171, "R1T0", "R1T1", 4, np.ones(174), xmax=3.0e5)
    for p, (lo, hi) in enumerate(ranges):
        assert 0 <= lo <= max(p - 1, 0) and min(p + 1, 3) <= hi <= 3, ranges
    print("coupling ranges at 171 cells, P = 4:", ranges)


def test_refuses_periodic_and_too_small_partitions():
    from scythe_jl_amd import _lib as L
    with pytest.raises(Exception):
        _solve(36, "PERIODIC", "PERIODIC", 4, np.ones(39))
    with pytest.raises(Exception):
        _solve(12, "R3", "R3", 4, np.ones(15))          # 9 unknowns in 4 partitions
