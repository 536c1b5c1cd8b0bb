"""CPU-only: the work lists of the native-ring DFT launches (csrc/sx_dft.hip), as sx_dft_work_list hands them out (the function
sx_create and the RL launchers build their lists with), against the rule stated here: one item per (ring, variable with planes) or
(ring, part), sorted by decreasing cost with ties in (ring, x) order, and - RLZ grids - the rings with kmax > 319 moved to the front
in that order.  Ring i (0-based) of a native grid has L = 8 + 4 i points and keeps wavenumbers 0 .. i + 1."""
import ctypes as C

import pytest

import scythe_jl_amd as S
from scythe_jl_amd import _lib as L

LIST_RLZ, LIST_RL_INVERSE, LIST_RL_FORWARD = 0, 1, 2      # include/scythe_hip.h
KMAX_SINGLE = 319
# derivative planes asked of the six variables: an equation-set mask with a variable that asks for none, every slot, the forward list
PLANES = {"eq": [3, 5, 5, 7, 0, 1], "full": [7] * 6, "forward": [1] * 6}


def library_list(kind, num_cells, planes=()):
    lib = S.load()
    counts = (C.c_int32 * 2)()
    pl = (C.c_int32 * max(len(planes), 1))(*planes)
    L.check(lib.sx_dft_work_list(kind, 0, num_cells, len(planes), pl, None, 0, counts))
    items = (C.c_int32 * (2 * counts[0]))()
    L.check(lib.sx_dft_work_list(kind, 0, num_cells, len(planes), pl, items, counts[0], counts))
    return [(items[2 * i], items[2 * i + 1]) for i in range(counts[0])], counts[1]


def rings(num_cells):
    return [(8 + 4 * i, i + 1) for i in range(3 * num_cells)]      # (L, kmax)


def rule_rlz(num_cells, planes):
    rg = rings(num_cells)
    it = [(rg[r][0] ** 2 * p, r, v) for r in range(len(rg)) for v, p in enumerate(planes) if p > 0]
    it.sort(key=lambda e: -e[0])                                     # stable
    it.sort(key=lambda e: rg[e[1]][1] <= KMAX_SINGLE)                # stable: big rings first
    return [(r, v) for _, r, v in it], sum(1 for _, r, _ in it if rg[r][1] > KMAX_SINGLE)


def rule_rl(num_cells, forward):
    rg = rings(num_cells)
    parts = lambda Lr, km: (km + 1 + 127) // 128 if forward else (Lr // 4 // 16 + 1 + 7) // 8
    it = [(rg[r][0], r, p) for r in range(len(rg)) for p in range(parts(*rg[r]))]
    it.sort(key=lambda e: -e[0])
    return [(r, p) for _, r, p in it]


@pytest.mark.parametrize("num_cells", [9, 110])
@pytest.mark.parametrize("mask", sorted(PLANES))
def test_rlz_lists(num_cells, mask):
    got, nbig = library_list(LIST_RLZ, num_cells, PLANES[mask])
    want, want_big = rule_rlz(num_cells, PLANES[mask])
    assert nbig == want_big and (nbig > 0) == (num_cells == 110)
    assert got == want


@pytest.mark.parametrize("forward", [False, True])
def test_rl_lists(forward):
    got, nbig = library_list(LIST_RL_FORWARD if forward else LIST_RL_INVERSE, 9)
    assert nbig == 0
    assert got == rule_rl(9, forward)
    # a grid whose larger rings have more than one part (L / 4 > 127 points, kmax > 127)
    got, _ = library_list(LIST_RL_FORWARD if forward else LIST_RL_INVERSE, 60)
    assert got == rule_rl(60, forward) and max(p for _, p in got) > 0


def test_refusals():
    lib = S.load()
    counts = (C.c_int32 * 2)()
    assert lib.sx_dft_work_list(7, 0, 9, 0, None, None, 0, counts) != 0
    assert lib.sx_dft_work_list(LIST_RLZ, 0, 9, 6, None, None, 0, counts) != 0
    assert lib.sx_dft_work_list(LIST_RL_INVERSE, 0, 0, 0, None, None, 0, counts) != 0
    assert lib.sx_dft_work_list(LIST_RL_INVERSE, 0, 2 ** 30, 0, None, None, 0, counts) != 0
    # a list that does not fit is refused, not cut short or silently left out
    assert lib.sx_dft_work_list(LIST_RL_INVERSE, 0, 9, 0, None, None, 0, counts) == 0 and counts[0] == 27
    items = (C.c_int32 * (2 * 26))()
    assert lib.sx_dft_work_list(LIST_RL_INVERSE, 0, 9, 0, None, items, 26, counts) != 0
