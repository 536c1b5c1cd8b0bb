"""-m gpu: sx_kernel_bytes answers from what each launcher stated at its TimedLaunch scope.

Parity: tests/golden/kernel_bytes_parent.json holds what the commit before that change answered - whose sx_kernel_bytes worked every
count out itself, from the handle's state at the time of the query - for the cases of tests/kernel_bytes.py: after two steps, then
after tileTransform!, every timer name plus k_solve, k_zinv, k_node_fft and the alloc.* keys.  The same cases on this build must
list the same timer names in the same order and give the same doubles (==), except where the two differences of the change apply
(DESIGN.md "Kernels and rooflines"), and there they must show the new reading exactly:

  * a name the handle has never launched (not among its timers: k_zinv without a vertical or on a fused RZ grid, k_node_fft without
    the node-space path) reads 0, where the parent evaluated its formula on the handle's default state;
  * k_phys_hrbl, k_phys_hrbl_inner and k_node_fft, which the parent worked out from node_active as it stood at the query: tileTransform!
    launches none of the three but clears node_active, so the parent's entries after it described no launch that had happened
    (k_node_fft read 0, the other two the ring-wise counts of the whole tile).  Here they still describe the step's launches: the second
    stage is held to the parent's FIRST-stage entry.

Every case also names the timers it exists for: a shape that silently takes another path fails instead of passing vacuously.

Semantics, on one small handle: an unknown name and a name before its first launch read 0; sx_enable_timers and sx_timer_only change
no count."""
import json
import os

import pytest

from tests import cases
from tests import kernel_bytes as KB

pytestmark = pytest.mark.gpu
PARENT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_bytes_parent.json")))
# followed node_active as of the query on the parent; describe their last launch now
LAUNCH_BOUND = ("k_phys_hrbl", "k_phys_hrbl_inner", "k_node_fft")


def test_the_fixture_covers_the_cases():
    assert set(PARENT["cases"]) == set(KB.CASES)
    for cid, (_, env, storage, tiles, _) in KB.CASES.items():
        rec = PARENT["cases"][cid]
        assert (rec["env"], rec["storage"], rec["tiles"]) == (env, storage, tiles), cid


def _expected(want, stage, t, name):
    """what this build must read for `name` of tile t at `stage`, from the parent's record `want`"""
    first, second = KB.STAGES
    if not name.startswith("alloc.") and name not in want[stage][t]["timers"]:
        return 0.0                                                     # never launched on this handle
    if stage == second and name in LAUNCH_BOUND:
        return float(want[first][t]["bytes"][name])                    # tileTransform! launches none of them
    return float(want[stage][t]["bytes"][name])


@pytest.mark.parametrize("cid", list(KB.CASES))
def test_every_count_equals_the_parents(cid):
    want, got = PARENT["cases"][cid]["stages"], KB.record(cid)
    for stage in KB.STAGES:
        assert len(got[stage]) == len(want[stage]) == KB.CASES[cid][3]
        for t, (g, w) in enumerate(zip(got[stage], want[stage])):
            print("%s %s tile %d: %s" % (cid, stage, t, g))
            assert g["timers"] == w["timers"], (cid, stage, t)              # the same names, in the order of their first launch
            assert set(g["bytes"]) == set(w["bytes"])
            for name in KB.CASES[cid][4]:
                assert name in g["timers"] and float(g["bytes"][name]) > 0, (cid, stage, t, name)
            for name, b in g["bytes"].items():
                assert float(b) == _expected(want, stage, t, name), (cid, stage, t, name, b, w["bytes"][name])


@pytest.fixture(scope="module")
def tile():
    import scythe_jl_amd as S
    case = cases.rlz_hrbl()
    gp, mp = cases.hip_params(case)
    g = S.Grid(gp, mp)
    yield g
    g.close()


def test_unknown_names_and_names_before_their_first_launch_read_zero(tile):
    assert tile.kernel_bytes("k_no_such_kernel") == 0 and tile.kernel_bytes("") == 0
    assert "k_rl_inverse" not in tile.timers()
    assert tile.kernel_bytes("k_zinv") == 0 and tile.kernel_bytes("k_rl_inverse") == 0 and tile.kernel_bytes("k_solve") == 0
    tile.tileTransform_()
    assert tile.kernel_bytes("k_zinv") > 0 and tile.kernel_bytes("k_rl_inverse") > 0
    assert "k_solve" not in tile.timers() and tile.kernel_bytes("k_solve") == 0       # still not launched
    assert tile.kernel_bytes("alloc.total") > 0                                       # the alloc.* keys need no launch


def test_timer_switches_change_no_count(tile):
    names = ("k_zinv", "k_rl_inverse", "k_fl_forward", "k_sbz", "k_solve")

    def run():
        tile.tileTransform_()
        tile.spectralTransform_()
        tile.splineTransform_()
        return [tile.kernel_bytes(k) for k in names]

    tile.enable_timers(False)
    off = run()
    assert all(b > 0 for b in off)
    tile.enable_timers(True)
    assert run() == off
    tile.timer_only("k_solve")
    tile.reset_timers()
    assert run() == off
    calls = {k: c for k, (_, c) in tile.timers().items()}
    assert calls["k_solve"] == 1 and calls["k_zinv"] == 0                             # the exclusion was in force
    tile.timer_only(None)
    tile.enable_timers(False)
