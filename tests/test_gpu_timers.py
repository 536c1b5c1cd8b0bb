"""-m gpu: what the timed-launch scope of the launchers (csrc/sx_internal.hpp: TimedLaunch) must preserve.

One row of CASES per launch path: with timers on, one tileTransform_ and three steps give the timer names in first-use order and
the calls of EXPECTED.  The table was recorded with the begin / end pairs the scope replaced; a launcher that opens its scope in
another place, under another name or not at all changes a row.  On the same handles: every ms is finite and positive, timer_only
singles one kernel out and gives the others back, reset_timers zeroes, two diagnostics entry points add their own names only, and
after all of it a further step is bit-identical to that of a handle that never had its timers on."""
import os
from unittest import mock

import numpy as np
import pytest

from tests import cases, rainfall

pytestmark = pytest.mark.gpu

HRBL32 = dict(num_cells=8, zDim=32, ring_L=32)      # 24 rings of 32 points, kDim 15: R_in = 15 > 0, levels for the matrix cores

# id: (case, SX_* switches read at sx_create, tiles)
CASES = {
    "r": (lambda: cases.r_bcs(num_cells=12), {}, 1),                                   # one column: k_solve_pcr
    "rz_semi_fused": (lambda: cases.rz_semiimplicit(num_cells=8, zDim=12), {}, 1),
    "rz_semi_general": (lambda: cases.rz_semiimplicit(num_cells=8, zDim=12), {"SX_RZ_FUSED": "0", "SX_SEMI_MFMA": "0"}, 1),
    "rz_rain": (lambda: rainfall.rz_rain(num_cells=8, zDim=12), {}, 1),
    "rl_native": (lambda: cases.rl_slab(num_cells=8), {}, 1),
    "rlz_native_dft": (lambda: cases.rlz_hrbl(num_cells=6, zDim=10), {}, 1),
    "rlz_node": (lambda: cases.rlz_hrbl(**HRBL32), {}, 1),
    "rlz_node_overlap": (lambda: cases.rlz_hrbl(**HRBL32), {"SX_OVERLAP": "1"}, 1),
    "rlz_node_ring_spectra": (lambda: cases.rlz_hrbl(**HRBL32), {"SX_SBW_MFMA": "2"}, 1),
    "rlz_node_small_tile": (lambda: cases.rlz_hrbl(**HRBL32), {"SX_SBW_MFMA": "3"}, 1),
    "rl_two_tiles": (lambda: cases.rl_slab(num_cells=12), {}, 2),                      # gather exchange: k_solve with offset tables
}

# per case and tile: (name, calls) in first-use order after one tileTransform_ and three steps
EXPECTED = {
    "r": [[("k_fl_forward", 3), ("k_sb", 3), ("k_solve", 3), ("k_rl_inverse", 4), ("k_phys_pointwise", 3)]],
    "rz_semi_fused": [[("k_rz_forward", 3), ("k_solve", 3), ("k_rz_inverse", 4), ("k_phys_pointwise", 3), ("k_semiimplicit", 3)]],
    "rz_semi_general": [[("k_fl_forward", 3), ("k_sbz", 3), ("k_solve", 3), ("k_zinv", 4), ("k_rl_inverse", 4), ("k_phys_pointwise", 3), ("k_semiimplicit", 3)]],
    "rz_rain": [[("k_rz_forward", 3), ("k_solve", 3), ("k_rz_inverse", 4), ("k_phys_rain", 3), ("k_semiimplicit", 3), ("k_condensation", 3)]],
    "rl_native": [[("k_fl_forward", 3), ("k_sb", 3), ("k_solve", 3), ("k_rl_inverse", 4), ("k_phys_pointwise", 3)]],
    "rlz_native_dft": [[("k_fl_forward", 3), ("k_sbz", 3), ("k_solve", 3), ("k_zinv", 4), ("k_rl_inverse", 4), ("k_phys_hrbl", 3)]],
    "rlz_node": [[("k_fl_forward", 3), ("k_sbz", 3), ("k_solve", 3), ("k_zinv", 4), ("k_rl_inverse", 4), ("k_node_fft", 3), ("k_phys_hrbl_inner", 3), ("k_phys_hrbl", 3)]],
    "rlz_node_overlap": [[("k_fl_forward", 3), ("k_sbz", 3), ("k_solve", 3), ("k_zinv", 4), ("k_rl_inverse", 4), ("k_phys_hrbl_inner", 3), ("k_node_fft", 3), ("k_phys_hrbl", 3)]],
    "rlz_node_ring_spectra": [[("k_fl_forward", 3), ("k_sbz", 3), ("k_solve", 3), ("k_zinv", 4), ("k_rl_inverse", 4), ("k_node_fft", 3), ("k_phys_hrbl_inner", 3), ("k_phys_hrbl", 3)]],
    "rlz_node_small_tile": [[("k_fl_forward", 3), ("k_sbz", 3), ("k_solve", 3), ("k_zinv", 4), ("k_rl_inverse", 4), ("k_node_fft", 3), ("k_phys_hrbl_inner", 3), ("k_phys_hrbl", 3)]],
    "rl_two_tiles": [[("k_fl_forward", 3), ("k_sb", 3), ("k_solve", 3), ("k_rl_inverse", 4), ("k_phys_pointwise", 3)],
                     [("k_fl_forward", 3), ("k_sb", 3), ("k_halo_add", 3), ("k_solve", 3), ("k_rl_inverse", 4), ("k_phys_pointwise", 3)]],
}


def make(cid):
    """The case's model, created under its switches (and under no other SX_* variable)."""
    build, env, tiles = CASES[cid]
    scoped = {k: v for k, v in os.environ.items() if not k.startswith("SX_")}
    scoped.update(env)
    with mock.patch.dict(os.environ, scoped, clear=True):
        return cases.HipModel(build(), num_tiles=tiles, exchange="gather")


def transform_and_step(hip, steps=3):
    for g in hip.run.tiles:
        g.tileTransform_()
    for _ in range(steps):
        hip.step()


def calls_of(tile):
    return [(k, v[1]) for k, v in tile.timers().items()]


def record(cid):
    hip = make(cid)
    for g in hip.run.tiles:
        g.enable_timers(True)
    transform_and_step(hip)
    return hip, [calls_of(g) for g in hip.run.tiles]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("cid", list(CASES))
def test_names_order_calls_and_everything_else_the_scope_keeps(cid):
    plain = make(cid)                   # never timed
    hip, got = record(cid)
    assert got == EXPECTED[cid], got
    tiles = hip.run.tiles
    for g in tiles:
        assert all(np.isfinite(ms) and ms > 0 for ms, _ in g.timers().values()), g.timers()

    # timer_only: two more steps advance that entry alone; None gives the others back
    per_step = [{k for k, c in rows if c >= 3} for rows in EXPECTED[cid]]          # hit by every step
    for g in tiles:
        g.timer_only("k_solve")
    before = [dict(calls_of(g)) for g in tiles]
    for _ in range(2):
        hip.step()
    for g, b in zip(tiles, before):
        now = dict(calls_of(g))
        assert {k for k in now if now[k] != b[k]} == {"k_solve"} and now["k_solve"] > b["k_solve"], (b, now)
        g.timer_only(None)
    before = [dict(calls_of(g)) for g in tiles]
    hip.step()
    for g, b, names in zip(tiles, before, per_step):
        now = dict(calls_of(g))
        assert list(now) == list(b) and len(names) > 1 and all(now[k] > b[k] for k in names), (b, now)

    for g in tiles:
        g.reset_timers()
        assert [k for k in g.timers()] == [k for k, _ in calls_of(g)] and all(v == (0.0, 0) for v in g.timers().values()), g.timers()

    # two diagnostics entry points: one kernel, and extrema's two
    import scythe_jl_amd as S
    g = tiles[0]
    g.evaluate(S.getGridpoints(g)[:5])
    assert [kc for kc in calls_of(g) if kc[1]] == [("k_evaluate", 1)], calls_of(g)
    g.extrema([(0, 1.0, 0, [(1, "")])], source="state")
    assert [kc for kc in calls_of(g) if kc[1]] == [("k_evaluate", 1), ("k_extrema", 1), ("k_extrema_final", 1)], calls_of(g)

    # timing brackets nothing but events: the same calls on the handle that was never timed, then one more step on both
    transform_and_step(plain, steps=6)
    hip.step()
    plain.step()
    for a, b in zip(tiles, plain.run.tiles):
        assert np.array_equal(_bits(a.get_state()), _bits(b.get_state()))
        assert np.array_equal(_bits(a.var_np1), _bits(b.var_np1))
    assert np.array_equal(_bits(hip.physical()), _bits(plain.physical()))


def test_refused_forward_transform_ends_its_bracket():
    """Uniform rings of 514 points are neither a power of two nor a multiple of 4 and too long for the scalar forward kernel
    (16 levels x 515 doubles > 64 KB of LDS): spectralTransform_ refuses with the documented text.  The refusal comes after the
    bracket of k_fl_forward has opened; the bracket ends all the same: timers() returns, with that one call under the name (and the
    one k_sb launch that sx_spectral_transform goes on to, as ever)."""
    import scythe_jl_amd as S
    case = cases.rl_advection(num_cells=3, ring_L=514)
    g = S.Grid(*cases.hip_params(case))
    pts = S.getGridpoints(g)
    g.set_physical_values(case["ic"](pts.reshape(len(pts), -1)))
    g.enable_timers(True)
    with pytest.raises(S.ScytheHipError, match="rings of 514 points are outside every transform path"):
        g.spectralTransform_()
    assert calls_of(g) == [("k_fl_forward", 1), ("k_sb", 1)]
    g.close()
    hip, got = record("rl_native")          # a valid call on a fresh handle times as ever
    assert got == EXPECTED["rl_native"], got
