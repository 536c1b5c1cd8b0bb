"""sx_kernel_bytes for the tests: the cases whose per-launch byte counts tests/golden/kernel_bytes_parent.json records, and the run
that reads them off a build.  One table drives the fixture's generator (tests/golden/make_kernel_bytes_fixture.py) and the replay
(tests/test_gpu_kernel_bytes.py)."""
import os
from unittest import mock

from tests import cases, rainfall

EXTRA = ("k_solve", "k_zinv", "k_node_fft", "alloc.d_Fl", "alloc.d_Fn", "alloc.total")   # asked of every handle, launched or not
STAGES = ("after_2_steps", "after_tile_transform")


def _node():
    """the smallest node-mode shape with inner rings (R_in > 0): 13 cells, 32 levels, 64-point rings"""
    return cases.rlz_hrbl(num_cells=13, zDim=32, ring_L=64)


_NODE_NAMES = ("k_phys_hrbl_inner", "k_phys_hrbl", "k_node_fft", "k_rl_inverse", "k_zinv", "k_fl_forward", "k_solve")

# id -> (case, SX_* switches, storage, tiles, timer names the case exists for)
CASES = {
    "r": (cases.r_bcs, {}, "f64", 1, ("k_sb", "k_phys_pointwise", "k_solve")),
    "rz_fused": (cases.rz_advection, {}, "f64", 1, ("k_rz_inverse", "k_rz_forward", "k_phys_pointwise")),
    "rz_unfused": (cases.rz_advection, {"SX_RZ_FUSED": "0"}, "f64", 1, ("k_zinv", "k_rl_inverse", "k_sbz")),
    "rz_semi": (cases.rz_semiimplicit, {}, "f64", 1, ("k_semiimplicit",)),
    "rz_semi_scalar": (cases.rz_semiimplicit, {"SX_SEMI_MFMA": "0"}, "f64", 1, ("k_semiimplicit",)),
    "rz_euler": (cases.rz_euler, {}, "f64", 1, ("k_phys_pointwise", "k_semiimplicit")),
    "rz_rain": (rainfall.rz_rain, {}, "f64", 1, ("k_phys_rain", "k_condensation", "k_semiimplicit")),
    "rl_native": (cases.rl_slab, {}, "f64", 1, ("k_rl_inverse", "k_fl_forward", "k_sb", "k_phys_pointwise")),
    "rl_uniform": (lambda: cases.rl_slab(ring_L=16), {}, "f64", 1, ("k_rl_inverse", "k_fl_forward", "k_sb")),
    "rlz_native": (cases.rlz_hrbl, {}, "f64", 1, ("k_zinv", "k_rl_inverse", "k_fl_forward", "k_sbz", "k_phys_hrbl")),
    "rlz_native_scalar": (cases.rlz_hrbl, {"SX_DFT_MFMA": "0"}, "f64", 1, ("k_zinv", "k_rl_inverse", "k_fl_forward", "k_sbz")),
    "node": (_node, {}, "f64", 1, _NODE_NAMES),
    "node_f32": (_node, {}, "f32", 1, _NODE_NAMES),
    "node_f32x": (_node, {}, "f32x", 1, _NODE_NAMES),
    "node_unfused": (_node, {"SX_FUSE_ZINV": "0"}, "f64", 1, _NODE_NAMES),
    "node_overlap": (_node, {"SX_OVERLAP": "1"}, "f64", 1, _NODE_NAMES),
    "node_deferred": (_node, {"SX_DEFER_DIAG": "1"}, "f64", 1, _NODE_NAMES),
    "node_graph": (_node, {"SX_GRAPH": "1"}, "f64", 1, _NODE_NAMES),
    "node_sliding_window": (_node, {"SX_SBW_MFMA": "2"}, "f64", 1, _NODE_NAMES + ("k_sbz",)),
    "two_tiles": (lambda: cases.rlz_hrbl(num_cells=6), {}, "f64", 2, ("k_zinv", "k_rl_inverse", "k_fl_forward", "k_sbz", "k_phys_hrbl", "k_solve")),
}


def _read(tile):
    """the tile's timer names in sx_get_timers' order (first launch), and repr(bytes) of each of them and of EXTRA"""
    timers = list(tile.timers())
    return dict(timers=timers, bytes={k: repr(tile.kernel_bytes(k)) for k in timers + [e for e in EXTRA if e not in timers]})


def record(cid):
    """{stage: [per tile {"timers": names, "bytes": {name: repr(bytes)}}]} of case `cid` on the library as it is built: two steps, then tileTransform!, under
    exactly the case's SX_* switches whatever the caller's environment holds"""
    make, env, storage, tiles, _ = CASES[cid]
    scoped = {k: v for k, v in os.environ.items() if not k.startswith("SX_")}
    scoped.update(env)
    with mock.patch.dict(os.environ, scoped, clear=True):
        m = cases.HipModel(make(), num_tiles=tiles, storage=storage)
        m.step()
        m.step()
        out = {STAGES[0]: [_read(g) for g in m.run.tiles]}
        for g in m.run.tiles:
            g.tileTransform_()
        out[STAGES[1]] = [_read(g) for g in m.run.tiles]
    return out
