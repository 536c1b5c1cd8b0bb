"""sx_physics, the one hot-path entry point no other test calls, against its extended-precision twin (tests/physics.py), point by
point: k_phys_pointwise, k_phys_rain, k_phys_hrbl, k_phys_hrbl_mfma, k_semiimplicit / k_semi_mfma and k_condensation at the
smallest shapes at which each launch of launch_physics_t can go wrong (tests/physics.py CASES).  The twin is fed the bits
sx_get_physical returns, so the only tolerance is its own bound c u S, validated on the Float64 oracle in tests/test_physics.py.
The column operators are inputs like `physical`: the Helmholtz operators of the semi-implicit solve are inverted in 80-bit
arithmetic at condition ~ nz^4, so the twin reads the ones the library builds (sx_semi_column_ops) - with its own, every
semi-implicit case was 1e5 .. 2e6 bounds out in w at the boundary levels.  Measured on one MI355X: the worst
|err| / bound of every case is between 0.011 and 0.12, as the Float64 oracle has on the CPU.
The timer names show which launches of launch_physics_t ran; k_phys_hrbl / k_phys_hrbl_mfma and k_semiimplicit / k_semi_mfma
share one name each, so which of a pair ran rests on the dispatch code (mfma_levels(nz), the switches read at sx_create), and the
worst ratio in w and xi - the only variables the semi-implicit kernels write - is printed to set the two side by side.
k_phys_hrbl_cell reads node-space planes that only sx_advance produces: sx_physics cannot reach it, and it stays with the
SX_NODE_MODE=0 and forward-cells parity tests."""
import numpy as np
import pytest

from tests import child_run, physics

pytestmark = pytest.mark.gpu


def check(cid, out):
    case, storage, env, timers = physics.case_of(cid)
    twin = physics.Twin(case, pts=out["pts"], semi_ops=out.get("semi_ops"))
    g = twin.g
    n_points, n_columns = (int(x) for x in out["dims"])             # sx_get_dims
    assert (n_points, n_columns) == (twin.N, twin.N // twin.nz)
    shapes = physics.check_tails(cid, n_points, n_columns)          # more than one workgroup and a partial last one, per kernel
    phys = {t: out["phys%d" % t] for t in (1, 2, 3, 4)}
    if storage == "f32":        # the derivative slots read back are what the fp32 planes hold: the case cannot run the fp64 path
        for t in phys:
            assert (phys[t][:, :, 1:].astype(np.float32).astype(np.float64) == phys[t][:, :, 1:]).all()
    solved = physics.solve(twin, phys)
    top, where, top_semi = 0.0, "", 0.0
    for t in (1, 2, 3, 4):
        after = out["phys_after%d" % t]
        w = after[:, 5, 0] if twin.sw else None
        q = physics.ratios(solved[t], out["np1_%d" % t], w)
        if twin.semi:       # the two variables the semi-implicit kernels write: where k_semi_mfma and k_semiimplicit can differ
            top_semi = max(top_semi, float(q[:, [g.vars["w"] - 1, g.vars["xi"] - 1]].max()))
        # no point keeps its old var_np1 where the new one differs (a stale workgroup, seen without the twin's bound)
        new, old, want = out["np1_%d" % t], out["np1_before%d" % t], np.asarray(solved[t][0][:, :g.V], dtype=np.float64)
        assert ((new != old) | (want == old)).all(), "t = %d: var_np1 kept its old value at %d points" % (t, ((new == old) & (want != old)).sum())
        if q.max() >= top:
            top, where = float(q.max()), "t = %d, %s" % (t, physics.worst(twin, q))
        keep = np.ones(after.shape[1:], dtype=bool)
        if twin.sw:
            keep[5, 0] = False          # the diagnostic w
        assert (after[:, keep].view(np.int64) == phys[t][:, keep].view(np.int64)).all(), "t = %d: sx_physics changed `physical`" % t
        assert float(solved[t][2].mean()) <= 0.01
    print("\n%-20s c = %3d  worst |err| / bound %.3f  (%s)%s\n%20s %s" % (
        cid, twin.c, top, where, "  in w, xi: %.3f" % top_semi if twin.semi else "", "", shapes))
    if case["eq"] == "rainfall_test":
        physics.check_clamp_mix(twin, solved)
    # the ring-wise kernel covers every ring after a full sx_tile_transform (no k_phys_hrbl_inner), and nothing else ran
    assert tuple(out["timers"]) == tuple(sorted(timers)), out["timers"]
    assert (out["timer_calls"] == 4).all()
    assert top <= 1.0, where
    return top


@pytest.mark.parametrize("cid", [c for c in physics.CASES if physics.CASES[c][3] is None])
def test_physics_against_twin(cid):
    check(cid, physics.device_run(cid))


@pytest.mark.parametrize("cid", [c for c in physics.CASES if physics.CASES[c][3] is not None])
def test_physics_against_twin_switched(cid, tmp_path):
    """SX_WIDE=0 and SX_SEMI_MFMA=0 are read once per handle, at sx_create: a fresh process with the switch set"""
    check(cid, child_run.run_in_child(tmp_path, {"kind": "physics", "id": cid}, physics.CASES[cid][3]))
