"""The twin of sx_physics (tests/physics.py) against the Float64 oracle, on the CPU: the bound c u S is validated here, on the
reference, and never fitted to a kernel.  (1) oracle_np in Float64 is bit for bit what it was before it learned to follow its
input's precision; (2) for every case of tests/test_gpu_physics.py the Float64 oracle lies inside the bound at every unmasked
point, and at most 1 % of the points are masked; (3) the bound is sharp: five deliberate errors of the size a wrong kernel
would make each push at least one point outside it, for every equation set."""
import os
import runpy

import numpy as np
import pytest

from tests import physics

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_float64_oracle_is_pinned():
    new = runpy.run_path(os.path.join(GOLDEN, "make_physics_pin_fixture.py"))["pin_arrays"]()
    with np.load(os.path.join(GOLDEN, "physics_f64_pin.npz")) as old:
        assert sorted(old.files) == sorted(new)
        assert {k.split(".")[0] for k in old.files} == set(physics.PER_SET)
        for k in old.files:
            assert old[k].dtype == new[k].dtype == np.float64
            assert old[k].tobytes() == new[k].tobytes(), k


def _run(cid, mutate=None):
    """worst |err| / bound over t = 1..4 of the Float64 oracle (with one deliberate error) against the twin"""
    case, twin, phys, solved = physics.solved_on_host(cid)
    run = physics.Float64Run(case, mutate=mutate)
    top, where = 0.0, ""
    for t in sorted(phys):
        q = physics.ratios(solved[t], *run.call(phys[t], t))
        if q.max() > top:
            top, where = float(q.max()), "t = %d, %s" % (t, physics.worst(twin, q))
    return top, where


# the cases whose twin differs from another's only in the kernel that runs them are one case here
HOST_CASES = [c for c in physics.CASES if physics.CASES[c][3] is None]


@pytest.mark.parametrize("cid", HOST_CASES)
def test_float64_oracle_inside_bound(cid):
    case, twin, phys, solved = physics.solved_on_host(cid)
    share = max(float(s[2].mean()) for s in solved.values())
    top, where = _run(cid)
    print("\n%-18s %-38s c = %3d  masked %.3f %%  worst |err| / bound %.3f  (%s)" % (cid, case["eq"], twin.c, 100 * share, top, where))
    print("%20s %s" % ("", physics.check_tails(cid, twin.N, twin.N // twin.nz)))      # the launch shapes, where there is no GPU
    if case["eq"] == "rainfall_test":
        print("%20s clamped columns (column_min, column_max) per t: %s" % ("", physics.check_clamp_mix(twin, solved)))
    assert share <= 0.01
    assert all(np.isfinite(np.asarray(s[0], dtype=np.float64)).all() for s in solved.values())
    assert top < 1.0, where


@pytest.mark.parametrize("mutate", ["term", "weight", "rotation", "f32", "stale"])
@pytest.mark.parametrize("cid", physics.PER_SET)
def test_bound_catches(cid, mutate):
    top, where = _run(cid, mutate)
    assert top > 1.0, "%s: the %s error stays inside the bound (worst ratio %.3g)" % (cid, mutate, top)


@pytest.mark.parametrize("cid", ["acoustic_z16", "euler_z32", "rain_z14_semi"])
def test_library_semi_operators_are_the_oracle_s_to_the_inversion_s_accuracy(cid):
    """sx_semi_column_ops (pure host helper: what sx_create uploads) against oracle_np.semi_matrices.  Both invert H in 80-bit
    arithmetic; they agree to cond(H) 2^-64 of the operator's norm (1e-13 .. 1e-12 here), not to u - which is why the GPU twin
    reads the library's operators instead of forming its own."""
    case = physics.case_of(cid)[0]
    for (W, X), (Wn, Xn) in zip(physics.semi_operators(case, device=True), physics.semi_operators(case)):
        for a, b in ((W, Wn), (X, Xn)):
            assert np.isfinite(a).all() and np.abs(a).max() > 0
            assert np.abs(a - b).max() <= 1e-11 * np.abs(b).max()


# the semi-implicit cases at 65, 128 and 200 levels (tests/physics.py SEMI_CASES), default kernel: one twin per level count
SEMI_DEEP = [c for c, v in physics.SEMI_CASES.items() if v[3] is None and v[1]["zDim"] in (65, 128, 200)]


@pytest.mark.parametrize("cid,mutate", [("acoustic", "semi"), ("euler_z16", "semi"), ("rain_z12_semi", "semi"),
                                        ("rain_z12", "condensation"), ("rain_z12_semi", "condensation")] + [(c, "semi") for c in SEMI_DEEP])
def test_bound_catches_an_error_inside_the_adjustments(cid, mutate):
    """The bound of w and xi carries the operator sums and up to 3 nz in c: it still bites at 1e-9 inside semiimplicit_adjustment
    (tau Pxi_bar of xi*_z) and inside condensation_adjustment (its time scale).  At 65, 128 and 200 levels (c = 157, 283 / 311, 427)
    the same 1e-9 change of tau Pxi_bar is still caught, by a factor of 5000 at 65 levels and 1400 at 200: the size did not have
    to be lowered.  This, not a bar scaled by zDim^4 on a five-step comparison, is the statement of what the per-point check of
    k_semi_mfma can see at those level counts."""
    top, where = _run(cid, mutate)
    assert top > 1.0, "%s: the %s error stays inside the bound (worst ratio %.3g)" % (cid, mutate, top)


def test_mask_takes_a_point_put_on_a_branch():
    """The slab sets take |w|: a point whose w = -Hb (ub / r + ub_r + vb_l / r) is made to cancel to rounding has no defined
    sign of w, the twin masks that point and no other, and the check then ignores what a kernel writes there."""
    case, _, phys, _ = physics.solved_on_host("slab_oneway")
    g = physics.cases.oracle_grid(case)
    r = g.gridpoints()[:, 0]
    ph = phys[1].copy()
    sl = {s: i for i, s in enumerate(g.slots)}
    p = 123
    ph[p, 3, sl["r"]] = -((ph[p, 3, 0] / r[p]) + (ph[p, 4, sl["l"]] / r[p]))
    twin = physics.Twin(case)
    mask = twin.mask(ph, 1)
    assert mask[p] and mask.sum() == 1
    np1, w = physics.Float64Run(case).call(ph, 1)
    np1[p] += 1.0
    assert physics.ratios(physics.solve(twin, {1: ph})[1], np1, w).max() < 1.0


def test_chained_level_sums_against_perturbing_level_by_level():
    """Twin.bound chains absolute values through the recorded operator inputs; the literal sum perturbs every plane one level at
    a time through the live operators.  The chained sum is never smaller, and by how much it is larger is measured here (HRBL,
    zDim 10, t = 2: the figures are in DESIGN.md section 18)."""
    case, _, phys, _ = physics.solved_on_host("hrbl_z10")
    a, b = physics.Twin(case), physics.Twin(case)
    for t in (1, 2):
        a.call(phys[t], t)
        chained = a.bound(phys[t], t)
        literal = b._solve(phys[t], t, by_level=True)["bound"]
        b.hist = a.hist         # the same history for the next t
    ok = literal > 0
    f = chained[ok] / literal[ok]
    print("\nchained / level-by-level bound, hrbl_z10 t = 2: min %.4f median %.4f max %.4f" % (f.min(), np.median(f), f.max()))
    assert f.min() >= 1.0 - 1e-6
    assert (chained[~ok] >= 0).all()
    assert f.max() < 2.0
