"""CPU-only: the host side of sx_antiderivative (include/scythe_hip.h "antiderivatives") - the symbols, the tables and
the kernel's arithmetic (sx_antiderivative_check) against the longdouble twin of tests/antiderivative.py, every refusal that needs
no device, and the twin itself against closed forms."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from tests import antiderivative as AD
from tests import elliptic as EL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = AD.EPS
CHEB_BCS = ("R0", "R1T0", "R1T1", "R1T2")
K0_BCL = "R1T1"            # the k = 0 class of the RL patches below differs from the k >= 1 class: `k` must select it


def _patch(geometry, nc, bcl="R0", bcr="R0", xmin=0.0, xmax=7.0, **over):
    import scythe_jl_amd as S
    kw = dict(geometry=geometry, xmin=xmin, xmax=xmax, num_cells=nc, vars={"f": 1, "F": 2}, BCL={"F": bcl}, BCR={"F": bcr})
    if "L" in geometry:
        kw["BCL_k0"] = {"F": K0_BCL}
    if "Z" in geometry:
        kw.update(zmin=0.0, zmax=3.0, zDim=9)
    kw.update(over)
    return S.GridParameters(**kw)


def test_symbols():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    header = open(os.path.join(ROOT, "include", "scythe_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "hipTile.jl")).read()
    for name in ("sx_antiderivative", "sx_antiderivative_check"):
        assert hasattr(lib, name) and name in L.SYMBOLS
        assert name + "(" in header and ":" + name in julia
    for text in ("enum { SX_INT_R = 0, SX_INT_Z = 1 };", "enum { SX_INT_FROM_LOW = 0, SX_INT_FROM_HIGH = 1 };", "enum { SX_INT_W_ONE = 0, SX_INT_W_R = 1 };"):
        assert text in header
    assert "#define SX_ABI_VERSION 2" in header
    assert callable(S.Grid.antiderivative) and callable(S.ModelRun.antiderivative)
    assert callable(S.ModelRun.column_integral) and callable(S.ModelRun.inside_radius)


@pytest.mark.parametrize("nc", [4, 5, 37])
@pytest.mark.parametrize("geometry", ["R", "RL"])
def test_radial_check_against_the_longdouble_twin(geometry, nc):
    """Every non-periodic (bcl, bcr) pair of the destination, both origins, both weights, k in {0, 1, 2, kDim} (R: k = 0 only).  The
    bar, per case: 10 x the error of the float64 twin against the longdouble twin on the same input + the derived bound
    (AD.radial_bound: band and running-sum rounding of the right-hand side, eps cond of the destination's solve).  Max norm, relative to
    the column's largest coefficient.  A class with fewer than 4 free unknowns must be refused (4 and 5 cells with the higher ranks)."""
    import scythe_jl_amd as S
    has_l = geometry == "RL"
    kDim = 3 * nc if has_l else 0
    grid = dict(has_l=has_l, xmin=0.0, xmax=7.0, nc=nc, kDim=kDim, Zb=1)
    rng = np.random.default_rng(11 + nc)
    a = rng.standard_normal(nc + 3)
    Px = {(o, w): AD.rhs_matrix(grid, o, w, True)[0] for o in ("low", "high") for w in (False, True)}
    P64 = {(o, w): AD.rhs_matrix(grid, o, w, False)[0] for o in ("low", "high") for w in (False, True)}
    worst, solved, refused = 0.0, 0, 0
    for bcl, bcr in itertools.product(EL.NONPERIODIC, EL.NONPERIODIC):
        gp = _patch(geometry, nc, bcl, bcr)
        for k in sorted({0, 1, 2, kDim} if has_l else {0}):
            left = K0_BCL if has_l and k == 0 else bcl
            for origin, wr in Px:
                if nc + 3 - EL.RANK[left] - EL.RANK[bcr] < 4:
                    with pytest.raises(S.ScytheHipError, match="too few cells"):
                        S.antiderivative_check(gp, "f", "F", "r", origin, wr, k, a)
                    refused += 1
                    continue
                got = S.antiderivative_check(gp, "f", "F", "r", origin, wr, k, a)
                truth = AD.radial(grid, a, origin, wr, left, bcr, 2.0, True, Px[origin, wr])
                f64 = AD.radial(grid, a, origin, wr, left, bcr, 2.0, False, P64[origin, wr])
                sc = float(np.abs(truth).max())
                e_new, e_f64 = float(np.abs(got - truth).max()) / sc, float(np.abs(f64 - truth).max()) / sc
                bound = 10.0 * e_f64 + AD.radial_bound(grid, a, origin, wr, left, bcr)
                worst = max(worst, e_new / bound)
                assert np.isfinite(got).all() and e_new <= bound, (bcl, bcr, k, origin, wr, e_new, e_f64, bound)
                solved += 1
    print("%s nc=%d: %d solved, %d refused, worst error / bar %.3f" % (geometry, nc, solved, refused, worst))
    assert solved > 0 and (refused > 0) == (nc < 7)            # ranks 3 + 3 leave nc - 3 free unknowns


@pytest.mark.parametrize("zDim", [9, 20, 40])
def test_vertical_check_against_the_longdouble_twin(zDim):
    """each supported (bcb, bct) of the source, both origins; bar: 10 x the float64 twin's error + AD.vertical_bound"""
    import scythe_jl_amd as S
    worst = 0.0
    for bcb, bct in itertools.product(CHEB_BCS, CHEB_BCS):
        gp = _patch("RZ", 5, zDim=zDim, BCB={"f": bcb}, BCT={"f": bct})
        grid = dict(has_l=False, xmin=0.0, xmax=7.0, nc=5, kDim=0, Zb=gp.b_zDim, zmin=0.0, zmax=3.0, zDim=zDim)
        b = np.random.default_rng(zDim).standard_normal(gp.b_zDim)
        for origin in ("low", "high"):
            got = S.antiderivative_check(gp, "f", "F", "z", origin, False, 0, b)
            truth, f64 = AD.vertical(grid, b, origin, bcb, bct, True), AD.vertical(grid, b, origin, bcb, bct, False)
            sc = float(np.abs(truth).max())
            e_new, e_f64 = float(np.abs(got - truth).max()) / sc, float(np.abs(f64 - truth).max()) / sc
            bound = 10.0 * e_f64 + AD.vertical_bound(grid, b, origin, bcb, bct)
            worst = max(worst, e_new / bound)
            assert e_new <= bound, (bcb, bct, origin, e_new, e_f64, bound)
    print("zDim=%d b_zDim=%d: worst error / bar %.3f" % (zDim, gp.b_zDim, worst))


@pytest.mark.parametrize("zDim", [9, 20, 40])
def test_twin_vertical_is_the_oracles_operator(zDim):
    """the twin's F at the levels is oracle_np.Cheb.Mint (b -> integral from the bottom) applied to the same b"""
    from oracle import oracle_np as onp
    for bcb, bct in (("R0", "R0"), ("R1T0", "R1T1"), ("R1T2", "R1T0")):
        ch = onp.Cheb(0.0, 3.0, zDim, None, bcb, bct)
        grid = dict(has_l=False, xmin=0.0, xmax=7.0, nc=5, kDim=0, Zb=ch.bdim, zmin=0.0, zmax=3.0, zDim=zDim)
        b = np.random.default_rng(3).standard_normal(ch.bdim)
        want = ch.Mint @ b
        got = AD.vertical_values(grid, b, "low", bcb, bct, True).astype(np.float64)
        assert np.abs(got - want).max() <= 8 * zDim * EPS * np.abs(ch.Mint).max() * np.abs(b).max()


def test_high_plus_low_is_the_projected_constant():
    """F_low + F_high = int w f over the patch, a constant: the two calls sum to its projection within the sum of their bars"""
    import scythe_jl_amd as S
    for geometry, nc, bcl, bcr in (("R", 37, "R0", "R0"), ("RL", 5, "R1T1", "R0"), ("R", 5, "R0", "R1T1")):
        has_l = geometry == "RL"
        grid = dict(has_l=has_l, xmin=0.0, xmax=7.0, nc=nc, kDim=3 * nc if has_l else 0, Zb=1)
        gp = _patch(geometry, nc, bcl, bcr)
        left = K0_BCL if has_l else bcl
        a = np.random.default_rng(nc).standard_normal(nc + 3)
        for wr in (False, True):
            total, tol = 0.0, 0.0
            for origin in ("low", "high"):
                got = S.antiderivative_check(gp, "f", "F", "r", origin, wr, 0, a)
                truth, f64 = AD.radial(grid, a, origin, wr, left, bcr, 2.0, True), AD.radial(grid, a, origin, wr, left, bcr, 2.0, False)
                sc = float(np.abs(truth).max())
                tol += sc * (10.0 * float(np.abs(f64 - truth).max()) / sc + AD.radial_bound(grid, a, origin, wr, left, bcr))
                total = total + got.astype(EL.XP)
            _, c, m = AD.rhs_matrix(grid, "low", wr, True)
            G, K = AD.radial_operator(grid, left, bcr, 2.0, True)
            const = G.T @ EL.dense_solve(K, G @ (m * (c @ a.astype(EL.XP))), True)
            assert float(np.abs(total - const).max()) <= tol, (geometry, wr, float(np.abs(total - const).max()), tol)


def _refused(match, fn, *args):
    import scythe_jl_amd as S
    with pytest.raises(S.ScytheHipError, match=match):
        fn(*args)


def test_refusals_without_a_device():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    a, out = np.ones(11), np.zeros(11)
    pa, po = a.ctypes.data_as(L.P_D), out.ctypes.data_as(L.P_D)
    ok = _patch("RL", 8)
    chk = S.antiderivative_check
    assert np.isfinite(chk(ok, "f", "F", "r", "low", True, 3, a)).all()
    assert lib.sx_antiderivative(None, 1, 0, 0, 0, None, 1) != 0 and b"null handle" in lib.sx_last_error()
    assert lib.sx_antiderivative_check(None, 1, 2, 0, 0, 0, 0, pa, po) != 0 and b"null" in lib.sx_last_error()
    d, keep = S.model.grid_desc(ok)
    assert lib.sx_antiderivative_check(C.byref(d), 1, 2, 0, 0, 0, 0, None, po) != 0 and b"null" in lib.sx_last_error()
    assert lib.sx_antiderivative_check(C.byref(d), 1, 2, 0, 0, 0, 0, pa, None) != 0 and b"null" in lib.sx_last_error()
    for axis, origin, weight, word in ((2, 0, 0, "axis"), (-1, 0, 0, "axis"), (0, 2, 0, "origin"), (0, -1, 0, "origin"), (0, 0, 2, "weight"), (0, 0, -1, "weight")):
        assert lib.sx_antiderivative_check(C.byref(d), 1, 2, axis, origin, weight, 0, pa, po) != 0 and word.encode() in lib.sx_last_error()
    for vs, vd in ((0, 2), (3, 2), (1, 0), (1, 3)):
        _refused("variable index out of range", chk, ok, vs, vd, "r", "low", False, 0, a)
    for k in (-1, 25):
        _refused("wavenumber out of range", chk, ok, "f", "F", "r", "low", False, k, a)
    _refused("wavenumber out of range", chk, _patch("R", 8), "f", "F", "r", "low", False, 1, a)
    d4, keep4 = S.model.grid_desc(ok, 0, 4)
    assert lib.sx_antiderivative_check(C.byref(d4), 1, 2, 0, 0, 0, 0, pa, po) != 0 and b"one-tile" in lib.sx_last_error()
    # the vertical axis: a grid without one, a weight
    _refused("RZ or RLZ", chk, ok, "f", "F", "z", "low", False, 0, a)
    zp = _patch("RZ", 8)
    b = np.ones(zp.b_zDim)
    assert np.isfinite(chk(zp, "f", "F", "z", "high", False, 0, b)).all()
    _refused("takes no weight", chk, zp, "f", "F", "z", "low", True, 0, b)
    # the conditions that are carried one to one
    _refused("PERIODIC", chk, _patch("R", 8, "PERIODIC", "PERIODIC"), "f", "F", "r", "low", False, 0, a)
    _refused("vertical boundary conditions differ", chk, _patch("RZ", 8, BCB={"f": "R1T0"}), "f", "F", "r", "low", False, 0, a)
    _refused("radial boundary conditions differ", chk, _patch("RZ", 8, "R1T0", "R0"), "f", "F", "z", "low", False, 0, b)
    _refused("radial boundary conditions differ", chk, _patch("RZ", 8, "R0", "R1T1"), "f", "F", "z", "low", False, 0, b)
    assert (out == 0).all()             # nothing was written by any refusal


# ---------------------------------------------------------------------------------------------- the twin against closed forms
def _project(grid, f):
    """Galerkin projection of f(r) onto the unconstrained spline space: M0 a = int phi f"""
    r, w = EL.quadrature(grid, True)
    ph = EL.basis(grid, r, 0, True)
    return EL.dense_solve(ph.T @ (w[:, None] * ph), ph.T @ (w * f(r)), True)


def _sampled_error(grid, a, exact, n=400):
    r = np.linspace(grid["xmin"], grid["xmax"], n).astype(EL.XP)
    return float(np.abs(EL.basis(grid, r, 0, True) @ a - exact(r)).max())


LQS = (2.0, 1e-3)          # the model's default filter length, and the filter as good as off


def _report(title, ncs, errs, l_q):
    """The figures are recorded in DESIGN.md 20, not fixed here; the floors only say that the error falls as a fourth-order scheme's
    does without the filter (> 8, the floor tests/test_elliptic.py uses) and still faster than second order with it: eps_q Q penalises
    the third derivative of F, and its natural conditions (third derivative zero at the two ends) leave a boundary layer."""
    ratio = errs[0] / errs[1]
    print("%s, l_q = %g: max error %.3e at %d cells, %.3e at %d cells, ratio %.2f" % (title, l_q, errs[0], ncs[0], errs[1], ncs[1], ratio))
    assert ratio > (4.0 if l_q > 1.0 else 8.0), (title, l_q, errs)


def test_twin_closed_form_sine():
    """int_0^x sin(pi s / L) ds = (L / pi) (1 - cos(pi x / L)), and from the other end"""
    Lx, ncs = 7.0, (10, 20)
    for origin, exact in (("low", lambda x: Lx / np.pi * (1 - np.cos(np.pi * x / Lx))), ("high", lambda x: Lx / np.pi * (1 + np.cos(np.pi * x / Lx)))):
        for l_q in LQS:
            errs = []
            for nc in ncs:
                grid = dict(has_l=False, xmin=0.0, xmax=Lx, nc=nc, kDim=0, Zb=1)
                a = _project(grid, lambda x: np.sin(np.pi * x / Lx))
                errs.append(_sampled_error(grid, AD.radial(grid, a, origin, False, "R0", "R0", l_q, True), exact))
            _report("R int sin from " + origin, ncs, errs, l_q)


def test_twin_closed_form_bessel():
    """int_0^r s J_0(kappa s) ds = r J_1(kappa r) / kappa (scipy's Bessel functions in float64: far below the errors compared)"""
    from scipy.special import jv
    R, kap, ncs = 5.0, 1.3, (10, 20)
    for l_q in LQS:
        errs = []
        for nc in ncs:
            grid = dict(has_l=True, xmin=0.0, xmax=R, nc=nc, kDim=3 * nc, Zb=1)
            a = _project(grid, lambda r: jv(0, kap * np.asarray(r, dtype=np.float64)).astype(EL.XP))
            F = AD.radial(grid, a, "low", True, "R0", "R0", l_q, True)
            errs.append(_sampled_error(grid, F, lambda r: (np.asarray(r, dtype=np.float64) * jv(1, kap * np.asarray(r, dtype=np.float64)) / kap).astype(EL.XP)))
        _report("RL int s J_0(kappa s)", ncs, errs, l_q)


def test_twin_closed_form_chebyshev():
    """b = e_3 with free ends is u = 2 T_3(x): int_{zmin}^{z} u dz' = -(Lz / 2) (T_4 / 4 - T_2 / 2 + 1 / 4), exact below the truncation;
    the library's column agrees with CB of it within the vertical bar"""
    import scythe_jl_amd as S
    zDim, Lz = 20, 3.0
    gp = _patch("RZ", 5, zDim=zDim)
    grid = dict(has_l=False, xmin=0.0, xmax=7.0, nc=5, kDim=0, Zb=gp.b_zDim, zmin=0.0, zmax=Lz, zDim=zDim)
    b = np.zeros(gp.b_zDim)
    b[3] = 1.0
    x = np.cos(np.arange(zDim).astype(EL.XP) * np.arccos(EL.XP(-1)) / (zDim - 1))
    T = lambda n: np.cos(n * np.arccos(x))
    exact = -(EL.XP(Lz) / 2) * (T(4) / 4 - T(2) / 2 + EL.XP(1) / 4)
    got = AD.vertical_values(grid, b, "low", "R0", "R0", True)
    assert float(np.abs(got - exact).max()) <= 64 * float(np.finfo(EL.XP).eps) * float(np.abs(exact).max())
    lib = S.antiderivative_check(gp, "f", "F", "z", "low", False, 0, b)
    truth = AD.vertical(grid, b, "low", "R0", "R0", True)
    assert float(np.abs(lib - truth).max()) <= AD.vertical_bound(grid, b, "low", "R0", "R0") * float(np.abs(truth).max()) + 10 * EPS * float(np.abs(truth).max())
