"""CPU-only: the host side of sx_elliptic_solve (include/scythe_hip.h "elliptic inversion") - the symbols, the matrix
construction and the banded sweep (sx_elliptic_check) against the dense longdouble twin of tests/elliptic.py, every refusal that needs no
device, and the twin itself against closed forms."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import elliptic as EL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
FIXES_VALUE = ("R1T0", "R2T10", "R2T20", "R3")        # boundary conditions under which every admissible function is zero at the end


def _patch(geometry, nc, bcl, bcr, bcl_k0=None, xmin=0.0, xmax=7.0):
    import scythe_jl_amd as S
    return S.GridParameters(geometry=geometry, xmin=xmin, xmax=xmax, num_cells=nc, vars={"psi": 1}, BCL={"psi": bcl}, BCR={"psi": bcr},
                            BCL_k0=None if bcl_k0 is None else {"psi": bcl_k0})


def test_symbols():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    header = open(os.path.join(ROOT, "include", "scythe_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "hipTile.jl")).read()
    for name in ("sx_elliptic_solve", "sx_elliptic_check"):
        assert hasattr(lib, name) and name in L.SYMBOLS
        assert name + "(" in header and ":" + name in julia
    assert "#define SX_ABI_VERSION 2" in header


def _expected_refusal(has_l, nc, bcl, bcr, k, alpha):
    """why the library must refuse the case, from the issue's list (None: it must solve it)"""
    if nc + 3 - EL.RANK[bcl] - EL.RANK[bcr] < 4:
        return "too few cells"
    if alpha == 0 and k == 0 and bcl not in FIXES_VALUE and bcr not in FIXES_VALUE:
        return "singular"
    if has_l and k >= 1 and bcl not in FIXES_VALUE:
        return "vanish at r = 0"
    return None


@pytest.mark.parametrize("nc", [4, 5, 37])
@pytest.mark.parametrize("geometry", ["R", "RL"])
def test_check_against_the_longdouble_twin(geometry, nc):
    """Every non-periodic (bcl, bcr) pair, k in {0, 1, 2, kDim} (R: k = 0 only, the one wavenumber it has), alpha in {0, 0.37}.
    The bar, per case: 10 x the error of the float64 twin against the longdouble twin on the same right-hand side (the rule of the GPU
    parity test) + 4 eps cond_2(K_k).  The second term is what any backward-stable solve of K_k x = b may lose (forward error <= cond x
    backward error of a few eps); it keeps a case in which the float64 twin happens to land within an ulp or two from asking more of the
    library than the problem's conditioning allows.  Max norm, relative to the column's largest coefficient."""
    import scythe_jl_amd as S
    has_l = geometry == "RL"
    kDim = 3 * nc if has_l else 0             # native rings: kmax = ring index
    grid = dict(has_l=has_l, xmin=0.0, xmax=7.0, nc=nc, kDim=kDim, Zb=1)
    mx, m64 = EL.matrices(grid, True), EL.matrices(grid, False)
    rng = np.random.default_rng(5 + nc)
    g = rng.standard_normal(nc + 3)
    worst, solved, refused = 0.0, 0, 0
    for bcl in EL.NONPERIODIC:
        for bcr in EL.NONPERIODIC:
            gp = _patch(geometry, nc, bcl, bcr)
            for k in sorted({0, 1, 2, kDim} if has_l else {0}):
                for alpha in (0.0, 0.37):
                    why = _expected_refusal(has_l, nc, bcl, bcr, k, alpha)
                    if why:
                        with pytest.raises(S.ScytheHipError, match=why):
                            S.elliptic_check(gp, "psi", k, alpha, g)
                        refused += 1
                        continue
                    got = S.elliptic_check(gp, "psi", k, alpha, g)
                    truth = EL.solve_rhs(grid, g, k, alpha, bcl, bcr, True, mx)
                    f64 = EL.solve_rhs(grid, g, k, alpha, bcl, bcr, False, m64)
                    sc = float(np.abs(truth).max())
                    e_new, e_f64 = float(np.abs(got - truth).max()) / sc, float(np.abs(f64 - truth).max()) / sc
                    cond = np.linalg.cond(EL.operator(grid, m64, k, alpha, bcl, bcr, False)[1])
                    bound = 10.0 * e_f64 + 4.0 * EPS * cond
                    worst = max(worst, e_new / bound)
                    assert np.isfinite(got).all() and e_new <= bound, (bcl, bcr, k, alpha, e_new, e_f64, cond)
                    solved += 1
    print("%s nc=%d: %d solved, %d refused, worst error / bound %.3f" % (geometry, nc, solved, refused, worst))
    assert solved > 0 and refused > 0


def _refused(match, fn, *args):
    import scythe_jl_amd as S
    with pytest.raises(S.ScytheHipError, match=match):
        fn(*args)


def test_refusals_without_a_device():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    g = np.ones(11)
    ok = _patch("RL", 8, "R1T0", "R1T0", bcl_k0="R1T1")
    assert np.isfinite(S.elliptic_check(ok, 1, 3, 0.0, g)).all()
    # null handles, a null descriptor, null arrays
    assert lib.sx_elliptic_solve(None, 0, 1, 0, 0.0, None, 1) != 0 and b"null handle" in lib.sx_last_error()
    a = np.zeros(11)
    assert lib.sx_elliptic_check(None, 1, 0, 0.0, g.ctypes.data_as(L.P_D), a.ctypes.data_as(L.P_D)) != 0 and b"null" in lib.sx_last_error()
    d, keep = S.model.grid_desc(ok)
    assert lib.sx_elliptic_check(C.byref(d), 1, 0, 0.0, None, a.ctypes.data_as(L.P_D)) != 0 and b"null" in lib.sx_last_error()
    # a variable index out of range, a wavenumber the patch does not have
    _refused("variable index out of range", S.elliptic_check, ok, 0, 0, 0.0, g)
    _refused("variable index out of range", S.elliptic_check, ok, 2, 0, 0.0, g)
    _refused("wavenumber out of range", S.elliptic_check, ok, 1, 25, 0.0, g)
    _refused("wavenumber out of range", S.elliptic_check, ok, 1, -1, 0.0, g)
    _refused("wavenumber out of range", S.elliptic_check, _patch("R", 8, "R1T0", "R1T0"), 1, 1, 0.0, g)
    # alpha
    for alpha in (-0.5, float("nan"), float("inf")):
        _refused("alpha must be finite", S.elliptic_check, ok, 1, 0, alpha, g)
    # PERIODIC radial conditions on the solution variable
    _refused("PERIODIC", S.elliptic_check, _patch("R", 8, "PERIODIC", "PERIODIC"), 1, 0, 0.5, g)
    # alpha = 0 with a k = 0 class that fixes the value on neither side; the same class with alpha > 0 is solved
    free = _patch("RL", 8, "R1T0", "R1T1", bcl_k0="R1T1")
    _refused("singular", S.elliptic_check, free, 1, 0, 0.0, g)
    assert np.isfinite(S.elliptic_check(free, 1, 0, 0.25, g)).all()
    # xmin == 0 on RL: a k >= 1 class that does not vanish at r = 0; with xmin > 0 the same class is solved
    _refused("vanish at r = 0", S.elliptic_check, _patch("RL", 8, "R1T1", "R1T0"), 1, 2, 0.0, g)
    assert np.isfinite(S.elliptic_check(_patch("RL", 8, "R1T1", "R1T0", xmin=1.0), 1, 2, 0.0, g)).all()
    # not a one-tile patch
    d, keep = S.model.grid_desc(ok, 0, 4)
    assert lib.sx_elliptic_check(C.byref(d), 1, 0, 0.0, g.ctypes.data_as(L.P_D), a.ctypes.data_as(L.P_D)) != 0
    assert b"one-tile" in lib.sx_last_error()
    assert (a == 0).all()           # nothing was written by any refusal


# ---------------------------------------------------------------------------------------------- the twin against closed forms
def _sampled_error(grid, a, exact, n=400):
    r = np.linspace(grid["xmin"], grid["xmax"], n).astype(EL.XP)
    return float(np.abs(EL.basis(grid, r, 0, True) @ a - exact(r)).max())


def _report(title, ncs, errs):
    ratio = errs[0] / errs[1]
    print("%s: max error %.3e at %d cells, %.3e at %d cells, ratio %.2f" % (title, errs[0], ncs[0], errs[1], ncs[1], ratio))
    assert ratio > 8.0, (title, errs)


def test_twin_closed_form_r():
    """psi = sin(pi x / L) on [0, L] with psi = 0 at both ends: f = -(pi / L)^2 psi"""
    Lx, ncs, errs = 7.0, (10, 20), []
    for nc in ncs:
        grid = dict(has_l=False, xmin=0.0, xmax=Lx, nc=nc, kDim=0, Zb=1)
        psi = lambda x: np.sin(np.pi * x / Lx)
        g = EL.load_vector(grid, lambda x: -(np.pi / Lx) ** 2 * psi(x), True)
        errs.append(_sampled_error(grid, EL.solve_rhs(grid, g, 0, 0.0, "R1T0", "R1T0", True), psi))
    _report("R sin(pi x / L)", ncs, errs)


@pytest.mark.parametrize("m", [0, 2])
def test_twin_closed_form_rl(m):
    """psi = J_m(kappa r) cos m lambda with kappa R the first zero of J_m: f = -kappa^2 psi; wavenumber m, psi(R) = 0, and at the
    centre zero slope (m = 0) or zero value (m = 2).  Bessel functions from scipy in float64: their error is far below the
    discretisation errors compared here."""
    from scipy.special import jn_zeros, jv
    R, ncs, errs = 5.0, (10, 20), []
    kap = jn_zeros(m, 1)[0] / R
    for nc in ncs:
        grid = dict(has_l=True, xmin=0.0, xmax=R, nc=nc, kDim=3 * nc, Zb=1)
        psi = lambda r: jv(m, kap * np.asarray(r, dtype=np.float64)).astype(EL.XP)
        g = EL.load_vector(grid, lambda r: -kap * kap * psi(r), True)
        a = EL.solve_rhs(grid, g, m, 0.0, "R1T1" if m == 0 else "R1T0", "R1T0", True)
        errs.append(_sampled_error(grid, a, psi))
    _report("RL J_%d(kappa r)" % m, ncs, errs)
