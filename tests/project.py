"""TEST INFRASTRUCTURE - the numpy twin of sx_project (include/scythe_hip.h).

The values of an output at the gridpoints are tests/distribution.py::program_values64, the rule k_project is held to bitwise.  The
projection is oracle_np's own: Grid.forward + Grid.spline_transform in float64 (the model's spectralTransform! + splineTransform!
of the companion's variables), and forward_xp followed by the same solve in longdouble as the arbiter.  oracle_np's l_q penalty is
on the THIRD derivative (Spline1D.P: eps_q ph3^T W ph3), so a field that is a cubic spline without a third derivative - r^2 - is
reproduced by an R0 / R0 variable whatever l_q is: the second pin below runs with the default l_q."""
import numpy as np

from oracle import oracle_np as O
from tests import distribution as D
from tests import elliptic as EL

XP = O.XP


def companion(grid, names, b_zDim=None, **bcs):
    """the oracle Grid of a companion of `grid` (an oracle Grid) with the variables `names`; bcs: BCL, BCL_k0, BCR, BCB, BCT dicts"""
    return O.Grid(grid.geometry, grid.xmin, grid.xmax, grid.nc, {n: i + 1 for i, n in enumerate(names)}, l_q=grid.l_q, zmin=grid.zmin,
                  zmax=grid.zmax, zDim=grid.zDim if grid.has_z else 0, b_zDim=b_zDim or (grid.b_zDim if grid.has_z else None),
                  ring_L=int(grid.L[0]) if grid.has_l and len(set(grid.L)) == 1 else None, **bcs)


def values(data, r, program, var_dst=None):
    """[N, n_out] float64: what k_project writes into the companion's var_np1, output o in column var_dst[o] - 1"""
    n_out = program[2]
    var_dst = range(1, n_out + 1) if var_dst is None else var_dst
    out = np.zeros((np.shape(data)[0], n_out))
    for o, v in enumerate(var_dst):
        out[:, v - 1] = D.program_values64(data, r, program, o)
    return out


def project64(dst, vals):
    """A [S_patch, V] of the companion in float64: oracle_np's forward and spline transform of a one-tile patch"""
    return dst.spline_transform(dst.forward(np.asfortranarray(vals)))      # a variable is a contiguous column, whatever V is


def _spline_xp(dst, bcl, bcr):
    """(Gamma, Gamma (P + eps_q Q) Gamma^T) of one class in longdouble, from the definitions Spline1D states in float64"""
    nb = dst.b_rDim
    ii = np.arange(dst.rDim)
    goff = np.array([-np.sqrt(XP(3) / XP(5)) / 2, XP(0), np.sqrt(XP(3) / XP(5)) / 2], dtype=XP)
    pos = (ii // O.MUBAR).astype(XP) + XP(0.5) + goff[ii % O.MUBAR]
    delta = pos[:, None] - (np.arange(nb, dtype=XP) - 1)[None, :]
    DX = XP(dst.DX)
    ph0, ph3 = O.bspline(delta, 0), O.bspline(delta, 3) / DX ** 3
    W = DX * (np.array([8, 5, 8], dtype=XP) / XP(21))[ii % O.MUBAR]
    eps_q = (XP(dst.l_q) * DX / (2 * O.PI_X)) ** 6
    P = ph0.T @ (W[:, None] * ph0) + eps_q * (ph3.T @ (W[:, None] * ph3))
    G = O.gamma_matrix(dst.nc, bcl, bcr).astype(XP)
    return G, G @ P @ G.T


def project_xp(dst, vals):
    """A [S_patch, V] in longdouble: forward_xp, then a = Gamma^T (Gamma (P + eps_q Q) Gamma^T)^-1 Gamma b by dense elimination"""
    B, _ = O.forward_xp(dst, np.asarray(vals, dtype=np.float64))
    A = np.zeros_like(B)
    ops = {}
    nb = dst.b_rDim
    for vi, v in enumerate(dst.names):
        for blk in range(dst.K2):
            key = (dst.BCL_k0[v] if blk == 0 else dst.BCL[v], dst.BCR[v])
            if key not in ops:
                ops[key] = _spline_xp(dst, *key)
            G, K = ops[key]
            rows = (np.arange(dst.b_zDim)[:, None] * dst.K2 + blk) * nb + np.arange(nb)[None, :]      # [zm, node]
            b = B[rows, vi].T                                                                          # [node, zm]
            A[rows, vi] = (G.T @ EL.dense_solve(K, G @ b)).T
    return A


def radial_values(dst, A, v, radii, zm=0, blk=0):
    """sum_j a_j phi_j(r) of column (zm, blk) of variable v (0-based) at arbitrary radii, in longdouble"""
    nb = dst.b_rDim
    a = np.asarray(A, dtype=XP)[(zm * dst.K2 + blk) * nb:(zm * dst.K2 + blk + 1) * nb, v]
    xm = XP(dst.xmin) + (np.arange(nb, dtype=XP) - 1) * XP(dst.DX)
    ph = O.bspline((np.asarray(radii, dtype=XP)[:, None] - xm[None, :]) / XP(dst.DX), 0)
    return ph @ a


def bar(A):
    """the project's parity bar (README, "Parity"): 1e-10 x max|A|"""
    return 1e-10 * float(np.max(np.abs(np.asarray(A, dtype=np.float64))))


def check_against_twins(got, A64, Axp, what=""):
    """|got - A64| within the parity bar, and got no further from the longdouble twin than the float64 twin is by more than the bar;
    returns the two distances in units of the bar"""
    b = bar(A64)
    d64 = float(np.max(np.abs(got - A64)))
    dxp = float(np.max(np.abs(got.astype(XP) - Axp)))
    txp = float(np.max(np.abs(A64.astype(XP) - Axp)))
    print("%s: |A - f64 twin| = %.3g bar, |A - xp twin| = %.3g bar, |f64 twin - xp twin| = %.3g bar" % (what, d64 / b, dxp / b, txp / b))
    assert d64 <= b, (what, d64, b)
    assert dxp <= txp + b, (what, dxp, txp, b)
    return d64 / b, dxp / b
