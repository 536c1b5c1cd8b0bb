"""TEST INFRASTRUCTURE - the numpy twin of sx_antiderivative / sx_antiderivative_check (include/scythe_hip.h), in float64
and in longdouble (the arbiter).

An independent statement.  Radial: Phi_j(r) = int_{xmin}^{r} w phi_j by EXACT integration of the cell polynomials of the cubic B-spline
(no band, no running sum), the dense P[i][j] = int phi_i Phi_j with this file's own Gauss nodes (tests/elliptic.py's), the projection
matrix Gamma (P + eps_q Q) Gamma^T from its definition (the exact Gram matrix as tests/elliptic.py forms M0; Q, eps_q and Gamma as
oracle_np.Spline1D has them) and a dense solve.  Vertical: numpy's chebint on the Chebyshev coefficients a = CA b, truncated to the
N coefficients the grid holds, evaluated at the levels and taken back to the truncated b with CB.

A grid is tests/elliptic.py's dict plus, with a vertical, zmin, zmax, zDim.  Coefficient arrays of one variable are [Zb, K2ref, nb]."""
import functools

import numpy as np
from numpy.polynomial import chebyshev as Ch
from numpy.polynomial import polynomial as Po

from tests import elliptic as EL

XP = EL.XP
EPS = float(np.finfo(np.float64).eps)
_ty = EL._ty


# ---------------------------------------------------------------------------------------------- radial
def _cell_polys(ty):
    """the four cubics of a cell in its local coordinate t in [0, 1]: node c + j, j = 0 .. 3 (ascending coefficients)"""
    one_minus, one_plus, two_minus, t = np.array([1, -1], ty), np.array([1, 1], ty), np.array([2, -1], ty), np.array([0, 1], ty)
    cube = lambda p: Po.polymul(Po.polymul(p, p), p)
    six = ty(6)
    return [cube(one_minus) / six, Po.polysub(cube(two_minus), 4 * cube(one_minus)) / six, Po.polysub(cube(one_plus), 4 * cube(t)) / six, cube(t) / six]


def primitives(grid, weight_r, xp=True):
    """(r, w, Phi [points, nb], c [nb]): tests/elliptic.py's quadrature points and weights, Phi_j = int_{xmin}^{r} w phi_j at them by
    exact polynomial integration cell by cell, and c_j = Phi_j(xmax)"""
    ty = _ty(xp)
    nc = grid["nc"]
    nb = nc + 3
    DX = (ty(grid["xmax"]) - ty(grid["xmin"])) / nc
    x, _ = EL.gauss_legendre(8, bool(xp))
    t = (1 + x.astype(ty)) / 2
    r, w = EL.quadrature(grid, xp)
    polys = _cell_polys(ty)
    Phi = np.zeros((nc * 8, nb), dtype=ty)
    below = np.zeros(nb, dtype=ty)
    for c in range(nc):
        Phi[c * 8:(c + 1) * 8, :] = below[None, :]
        for j in range(4):
            p = polys[j]
            if weight_r:
                p = Po.polymul(p, np.array([ty(grid["xmin"]) + c * DX, DX], ty))
            q = Po.polyint(p) * DX               # dr = DX dt; zero at t = 0
            Phi[c * 8:(c + 1) * 8, c + j] += Po.polyval(t, q)
            below[c + j] += Po.polyval(ty(1), q)
    return r, w, Phi, below


def rhs_matrix(grid, origin, weight_r, xp=True):
    """dense [nb, nb] P[i][j] = int phi_i Phi_j dr (origin "low") or int phi_i (c_j - Phi_j) dr ("high"), with (c, m)"""
    r, w, Phi, c = primitives(grid, weight_r, xp)
    ph = EL.basis(grid, r, 0, xp)
    if origin == "high":
        Phi = c[None, :] - Phi
    return ph.T @ (w[:, None] * Phi), c, ph.T @ w


def projection_matrix(grid, l_q=2.0, xp=True):
    """P + eps_q Q [nb, nb] with the EXACT Gram matrix P = int phi phi (8-point rule, as tests/elliptic.py forms M0) and Q = int phi3 phi3
    of the third derivatives (constant on a cell: the rule is exact), eps_q = (l_q DX / 2 pi)^6 as oracle_np.Spline1D has them.  The
    model's own P is its 3-point quadrature of the Gram matrix (weights 8 : 5 : 8: 0.355 DX on the diagonal against 0.336 DX) and pairs
    only with right-hand sides formed by that rule; the exact right-hand side of the antiderivative needs the exact matrix."""
    ty = _ty(xp)
    nc = grid["nc"]
    DX = (ty(grid["xmax"]) - ty(grid["xmin"])) / nc
    mish, W = EL.quadrature(grid, xp)
    nodes = ty(grid["xmin"]) + (np.arange(nc + 3) - 1).astype(ty) * DX
    delta = (mish[:, None] - nodes[None, :]) / DX
    ph0 = EL.bspl(delta, 0)
    z = np.abs(delta)
    ph3 = np.where(z < 2, np.sign(delta) * np.where(z < 1, 3.0, -1.0), 0.0).astype(ty) / DX ** 3
    eps_q = (ty(l_q) * DX / (2 * np.arccos(ty(-1)))) ** 6
    return ph0.T @ (W[:, None] * ph0) + eps_q * (ph3.T @ (W[:, None] * ph3))


def radial_operator(grid, bcl, bcr, l_q=2.0, xp=True):
    """(Gamma, Gamma (P + eps_q Q) Gamma^T) of the destination's class"""
    G = EL.gamma(grid["nc"], bcl, bcr).astype(_ty(xp))
    return G, G @ projection_matrix(grid, l_q, xp) @ G.T


def radial(grid, a, origin, weight_r, bcl, bcr, l_q=2.0, xp=True, P=None):
    """a_dst [nb, ...] of source columns a [nb, ...]: the twin of sx_antiderivative_check along r"""
    ty = _ty(xp)
    P = rhs_matrix(grid, origin, weight_r, xp)[0] if P is None else P
    G, K = radial_operator(grid, bcl, bcr, l_q, xp)
    return G.T @ EL.dense_solve(K, G @ (P @ np.asarray(a, dtype=ty)), xp)


def radial_bound(grid, a, origin, weight_r, bcl, bcr, l_q=2.0):
    """Derived rounding bound of an output coefficient, relative to the column's largest: the right-hand side is formed with errors of
    at most 8 eps sum_j |P_ij a_j| (7 fma and the rounded table) in the band and m_i nb eps sum_j |c_j a_j| in the running sum (nb serial
    fma, each entry of c rounded once); a backward-stable solve loses a few eps cond_2 of its own (4, as tests/test_elliptic.py allows)
    and carries the right-hand side's relative error times cond_2 at most."""
    P, c, m, cond = _bound_parts(tuple(sorted(grid.items())), origin, weight_r, bcl, bcr, l_q)
    a = np.asarray(a, dtype=np.float64)
    b = P @ a
    nb = grid["nc"] + 3
    db = 8.0 * (np.abs(P) @ np.abs(a)).max() + nb * np.abs(m).max() * np.abs(c * a).sum()
    return EPS * cond * (4.0 + db / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def _bound_parts(items, origin, weight_r, bcl, bcr, l_q):
    grid = dict(items)
    return rhs_matrix(grid, origin, weight_r, False) + (np.linalg.cond(radial_operator(grid, bcl, bcr, l_q, False)[1]),)


def apply_radial(grid, a, origin, weight_r, bcl_k0, bcl, bcr, l_q=2.0, xp=True):
    """one variable [Zb, K2ref, nb] -> the same shape, every column with the class of its wavenumber"""
    ty = _ty(xp)
    a = np.asarray(a, dtype=ty)
    P = rhs_matrix(grid, origin, weight_r, xp)[0]
    out = np.zeros(a.shape, dtype=ty)
    out[:, 0] = radial(grid, a[:, 0].T, origin, weight_r, bcl_k0, bcr, l_q, xp, P).T
    if a.shape[1] > 1:
        rest = a[:, 1:].reshape(-1, a.shape[2]).T
        out[:, 1:] = radial(grid, rest, origin, weight_r, bcl, bcr, l_q, xp, P).T.reshape(a.shape[0], a.shape[1] - 1, a.shape[2])
    return out


# ---------------------------------------------------------------------------------------------- vertical
def _cheb(grid, bcb, bct):
    return _cheb_cached(grid["zmin"], grid["zmax"], grid["zDim"], grid["Zb"], bcb, bct)


@functools.lru_cache(maxsize=None)
def _cheb_cached(zmin, zmax, zDim, Zb, bcb, bct):
    from oracle import oracle_np as onp
    return onp.Cheb(zmin, zmax, zDim, Zb, bcb, bct)


def vertical_values(grid, b, origin, bcb, bct, xp=True):
    """F at the levels [zDim, ...] (bottom first) of source columns b [Zb, ...]: chebint of the series of a = CA b (DCT-I
    normalisation u = a_0 + 2 sum a_k T_k + a_{N-1} T_{N-1}, x = +1 at the bottom, dz = -(Lz / 2) dx), the T_N term dropped
    (the grid holds N coefficients) and the constant set so that the truncated series is zero at the bottom."""
    ty = _ty(xp)
    ch = _cheb(grid, bcb, bct)
    N = grid["zDim"]
    CA = ch._x["CA"] if xp else ch.CAm
    a = CA.astype(ty) @ np.asarray(b, dtype=ty).reshape(len(b), -1)
    c = a.copy()
    c[1:N - 1] *= 2
    Lz = ty(grid["zmax"]) - ty(grid["zmin"])
    ci = Ch.chebint(c, scl=-Lz / 2, axis=0)[:N]
    ci[0] = -ci[1:].sum(axis=0)                           # every T_k(+1) = 1
    n = np.arange(N)
    pi = np.arccos(ty(-1))
    Tn = np.cos(np.outer(n, n).astype(ty) * pi / ty(N - 1))             # T_k(x_n), plain
    F = Tn @ ci
    if origin == "high":
        F = F[N - 1][None] - F
    return F.reshape((N,) + np.shape(b)[1:])


def vertical(grid, b, origin, bcb, bct, xp=True):
    """b_dst [Zb, ...] of source columns b [Zb, ...]: the twin of sx_antiderivative_check along z"""
    ty = _ty(xp)
    ch = _cheb(grid, bcb, bct)
    CB = ch._x["CB"] if xp else ch.CBm
    F = vertical_values(grid, b, origin, bcb, bct, xp)
    return (CB.astype(ty) @ F.reshape(len(F), -1)).reshape(np.shape(b))


def vertical_matrix(grid, origin, bcb, bct, xp=False):
    return vertical(grid, np.eye(grid["Zb"]), origin, bcb, bct, xp)


def vertical_bound(grid, b, origin, bcb, bct):
    """Derived rounding bound, relative to the column's largest output: Zb fma with entries of Z rounded once:
    (Zb + 1) eps max_i sum_j |Z_ij b_j| / max_i |sum_j Z_ij b_j|; b [Zb] or columns [Zb, n]"""
    Z = vertical_matrix(grid, origin, bcb, bct)
    b = np.asarray(b, dtype=np.float64)
    return (grid["Zb"] + 1) * EPS * (np.abs(Z) @ np.abs(b)).max(axis=0) / np.abs(Z @ b).max(axis=0)


def apply_vertical(grid, a, origin, bcb, bct, xp=True):
    """one variable [Zb, K2ref, nb] -> the same shape"""
    a = np.asarray(a, dtype=_ty(xp))
    return vertical(grid, a.reshape(a.shape[0], -1), origin, bcb, bct, xp).reshape(a.shape)


# ---------------------------------------------------------------------------------------------- errors
def column_error(got, truth):
    """[Zb, K2ref] (axis -1 = the column) max |got - truth| / max |truth| of each column; a zero column must be reproduced exactly"""
    got, truth = np.asarray(got, dtype=XP), np.asarray(truth, dtype=XP)
    diff, sc = np.abs(got - truth).max(axis=-1), np.abs(truth).max(axis=-1)
    return np.where(sc > 0, diff / np.where(sc > 0, sc, 1), np.where(diff > 0, np.inf, 0)).astype(np.float64)


def grid_of(gp, kDim):
    g = EL.grid_of(gp, kDim)
    if "Z" in gp.geometry:
        g.update(zmin=gp.zmin, zmax=gp.zmax, zDim=gp.zDim)
    return g
