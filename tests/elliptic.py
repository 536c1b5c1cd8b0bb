"""TEST INFRASTRUCTURE - the numpy twin of sx_elliptic_solve / sx_elliptic_check (include/scythe_hip.h), in float64 and
in longdouble (the arbiter).

An independent statement: the five matrices come from the definition by Gauss-Legendre quadrature with 8 points per cell and this
file's own nodes, Gamma from this file's own table of the boundary conditions, and every solve is a DENSE Gamma K Gamma^T with dense
elimination - no band storage, no Cholesky sweep, no code shared with the library or with oracle/.

    (lap_h - alpha) psi = f,   K_k = Gamma_k (S + k^2 T + alpha M) Gamma_k^T,   K_k x = -Gamma_k g,   a = Gamma_k^T x

A grid is a plain dict: has_l, xmin, xmax, nc, kDim, Zb (b_zDim, 1 without a vertical).  Coefficient arrays of one variable are
[Zb, K2ref, nb] in the reference's block order (block 0 = wavenumber 0, block 2k - 1 / 2k = Re / Im of wavenumber k), i.e. one
variable's column of Grid.patchSpectral reshaped."""
import functools

import numpy as np

XP = np.longdouble
RANK = {"R0": 0, "R1T0": 1, "R1T1": 1, "R1T2": 1, "R2T10": 2, "R2T20": 2, "R3": 3}
# dependent boundary coefficients in terms of the first two free ones: row q -> (weight of free 0, weight of free 1)
ROWS = {"R0": [], "R3": [(0.0, 0.0)] * 3, "R1T0": [(-4.0, -1.0)], "R1T1": [(0.0, 1.0)], "R1T2": [(2.0, -1.0)],
        "R2T10": [(1.0, 0.0), (-0.5, 0.0)], "R2T20": [(-1.0, 0.0), (0.0, 0.0)]}
NONPERIODIC = ("R0", "R1T0", "R1T1", "R1T2", "R2T10", "R2T20", "R3")


def _ty(xp):
    return XP if xp else np.float64


@functools.lru_cache(maxsize=None)
def gauss_legendre(n, xp):
    """nodes on [-1, 1] and weights of the n-point rule; xp: Newton's iteration on P_n in longdouble from numpy's float64 nodes"""
    x, w = np.polynomial.legendre.leggauss(n)
    if not xp:
        return x, w
    x = x.astype(XP)
    for _ in range(4):
        p0, p1 = np.ones_like(x), x.copy()
        for j in range(2, n + 1):
            p0, p1 = p1, ((2 * j - 1) * x * p1 - (j - 1) * p0) / j
        dp = n * (x * p1 - p0) / (x * x - 1)
        x = x - p1 / dp
    p0, p1 = np.ones_like(x), x.copy()
    for j in range(2, n + 1):
        p0, p1 = p1, ((2 * j - 1) * x * p1 - (j - 1) * p0) / j
    dp = n * (x * p1 - p0) / (x * x - 1)
    return x, 2 / ((1 - x * x) * dp * dp)


def bspl(delta, d):
    """d-th derivative (d = 0, 1) of the cardinal cubic B-spline, in the type of delta"""
    z = np.abs(delta)
    p, q = np.maximum(2 - z, 0), np.maximum(1 - z, 0)
    if d == 0:
        return p ** 3 / 6 - 4 * q ** 3 / 6
    return -np.sign(delta) * (p * p / 2 - 2 * q * q)


def basis(grid, r, d, xp=True):
    """[len(r), nb]: d-th derivative of phi_m at the radii r"""
    ty = _ty(xp)
    nc = grid["nc"]
    DX = (ty(grid["xmax"]) - ty(grid["xmin"])) / nc
    nodes = ty(grid["xmin"]) + (np.arange(nc + 3) - 1).astype(ty) * DX
    return bspl((np.asarray(r, dtype=ty)[:, None] - nodes[None, :]) / DX, d) / DX ** d


def quadrature(grid, xp=True, npts=8):
    """(r, w): the Gauss-Legendre points of every cell and their weights (the cell's length included)"""
    ty = _ty(xp)
    x, w = gauss_legendre(npts, bool(xp))
    nc = grid["nc"]
    DX = (ty(grid["xmax"]) - ty(grid["xmin"])) / nc
    t = (1 + x.astype(ty)) / 2
    r = ty(grid["xmin"]) + (np.arange(nc).astype(ty)[:, None] + t[None, :]) * DX
    return r.reshape(-1), np.tile(w.astype(ty) * DX / 2, nc)


def matrices(grid, xp=True):
    """dense [nb, nb] S, T, M, N, M0 from the definition"""
    r, w = quadrature(grid, xp)
    ph, dph = basis(grid, r, 0, xp), basis(grid, r, 1, xp)
    J = r if grid["has_l"] else np.ones_like(r)
    out = dict(S=dph.T @ ((w * J)[:, None] * dph), M=ph.T @ ((w * J)[:, None] * ph), M0=ph.T @ (w[:, None] * ph),
               N=ph.T @ ((w * r)[:, None] * dph))
    out["T"] = ph.T @ ((w / r)[:, None] * ph) if grid["has_l"] else np.zeros_like(out["S"])
    return out


def gamma(nc, bcl, bcr):
    """[nfree, nb] boundary-condition projection: a = Gamma^T a_free (float64: its entries are small integers and halves)"""
    nb, rl, rr = nc + 3, RANK[bcl], RANK[bcr]
    n = nb - rl - rr
    G = np.zeros((n, nb))
    G[np.arange(n), rl + np.arange(n)] = 1.0
    for q, (w0, w1) in enumerate(ROWS[bcl]):
        G[0, q] += w0
        G[1, q] += w1
    for q, (w0, w1) in enumerate(ROWS[bcr]):
        G[n - 1, nb - 1 - q] += w0
        G[n - 2, nb - 1 - q] += w1
    return G


def dense_solve(K, B, xp=True):
    """K X = B by dense elimination with partial pivoting: numpy's in float64, this loop in longdouble"""
    if not xp:
        return np.linalg.solve(K, B)
    n = len(K)
    W = np.concatenate([K.astype(XP), np.asarray(B, dtype=XP).reshape(n, -1)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(W[c:, c])))
        if p != c:
            W[[c, p]] = W[[p, c]]
        W[c] = W[c] / W[c, c]
        f = W[:, c].copy()
        f[c] = 0
        W -= f[:, None] * W[c][None, :]
    return W[:, n:].reshape(np.shape(B))


def operator(grid, mats, k, alpha, bcl, bcr, xp=True):
    """(Gamma, K_k) of one wavenumber and one boundary-condition class"""
    ty = _ty(xp)
    G = gamma(grid["nc"], bcl, bcr).astype(ty)
    return G, G @ (mats["S"] + ty(k * k) * mats["T"] + ty(alpha) * mats["M"]) @ G.T


def solve_rhs(grid, g, k, alpha, bcl, bcr, xp=True, mats=None):
    """a [nb, ...] = Gamma^T K_k^-1 (-Gamma g) for right-hand side columns g [nb, ...]: the twin of sx_elliptic_check"""
    ty = _ty(xp)
    mats = matrices(grid, xp) if mats is None else mats
    G, K = operator(grid, mats, k, alpha, bcl, bcr, xp)
    return G.T @ dense_solve(K, -(G @ np.asarray(g, dtype=ty)), xp)


def blocks_of(k):
    """reference block indices (Re, Im) of wavenumber k; Im of k = 0 does not exist"""
    return (0, None) if k == 0 else (2 * k - 1, 2 * k)


def invert(grid, kind, a, b, alpha, bcl_k0, bcl, bcr, xp=True):
    """The twin of sx_elliptic_solve: a, b [Zb, K2ref, nb] = the coefficients of the source variable(s) (kind "field": a = f, b
    ignored; "vorticity" / "divergence": a = u, b = v) -> the coefficients of the solution, same shape, in the twin's type."""
    ty = _ty(xp)
    m = matrices(grid, xp)
    a = np.asarray(a, dtype=ty)
    b = None if kind == "field" else np.asarray(b, dtype=ty)
    out = np.zeros(a.shape, dtype=ty)
    NM0 = m["N"] + m["M0"]
    for k in range(grid["kDim"] + 1):
        re, im = blocks_of(k)
        if kind == "field":
            cols = [(re, m["M"] @ a[:, re].T)] + ([(im, m["M"] @ a[:, im].T)] if k else [])
        else:
            p, q, sgn = (b, a, 1) if kind == "vorticity" else (a, b, -1)       # g = (N + M0) p_re/im +- k M0 q_im/re
            if k == 0:
                cols = [(re, NM0 @ p[:, re].T)]
            else:
                cols = [(re, NM0 @ p[:, re].T + ty(sgn * k) * (m["M0"] @ q[:, im].T)),
                        (im, NM0 @ p[:, im].T - ty(sgn * k) * (m["M0"] @ q[:, re].T))]
        for blk, g in cols:             # g [nb, Zb]
            out[:, blk] = solve_rhs(grid, g, k, alpha, bcl_k0 if k == 0 else bcl, bcr, xp, m).T
    return out


def to_blocks(grid, col):
    """one variable's column of Grid.patchSpectral [s_patch] -> [Zb, K2ref, nb]"""
    return np.asarray(col).reshape(grid["Zb"], 2 * grid["kDim"] + 1, grid["nc"] + 3)


def per_k_error(grid, a, truth):
    """[kDim + 1]: per wavenumber, the largest over its columns (z-mode, Re / Im) of max |a - truth| / max |truth| of the column"""
    a, truth = np.asarray(a, dtype=XP), np.asarray(truth, dtype=XP)
    diff, sc = np.abs(a - truth).max(axis=2), np.abs(truth).max(axis=2)            # [Zb, K2ref]
    rel = np.where(sc > 0, diff / np.where(sc > 0, sc, 1), np.where(diff > 0, np.inf, 0)).astype(np.float64)
    return np.array([rel[:, [b for b in blocks_of(k) if b is not None]].max() for k in range(grid["kDim"] + 1)])


def load_vector(grid, f, xp=True):
    """g_i = int J phi_i f dr of a function f(r) by the 8-point rule: what M a_f is for the Galerkin projection a_f of f"""
    r, w = quadrature(grid, xp)
    J = r if grid["has_l"] else np.ones_like(r)
    return basis(grid, r, 0, xp).T @ (w * J * f(r))


def grid_of(gp, kDim):
    """the twin's grid dict of a GridParameters-like object (geometry, xmin, xmax, num_cells, b_zDim) and the patch's kDim"""
    has_z = "Z" in gp.geometry
    return dict(has_l="L" in gp.geometry, xmin=gp.xmin, xmax=gp.xmax, nc=gp.num_cells, kDim=kDim, Zb=gp.b_zDim if has_z else 1)


def field(grid, a, r, lam, xp=True):
    """the function the coefficients a [1, K2ref, nb] stand for at the points (r, lam), every wavenumber summed:
    sum_m phi_m(r) (a[0] + sum_k 2 (a[2k - 1] cos k lam - a[2k] sin k lam))"""
    ty = _ty(xp)
    lam = np.asarray(lam, dtype=ty)
    c = basis(grid, r, 0, xp) @ np.asarray(a, dtype=ty)[0].T            # [points, K2ref]
    out = c[:, 0].copy()
    for k in range(1, grid["kDim"] + 1):
        out += 2 * (c[:, 2 * k - 1] * np.cos(k * lam) - c[:, 2 * k] * np.sin(k * lam))
    return out
