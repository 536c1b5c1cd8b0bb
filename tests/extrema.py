"""TEST INFRASTRUCTURE - the numpy twin of sx_extrema / sx_extremum_refine / sx_newton_step (include/scythe_hip.h), in
float64 or numpy.longdouble (the arbiter).

The scan is plain np.min / argmin over the program evaluated pointwise (tests/reduce.py's term_values), with the tie and NaN rules of
the header.  The ten derivatives of order <= 2 come from tests/evaluate.py's weight functions extended by the mixed products; the
Newton step is written from the header's statement, in whichever type its arguments have.

Rounding bound of ONE derivative d = d_r^a d_l^b d_z^c u (deriv_bound), in the manner of tests/parcels.py's velocity bound:
    d = sum_col (sum_j phi^(a)_j a[j, col]) F^(b)_blk(col) w^(c)_zm(col),      S = sum |a phi^(a) F^(b) w^(c)|,     eps = 2^-53
  the sums       4-node dot product (4 roundings), the products F w and s (F w) (2), the factors k, k^2 and 1 / DX^a (3), and the
                 accumulation, at most ncol = b_zDim K2 deep:                                          eps (ncol + 9) S
  phi^(a)        delta is off by eps (2 X + 6), X = max(|xmin|, |xmax|) / DX, and |phi^(a + 1)| <= M = (1, 2, 3) in cardinal units; the
                 piecewise polynomial itself by 16 eps: an ABSOLUTE error (eps ((2 X + 6) M + 16)) / DX^a of every weight:
                                                                                                       d_phi sum |a| |F^(b)| |w^(c)|
  F^(b)          k lambda is off by k pi eps (lambda in (-pi, pi]), sincos 1 ulp, the factors 2 and k^b:  sum |a phi w| 2 k^b eps (k pi + 4)
  w^(c)          w = sum_n t_n W_c[n, zm], t_n = c_n cos(n acos x), W_c = Dc^c CA rounded once: x is off by 4 eps, |T_n'| <= n^2, the
                 product n theta by n pi eps, cos 1 ulp, the rounding of W, a sum zDim deep:
                                                       d_w[zm] = eps sum_n c_n |W_c[n, zm]| (4 n^2 + n pi + 3 + zDim),   sum |a phi F| d_w
The bound is the sum of the four parts.

Rounding bound of a scanned value (SCAN): output o at a point is the float64 sum of nt terms coef r^p prod field; a term passes through
at most 3 roundings for coef r^p (r r, 1 / (r r), the product), 4 for the factors, and the sum adds one per term:
    |q - truth| <= (8 + nt) eps sum |term|."""
import collections
import math

import numpy as np

from oracle import oracle_np as O
from tests import evaluate as E
from tests import reduce as R

XP = O.XP
EPS = 2.0 ** -53
NAMES = ("u", "r", "l", "z", "rr", "rl", "rz", "ll", "lz", "zz")
ORDERS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2))
FREE_R, FREE_L, FREE_Z = 1, 2, 4


def _ty(xp):
    return XP if xp else np.float64


# ----------------------------------------------------------------------------- the scan
def integrand(data, r, program):
    """(q [n_out, N], S_abs [n_out, N], nt [n_out]) in longdouble: every output of the program at every point, the sum of its absolute
    terms, and its term count; data [N, V, D] or [N, V], r [N]"""
    coef, packed, n_out = program
    tv = R.term_values(data, r, coef, packed)
    q, s = np.zeros((n_out, tv.shape[1]), dtype=XP), np.zeros((n_out, tv.shape[1]), dtype=XP)
    nt = np.zeros(n_out, dtype=int)
    for t in range(len(coef)):
        o = int(packed[t, 0])
        q[o] += tv[t]
        s[o] += np.abs(tv[t])
        nt[o] += 1
    return q, s, nt


def _pick(q, rows, sign):
    """(value, row) of the minimum (sign < 0) or maximum of q [n] whose points are `rows`: the lowest row among equals (numpy's argmin
    returns the first, and -0.0 == +0.0), and the lowest NaN row if there is a NaN"""
    nan = np.isnan(q)
    j = int(np.argmax(nan)) if nan.any() else int(np.argmin(q) if sign < 0 else np.argmax(q))
    return q[j], int(rows[j])


def scan(q, L, nz, kind="domain"):
    """What sx_extrema returns for the pointwise outputs q [n_out, N] (any float type) of a tile with ring lengths L and nz levels:
    (val, idx) [2, n_out] or [2, rings, nz, n_out]"""
    q = np.asarray(q)
    n_out, N = q.shape
    L = np.asarray(L)
    start = np.concatenate([[0], np.cumsum(L * nz)])
    assert start[-1] == N
    rows = np.arange(N)
    if kind == "domain":
        val, idx = np.zeros((2, n_out), dtype=q.dtype), np.zeros((2, n_out), dtype=np.int64)
        for o in range(n_out):
            for w, sign in ((0, -1), (1, +1)):
                val[w, o], idx[w, o] = _pick(q[o], rows, sign)
        return val, idx
    val, idx = np.zeros((2, len(L), nz, n_out), dtype=q.dtype), np.zeros((2, len(L), nz, n_out), dtype=np.int64)
    for o in range(n_out):
        for i in range(len(L)):
            blk, rw = q[o, start[i]:start[i + 1]].reshape(int(L[i]), nz), rows[start[i]:start[i + 1]].reshape(int(L[i]), nz)
            for z in range(nz):
                for w, sign in ((0, -1), (1, +1)):
                    val[w, i, z, o], idx[w, i, z, o] = _pick(blk[:, z], rw[:, z], sign)
    return val, idx


def scan_bound(s_abs, nt):
    """[n_out, N]: the bound of the module docstring on a scanned value"""
    return (8.0 + np.asarray(nt, dtype=np.float64))[:, None] * EPS * np.asarray(s_abs, dtype=np.float64)


# ----------------------------------------------------------------------------- the ten derivatives at a point
def derivatives(g, A, var, point, xp=True, with_bound=False):
    """d [10] = u, u_r, u_l, u_z, u_rr, u_rl, u_rz, u_ll, u_lz, u_zz of variable var (1-based) at point (r[, lambda][, z]) with every
    wavenumber of the patch (SX_EVAL_ALL_K); with_bound: (d, S [10], bound [10]) as the module docstring derives them"""
    T = _ty(xp)
    p = np.atleast_1d(np.asarray(point, dtype=np.float64))
    r = float(p[0])
    name = g.names[var - 1]
    n0 = E.node0_of(g, r)
    PH = E.radial_weights(g, r, n0, xp)                                                  # [3, 4]
    F = E.fourier_weights(g.kDim, p[1], xp) if g.has_l else np.array([[1], [0], [0]], dtype=T)      # [3, nb]
    W = E.vertical_weights(g, name, p[-1], xp) if g.has_z else np.array([[1], [0], [0]], dtype=T)    # [3, Zb]
    nb = F.shape[1]
    a = A[:, var - 1].reshape(g.b_zDim, g.K2, g.b_rDim)[:, :nb, n0:n0 + 4].astype(T)      # [zm, blk, node]
    d, S, B = np.zeros(10, dtype=T), np.zeros(10), np.zeros(10)
    if with_bound:
        aa = np.abs(a).astype(np.float64)
        kk = np.concatenate([[0], np.repeat(np.arange(1, g.kDim + 1), 2)]).astype(np.float64) if g.has_l else np.zeros(1)
        X = max(abs(g.xmin), abs(g.xmax)) / g.DX
        ncol = g.b_zDim * g.K2
        if g.has_z:
            x = g.cheb(name)._x
            CA, Dc = np.asarray(x["CA"], dtype=XP), np.asarray(x["Dc"], dtype=XP)
            Wc = [np.abs(np.asarray(m, dtype=np.float64)) for m in (CA, Dc @ CA, Dc @ Dc @ CA)]
            n = np.arange(g.zDim)
            cn = np.where((n == 0) | (n == g.zDim - 1), 1.0, 2.0)
    for m, (da, db, dc) in enumerate(ORDERS):
        if (db and not g.has_l) or (dc and not g.has_z):
            continue
        terms = a * PH[da][None, None, :] * F[db][None, :, None] * W[dc][:, None, None]
        d[m] = terms.sum()
        if with_bound:
            S[m] = float(np.abs(terms).sum())
            fp, ff, ww = np.abs(PH[da]).astype(np.float64), np.abs(F[db]).astype(np.float64), np.abs(W[dc]).astype(np.float64)
            d_phi = EPS * ((2.0 * X + 6.0) * (1.0, 2.0, 3.0)[da] + 16.0) / g.DX ** da
            d_F = 2.0 * kk ** db * EPS * (kk * np.pi + 4.0)
            d_w = EPS * ((cn * (4.0 * n * n + n * np.pi + 3.0 + g.zDim)) @ Wc[dc]) if g.has_z else np.zeros(1)
            B[m] = (EPS * (ncol + 9.0) * S[m] + d_phi * np.einsum("zbn,b,z->", aa, ff, ww) + np.einsum("zbn,n,b,z->", aa, fp, d_F, ww)
                    + np.einsum("zbn,n,b,z->", aa, fp, ff, d_w))
    return (d, S, B) if with_bound else d


# ----------------------------------------------------------------------------- the Newton step
def _fn(T):
    """sin, cos, hypot, atan2, rint in the type of the step: the C library's for float64 (what the host helper calls), numpy's for longdouble"""
    if T is np.float64:
        return (lambda x: np.float64(math.sin(x)), lambda x: np.float64(math.cos(x)), lambda x, y: np.float64(math.hypot(x, y)),
                lambda y, x: np.float64(math.atan2(y, x)), lambda x: np.float64(round(float(x))))
    return np.sin, np.cos, np.hypot, np.arctan2, np.rint


def cartesian(d, r, lam, T=XP):
    """gradient [3] and Hessian [3, 3] in (X, Y, z) from the native derivatives d [10], by the chain rule as the header writes it"""
    sin, cos, _, _, _ = _fn(T)
    u, ur, ul, uz, urr, url, urz, ull, ulz, uzz = [T(x) for x in d]
    r = T(r)
    s, c = sin(T(lam)), cos(T(lam))
    ri = T(1) / r
    a = (url * ri) - (ul * ri) * ri
    b = (ur * ri) + (ull * ri) * ri
    g = np.array([(ur * c) - ((ul * ri) * s), (ur * s) + ((ul * ri) * c), uz], dtype=T)
    H = np.zeros((3, 3), dtype=T)
    H[0, 0] = ((c * c) * urr - (T(2) * (s * c)) * a) + (s * s) * b
    H[1, 1] = ((s * s) * urr + (T(2) * (s * c)) * a) + (c * c) * b
    H[0, 1] = H[1, 0] = (s * c) * (urr - b) + ((c * c) - (s * s)) * a
    H[0, 2] = H[2, 0] = (urz * c) - ((ulz * ri) * s)
    H[1, 2] = H[2, 1] = (urz * s) + ((ulz * ri) * c)
    H[2, 2] = uzz
    return g, H


def newton_step(g, want, mask, tol, pos, d, T=XP, info=None):
    """(new_pos [n_coord], status) as sx_newton_step states it, in type T; want -1 / 0 / 1, mask of FREE_* bits, pos (r[, lambda][, z]),
    d [10].  info (a dict): receives the step vector, its horizontal and vertical length, the cap factor, the reduced Hessian."""
    sin, cos, hypot, atan2, rint = _fn(T)
    pos = np.atleast_1d(pos)
    r, lam, z = T(pos[0]), T(pos[1]) if g.has_l else T(0), T(pos[-1]) if g.has_z else T(0)
    DX = T(g.DX)

    def out(rn, ln, zn, st):
        q = [rn] + ([ln] if g.has_l else []) + ([zn] if g.has_z else [])
        return np.array(q, dtype=T), st
    fr, fl, fz = bool(mask & 1), bool(mask & 2), bool(mask & 4)
    cart = fr and fl
    if mask == 0:
        return out(r, lam, z, 0)
    pole = g.has_l and g.xmin == 0.0
    if cart and pole and r < T(1e-6) * DX:
        return out(r, lam, z, 3)
    dd = [T(x) for x in d]
    grad = np.array([dd[1], dd[2], dd[3]], dtype=T)
    H = np.array([[dd[4], dd[5], dd[6]], [dd[5], dd[7], dd[8]], [dd[6], dd[8], dd[9]]], dtype=T)
    c, s = T(1), T(0)
    if cart:
        s, c = sin(lam), cos(lam)
        grad, H = cartesian(d, r, lam, T)
    act = [i for i, f in enumerate((fr, fl, fz)) if f]
    n = len(act)
    M = H[np.ix_(act, act)]
    b = -grad[act]
    D, Lm = np.zeros(n, dtype=T), np.zeros((n, n), dtype=T)
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = M[j, j]
            for k in range(j):
                dj = dj - (Lm[j, k] * Lm[j, k]) * D[k]
            D[j] = dj
            ok = dj < 0 if want > 0 else dj > 0 if want < 0 else (dj < 0 or dj > 0)
            if not ok or not np.isfinite(dj):
                return out(r, lam, z, 4)
            for i in range(j + 1, n):
                x = M[i, j]
                for k in range(j):
                    x = x - (Lm[i, k] * Lm[j, k]) * D[k]
                Lm[i, j] = x / dj
        y, st = np.zeros(n, dtype=T), np.zeros(3, dtype=T)
        for i in range(n):
            x = b[i]
            for k in range(i):
                x = x - Lm[i, k] * y[k]
            y[i] = x
        for i in range(n - 1, -1, -1):
            x = y[i] / D[i]
            for k in range(i + 1, n):
                x = x - Lm[k, i] * st[act[k]]
            st[act[i]] = x
        zlen = T(g.zmax) - T(g.zmin) if g.has_z else T(0)
        hl = hypot(st[0], st[1]) if cart else abs(st[0]) if fr else abs(r * st[1]) if fl else T(0)
        vl = abs(st[2]) if fz else T(0)
        f = T(1)
        if hl > DX:
            f = DX / hl
        if fz and vl > zlen / T(8):
            f = min(f, (zlen / T(8)) / vl)
        if not (f >= 0 and f <= 1):
            return out(r, lam, z, 4)
        if f != 1:
            st, hl, vl = st * f, hl * f, vl * f
        if info is not None:
            info.update(step=st.copy(), hl=hl, vl=vl, f=f, M=M.copy(), grad=grad.copy())
        rn, ln, zn = r, lam, z
        if cart:
            X, Y = (r * c) + st[0], (r * s) + st[1]
            rn = hypot(X, Y)
            ln = T(0) if rn == 0 else atan2(Y, X)
            if ln <= -T(np.pi):
                ln = T(np.pi)
        elif fr:
            rn = r + st[0]
        elif fl:
            ln = lam + st[1]
            ln = ln - T(6.283185307179586) * rint(ln / T(6.283185307179586))
            if ln <= -T(np.pi) or ln > T(np.pi):
                ln = T(np.pi)
        if fz:
            zn = z + st[2]
        if not (rn >= g.xmin and rn <= g.xmax):
            return out(r, lam, z, 1)
        if fz and not (zn >= g.zmin and zn <= g.zmax):
            return out(r, lam, z, 2)
        return out(rn, ln, zn, 0 if (hl <= T(tol) * DX and vl <= T(tol) * zlen) else -1)


Result = collections.namedtuple("Result", "pos value grad status iters d")


def refine(g, A, var, start, want=1, mask=None, tol=1e-9, max_iter=20, xp=True):
    """The iteration of sx_extremum_refine for ONE start point with the arithmetic in type T: evaluate, step, ... and one more
    evaluation at the final position.  As on the device the position is a float64 between the steps (the coordinates are float64
    in the interface), so the longdouble twin differs from exact Newton only by that rounding, 2^-53 of a coordinate per step."""
    T = _ty(xp)
    if mask is None:
        mask = FREE_R | (FREE_L if g.has_l else 0) | (FREE_Z if g.has_z else 0)
    from tests import parcels as P
    pos = np.array(np.atleast_1d(start), dtype=np.float64)
    if g.has_l and abs(pos[1]) > 6.283185307179586:
        pos[1] = P.reduce_lambda(pos[1])
    steps, status = 0, 0
    while True:
        d = derivatives(g, A, var, pos, xp)
        new, st = newton_step(g, want, mask, tol, pos, d, T)
        if st == 0 and mask == 0:
            break
        if st <= 0:
            pos = np.asarray(new, dtype=np.float64)
            steps += 1
            status = 0 if st == 0 else 5
            if st == 0 or steps >= max_iter:
                d = derivatives(g, A, var, pos, xp)
                break
        else:
            status = st
            break
    grad = [d[1]] + ([d[2]] if g.has_l else []) + ([d[3]] if g.has_z else [])
    return Result(pos, d[0], np.array(grad, dtype=T), status, steps, d)
