"""TEST INFRASTRUCTURE - the numpy twin of sx_isosurface / sx_column_series (include/scythe_hip.h), in float64 (xp=False)
or numpy.longdouble (xp=True, the arbiter).

The column profiles come from their definition - dense sums over (block, node) with the weight functions of tests/evaluate.py, never
from the library.  CA and Dc are the oracle's extended-precision factors; the series at a height is written from the header's
statement: in float64 operation for operation (the recurrence, no fused multiply-add), so that it is bitwise sx_column_series; in
longdouble as c_n cos(n acos x), which does not share the recurrence's error.  Stations, the sign rule, the scan and the selection
are the header's; the bracket step is tests/crossings.py's Bracket.

Rounding bounds, u = 2^-53.
ONE profile entry (profile_bound), C[zm] = sum_{blk, node} a phi F, S = sum |a phi F|:
  the sum     the product phi F (1 rounding), the multiply-add of the matrix unit (1), the accumulation 4 K2 deep:     u (4 K2 + 2) S
  F           as tests/crossings.py: |lambda| <= 2 pi, sincos 1 ulp, the factors 2, k, k^2:          sum |a phi| 2 k^sl u (2 k pi + 4)
  phi         delta = (r - x_node) / DX is off by u (2 R / DX + 6), R = max(|xmin|, |xmax|) (the node position 2 roundings of
              size R, the difference and the quotient); phi^(d) has the Lipschitz constants 1, 2, 3 and its polynomial and the
              division by DX^d add at most 20 u:                       sum |a F| u (L_d (2 R / DX + 6) + 20) / DX^d
ONE series value (series_bound), s = sum_n a_n c_n T_n(x):
  T_n         the recurrence's local error is 3 u per step and is carried by U_{n-1-j}, |U_m| <= m + 1:              1.5 n^2 u
  x           mid, half, the difference and the quotient: u (|mid| / half + 3), times |T_n'| <= n^2
  the sum     one product and zDim additions:                                                                    (zDim + 1) u
  together    u sum_n c_n |a_n| (n^2 (4.5 + |mid| / half) + zDim + 1), with 1 % for the second-order terms.
A series whose coefficients carry an error da adds sum_n c_n da_n; Dc a in float64 adds u (zDim + 2) |Dc| |a| per application
(coeff_bound)."""
import collections

import numpy as np

from oracle import oracle_np as O
from tests import crossings as X
from tests import evaluate as E
from tests import parcels as PA

XP = O.XP
EPS = 2.0 ** -53
# slot -> profile kind (sr, sl) = (0, 0) (1, 0) (2, 0) (0, 1) (0, 2), z order
KIND = {"": (0, 0), "r": (1, 0), "rr": (2, 0), "l": (3, 0), "ll": (4, 0), "z": (0, 1), "zz": (0, 2)}
ORDERS = ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2))

_ty = X._ty

Plan = collections.namedtuple("Plan", "planes keys pprof pz")


def plan(g, packed):
    """The planes (var, slot index) of a packed program in first-use order (all outputs, term by term), the profile keys
    (var, kind) in first-use order, and per plane its profile number and z order"""
    planes, keys, pprof, pz = [], [], [], []
    for t in range(len(packed)):
        for f in range(int(packed[t, 2])):
            pl = (int(packed[t, 3 + f]), int(packed[t, 7 + f]))
            if pl in planes:
                continue
            planes.append(pl)
            name = g.slots[pl[1]] if g.slots[pl[1]] != "u" else ""
            kind, zo = KIND[name]
            key = (pl[0], kind)
            if key not in keys:
                keys.append(key)
            pprof.append(keys.index(key))
            pz.append(zo)
    return Plan(planes, keys, pprof, pz)


def reduce_columns(g, columns):
    """[n, n_coord - 1] float64 with lambda as the device takes it: as given within [-2 pi, 2 pi], else reduced into (-pi, pi]"""
    q = np.array(columns, dtype=np.float64).reshape(-1, 1 + int(g.has_l))
    if g.has_l:
        big = np.abs(q[:, 1]) > 6.283185307179586
        q[big, 1] = PA.reduce_lambda(q[big, 1])
    return q


# ----------------------------------------------------------------------------- the profiles
def _weights(g, kind, col, xp):
    sr, sl = ORDERS[kind]
    cell = E.node0_of(g, col[0])
    phi = E.radial_weights(g, col[0], cell, xp)[sr]
    F = E.fourier_weights(g.kDim, col[1], xp)[sl] if g.has_l else np.ones(1, dtype=_ty(xp))
    return cell, phi, F


def profiles(g, A, pl, cols, xp=True):
    """C [b_zDim, n_profiles, n_cols] in the twin's type from A [S_patch, V] (reference layout) and columns as reduce_columns gives them"""
    T = _ty(xp)
    out = np.zeros((g.b_zDim, len(pl.keys), len(cols)), dtype=T)
    for p, (var, kind) in enumerate(pl.keys):
        a = A[:, var - 1].reshape(g.b_zDim, g.K2, g.b_rDim).astype(T)
        for q, col in enumerate(cols):
            cell, phi, F = _weights(g, kind, col, xp)
            out[:, p, q] = np.einsum("zbm,b,m->z", a[:, :, cell:cell + 4], F, phi)
    return out


def profile_bound(g, A, pl, cols):
    """[b_zDim, n_profiles, n_cols] float64: the rounding bound of the module docstring"""
    out = np.zeros((g.b_zDim, len(pl.keys), len(cols)))
    kk = np.concatenate([[0], np.repeat(np.arange(1, g.kDim + 1), 2)]).astype(np.float64) if g.has_l else np.zeros(1)
    R = max(abs(g.xmin), abs(g.xmax))
    for p, (var, kind) in enumerate(pl.keys):
        sr, sl = ORDERS[kind]
        aa = np.abs(A[:, var - 1].reshape(g.b_zDim, g.K2, g.b_rDim))
        d_F = 2.0 * kk ** sl * EPS * (2.0 * kk * np.pi + 4.0) if g.has_l else np.zeros(1)
        d_phi = np.full(4, EPS * ((1.0, 2.0, 3.0)[sr] * (2.0 * R / g.DX + 6.0) + 20.0) / g.DX ** sr)
        for q, col in enumerate(cols):
            cell, phi, F = _weights(g, kind, col, False)
            a4, ff, pp = aa[:, :, cell:cell + 4], np.abs(F), np.abs(phi)
            S = np.einsum("zbm,b,m->z", a4, ff, pp)
            out[:, p, q] = EPS * (4.0 * g.K2 + 2.0) * S + np.einsum("zbm,b,m->z", a4, d_F, pp) + np.einsum("zbm,b,m->z", a4, ff, d_phi)
    return out


# ----------------------------------------------------------------------------- CA, Dc and the series at a height
def operators(g, v, xp=True):
    """(CA [zDim, b_zDim], Dc [zDim, zDim]) of variable v (a name): the oracle's extended-precision factors, rounded once for float64"""
    x = g.cheb(v)._x
    T = _ty(xp)
    return np.asarray(x["CA"], dtype=T), np.asarray(x["Dc"], dtype=T)


def dc_of(zDim, zmin, zmax, xp=True):
    """Dc alone, from the vertical grid (the header's recurrence ax_{k-1} = ax_{k+1} + k c_k, scaled by -2 / Lz) in longdouble"""
    Dc = np.zeros((zDim, zDim), dtype=XP)
    for j in range(zDim):
        ax = np.zeros(zDim + 2, dtype=XP)
        for k in range(zDim - 1, 0, -1):
            ck = (XP(1) if k == zDim - 1 else XP(2)) if k == j else XP(0)
            ax[k - 1] = ax[k + 1] + k * ck
        Dc[:, j] = ax[:zDim] * (XP(-2) / (XP(zmax) - XP(zmin)))
    return Dc.astype(_ty(xp))


def apply_dc(Dc, a, xp):
    """Dc a: float64 in the library's order (every entry summed over m ascending from +0.0, product then sum)"""
    if xp:
        return Dc @ a
    acc = np.zeros(len(a))
    for m in range(len(a)):
        acc = acc + Dc[:, m] * a[m]
    return acc


def expand(CA, C, xp):
    """a = CA C in the library's order"""
    if xp:
        return CA @ C.astype(XP)
    acc = np.zeros(CA.shape[0])
    for zm in range(CA.shape[1]):
        acc = acc + CA[:, zm] * C[zm]
    return acc


def series(zmin, zmax, a, z, xp=True):
    """sum_n a_n t_n(x) at height z.  float64: sx_column_series operation for operation; longdouble: c_n cos(n acos x)"""
    N = len(a)
    if xp:
        mid, half = (XP(zmin) + XP(zmax)) / XP(2), (XP(zmax) - XP(zmin)) / XP(2)
        x = min(max((XP(z) - mid) / (-half), XP(-1)), XP(1))
        c = np.full(N, 2, dtype=XP)
        c[0] = c[-1] = 1
        return np.sum(np.asarray(a, dtype=XP) * c * np.cos(np.arange(N).astype(XP) * np.arccos(x)))
    f = np.float64
    mid, half = (f(zmin) + f(zmax)) / f(2.0), (f(zmax) - f(zmin)) / f(2.0)
    with np.errstate(all="ignore"):
        x = min(max((f(z) - mid) / (-half), f(-1.0)), f(1.0))
        x2 = f(2.0) * x
        tm, t, s = f(1.0), x, f(a[0])
        for n in range(1, N):
            s = s + f(a[n]) * (t if n == N - 1 else f(2.0) * t)
            tm, t = t, x2 * t - tm
    return s


def series_bound(zmin, zmax, a_abs, da=None):
    """the rounding bound of one series value with |a| = a_abs (any z), plus sum c_n da_n for coefficients that carry an error da"""
    N = len(a_abs)
    n = np.arange(N, dtype=np.float64)
    c = np.where((n == 0) | (n == N - 1), 1.0, 2.0)
    mid, half = 0.5 * (zmin + zmax), 0.5 * (zmax - zmin)
    b = 1.01 * EPS * float(np.sum(c * np.asarray(a_abs, dtype=np.float64) * (n * n * (4.5 + abs(mid) / half) + N + 1.0)))
    return b + (float(np.sum(c * da)) if da is not None else 0.0)


def coeff_bound(Dc_abs, a_abs, da):
    """(|a'| bound, da') of a' = Dc a formed in float64 from coefficients |a| <= a_abs that carry an error da"""
    N = len(a_abs)
    a1 = Dc_abs @ (a_abs + da)
    return a1, Dc_abs @ da + EPS * (N + 2.0) * (Dc_abs @ a_abs)


# ----------------------------------------------------------------------------- the program in a column
def column_series_set(g, C, pl, xp=True):
    """per plane the coefficients of its series: a = CA C, a' = Dc a, a'' = Dc a' of the plane's profile C[:, prof]"""
    out, cache = [], {}
    for j, (var, _) in enumerate(pl.planes):
        key = (pl.pprof[j], pl.pz[j])
        if key not in cache:
            CA, Dc = operators(g, g.names[var - 1], xp)
            a = expand(CA, np.asarray(C[:, pl.pprof[j]], dtype=_ty(xp)), xp)
            for _ in range(pl.pz[j]):
                a = apply_dc(Dc, a, xp)
            cache[key] = a
        out.append(cache[key])
    return out


def value(g, ser, pl, program, r, z, out=0, xp=True):
    """output `out` of the program at height z of a column at radius r, in the twin's type: the planes from their series, then the
    terms of that output in term order from +0.0"""
    T = _ty(xp)
    coef, packed, _ = program
    val = [series(g.zmin, g.zmax, a, z, xp) for a in ser]
    rT = T(float(r))
    rr = rT * rT
    q = T(0)
    with np.errstate(all="ignore"):
        for t in range(len(coef)):
            if int(packed[t, 0]) != out:
                continue
            p, nf = int(packed[t, 1]), int(packed[t, 2])
            x = T(coef[t])
            if p != 0:
                x = x * (rT if p == 1 else rr if p == 2 else T(1) / rT if p == -1 else T(1) / rr)
            for f in range(nf):
                x = x * val[pl.planes.index((int(packed[t, 3 + f]), int(packed[t, 7 + f])))]
            q = q + x
    return q


# ----------------------------------------------------------------------------- scan and refine
Result = collections.namedtuple("Result", "height dir count status carry values")


def stations(g, heights=None):
    """the zDim levels, bottom to top (default: the oracle's; the tests pass the doubles the gridpoints print)"""
    return np.asarray(g.cheb(g.names[0]).z if heights is None else heights, dtype=np.float64)


def scan_column(g, fn, levels, n_carry=0, tol=1e-9, max_iter=60, max_cross=4, xp=True, heights=None):
    """What sx_isosurface returns for ONE column whose output o at height z is fn(z, o) (type T): height [max_cross, n_levels] as
    float64 (a longdouble root is rounded once), dir, count [n_levels], status, carry [n_carry, max_cross, n_levels] in type T,
    values [zDim] in type T"""
    T = _ty(xp)
    st = stations(g, heights)
    gv = [fn(z, 0) for z in st]
    nl = len(levels)
    height, dirs = np.full((max_cross, nl), np.nan), np.zeros((max_cross, nl), dtype=np.int32)
    carry = np.full((n_carry, max_cross, nl), np.nan, dtype=T)
    count, status = np.zeros(nl, dtype=np.int32), 0
    wtol = T(tol) * (T(g.zmax) - T(g.zmin))
    for j, c in enumerate(levels):
        d = [v - T(c) for v in gv]
        for i in range(len(st) - 1):
            d0, d1 = d[i], d[i + 1]
            if d0 != d0 or d1 != d1:
                status |= 1
                continue
            if (d0 < 0) == (d1 < 0):
                continue
            pos = int(count[j])
            count[j] += 1
            if pos >= max_cross:
                continue
            B = X.Bracket(st[i], d0, st[i + 1], d1, T)
            s = B.start(wtol)
            it = 0
            while s < 0 and it < max_iter:
                s = B.step(fn(B.x, 0) - T(c), wtol)
                it += 1
            if s != 0:
                status |= 2 if s < 0 else 4
            height[pos, j] = float(B.root())
            dirs[pos, j] = 1 if d0 < 0 else -1
            for o in range(n_carry):
                carry[o, pos, j] = fn(height[pos, j] if not xp else B.root(), 1 + o)
    return Result(height, dirs, count, status, carry, np.array(gv, dtype=T))


def isosurface(g, A, program, levels, columns, n_carry=0, tol=1e-9, max_iter=60, max_cross=4, xp=True, heights=None, C=None):
    """The call as Grid.isosurface returns it: Result(height [max_cross, n_levels, n_cols], dir, count [n_levels, n_cols], status
    [n_cols], carry [n_carry, max_cross, n_levels, n_cols], values [zDim, n_cols]); C: profiles to use instead of the twin's own"""
    pl = plan(g, program[1])
    q = reduce_columns(g, columns)
    Cq = profiles(g, A, pl, q, xp) if C is None else C
    out = []
    for i in range(len(q)):
        ser = column_series_set(g, Cq[:, :, i], pl, xp)
        out.append(scan_column(g, lambda z, o, ser=ser, i=i: value(g, ser, pl, program, q[i, 0], z, o, xp), levels, n_carry, tol,
                               max_iter, max_cross, xp, heights))
    return Result(np.stack([o.height for o in out], axis=2), np.stack([o.dir for o in out], axis=2),
                  np.stack([o.count for o in out], axis=1), np.array([o.status for o in out], dtype=np.int32),
                  np.stack([o.carry for o in out], axis=3), np.stack([o.values for o in out], axis=1))


# ----------------------------------------------------------------------------- the selection
def select(res, level=0, which="lowest", rising=None):
    """[n_cols]: the lowest / highest kept crossing of a level per column (rising: among dir == +1, False: -1), NaN without one"""
    hgt, dr = res.height[:, level, :], res.dir[:, level, :]
    ok = ~np.isnan(hgt) & (True if rising is None else dr == (1 if rising else -1))
    out = np.full(hgt.shape[1], np.nan)
    for q in range(hgt.shape[1]):
        h = hgt[ok[:, q], q]
        if len(h):
            out[q] = h[0] if which == "lowest" else h[-1]
    return out


def project(g, values):
    """A [S_patch, V] of one-tile physical values through the oracle's forward and spline transforms"""
    return g.spline_transform(g.forward(values))
