"""TEST INFRASTRUCTURE - the numpy twin of sx_crossings / sx_bracket_step (include/scythe_hip.h), in float64 (xp=False)
or numpy.longdouble (xp=True, the arbiter).

The profiles come from their definition - dense sums over (z-mode, block) with the weight functions of tests/evaluate.py (its own
cos / sin k lambda and Chebyshev rows, in the twin's type), never from the library.  Stations, the sign rule, the bracket step and the
selection rules are written from the header's statement; the bracket step uses the operations of the library's function one for one,
so that in float64 it is bitwise the host helper.

Rounding bound of ONE profile entry (profile_bound), in the manner of tests/parcels.py's velocity bound:
    P[m] = sum_col a[m, col] F_blk(col) w_zm(col),      S = sum |a F w|,     eps = 2^-53
  the sum        the product F w (1 rounding), the multiply-add of the matrix unit (1) and the accumulation, ncol = b_zDim K2 deep:
                                                                                                       eps (ncol + 2) S
  F              |lambda| <= 2 pi, so k lambda is off by at most 2 k pi eps; sincos 1 ulp, the factors 2, k, k^2 (3):
                                                                                                       sum |a w| 2 k^b eps (2 k pi + 4)
  w              as tests/extrema.py derives it:  d_w[zm] = eps sum_n c_n |W_c[n, zm]| (4 n^2 + n pi + 3 + zDim),    sum |a F| d_w
The bound is the sum of the three parts."""
import collections

import numpy as np

from oracle import oracle_np as O
from tests import evaluate as E
from tests import parcels as PA

XP = O.XP
EPS = 2.0 ** -53
KIND = {"": 0, "r": 0, "rr": 0, "l": 1, "ll": 2, "z": 3, "zz": 4}      # profile kind of a slot: (lambda order, z order) = (0, 0) (1, 0) (2, 0) (0, 1) (0, 2)
RORD = {"": 0, "r": 1, "rr": 2}                                        # radial order of a slot
ORDERS = ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2))


def _ty(xp):
    return XP if xp else np.float64


Plan = collections.namedtuple("Plan", "planes keys pprof pd")


def plan(g, packed):
    """The planes (var, slot index) of a packed program in first-use order, the profile keys (var, kind) in first-use order, and per
    plane its profile number and radial order"""
    planes, keys, pprof, pd = [], [], [], []
    for t in range(len(packed)):
        for f in range(int(packed[t, 2])):
            pl = (int(packed[t, 3 + f]), int(packed[t, 7 + f]))
            if pl in planes:
                continue
            planes.append(pl)
            name = g.slots[pl[1]] if g.slots[pl[1]] != "u" else ""
            key = (pl[0], KIND[name])
            if key not in keys:
                keys.append(key)
            pprof.append(keys.index(key))
            pd.append(RORD.get(name, 0))
    return Plan(planes, keys, pprof, pd)


def reduce_rays(g, rays, n=None):
    """[n, n_coord - 1] float64 with lambda as the device takes it: as given within [-2 pi, 2 pi], else reduced into (-pi, pi]"""
    nrc = int(g.has_l) + int(g.has_z)
    if nrc == 0:
        return np.zeros((1 if rays is None else int(rays) if np.ndim(rays) == 0 else len(rays), 0))
    q = np.array(rays, dtype=np.float64).reshape(-1, nrc)
    if g.has_l:
        big = np.abs(q[:, 0]) > 6.283185307179586
        q[big, 0] = PA.reduce_lambda(q[big, 0])
    return q


def _weights(g, key, ray, xp):
    T = _ty(xp)
    var, kind = key
    sl, sz = ORDERS[kind]
    F = E.fourier_weights(g.kDim, ray[0], xp)[sl] if g.has_l else np.ones(1, dtype=T)
    W = E.vertical_weights(g, g.names[var - 1], ray[-1], xp)[sz] if g.has_z else np.ones(1, dtype=T)
    return F, W


def profiles(g, A, pl, rays, xp=True):
    """P [b_rDim, n_profiles, n_rays] in the twin's type from A [S_patch, V] (reference layout) and rays as reduce_rays gives them"""
    T = _ty(xp)
    out = np.zeros((g.b_rDim, len(pl.keys), len(rays)), dtype=T)
    for p, key in enumerate(pl.keys):
        a = A[:, key[0] - 1].reshape(g.b_zDim, g.K2, g.b_rDim).astype(T)
        for q, ray in enumerate(rays):
            F, W = _weights(g, key, ray, xp)
            out[:, p, q] = np.einsum("zbm,b,z->m", a, F, W)
    return out


def profile_bound(g, A, pl, rays):
    """[b_rDim, n_profiles, n_rays] float64: the rounding bound of the module docstring"""
    out = np.zeros((g.b_rDim, len(pl.keys), len(rays)))
    kk = np.concatenate([[0], np.repeat(np.arange(1, g.kDim + 1), 2)]).astype(np.float64) if g.has_l else np.zeros(1)
    ncol = g.b_zDim * (g.K2 + 1 if g.has_l else 1)
    n = np.arange(g.zDim)
    cn = np.where((n == 0) | (n == g.zDim - 1), 1.0, 2.0)
    for p, key in enumerate(pl.keys):
        sl, sz = ORDERS[key[1]]
        aa = np.abs(A[:, key[0] - 1].reshape(g.b_zDim, g.K2, g.b_rDim))
        if g.has_z:
            x = g.cheb(g.names[key[0] - 1])._x
            CA, Dc = np.asarray(x["CA"], dtype=XP), np.asarray(x["Dc"], dtype=XP)
            Wc = np.abs(np.asarray((CA, Dc @ CA, Dc @ Dc @ CA)[sz], dtype=np.float64))
            d_w = EPS * ((cn * (4.0 * n * n + n * np.pi + 3.0 + g.zDim)) @ Wc)
        else:
            d_w = np.zeros(1)
        d_F = 2.0 * kk ** sl * EPS * (2.0 * kk * np.pi + 4.0)
        for q, ray in enumerate(rays):
            F, W = _weights(g, key, ray, False)
            ff, ww = np.abs(F), np.abs(W)
            S = np.einsum("zbm,b,z->m", aa, ff, ww)
            out[:, p, q] = EPS * (ncol + 2.0) * S + np.einsum("zbm,b,z->m", aa, d_F, ww) + np.einsum("zbm,b,z->m", aa, ff, d_w)
    return out


def stations(g, radii=None):
    """the tile's inner end, its radial gridpoints (default: oracle_np.mish_points, the doubles the gridpoints print) and its outer end"""
    r = O.mish_points(g.xmin, g.DX, 0, g.nc) if radii is None else np.asarray(radii, dtype=np.float64)
    return np.concatenate([[g.xmin], r, [g.xmax]])


def basis64(g, r):
    """(cell, phi [3, 4]) in plain float64, the operations of the library's function: delta = (r - x_node) / DX"""
    r, xmin, DX = np.float64(r), np.float64(g.xmin), np.float64(g.DX)
    cell = min(max(int(np.floor((r - xmin) / DX)), 0), g.nc - 1)
    phi = np.zeros((3, 4))
    for j in range(4):
        delta = (r - (xmin + np.float64(cell - 1 + j) * DX)) / DX
        z = abs(delta)
        if z >= 2.0:
            continue
        s = 1.0 if delta > 0 else -1.0
        p, q = 2.0 - z, (1.0 - z if z < 1.0 else 0.0)
        phi[0, j] = p * p * p / 6.0 - 4.0 * q * q * q / 6.0
        phi[1, j] = -s * (p * p / 2.0 - 2.0 * q * q) / DX
        phi[2, j] = (p - 4.0 * q) / (DX * DX)
    return cell, phi


def value(g, Pq, pl, program, r, xp=True):
    """g_q(r) in the twin's type: the planes from the ray's profiles Pq [b_rDim, n_profiles] (4-node spline sums), then the program in
    term order from +0.0.  float64: the library's order of operations (without its fused multiply-adds)."""
    T = _ty(xp)
    coef, packed, _ = program
    r64 = float(r)
    if xp:
        cell = E.node0_of(g, r64)
        phi = E.radial_weights(g, r64, cell, True)
    else:
        cell, phi = basis64(g, r64)
    val = []
    for j in range(len(pl.planes)):
        p = np.asarray(Pq[cell:cell + 4, pl.pprof[j]], dtype=T)
        w = np.asarray(phi[pl.pd[j]], dtype=T)
        val.append(w[3] * p[3] + (w[2] * p[2] + (w[1] * p[1] + w[0] * p[0])))
    rT = T(r64)
    rr = rT * rT
    q = T(0)
    with np.errstate(all="ignore"):
        for t in range(len(coef)):
            p, nf = int(packed[t, 1]), int(packed[t, 2])
            x = T(coef[t])
            if p != 0:
                x = x * (rT if p == 1 else rr if p == 2 else T(1) / rT if p == -1 else T(1) / rr)
            for f in range(nf):
                x = x * val[pl.planes.index((int(packed[t, 3 + f]), int(packed[t, 7 + f])))]
            q = q + x
    return q


# ----------------------------------------------------------------------------- the bracket step
class Bracket:
    """a, fa, b, fb, ga, gb, x, side, bis as the header's sx_bracket_step holds them, in type T"""

    def __init__(self, a, fa, b, fb, T=np.float64):
        self.T = T
        self.a, self.fa, self.b, self.fb = T(a), T(fa), T(b), T(fb)
        self.ga, self.gb, self.x, self.side, self.bis = self.fa, self.fb, self.a, 0, 0

    def state(self):
        return np.array([self.a, self.fa, self.b, self.fb, self.ga, self.gb, self.x], dtype=self.T), np.array([self.side, self.bis], dtype=np.int32)

    def done(self, wtol):
        return self.fa == 0 or self.fb == 0 or not (self.b - self.a > self.T(wtol))

    def trial(self):
        with np.errstate(all="ignore"):
            x = self.b - (self.gb * (self.b - self.a)) / (self.gb - self.ga)
        if self.bis or not (x > self.a and x < self.b):
            x = self.a + self.T(0.5) * (self.b - self.a)
        self.x = x

    def start(self, wtol):
        if self.done(wtol):
            return 0
        self.trial()
        return -1

    def step(self, fx, wtol):
        T = self.T
        fx = T(fx)
        if fx != fx:
            return 2
        w0 = self.b - self.a
        if fx == 0:
            self.a = self.b = self.x
            self.fa = self.fb = self.ga = self.gb = T(0)
            return 0
        if (fx < 0) == (self.fa < 0):
            self.a, self.fa, self.ga = self.x, fx, fx
            if self.side < 0:
                self.gb = self.gb * T(0.5)
            self.side = -1
        else:
            self.b, self.fb, self.gb = self.x, fx, fx
            if self.side > 0:
                self.ga = self.ga * T(0.5)
            self.side = 1
        self.bis = int(self.b - self.a > T(0.5) * w0)
        if self.done(wtol):
            return 0
        self.trial()
        return -1

    def root(self):
        return self.a if abs(self.fa) <= abs(self.fb) else self.b


# ----------------------------------------------------------------------------- scan and refine
Result = collections.namedtuple("Result", "radius dir count status")


def scan_ray(g, fn, levels, tol=1e-9, max_iter=60, max_cross=4, xp=True, radii=None):
    """What sx_crossings returns for ONE ray whose program value at r is fn(r) (type T): radius [max_cross, n_levels] as float64
    (the device returns doubles: a longdouble root is rounded once), dir, count [n_levels], status"""
    T = _ty(xp)
    st = stations(g, radii)
    gv = [fn(r) for r in st]
    nl = len(levels)
    radius, dirs = np.full((max_cross, nl), np.nan), np.zeros((max_cross, nl), dtype=np.int32)
    count, status = np.zeros(nl, dtype=np.int32), 0
    wtol = T(tol) * T(g.DX)
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
            B = Bracket(st[i], d0, st[i + 1], d1, T)
            s = B.start(wtol)
            it = 0
            while s < 0 and it < max_iter:
                # the position is a float64 between the steps only in the device's type; the longdouble twin keeps its own
                s = B.step(fn(B.x) - T(c), wtol)
                it += 1
            if s != 0:
                status |= 2 if s < 0 else 4
            radius[pos, j] = float(B.root())
            dirs[pos, j] = 1 if d0 < 0 else -1
    return Result(radius, dirs, count, status)


def crossings(g, A, program, levels, rays, tol=1e-9, max_iter=60, max_cross=4, xp=True, radii=None, P=None):
    """The call as Grid.crossings returns it: Result(radius [max_cross, n_levels, n_rays], dir, count [n_levels, n_rays], status
    [n_rays]); P: profiles to use instead of the twin's own (the device's, to separate the stages)"""
    pl = plan(g, program[1])
    q = reduce_rays(g, rays)
    Pr = profiles(g, A, pl, q, xp) if P is None else P
    out = [scan_ray(g, lambda r, i=i: value(g, Pr[:, :, i], pl, program, r, xp), levels, tol, max_iter, max_cross, xp, radii)
           for i in range(len(q))]
    return Result(np.stack([o.radius for o in out], axis=2), np.stack([o.dir for o in out], axis=2),
                  np.stack([o.count for o in out], axis=1), np.array([o.status for o in out], dtype=np.int32))


# ----------------------------------------------------------------------------- the selection rules
def select(res, level=0, which="outermost", falling=False):
    """[n_rays]: the innermost / outermost kept crossing of a level per ray (falling: among those with dir == -1), NaN without one"""
    rad, dr = res.radius[:, level, :], res.dir[:, level, :]
    ok = ~np.isnan(rad) & ((dr == -1) if falling else True)
    out = np.full(rad.shape[1], np.nan)
    for q in range(rad.shape[1]):
        r = rad[ok[:, q], q]
        if len(r):
            out[q] = r[0] if which == "innermost" else r[-1]
    return out


def quadrant_max(lam, radii):
    """[4]: the largest radius over the rays of the NE, SE, SW, NW quadrant (lambda = 0 east, counter-clockwise), NaN without one"""
    q = np.floor(np.mod(lam, 2.0 * np.pi) / (np.pi / 2.0)).astype(int) % 4
    out = np.full(4, np.nan)
    for col, which in enumerate((0, 3, 2, 1)):
        r = radii[(q == which) & ~np.isnan(radii)]
        if len(r):
            out[col] = r.max()
    return out


def project(g, values):
    """A [S_patch, V] of one-tile physical values through the oracle's forward and spline transforms"""
    return g.spline_transform(g.forward(values))
