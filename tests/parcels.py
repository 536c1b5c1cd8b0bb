"""TEST INFRASTRUCTURE - the numpy twin of sx_parcels_* (include/scythe_hip.h): Lagrangian parcels moved by the
velocity the A coefficients give, in float64 (xp=False) or numpy.longdouble (xp=True, the arbiter).  The velocity is the value slot of
the twin in tests/evaluate.py with the ALL_K truncation (its weight functions, summed here so that the sum of absolute terms S comes
out beside the value); the Cartesian update and the Euler -> AB2 -> AB3 start are written from the definition in the header.

Rounding bound of ONE velocity component of one parcel (velocity_bound), derived from the operation count of a Float64 evaluation
    u = sum_col (sum_j phi_j a[j, col]) F_blk(col) w_zm(col),      S = sum |a phi F w|,     eps = 2^-53,
to first order in eps:
  the sums       every term passes through the 4-node dot product (4 roundings), the products F w and s (F w) (2) and the
                 accumulation, whose depth is at most the number of live columns ncol = b_zDim (2 kDim + 1) whatever the order:
                                                                                                   eps (ncol + 6) S
  phi            delta = (r - x_node) / DX is off by eps (|r| + |x_node|) / DX + 2 eps |delta| <= eps (2 X + 6), X = max(|xmin|, |xmax|) / DX,
                 |phi'| <= 1, and the cubic itself by 8 eps: an ABSOLUTE error d_phi = eps (2 X + 14) of every weight - near the
                 end of its support a weight is far smaller than its error, so this part scales with S_phi = sum |a| |F| |w|
                 (phi replaced by 1), not with S:                                                  d_phi S_phi
  F              lambda is kept in (-pi, pi], so the Float64 product k lambda is off by at most k pi eps; sincos adds 1 ulp
                 and the factor 2 one rounding:                                                    sum |a phi w| 2 eps (k pi + 2)
  w              w_zm = sum_n t_n CA[n, zm], t_n = c_n cos(n acos x): x is off by 4 eps and |T_n'| <= n^2, the product
                 n theta by n pi eps, cos by 1 ulp; the sum is zDim deep:
                                                       d_w[zm] = eps sum_n c_n |CA[n, zm]| (4 n^2 + n pi + 2 + zDim),   sum |a phi F| d_w
The bound is the sum of the four parts.  The longdouble twin's own error is 2^-11 of it."""
import numpy as np

from oracle import oracle_np as O
from tests import evaluate as E

XP = O.XP
EPS = 2.0 ** -53

# Largest position difference between the Float64 twin and the longdouble twin over 6 steps on the four test grids, in units of
# dt eps S (S: the parcel's largest sum of absolute terms over steps and components): measured by
# tests/test_parcels.py::test_twin_spread, which holds the twins to it; the GPU tests allow 8 x this ("Figures").
TWIN_SPREAD = 7700.0        # measured: R 7611.5, RZ 3926.8, RL 4904.9, RLZ 3135.0


def _ty(xp):
    return XP if xp else np.float64


def reduce_lambda(lam):
    """lambda into (-pi, pi], in extended precision and rounded once (what sx_parcels_set does on the host)"""
    two_pi = XP(8) * np.arctan(XP(1))
    r = np.fmod(np.asarray(lam, dtype=XP), two_pi)                 # exact
    r = np.where(r > two_pi / 2, r - two_pi, r)
    r = np.where(r <= -two_pi / 2, r + two_pi, r)
    out = np.asarray(r, dtype=np.float64)
    return np.where(out <= -np.pi, np.pi, out)


def ab_value(t, ts, u, e, e1, e2):
    """explicit_timestep's coefficients (src/semiimplicit.jl:672-698), as oracle_np states them"""
    if t == 1:
        return u + (ts * e)
    if t == 2:
        return u + (0.5 * ts) * ((3.0 * e) - e1)
    return u + ((ts / 12.0) * ((23.0 * e) - (16.0 * e1) + (5.0 * e2)))


def velocity(g, A, pts, var, xp=True, with_bound=False):
    """(vel [n, n_coord], S [n, n_coord][, bound [n, n_coord]]): the value slot of the variables var (1-based per coordinate, 0 = none)
    at pts with every wavenumber of the patch, S = sum |A phi F C| and the rounding bound of the module docstring"""
    T = _ty(xp)
    pts = np.asarray(pts).reshape(len(pts), -1)
    nco = pts.shape[1]
    vel, S, B = np.zeros((len(pts), nco), dtype=T), np.zeros((len(pts), nco)), np.zeros((len(pts), nco))
    Av = {v: A[:, v - 1].reshape(g.b_zDim, g.K2, g.b_rDim).astype(T) for v in set(var) if v}
    kk = np.concatenate([[0], np.repeat(np.arange(1, g.kDim + 1), 2)]) if g.has_l else np.zeros(1)
    d_phi = EPS * (2.0 * max(abs(g.xmin), abs(g.xmax)) / g.DX + 14.0)
    d_F = 2.0 * EPS * (kk * np.pi + 2.0)
    ncol = g.b_zDim * g.K2
    for i, p in enumerate(pts):
        r = float(p[0])
        n0 = E.node0_of(g, r)
        ph = E.radial_weights(g, r, n0, xp)[0]
        F = E.fourier_weights(g.kDim, p[1], xp)[0] if g.has_l else np.ones(1, dtype=T)
        for c, v in enumerate(var):
            if not v:
                continue
            if g.has_z:
                name = g.names[v - 1]
                wz = E.vertical_weights(g, name, p[-1], xp)[0]
            else:
                wz = np.ones(1, dtype=T)
            a = Av[v][:, :, n0:n0 + 4]                                           # [zm, blk, node]
            terms = a * ph[None, None, :] * F[None, :, None] * wz[:, None, None]
            vel[i, c] = terms.sum()
            S[i, c] = float(np.abs(terms).sum())
            if with_bound:
                aa, fp, ff, ww = np.abs(a).astype(np.float64), np.abs(ph).astype(np.float64), np.abs(F).astype(np.float64), np.abs(wz).astype(np.float64)
                if g.has_z:
                    x = g.cheb(name)._x
                    CA = np.abs(np.asarray(x["CA"], dtype=np.float64))                # [zDim, b_zDim]
                    n = np.arange(g.zDim)
                    cn = np.where((n == 0) | (n == g.zDim - 1), 1.0, 2.0)
                    d_w = EPS * ((cn * (4.0 * n * n + n * np.pi + 2.0 + g.zDim)) @ CA)
                else:
                    d_w = np.zeros(1)
                s_phi = np.einsum("zbn,b,z->", aa, ff, ww)
                s_F = np.einsum("zbn,n,b,z->", aa, fp, d_F, ww)
                s_w = np.einsum("zbn,n,b,z->", aa, fp, ff, d_w)
                B[i, c] = EPS * (ncol + 6.0) * S[i, c] + d_phi * s_phi + s_F + s_w
    return (vel, S, B) if with_bound else (vel, S)


class Parcels:
    """The parcel set of the definition: positions [n, n_coord], Cartesian history, per-parcel step counters and status."""

    def __init__(self, g, points, var, xp=True, field=None):
        """var: 1-based variable index per coordinate (0 = no motion); field: an analytic velocity pos -> [n, n_coord] used instead of A"""
        self.g, self.xp, self.T, self.field = g, xp, _ty(xp), field
        p = np.array(points, dtype=np.float64).reshape(len(points), -1)
        if g.has_l:
            p[:, 1] = reduce_lambda(p[:, 1])
        self.pos = p.astype(self.T)
        self.var = tuple(int(v) for v in var)
        n, nco = self.pos.shape
        self.h1, self.h2 = np.zeros((n, nco), dtype=self.T), np.zeros((n, nco), dtype=self.T)
        self.vel, self.S = np.zeros((n, nco), dtype=self.T), np.zeros((n, nco))
        self.cnt, self.status = np.zeros(n, dtype=int), np.zeros(n, dtype=np.int32)
        self.S_max = np.zeros(n)
        v_r = g.names[self.var[0] - 1] if self.var[0] else None
        self.wrap = (not g.has_l) and v_r is not None and g.BCL[v_r] == "PERIODIC" and g.BCR[v_r] == "PERIODIC"

    def advance(self, A, dt):
        g, T = self.g, self.T
        act = np.nonzero(self.status == 0)[0]
        if len(act) == 0:
            return
        pos = self.pos[act]
        if self.field is not None:
            vel, S = np.asarray(self.field(pos), dtype=T), np.zeros(pos.shape)
        else:
            vel, S = velocity(g, A, np.asarray(pos, dtype=np.float64), self.var, self.xp)
        self.vel[act], self.S[act] = vel, S
        self.S_max[act] = np.maximum(self.S_max[act], S.max(axis=1))
        dt = T(dt)
        iz = pos.shape[1] - 1
        for j, i in enumerate(act):
            x, e = pos[j].copy(), vel[j].copy()
            if g.has_l:
                c, s = np.cos(pos[j, 1]), np.sin(pos[j, 1])
                x[0], x[1] = pos[j, 0] * c, pos[j, 0] * s
                e[0], e[1] = (vel[j, 0] * c) - (vel[j, 1] * s), (vel[j, 0] * s) + (vel[j, 1] * c)
            t = min(self.cnt[i] + 1, 3)
            new = np.array([ab_value(t, dt, x[c], e[c], self.h1[i, c], self.h2[i, c]) for c in range(len(x))], dtype=T)
            if g.has_l:
                rn = np.hypot(new[0], new[1])
                ln = T(0) if rn == 0 else np.arctan2(new[1], new[0])
                if float(ln) <= -np.pi:
                    ln = T(np.pi)
                new[0], new[1] = rn, ln
            elif self.wrap:
                L = T(g.xmax) - T(g.xmin)
                rn = new[0] - np.floor((new[0] - T(g.xmin)) / L) * L
                if rn >= T(g.xmin) + L or rn < T(g.xmin):
                    rn = T(g.xmin)
                new[0] = rn
            if not (new[0] >= g.xmin and new[0] <= g.xmax):
                self.status[i] = 1
            elif g.has_z and not (new[iz] >= g.zmin and new[iz] <= g.zmax):
                self.status[i] = 2
            else:
                self.h2[i], self.h1[i] = self.h1[i], e
                self.pos[i] = new
                self.cnt[i] += 1


def distance(g, p, q):
    """[n]: how far apart two position arrays are - Cartesian in the horizontal on RL / RLZ grids, the larger of that and |dz|"""
    p, q = np.asarray(p, dtype=XP), np.asarray(q, dtype=XP)
    if g.has_l:
        d = np.hypot(p[:, 0] * np.cos(p[:, 1]) - q[:, 0] * np.cos(q[:, 1]), p[:, 0] * np.sin(p[:, 1]) - q[:, 0] * np.sin(q[:, 1]))
    else:
        d = np.abs(p[:, 0] - q[:, 0])
    if g.has_z:
        d = np.maximum(d, np.abs(p[:, -1] - q[:, -1]))
    return np.asarray(d, dtype=np.float64)


# ----------------------------------------------------------------------------- the four test grids and their states
def grid_case(geom, wide=False):
    """the smallest grids that exercise every branch: R 8 cells PERIODIC, RZ 6 x zDim 8, RL 6 cells and RLZ 5 x zDim 8 on native rings;
    wide (RLZ only): RLZ 12 x zDim 24, whose 16 x 73 = 1,168 columns per variable are the smallest of this family above the 1,024 at which
    a parcel's workgroup goes from one wave to four (k_parcels with 256 lanes: the waves added in order, the strided table fills)"""
    from tests import cases
    if geom == "R":
        return cases.r_bcs("PERIODIC", "PERIODIC", num_cells=8)
    if geom == "RZ":
        return cases.rz_advection(num_cells=6, zDim=8)
    if geom == "RL":
        return cases.rl_advection(num_cells=6)
    if wide:
        assert geom == "RLZ"
        return cases.rlz_advection(num_cells=12, zDim=24)
    return cases.rlz_advection(num_cells=5, zDim=8)


VELOCITY = {"R": ("u",), "RZ": ("u", "w"), "RL": ("u", "v"), "RLZ": ("u", "v", "h")}     # rlz_advection has no w: h stands in for it


def velocity_vars(g):
    return tuple(g.names.index(n) + 1 for n in VELOCITY[g.geometry])


def smooth_state(g, seed):
    """seeded random A [S_patch, V] whose coefficients decay with the wavenumber and the vertical mode"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((g.b_zDim, g.K2, g.b_rDim, g.V))
    k = np.concatenate([[0], np.repeat(np.arange(1, g.kDim + 1), 2)]) if g.has_l else np.zeros(1)
    a = a / (1.0 + k[None, :, None, None]) ** 2 / (1.0 + np.arange(g.b_zDim)[:, None, None, None]) ** 2
    return np.ascontiguousarray(a.reshape(-1, g.V))


def interior_points(g, n, seed):
    """n seeded points away from the edges (a parcel moves 1e-3 of the domain per step at most)"""
    rng = np.random.default_rng(seed)
    L = g.xmax - g.xmin
    cols = [rng.uniform(g.xmin + 0.05 * L, g.xmax - 0.05 * L, n)]
    if g.has_l:
        cols.append(rng.uniform(-np.pi, np.pi, n))
    if g.has_z:
        H = g.zmax - g.zmin
        cols.append(rng.uniform(g.zmin + 0.05 * H, g.zmax - 0.05 * H, n))
    return np.stack(cols, axis=1)


def special_points(g):
    """the points of the velocity test: r = 0 (the left edge), both tile edges, a cell boundary, z = zmin and z = zmax, lambda = 1e6,
    duplicates; the rest seeded"""
    p = interior_points(g, 24, seed=5)
    p[0, 0], p[1, 0], p[2, 0], p[3, 0] = g.xmin, g.xmax, g.xmin + 2 * g.DX, g.xmin + 3 * g.DX
    if g.has_l:
        p[4, 1], p[0, 1], p[5, 1] = 1.0e6, 0.7, -1.0e6
    if g.has_z:
        p[6, -1], p[7, -1], p[1, -1] = g.zmin, g.zmax, g.zmax
    p[8], p[9] = p[4], p[2]
    return p


def crossing_dt(g, A, pts, var):
    """1e-3 of the domain's crossing time at the largest parcel speed of the state"""
    vel, _ = velocity(g, A, pts, var, xp=False)
    return 1.0e-3 * (g.xmax - g.xmin) / float(np.abs(vel).max())
