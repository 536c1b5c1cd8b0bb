"""TEST INFRASTRUCTURE - the numpy twin of sx_distribution / sx_distribution_slot (include/scythe_hip.h).

The binned quantity q is formed in plain float64, operation for operation as the kernels form an output (the rule tests/extrema.py's
scan is held to exactly: coef, then r^p as r, r r, 1 / r or 1 / (r r), then the factors in order, the terms added in term order
from +0.0), so a point's slot is reproduced exactly.  The slot is np.searchsorted(edges, q, side="right") with the NaN rule.  The
weights are tests/reduce.py's (longdouble, from the definition), the sums per slot are longdouble with S_abs per slot, and the bound of
a sum is tests/reduce.py::BOUND applied to that slot's S_abs: the roundings of a slot's sum are those of sx_reduce's sum over the same
points (derived there, not fitted to the kernel).  The weighted quantile is by sorting."""
import numpy as np

from tests import reduce as R

XP = R.XP


def program_values64(data, r, program, out=0):
    """[N] float64: output `out` of the program at every point, as ext_point / dist_point form it; data [N, V, D] or [N, V]"""
    coef, packed, n_out = program
    data = np.asarray(data, dtype=np.float64)
    data = data[:, :, None] if data.ndim == 2 else data
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(all="ignore"):
        rr = r * r
        ri, rri = 1.0 / r, 1.0 / rr
        q = np.zeros(data.shape[0])
        for t in range(len(coef)):
            if int(packed[t, 0]) != out:
                continue
            p, nf = int(packed[t, 1]), int(packed[t, 2])
            x = np.full(data.shape[0], float(coef[t]))
            if p != 0:
                x = x * {1: r, 2: rr, -1: ri, -2: rri}[p]
            for f in range(nf):
                x = x * data[:, packed[t, 3 + f] - 1, packed[t, 7 + f]]
            q = q + x
    return q


def slots(edges, q):
    """the slot of every q among len(edges) + 2: searchsorted from the right, NaN last"""
    edges = np.asarray(edges, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    s = np.searchsorted(edges, q, side="right")
    return np.where(np.isnan(q), len(edges) + 1, s).astype(np.int64)


def point_weights(g, points, kind="domain", cell0=0, ncells=None):
    """(w [N] longdouble, level [N], ring [N]): the weight of every point of the tile (domain: w_r w_l w_z, level: w_r w_l)"""
    ncells = g.nc if ncells is None else ncells
    pts = np.asarray(points, dtype=np.float64)
    r = pts.reshape(len(pts), -1)[:, 0]
    nz = g.zDim
    L = np.asarray(g.L[3 * cell0:3 * (cell0 + ncells)])
    start = np.concatenate([[0], np.cumsum(L * nz)])
    assert start[-1] == len(r)
    w_r, w_l, w_z = R.weights(g, cell0, ncells, radii=r[start[:-1]])
    ring = np.repeat(np.arange(len(L)), L * nz)
    level = np.arange(len(r)) % nz
    w = w_r[ring] * w_l[ring]
    if kind == "domain":
        w = w * w_z[level]
    return w, level, ring


def distribution(g, data, points, program, edges, kind="domain", cell0=0, ncells=None):
    """What sx_distribution returns: (count int64 [S, groups], sums longdouble [S, n_out, groups], S_abs of the same shape, slot [N]);
    program = (coef, packed, n_out) as pack_reduce_program gives it"""
    coef, packed, n_out = program
    pts = np.asarray(points, dtype=np.float64)
    r = pts.reshape(len(pts), -1)[:, 0]
    w, level, _ = point_weights(g, pts, kind, cell0, ncells)
    groups = g.zDim if kind == "level" else 1
    grp = level if kind == "level" else np.zeros(len(r), dtype=int)
    sl = slots(edges, program_values64(data, r, program))
    S = len(edges) + 2
    tv = R.term_values(data, r, coef, packed)
    val = np.zeros((n_out, len(r)), dtype=XP)
    ab = np.zeros((n_out, len(r)), dtype=XP)
    val[0], ab[0] = w, np.abs(w)
    for t in range(len(coef)):
        o = int(packed[t, 0])
        if o > 0:
            val[o] += tv[t] * w
            ab[o] += np.abs(tv[t] * w)
    count = np.zeros((S, groups), dtype=np.int64)
    sums, sabs = np.zeros((S, n_out, groups), dtype=XP), np.zeros((S, n_out, groups), dtype=XP)
    key = grp * S + sl
    for k in np.unique(key):
        sel = key == k
        gi, si = int(k) // S, int(k) % S
        count[si, gi] = sel.sum()
        sums[si, :, gi] = val[:, sel].sum(axis=1)
        sabs[si, :, gi] = ab[:, sel].sum(axis=1)
    return count, sums, sabs, sl


def check(got, truth, sabs, what=""):
    """|got - truth| <= BOUND S_abs per slot, output and group; NaN sums (the NaN slot of a NaN integrand) are skipped where the twin
    is NaN too"""
    got, truth = np.asarray(got), np.asarray(truth)
    both_nan = np.isnan(got) & np.isnan(truth.astype(np.float64))
    R.check(np.where(both_nan, 0.0, got), np.where(both_nan, XP(0), truth), np.where(both_nan, XP(0), sabs), what)


def weighted_quantile(q, w, p):
    """(Q, cum, M): the sorted weighted quantile of the non-NaN q - the value q_(i) with measure{q < q_(i)} <= p M < measure{q <=
    q_(i)} - the cumulative sums of the weights in sorted order, and M"""
    q, w = np.asarray(q, dtype=np.float64), np.asarray(w, dtype=XP)
    ok = ~np.isnan(q)
    order = np.argsort(q[ok], kind="stable")
    qs, cum = q[ok][order], np.cumsum(w[ok][order])
    M = cum[-1]
    i = int(np.searchsorted(cum, XP(p) * M, side="right"))
    # equal values share one cumulative step: the quantile is the value, so ties need no care
    return float(qs[min(i, len(qs) - 1)]), cum, M
