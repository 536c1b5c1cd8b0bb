"""TEST INFRASTRUCTURE - the numpy twin of sx_regrid / sx_regrid_columns (include/scythe_hip.h), in float64 (xp=False) or
numpy.longdouble (xp=True, the arbiter).

The column map is written from its definition (column_map); the VALUES are summed at the float64 source coordinates that
sx_regrid_columns returns - those doubles are the definition, the twin does not re-derive them (a lambda beyond 2 pi in magnitude is
reduced as tests/isosurface.py::reduce_columns reduces it, which is what the device is sent).  A value is the dense sum
    u = sum_zm E[zm] C[zm],   C[zm] = sum_{blk, node} a phi F      (tests/isosurface.py::profiles: tests/evaluate.py's weights, every k)
with E the vertical row of tests/evaluate.py::vertical_weights of the SOURCE variable at the destination's level.  The destination's
coefficients are oracle_np's forward + spline_transform of those values (tests/project.py::project64 / project_xp).

Rounding bound of ONE value (value_bound), u = 2^-53, S2 = sum_zm |E[zm]| |C[zm]|:
  stage 1   every profile entry C[zm] carries tests/isosurface.py::profile_bound pb[zm] (the sum 4 K2 deep, the product phi F, the
            multiply-add, sincos and the spline weights - derived there); it enters the value through E:      sum_zm |E[zm]| pb[zm]
  E         formed in extended precision and rounded to float64 ONCE: 1 rounding per entry:                                  u S2
  stage 2   the chain over zm: b_zDim products (1 rounding each, none where the multiply-add is fused) and b_zDim additions, in any
            order a chain or a matrix unit takes them: at most b_zDim + 1 roundings on a term:                 (b_zDim + 1) u S2
  together  (b_zDim + 2) u S2 + sum |E| pb, with 1 % for the second-order terms.
Without a vertical b_zDim = 1 and E = (1): the value is the profile entry and the bound is pb + 3 u |C|.  The count is from the
operations; it is not tuned to what the GPU returns."""
import numpy as np

from oracle import oracle_np as O
from tests import evaluate as E
from tests import isosurface as IS
from tests import project as PJ

XP = O.XP
EPS = IS.EPS


def oracle_pair(spec):
    """(GridParameters, oracle Grid) of one grid given as the oracle's keywords (ring_L None: native rings)"""
    import scythe_jl_amd as S
    g = dict(spec)
    ring_L = g.pop("ring_L", None)
    gp = S.GridParameters(ring_uniform_L=ring_L or 0, **g)
    og = O.Grid(g.pop("geometry"), g.pop("xmin"), g.pop("xmax"), g.pop("num_cells"), g.pop("vars"), ring_L=ring_L, **g)
    return gp, og


def dst_columns(og):
    """(r, lambda) of the destination's columns in gridpoint order, float64 [n_cols, 1 or 2], and its levels [zDim]"""
    pts = og.gridpoints()
    pts = pts.reshape(len(pts), -1)
    z = pts[:og.zDim, -1].copy() if og.has_z else np.zeros(1)
    return pts[::og.zDim, :1 + int(og.has_l)].copy(), z


def column_map(og_dst, centre=None):
    """The map from its definition in longdouble: [n_cols, 1 or 2] (r_s[, lambda_s]) of every destination column about `centre`"""
    q, _ = dst_columns(og_dst)
    if not og_dst.has_l:
        return q.astype(XP)
    x0, y0 = (XP(0), XP(0)) if centre is None else (XP(float(centre[0])), XP(float(centre[1])))
    r, lam = q[:, 0].astype(XP), q[:, 1].astype(XP)
    if x0 == 0 and y0 == 0:
        return np.stack([r, lam], axis=1)
    x, y = x0 + r * np.cos(lam), y0 + r * np.sin(lam)
    return np.stack([np.hypot(x, y), np.arctan2(y, x)], axis=1)


def inside(og_src, r_s):
    """a column is inside when xmin <= r_s <= xmax of the source (the ends included)"""
    r_s = np.asarray(r_s)
    return (r_s >= og_src.xmin) & (r_s <= og_src.xmax)


def _plan(var_src):
    keys = []
    for v in var_src:
        if (int(v), 0) not in keys:
            keys.append((int(v), 0))
    return IS.Plan([], keys, [], []), [keys.index((int(v), 0)) for v in var_src]


def _rows(og_src, var_src, levels, xp):
    """E [V_dst][zDim_dst, b_zDim_src] in the twin's type"""
    T = XP if xp else np.float64
    if not og_src.has_z:
        return [np.ones((1, 1), dtype=T) for _ in var_src]
    cache = {}
    out = []
    for v in var_src:
        name = og_src.names[int(v) - 1]
        key = (og_src.BCB[name], og_src.BCT[name])
        if key not in cache:
            cache[key] = np.stack([E.vertical_weights(og_src, name, z, xp)[0] for z in levels]).astype(T)
        out.append(cache[key])
    return out


def values(og_src, A, var_src, columns, inside_mask, levels, fill=None, xp=True):
    """[n_cols zDim_dst, V_dst] in the twin's type, the destination's var_np1 order (z fastest): the continuous function of the source
    (every wavenumber) at columns [n_cols, 1 or 2] - the doubles sx_regrid_columns returned - and the destination's levels; fill[v] in
    the columns that are not inside"""
    T = XP if xp else np.float64
    cols = IS.reduce_columns(og_src, columns)
    pl, prof = _plan(var_src)
    sel = np.nonzero(inside_mask)[0]
    C = IS.profiles(og_src, A, pl, cols[sel], xp)                            # [Zb, nprof, n_in]
    Ev = _rows(og_src, var_src, levels, xp)
    nz = len(levels)
    out = np.zeros((len(cols), nz, len(var_src)), dtype=T)
    for vi in range(len(var_src)):
        out[:, :, vi] = T(0.0 if fill is None else float(np.broadcast_to(fill, (len(var_src),))[vi]))
        out[sel, :, vi] = np.einsum("nz,zq->qn", Ev[vi], C[:, prof[vi], :])
    return out.reshape(len(cols) * nz, len(var_src))


def value_bound(og_src, A, var_src, columns, inside_mask, levels):
    """[n_cols zDim_dst, V_dst] float64: the rounding bound of the module docstring (0 in a column that is filled)"""
    cols = IS.reduce_columns(og_src, columns)
    pl, prof = _plan(var_src)
    sel = np.nonzero(inside_mask)[0]
    A64 = np.asarray(A, dtype=np.float64)
    Ca = np.abs(IS.profiles(og_src, A64, pl, cols[sel], False))
    pb = IS.profile_bound(og_src, A64, pl, cols[sel])
    Ev = _rows(og_src, var_src, levels, False)
    nz = len(levels)
    out = np.zeros((len(cols), nz, len(var_src)))
    for vi in range(len(var_src)):
        Ea = np.abs(Ev[vi])
        S2 = np.einsum("nz,zq->qn", Ea, Ca[:, prof[vi], :])
        out[sel, :, vi] = 1.01 * (EPS * (og_src.b_zDim + 2.0) * S2 + np.einsum("nz,zq->qn", Ea, pb[:, prof[vi], :]))
    return out.reshape(len(cols) * nz, len(var_src))


def coefficients(og_dst, vals, xp=True):
    """A [S_patch, V] of the destination from its var_np1 values: oracle_np's forward + spline transform (tests/project.py)"""
    vals = np.asarray(vals, dtype=np.float64)
    return PJ.project_xp(og_dst, vals) if xp else PJ.project64(og_dst, vals)
