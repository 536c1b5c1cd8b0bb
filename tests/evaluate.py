"""TEST INFRASTRUCTURE - the numpy twin of sx_evaluate / sx_eval_basis: u(r, lambda, z) = sum A phi F C at arbitrary points from
Float64 A coefficients and Float64 coordinates, in float64 (xp=False) or in numpy.longdouble (xp=True, the arbiter, as
oracle_np.inverse_xp is for the gridpoints).  Built on oracle_np: bspline, the ring tables of Grid, the factors Cheb._x."""
import numpy as np

from oracle import oracle_np as O

XP = O.XP


def _ty(xp):
    return XP if xp else np.float64


def tile_range(g, cell0=0, ncells=None):
    ncells = g.nc if ncells is None else ncells
    lo = g.xmin if cell0 == 0 else g.xmin + cell0 * g.DX
    hi = g.xmax if cell0 + ncells == g.nc else g.xmin + (cell0 + ncells) * g.DX
    return lo, hi


def node0_of(g, r, cell0=0, ncells=None):
    """the cell of r among the tile's cells = patch row of the first of its 4 nodes"""
    ncells = g.nc if ncells is None else ncells
    c = int(np.floor((float(r) - g.xmin) / g.DX))
    return min(max(c, cell0), cell0 + ncells - 1)


def kcap_of(g, r, all_k=False):
    """SX_EVAL_RING_K: kmax of the last patch ring whose radius, as gridpoints() prints it, is <= r (ring 1 below the first)"""
    if not g.has_l:
        return 0
    if all_k:
        return g.kDim
    rad = O.mish_points(g.xmin, g.DX, 0, g.nc)
    i = int(np.searchsorted(rad, float(r), side="right")) - 1
    return int(g.kmax[max(i, 0)])


def radial_weights(g, r, n0, xp):
    """[3, 4]: phi, phi', phi'' of nodes n0 .. n0 + 3 at r (oracle_np.inverse_xp's statement, at any r)"""
    T = _ty(xp)
    xm = T(g.xmin) + (np.arange(n0, n0 + 4).astype(T) - 1) * T(g.DX)
    delta = (T(r) - xm) / T(g.DX)
    return np.stack([O.bspline(delta, d) / T(g.DX) ** d for d in range(3)]).astype(T)


def vertical_weights(g, v, z, xp):
    """[3, b_zDim]: rows of the b -> (value, d/dz, d2/dz2) operator of variable v at z: the DCT-I series at x = (z - mid) / (-Lz / 2)
    on a = CA b and its coefficient-space derivatives"""
    T = _ty(xp)
    x = g.cheb(v)._x
    CA, Dc = np.asarray(x["CA"], dtype=T), np.asarray(x["Dc"], dtype=T)
    N = g.zDim
    mid, half = (T(g.zmin) + T(g.zmax)) / T(2), (T(g.zmax) - T(g.zmin)) / T(2)
    xx = np.clip((T(z) - mid) / (-half), T(-1), T(1))
    w = np.full(N, 2, dtype=T)
    w[0] = w[-1] = 1
    t = w * np.cos(np.arange(N).astype(T) * np.arccos(xx))
    return np.stack([t @ CA, t @ Dc @ CA, t @ Dc @ Dc @ CA]).astype(T)


def fourier_weights(kcap, lam, xp):
    """[3, 1 + 2 kcap]: F_blk(lambda) and its first two derivatives (oracle_np.Ring.FI at any lambda)"""
    T = _ty(xp)
    F = np.zeros((3, 1 + 2 * kcap), dtype=T)
    F[0, 0] = 1
    k = np.arange(1, kcap + 1).astype(T)
    c, s = np.cos(k * T(lam)), np.sin(k * T(lam))
    F[0, 1::2], F[0, 2::2] = 2 * c, -2 * s
    F[1, 1::2], F[1, 2::2] = -2 * k * s, -2 * k * c
    F[2, 1::2], F[2, 2::2] = -2 * k * k * c, 2 * k * k * s
    return F


def basis(g, v, point, all_k=False, cell0=0, ncells=None, xp=True):
    """what sx_eval_basis returns: (node0, w_r [3, 4], kcap, w_z [3, b_zDim] or None)"""
    point = np.atleast_1d(point)
    r = point[0]
    n0 = node0_of(g, r, cell0, ncells)
    wz = vertical_weights(g, v, point[-1], xp) if g.has_z else None
    return n0, radial_weights(g, r, n0, xp), kcap_of(g, r, all_k), wz


def evaluate(g, A, points, all_k=False, cell0=0, ncells=None, xp=True):
    """[n, V, D] in the twin's precision; A [S_patch, V] Float64 in the reference layout.  Points that share a radius (the rings of
    the model's own gridpoints) share the radial sums; every point is summed in full."""
    T = _ty(xp)
    pts = np.asarray(points, dtype=np.float64)
    pts = pts.reshape(len(pts), -1)
    sl = {s: i for i, s in enumerate(g.slots)}
    out = np.zeros((len(pts), g.V, g.D), dtype=T)
    Av = [A[:, vi].reshape(g.b_zDim, g.K2, g.b_rDim) for vi in range(g.V)]
    wz_cache = {}
    radii, inv = np.unique(pts[:, 0], return_inverse=True)
    for ri, r in enumerate(radii):
        idx = np.nonzero(inv == ri)[0]
        n0 = node0_of(g, r, cell0, ncells)
        PH = radial_weights(g, r, n0, xp)
        kc = kcap_of(g, r, all_k)
        nb = 1 + 2 * kc
        F = np.stack([fourier_weights(kc, p[1] if g.has_l else 0.0, xp) for p in pts[idx]])     # [n, 3, nb]
        for vi, v in enumerate(g.names):
            a = Av[vi][:, :nb, n0:n0 + 4].astype(T)                     # [zm, blk, node]
            coef = np.einsum("zbn,dn->dzb", a, PH)                       # [d, zm, blk]
            f0 = np.einsum("dzb,nb->ndz", coef, F[:, 0])                 # [n, d, zm]
            f1 = np.einsum("zb,nb->nz", coef[0], F[:, 1])
            f2 = np.einsum("zb,nb->nz", coef[0], F[:, 2])
            if g.has_z:
                wz = []
                for p in pts[idx]:
                    key = (g.BCB[v], g.BCT[v], float(p[-1]))
                    if key not in wz_cache:
                        wz_cache[key] = vertical_weights(g, v, p[-1], xp)
                    wz.append(wz_cache[key])
                wz = np.stack(wz)                                        # [n, 3, zm]
            else:
                wz = np.tile(np.array([[1], [0], [0]], dtype=T), (len(idx), 1, 1))
            out[idx, vi, sl["u"]] = np.einsum("nz,nz->n", wz[:, 0], f0[:, 0])
            out[idx, vi, sl["r"]] = np.einsum("nz,nz->n", wz[:, 0], f0[:, 1])
            out[idx, vi, sl["rr"]] = np.einsum("nz,nz->n", wz[:, 0], f0[:, 2])
            if g.has_l:
                out[idx, vi, sl["l"]] = np.einsum("nz,nz->n", wz[:, 0], f1)
                out[idx, vi, sl["ll"]] = np.einsum("nz,nz->n", wz[:, 0], f2)
            if g.has_z:
                out[idx, vi, sl["z"]] = np.einsum("nz,nz->n", wz[:, 1], f0[:, 0])
                out[idx, vi, sl["zz"]] = np.einsum("nz,nz->n", wz[:, 2], f0[:, 0])
    return out


def scattered_points(g, n, seed, cell0=0, ncells=None):
    """n seeded points of the tile: uniform in r / z, lambda in [-2 pi, 4 pi] (so < 0 and > 2 pi), with both radial and vertical ends,
    cell edges and exact ring radii among them"""
    rng = np.random.default_rng(seed)
    ncells = g.nc if ncells is None else ncells
    lo, hi = tile_range(g, cell0, ncells)
    r = rng.uniform(lo, hi, n)
    edges = g.xmin + np.arange(cell0 + 1, cell0 + ncells) * g.DX
    rings = O.mish_points(g.xmin, g.DX, cell0, ncells)
    special = np.concatenate([[lo, hi], edges, rings])
    special = special[(special >= lo) & (special <= hi)][:n // 2]
    r[:len(special)] = special
    cols = [r]
    if g.has_l:
        lam = rng.uniform(-2 * np.pi, 4 * np.pi, n)
        lam[:4] = [-1.0, 7.0, 0.0, 2 * np.pi]
        cols.append(rng.permutation(lam))
    if g.has_z:
        z = rng.uniform(g.zmin, g.zmax, n)
        lev = g.cheb(g.names[0]).z
        sp = np.concatenate([[g.zmin, g.zmax], lev[1:-1]])[:n // 2]
        z[:len(sp)] = sp
        cols.append(rng.permutation(z))
    return np.stack(cols, axis=1)


def slot_errors(a, t):
    """[D]: max over variables and points of |a - t| / max|t[:, :, d]| against the longdouble truth t"""
    t = np.asarray(t)
    return np.array([float(np.abs(np.asarray(a[:, :, d], dtype=XP) - t[:, :, d]).max() / max(float(np.abs(t[:, :, d]).max()), 1e-300))
                     for d in range(t.shape[2])])


# ----------------------------------------------------------------------------- the read-only job, here or in a child process
def read_only_job(maker, kw, steps=9, n_points=300):
    """Two runs of `steps` steps of cases.<maker>(**kw), one calling evaluate after every step: {state0, np10, state1, np11, got,
    w_err (the diagnostic variable mid-run against the twin on the flushed A), kernels (timer names of one timed step of a third
    handle: which equation-set kernels the handle launches)}.  The SX_* switches come from the environment of this process."""
    from tests import cases
    case = getattr(cases, maker)(**kw)
    g = cases.oracle_grid(case)
    pts = scattered_points(g, n_points, seed=31)
    out = {}
    for with_eval in (0, 1):
        hip = cases.HipModel(case)
        tile = hip.run.tiles[0]
        for s in range(steps):
            hip.step()
            if with_eval:
                got = tile.evaluate(pts)
                if s == steps // 2:
                    truth = evaluate(g, tile.patchSpectral, pts, xp=True)       # patchSpectral: the flushed A
                    w = g.V - 1
                    out["w_err"] = np.array(float(np.abs(got[:, w, 0].astype(XP) - truth[:, w, 0]).max()
                                                  / max(float(np.abs(truth[:, w, 0]).max()), 1e-300)))
                    out["w_max"] = np.array(np.abs(got[:, w, 0]).max())
        out["state%d" % with_eval], out["np1%d" % with_eval] = tile.get_state(), tile.var_np1
        hip.run.close()
    out["got"] = got
    hip = cases.HipModel(case)
    hip.run.tiles[0].enable_timers(True)
    hip.step()
    out["kernels"] = np.array(sorted(hip.run.tiles[0].timers()))
    hip.run.close()
    return out


def read_only_in_child(tmp_path, maker, kw, overrides, timeout=300):
    """read_only_job in a fresh `python -m tests.evaluate` with os.environ | overrides, as tests/child_run.py runs its jobs: one
    child, under a time limit; a child that dies on a signal or hangs ends the session - nothing more starts on the GPU."""
    import json
    import os
    import subprocess
    import sys
    import pytest
    from tests.child_run import ROOT, _tail
    path = os.path.join(str(tmp_path), "read_only_%s.npz" % "_".join(sorted(overrides)))
    cmd = [sys.executable, "-m", "tests.evaluate", json.dumps([maker, kw]), path]
    env = os.environ | {k: str(v) for k, v in overrides.items()}
    try:
        p = subprocess.run(cmd, cwd=ROOT, env=env, timeout=timeout, capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        pytest.exit("child GPU process with %s hung (no exit within %d s); nothing more starts on the GPU in this session\n%s"
                    % (overrides, timeout, _tail(e.stderr)), returncode=3)
    if p.returncode < 0:
        pytest.exit("child GPU process with %s died on signal %d; nothing more starts on the GPU in this session\n%s"
                    % (overrides, -p.returncode, _tail(p.stderr)), returncode=3)
    assert p.returncode == 0, "child with %s failed (exit %d):\n%s" % (overrides, p.returncode, _tail(p.stderr))
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    import json
    import sys
    _maker, _kw = json.loads(sys.argv[1])
    np.savez(sys.argv[2], **read_only_job(_maker, _kw))
