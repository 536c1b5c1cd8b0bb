"""TEST INFRASTRUCTURE - the numpy twin of sx_reduce / sx_reduce_weights in numpy.longdouble (the arbiter): integrals and azimuthal
means of field products from Float64 fields and Float64 gridpoints.  The weights come from the definition (include/scythe_hip.h):
Gauss-Legendre 5:8:5 on every cell times the radius the gridpoints print, 2 pi / L, Clenshaw-Curtis from the cosine formula - never
from the library.  Built on oracle_np's ring tables and mish points."""
import numpy as np

from oracle import oracle_np as O

XP = O.XP
PI_X = XP(4) * np.arctan(XP(1))

# |got - truth| <= BOUND * S_abs wherever a device or library number is held to a longdouble number, S_abs = sum |w term| per output
# (azimuth: (1 / L) sum |term| per entry).  Derived, not measured: a term passes through at most 16 roundings - up to 3 for the factor
# product, 1 for coef, up to 3 for r^p, up to 6 for the weights and their product, the rest the widenings - and the same amount again
# is allowed for the two summation stages (double-double: their own error is of second order).
BOUND = 32.0 * 2.0 ** -53


def cc_weights(N):
    """Clenshaw-Curtis weights of the N Chebyshev-Gauss-Lobatto points cos(j pi / (N - 1)) on [-1, 1] (they sum to 2)"""
    n = N - 1
    j = np.arange(N).astype(XP)
    s = np.ones(N, dtype=XP)
    for k in range(1, n // 2 + 1):
        b = XP(1) if 2 * k == n else XP(2)
        s -= b / XP(4 * k * k - 1) * np.cos(XP(2 * k) * j * PI_X / XP(n))
    c = np.full(N, 2, dtype=XP)
    c[0] = c[-1] = 1
    return c / XP(n) * s


def weights(g, cell0=0, ncells=None, radii=None):
    """(w_r [rings], w_l [rings], w_z [levels]) of the tile in longdouble; radii: the Float64 ring radii (default: mish_points)"""
    ncells = g.nc if ncells is None else ncells
    DX = (XP(g.xmax) - XP(g.xmin)) / XP(g.nc)
    r = O.mish_points(g.xmin, g.DX, cell0, ncells) if radii is None else np.asarray(radii, dtype=np.float64)
    gw = np.tile(np.array([5, 8, 5], dtype=XP) / XP(18), ncells)
    w_r = DX * gw * (r.astype(XP) if g.has_l else XP(1))
    L = np.asarray(g.L[3 * cell0:3 * (cell0 + ncells)])
    w_l = XP(2) * PI_X / L.astype(XP) if g.has_l else np.ones(3 * ncells, dtype=XP)
    w_z = cc_weights(g.zDim) * (XP(g.zmax) - XP(g.zmin)) / XP(2) if g.has_z else np.ones(1, dtype=XP)
    return w_r, w_l, w_z


def term_values(data, r, coef, packed):
    """[n_terms, N] longdouble: coef r^p prod field at every point; data [N, V, D] or [N, V] Float64, r [N] Float64"""
    data = np.asarray(data)
    data = data[:, :, None] if data.ndim == 2 else data
    rx = np.asarray(r, dtype=np.float64).astype(XP)
    out = np.zeros((len(coef), data.shape[0]), dtype=XP)
    for t in range(len(coef)):
        p, nf = int(packed[t, 1]), int(packed[t, 2])
        x = np.full(data.shape[0], XP(coef[t]))
        if p > 0:
            x = x * rx ** p
        elif p < 0:
            x = x / rx ** (-p)
        for f in range(nf):
            x = x * data[:, packed[t, 3 + f] - 1, packed[t, 7 + f]].astype(XP)
        out[t] = x
    return out


def reduce(g, data, points, program, kind="domain", cell0=0, ncells=None):
    """What sx_reduce returns, and S_abs, in longdouble.  program = (coef, packed [n, 11], n_out) as pack_reduce_program gives it;
    points: the tile's gridpoints (column 0 = r).  domain: ([n_out], [n_out]); azimuth: ([rings, levels, n_out]) twice."""
    coef, packed, n_out = program
    ncells = g.nc if ncells is None else ncells
    pts = np.asarray(points, dtype=np.float64)
    r = pts.reshape(len(pts), -1)[:, 0]
    nz = g.zDim
    L = np.asarray(g.L[3 * cell0:3 * (cell0 + ncells)])
    start = np.concatenate([[0], np.cumsum(L * nz)])
    assert start[-1] == len(r)
    w_r, w_l, w_z = weights(g, cell0, ncells, radii=r[start[:-1]])
    tv = term_values(data, r, coef, packed)
    nr = len(L)
    if kind == "azimuth":
        res, sabs = np.zeros((nr, nz, n_out), dtype=XP), np.zeros((nr, nz, n_out), dtype=XP)
    else:
        res, sabs = np.zeros(n_out, dtype=XP), np.zeros(n_out, dtype=XP)
    for t in range(len(coef)):
        o = int(packed[t, 0])
        for i in range(nr):
            blk = tv[t, start[i]:start[i + 1]].reshape(int(L[i]), nz)
            if kind == "azimuth":
                res[i, :, o] += blk.sum(axis=0) / XP(int(L[i]))
                sabs[i, :, o] += np.abs(blk).sum(axis=0) / XP(int(L[i]))
            else:
                w = w_r[i] * w_l[i] * w_z
                res[o] += (blk.sum(axis=0) * w).sum()
                sabs[o] += (np.abs(blk).sum(axis=0) * np.abs(w)).sum()
    return res, sabs


def check(got, truth, sabs, what=""):
    """assert |got - truth| <= BOUND S_abs everywhere, after printing the worst ratio to the bound"""
    err = np.abs(np.asarray(got).astype(XP) - truth)
    lim = XP(BOUND) * sabs
    worst = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), np.where(err > 0, np.inf, 0))))
    print("%s: worst |got - truth| / (32 ulp S_abs) = %.3g" % (what, worst))
    assert (err <= lim).all(), (what, worst)


def random_program(g, seed, n_terms=12, n_out=5, source="physical"):
    """A seeded program that uses every slot of the geometry (values only for source="state"), p from -2 to 2 and 0 to 4 factors, as
    Grid.reduce takes it"""
    rng = np.random.default_rng(seed)
    D = 1 if source == "state" else g.D
    terms = []
    for t in range(n_terms):
        nf = t % 5
        p = (t % 5) - 2 if t < 10 else int(rng.integers(-2, 3))
        facs = [(int(rng.integers(1, min(g.V, 2) + 1)), int((t + f) % D)) for f in range(nf)]      # 2 variables x 7 slots <= 16 planes
        terms.append((t % n_out, float(rng.uniform(-2.0, 2.0)), p, facs))
    return terms


# ----------------------------------------------------------------------------- the read-only job, here or in a child process
def read_only_job(maker, kw, before=4, after=3):
    """Two runs of cases.<maker>(**kw): `before` steps (with SX_GRAPH=1 the last two are graph replays) and a tileTransform!, then (second run only) both kinds of reduce on both sources,
    then `after` more.
    {state0 / np10 / phys0: before the reduce calls, state1 / np11 / phys1: after them (second run), end0 / end1: var_np1 at the end
    of the run without / with the calls, dom, azi: what the calls returned}"""
    from tests import cases
    case = getattr(cases, maker)(**kw)
    g = cases.oracle_grid(case)
    prog = random_program(g, 5)
    out = {}
    for with_reduce in (0, 1):
        hip = cases.HipModel(case)
        tile = hip.run.tiles[0]
        for _ in range(before):
            hip.step()
        tile.tileTransform_()
        if with_reduce:
            out["state0"], out["np10"], out["phys0"] = tile.get_state(), tile.var_np1, tile.physical
            out["dom"] = tile.reduce(prog, "domain")
            out["azi"] = tile.reduce(prog, "azimuth")
            tile.reduce(random_program(g, 6, source="state"), "domain", "state")
            tile.reduce(random_program(g, 6, source="state"), "azimuth", "state")
            out["state1"], out["np11"], out["phys1"] = tile.get_state(), tile.var_np1, tile.physical
        for _ in range(after):
            hip.step()
        out["end%d" % with_reduce] = tile.var_np1
        hip.run.close()
    return out


def read_only_in_child(tmp_path, maker, kw, overrides, timeout=300):
    """read_only_job in a fresh `python -m tests.reduce` with os.environ | overrides (the pattern of tests/evaluate.py): one child,
    under a time limit; a child that dies on a signal or hangs ends the session - nothing more starts on the GPU."""
    import json
    import os
    import subprocess
    import sys
    import pytest
    from tests.child_run import ROOT, _tail
    path = os.path.join(str(tmp_path), "reduce_read_only_%s.npz" % "_".join(sorted(overrides)))
    cmd = [sys.executable, "-m", "tests.reduce", json.dumps([maker, kw]), path]
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
