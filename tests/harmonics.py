"""TEST INFRASTRUCTURE - the numpy twin of sx_harmonics and sx_evaluate_band, from the definition

    c_k(r, z) = sum_node sum_zm (A[zm, 2k, node] + i A[zm, 2k + 1, node]) phi_node(r) Wz[zm](z)

with the basis functions of tests/evaluate.py (radial_weights, vertical_weights, kcap_of, node0_of), in float64 (xp=False) or in
numpy.longdouble (xp=True, the arbiter).  A is Float64 in the reference layout [b_zDim, 1 + 2 kDim, b_rDim] per variable: block 0 is
k = 0, blocks 2k - 1 / 2k the real / imaginary part of wavenumber k (the device's padding block does not exist there)."""
import numpy as np

from oracle import oracle_np as O
from tests import evaluate as E

XP = O.XP
SLOTS = ("u", "r", "rr", "z", "zz")
_RAD = {"u": 0, "r": 1, "rr": 2, "z": 0, "zz": 0}       # radial weights: phi, phi', phi''
_ROW = {"u": 0, "r": 0, "rr": 0, "z": 1, "zz": 2}       # vertical operator row


def grid_slots(g):
    return SLOTS if g.has_z else SLOTS[:3]


def harmonics(g, A, radii, heights=None, all_k=False, slots=("u",), cell0=0, ncells=None, xp=True):
    """complex [n_r, n_z, kDim + 1, V, n_slots] in the twin's precision; entries above the wavenumber cap of a radius are zero"""
    T = XP if xp else np.float64
    CT = np.clongdouble if xp else np.complex128
    radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    hs = [0.0] if heights is None else list(np.asarray(heights, dtype=np.float64).reshape(-1))
    slots = [s for s in SLOTS if s in slots]
    out = np.zeros((len(radii), len(hs), g.kDim + 1, g.V, len(slots)), dtype=CT)
    Av = [A[:, vi].reshape(g.b_zDim, g.K2, g.b_rDim) for vi in range(g.V)]
    wz = {}
    for vi, v in enumerate(g.names):
        key = (g.BCB[v], g.BCT[v]) if g.has_z else None
        if key not in wz:
            wz[key] = (np.stack([E.vertical_weights(g, v, z, xp) for z in hs]) if g.has_z
                       else np.array([[[1], [0], [0]]], dtype=T))                         # [n_z, 3, zm]
    for ir, r in enumerate(radii):
        n0 = E.node0_of(g, r, cell0, ncells)
        PH = E.radial_weights(g, r, n0, xp)
        kc = E.kcap_of(g, r, all_k)
        for vi, v in enumerate(g.names):
            a = Av[vi][:, :1 + 2 * kc, n0:n0 + 4].astype(T)                                # [zm, blk, node]
            W = wz[(g.BCB[v], g.BCT[v]) if g.has_z else None]
            for si, s in enumerate(slots):
                coef = np.einsum("zbn,n->zb", a, PH[_RAD[s]])                             # [zm, blk]
                val = W[:, _ROW[s], :] @ coef                                              # [n_z, blk]
                out[ir, :, 0, vi, si] = val[:, 0]
                out[ir, :, 1:kc + 1, vi, si] = val[:, 1::2] + 1j * val[:, 2::2]
    return out


def band_coefficients(g, A, kmin, kmax):
    """A with every block outside kmin <= k <= kmax set to zero (exact: a zero coefficient adds an exact zero in the twin)"""
    a = A.reshape(g.b_zDim, g.K2, g.b_rDim, g.V).copy()
    k_of = (np.arange(g.K2) + 1) // 2
    a[:, (k_of < kmin) | (k_of > kmax)] = 0.0
    return a.reshape(A.shape)


def evaluate_band(g, A, points, kmin, kmax, all_k=False, cell0=0, ncells=None, xp=True):
    """sx_evaluate_band's twin: tests/evaluate.py's evaluate on the band's coefficients"""
    return E.evaluate(g, band_coefficients(g, A, kmin, kmax), points, all_k, cell0, ncells, xp)


def from_harmonic(g, c, k, lam, xp=True):
    """eps_k Re(c_k e^{i k lambda}) in the slots of `physical`: c [n, V, 5 or 3] = the harmonic k in the slots u r rr [z zz] at each
    point's (r, z), lam [n] -> [n, V, D]; the l, ll slots are eps_k Re(i k c e^{..}), eps_k Re(-k^2 c e^{..})"""
    T = XP if xp else np.float64
    ph = T(k) * np.asarray(lam, dtype=T)
    e = (np.cos(ph) + 1j * np.sin(ph))[:, None]
    eps = 1 if k == 0 else 2
    sl = {s: i for i, s in enumerate(g.slots)}
    out = np.zeros((len(lam), g.V, g.D), dtype=T)
    for si, s in enumerate(grid_slots(g)):
        out[:, :, sl[s]] = eps * (c[:, :, si] * e).real
    if g.has_l:
        out[:, :, sl["l"]] = eps * (1j * k * c[:, :, 0] * e).real
        out[:, :, sl["ll"]] = eps * (-(k * k) * c[:, :, 0] * e).real
    return out


def ring_dft(u, lam):
    """(1 / L) sum_j u_j e^{-i k lambda_j} for k = 0 .. L // 2 (the definition, in the precision of u and lam): u [L, ...] -> [K, ...]"""
    L = len(lam)
    k = np.arange(L // 2 + 1).astype(lam.dtype)
    ph = k[:, None] * lam[None, :]
    W = (np.cos(ph) - 1j * np.sin(ph)) / lam.dtype.type(L)
    return np.tensordot(W, u, axes=(1, 0))


def ring_angles_xp(g, ring):
    L = int(g.L[ring])
    return XP(g.off[ring]) + 2 * O.PI_X * np.arange(L, dtype=XP) / XP(L)


def rel_err(a, t):
    """max |a - t| / max |t| against the longdouble truth t"""
    t = np.asarray(t)
    CT = np.clongdouble if np.iscomplexobj(t) else XP
    return float(np.abs(np.asarray(a, dtype=CT) - t).max() / max(float(np.abs(t).max()), 1e-300))


def sample_radii(g, n, seed, cell0=0, ncells=None):
    """n unsorted radii of the tile: its two ends, every cell edge, ring radii, random ones and one duplicate"""
    rng = np.random.default_rng(seed)
    ncells = g.nc if ncells is None else ncells
    lo, hi = E.tile_range(g, cell0, ncells)
    edges = g.xmin + np.arange(cell0 + 1, cell0 + ncells) * g.DX
    rings = O.mish_points(g.xmin, g.DX, cell0, ncells)[::2][:8]
    r = np.concatenate([[lo, hi], edges, rings])[:n - 1]
    r = np.concatenate([r, rng.uniform(lo, hi, n - 1 - len(r))])
    r = np.concatenate([r, r[5:6]])
    return rng.permutation(r)


# ----------------------------------------------------------------------------- the read-only job, here or in a child process
def read_only_job(maker, kw, steps=5):
    """Two runs of `steps` steps of cases.<maker>(**kw); the second calls harmonics and evaluate(k_band=...) between the steps:
    {state0, np10, state1, np11, got, band}.  The SX_* switches come from the environment of this process."""
    from tests import cases
    case = getattr(cases, maker)(**kw)
    g = cases.oracle_grid(case)
    radii = sample_radii(g, 20, seed=5)
    heights = np.linspace(g.zmin, g.zmax, 5) if g.has_z else None
    pts = E.scattered_points(g, 100, seed=31)
    out = {}
    for with_calls in (0, 1):
        hip = cases.HipModel(case)
        tile = hip.run.tiles[0]
        for s in range(steps):
            hip.step()
            if with_calls and s < steps - 1:
                st0, np0 = tile.get_state(), tile.var_np1
                got = tile.harmonics(radii, heights, slots=grid_slots(g))
                band = tile.evaluate(pts, k_band=(1, 2))
                st1, np1 = tile.get_state(), tile.var_np1
                out["same_state"] = np.array(out.get("same_state", True) and st0.tobytes() == st1.tobytes())
                out["same_np1"] = np.array(out.get("same_np1", True) and np0.tobytes() == np1.tobytes())
        out["state%d" % with_calls], out["np1%d" % with_calls] = tile.get_state(), tile.var_np1
        hip.run.close()
    out["got"], out["band"] = np.ascontiguousarray(got), band
    return out


def read_only_in_child(tmp_path, maker, kw, overrides, timeout=300):
    """read_only_job in a fresh `python -m tests.harmonics` with os.environ | overrides, as tests/child_run.py runs its jobs: one
    child, under a time limit; a child that dies on a signal or hangs ends the session - nothing more starts on the GPU."""
    import json
    import os
    import subprocess
    import sys
    import pytest
    from tests.child_run import ROOT, _tail
    path = os.path.join(str(tmp_path), "harm_read_only_%s.npz" % "_".join(sorted(overrides)))
    cmd = [sys.executable, "-m", "tests.harmonics", json.dumps([maker, kw]), path]
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
