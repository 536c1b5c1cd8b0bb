"""TEST INFRASTRUCTURE - the numpy twin of sx_spectrum, from the definition

    P_k(ring, level) = eps_k (a[2k] b[2k] + a[2k + 1] b[2k + 1]),   eps_0 = 1, eps_k = 2,
    ring kind    sum_level w_z[level] P_k(ring, level)
    domain kind  sum_ring 2 pi w_r[ring] (the ring value),   2 pi = w_l[ring] L[ring] (1 without an azimuth)

in numpy.longdouble (xp=True, the arbiter) or float64.  The harmonics a, b are tests/harmonics.py::harmonics at the Float64 ring radii
and level heights the gridpoints print, the weights tests/reduce.py::weights: neither is restated here."""
import numpy as np

from oracle import oracle_np as O
from tests import harmonics as H
from tests import reduce as R

XP = O.XP


def resolve(g, pairs):
    """pairs of ((var, slot), (var, slot)), var a name or a 1-based index, slot a name of H.SLOTS or its index -> int [n, 4]"""
    out = np.zeros((len(pairs), 4), dtype=np.int64)
    for i, pair in enumerate(pairs):
        for s, (var, slot) in enumerate(pair):
            out[i, 2 * s] = g.names.index(var) + 1 if isinstance(var, str) else int(var)
            out[i, 2 * s + 1] = H.SLOTS.index(slot) if isinstance(slot, str) else int(slot)
    return out


def all_pairs(g, variables=(1, 2)):
    """every legal slot pair of the given variables, a <= b: power spectra and cross spectra over all slots of the geometry"""
    planes = [(v, s) for v in variables for s in range(len(H.grid_slots(g)))]
    return [(planes[i], planes[j]) for i in range(len(planes)) for j in range(i, len(planes))]


def level_heights(g):
    """the Float64 level heights as the gridpoints print them (one "height" without a vertical)"""
    return np.asarray(g.cheb(g.names[0]).z, dtype=np.float64) if g.has_z else None


def spectrum(g, A, pairs, cell0=0, ncells=None, xp=True):
    """(ring [kDim + 1, rings, n_pairs], S_abs of it, domain [kDim + 1, n_pairs], S_abs of it) in the twin's precision;
    S_abs = sum |w| |a[blk]| |b[blk]| over everything that enters an entry (eps_k and the weights included)"""
    T = XP if xp else np.float64
    ncells = g.nc if ncells is None else ncells
    q = resolve(g, pairs)
    radii = O.mish_points(g.xmin, g.DX, cell0, ncells)
    c = H.harmonics(g, A, radii, level_heights(g), False, H.grid_slots(g), cell0, ncells, xp)        # [ring, level, k, v, slot]
    w_r, w_l, w_z = (w.astype(T) for w in R.weights(g, cell0, ncells, radii=radii))
    L = np.asarray(g.L[3 * cell0:3 * (cell0 + ncells)]).astype(T)
    w_ring = w_r * (w_l * L)
    eps = np.full(g.kDim + 1, 2, dtype=T)
    eps[0] = 1
    K, nr = g.kDim + 1, len(radii)
    ring, ring_abs = np.zeros((K, nr, len(q)), dtype=T), np.zeros((K, nr, len(q)), dtype=T)
    for p, (va, sa, vb, sb) in enumerate(q):
        a, b = c[:, :, :, va - 1, sa], c[:, :, :, vb - 1, sb]                                        # [ring, level, k]
        prod = a.real * b.real + a.imag * b.imag
        mag = np.abs(a.real) * np.abs(b.real) + np.abs(a.imag) * np.abs(b.imag)
        ring[:, :, p] = (eps[None, :] * np.einsum("z,rzk->rk", w_z, prod)).T
        ring_abs[:, :, p] = (eps[None, :] * np.einsum("z,rzk->rk", np.abs(w_z), mag)).T
    dom = np.einsum("r,krp->kp", w_ring, ring)
    dom_abs = np.einsum("r,krp->kp", np.abs(w_ring), ring_abs)
    return ring, ring_abs, dom, dom_abs


def product_program(g, pairs):
    """the one-term programs field(a) field(b), one output per pair, as tests/reduce.py::reduce takes them (slots of `physical`)"""
    q = resolve(g, pairs)
    slots = H.grid_slots(g)
    packed = np.zeros((len(q), 11), dtype=np.int32)
    for p, (va, sa, vb, sb) in enumerate(q):
        packed[p, :3] = p, 0, 2
        packed[p, 3:5] = va, vb
        packed[p, 7:9] = g.slots.index(slots[sa]), g.slots.index(slots[sb])
    return np.ones(len(q)), packed, len(q)


def product_terms(g, pairs):
    """the same programs as Grid.reduce takes them"""
    coef, packed, _ = product_program(g, pairs)
    return [(int(t[0]), 1.0, 0, [(int(t[3]), int(t[7])), (int(t[4]), int(t[8]))]) for t in packed]


def sixteen_pairs(g):
    """16 pairs for one call: the power spectrum of every slot, then cross pairs that use every slot of the geometry on either side
    and two variables where the grid has them"""
    ns, v2 = len(H.grid_slots(g)), min(2, g.V)
    pairs = [((1, s), (1, s)) for s in range(ns)]
    pairs += [((1, s), (v2, (s + 1) % ns)) for s in range(ns)]
    pairs += [((v2, s), (1, 0)) for s in range(ns)]
    pairs += [((v2, s), (v2, (s + 2) % ns)) for s in range(ns)]
    pairs += [((v2, s), (v2, s)) for s in range(ns)]
    pairs += [((1, (s + 1) % ns), (1, s)) for s in range(ns)]
    assert len(pairs) >= 16
    return pairs[:16]


# ----------------------------------------------------------------------------- the read-only job, here or in a child process
def read_only_job(maker, kw, steps=5):
    """tests/harmonics.py::read_only_job with spectrum (both kinds) between the steps: two runs of `steps` steps of
    cases.<maker>(**kw), the second with the calls: {state0, np10, state1, np11, ring, dom, same_state, same_np1}.  The SX_* switches
    come from the environment of this process."""
    from tests import cases
    case = getattr(cases, maker)(**kw)
    g = cases.oracle_grid(case)
    pairs = sixteen_pairs(g)
    out = {}
    for with_calls in (0, 1):
        hip = cases.HipModel(case)
        tile = hip.run.tiles[0]
        for s in range(steps):
            hip.step()
            if with_calls and s < steps - 1:
                st0, np0 = tile.get_state(), tile.var_np1
                ring, dom = tile.spectrum(pairs, "ring"), tile.spectrum(pairs, "domain")
                st1, np1 = tile.get_state(), tile.var_np1
                out["same_state"] = np.array(out.get("same_state", True) and st0.tobytes() == st1.tobytes())
                out["same_np1"] = np.array(out.get("same_np1", True) and np0.tobytes() == np1.tobytes())
        out["state%d" % with_calls], out["np1%d" % with_calls] = tile.get_state(), tile.var_np1
        hip.run.close()
    out["ring"], out["dom"] = ring, dom
    return out


def read_only_in_child(tmp_path, maker, kw, overrides, timeout=300):
    """read_only_job in a fresh `python -m tests.spectrum` with os.environ | overrides (tests/harmonics.py::read_only_in_child for
    this module's job): one child, under a time limit; a child that dies on a signal or hangs ends the session - nothing more starts
    on the GPU."""
    import json
    import os
    import subprocess
    import sys
    import pytest
    from tests.child_run import ROOT, _tail
    path = os.path.join(str(tmp_path), "spec_read_only_%s.npz" % "_".join(sorted(overrides)))
    cmd = [sys.executable, "-m", "tests.spectrum", json.dumps([maker, kw]), path]
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
