"""TEST INFRASTRUCTURE - the numpy twin of sx_vortex_harmonics / sx_vortex_check (include/scythe_hip.h): the azimuthal
harmonics of the state about a centre (x0, y0) that is not the grid's, in float64 (xp=False) or numpy.longdouble (xp=True, the arbiter).
Written from the definition with the weight functions of tests/evaluate.py and the ALL_K truncation: every sample f(x_j, y_j, z_l) is
formed at its height, the wind is rotated sample by sample, and the harmonic is the direct sum (1 / n_az) sum_j f_j e^{-i k phi_j} - not
the mode-space form of the kernels.  cos / sin phi_j are taken in the twin's precision except at the multiples of a quarter turn, which
are 0 and +-1 exactly (as in the library's table): a circle through r = 0 then has its sample AT r = 0 in either precision, where
lambda = 0 by rule, and not at 1e-20 with an arbitrary lambda.

Beside each harmonic the twin returns S, the mean over j of the sum of absolute terms of the sample, and a rounding bound.

Rounding bound of one harmonic (the same for every k: e^{-i k phi_j} comes from a table indexed exactly), u = 2^-53, first order in u.
Per sample and contributing component (a scalar; u and v of a wind field), the four parts of tests/parcels.py's velocity_bound with the
sample's own (r_j, lambda_j) - test_vortex.py holds the sums to P.velocity(..., with_bound=True) - with two changes:
  w      the vertical rows are formed on the host in extended precision and rounded once: u sum |a phi F w| = u S in place of d_w;
  r, lam the device forms the position itself.  x = x0 + rho c~: the table entry (u rho), the product (u rho), the sum (u |x|), the
         same for y, and hypot (2 u r):   d_r = u (4 rho + 4 r_j);   lambda = atan2 (2 u pi) moves by the position error over r_j:
         d_lam = u ((4 rho + 2 r_j) / r_j + 2 pi), 0 at r_j = 0 where lambda is 0 by rule.  |phi'| <= 1 in units of DX and
         |dF_blk / dlambda| <= 2 k:                      (d_r / DX) sum |a F w|  +  d_lam sum |a phi w| 2 k.
The mean over j of these per-sample bounds (|e^{-i k phi}| = 1; a wind output takes b_u + b_v, since |Re w|, |Im w| <= 1) is the first
part.  The roundings the device adds, each times the S it scales with (Sm = the mean over j of S):
  rotation   w = e^{i lambda} e^{-i phi}: two sincos (2 u), the table (u), two products and a sum (3 u), d_lam, and the product
             q g (u): (7 u + d_lam) S per sample, wind outputs only;
  update     H += f (q g): the table entry (u) and one fma per sample, VORTEX_CHUNK = 16 deep:      u (16 + 1) Sm
  chunks     the chunk partials are added in order:                                                  u ceil(n_az / 16) Sm
  vertical   the rows are applied after the sum, b_zDim fma deep; a wind output adds two products:   u (b_zDim + 1) Sm
  scale      the division by n_az, the motion term:                                                  2 u Sm + u |motion|
The longdouble twin's own error is 2^-11 of the bound."""
import numpy as np

from oracle import oracle_np as O
from tests import evaluate as E

XP = O.XP
EPS = 2.0 ** -53
CHUNK = 16
N_AZ_MAX, KMAX_MAX, FIELDS_MAX, LDS_DOUBLES = 4096, 32, 8, 8192


def _ty(xp):
    return XP if xp else np.float64


def phase_table(n_az, xp):
    """(cos, sin) of 2 pi m / n_az in the twin's precision, the multiples of a quarter turn exact"""
    T = _ty(xp)
    m = np.arange(n_az)
    ang = 2 * (O.PI_X if xp else np.pi) * m.astype(T) / T(n_az)
    c, s = np.cos(ang).astype(T), np.sin(ang).astype(T)
    q = (4 * m) % n_az == 0
    quad = (4 * m[q]) // n_az
    c[q] = np.array([1, 0, -1, 0], dtype=T)[quad]
    s[q] = np.array([0, 1, 0, -1], dtype=T)[quad]
    return c, s


def parse_fields(g, fields):
    """[(kind, var_a, var_b)] 0-based from names / 1-based indices / ("wind", u, v), and n_out"""
    def var(v):
        return g.names.index(v) if isinstance(v, str) else int(v) - 1
    out = []
    for f in fields:
        out.append((1, var(f[1]), var(f[2])) if isinstance(f, (tuple, list)) else (0, var(f), -1))
    return out, sum(1 + k for k, _, _ in out)


def circle_status(g, centre, radii):
    """the circle rule: 1 where the circle leaves [xmin, xmax] (one-tile patches), a few ulp of what enters absorbed"""
    d = float(np.hypot(centre[0], centre[1]))
    rho = np.asarray(radii, dtype=np.float64)
    tol = 8.0 * 2.0 ** -52 * (d + rho + g.xmax)
    out = d + rho > g.xmax + tol
    if g.xmin > 0:
        out |= np.abs(d - rho) < g.xmin - tol
    return out.astype(np.int32)


def refusal(g, centre, radii, n_az, kmax, fields, heights=None, motion=None):
    """the validation as the header lists it: a phrase of the library's message, or None for a call that is taken"""
    if not g.has_l:
        return "RL and RLZ grids only"
    vals = [np.asarray(centre, dtype=np.float64), np.asarray(radii, dtype=np.float64)]
    if not np.isfinite(vals[0]).all():
        return "the centre is NaN or Inf"
    if not np.isfinite(vals[1]).all():
        return "is NaN or Inf"
    if (vals[1] < 0).any():
        return "is negative"
    if n_az < 4 or n_az % 4 or n_az > N_AZ_MAX:
        return "n_az must be a multiple of 4 in 4 .. 4096"
    if kmax < 0 or 2 * kmax >= n_az or kmax > KMAX_MAX:
        return "kmax must be 0 .. 32 with 2 kmax < n_az"
    if not 1 <= len(fields) <= FIELDS_MAX:
        return "n_fields must be 1 .. 8"
    src, nacc = set(), 0
    for kind, va, vb in fields:                       # packed rows: kind, 1-based var_a, var_b
        if kind not in (0, 1):
            return "kind must be SX_VORTEX_SCALAR or SX_VORTEX_WIND"
        if not 1 <= va <= g.V:
            return "var_a"
        if kind == 1 and not 1 <= vb <= g.V:
            return "var_b"
        src |= {va} | ({vb} if kind == 1 else set())
        nacc += 4 if kind == 1 else 1
    Zb = g.b_zDim if g.has_z else 1
    if 2 * (g.kDim + 1) + 2 * nacc * (kmax + 1) * Zb + len(src) * Zb > LDS_DOUBLES or 4 * (kmax + 1) * Zb > LDS_DOUBLES:
        return "do not fit the LDS"
    if motion is not None and not np.isfinite(np.asarray(motion, dtype=np.float64)).all():
        return "the motion is NaN or Inf"
    if heights is not None:
        h = np.asarray(heights, dtype=np.float64)
        if not np.isfinite(h).all():
            return "NaN or Inf"
        if ((h < g.zmin) | (h > g.zmax)).any():
            return "outside"
    return None


def _sample_sums(g, Av, r, lam, xp):
    """per source variable: G [zm] = sum_blk sum_node a phi F and the absolute sums of the bound (float64), at one sample"""
    T = _ty(xp)
    n0 = E.node0_of(g, float(r))
    ph = E.radial_weights(g, r, n0, xp)[0]
    F = E.fourier_weights(g.kDim, lam, xp)[0]
    kk = np.concatenate([[0], np.repeat(np.arange(1, g.kDim + 1), 2)]).astype(np.float64)
    aph, aF = np.abs(ph).astype(np.float64), np.abs(F).astype(np.float64)
    d_F = 2.0 * EPS * (kk * np.pi + 2.0)
    out = {}
    for v, a_all in Av.items():
        a = a_all[:, :, n0:n0 + 4]                                            # [zm, blk, node]
        aa = np.abs(a).astype(np.float64)
        out[v] = dict(G=np.einsum("zbn,n,b->z", a, ph, F).astype(T), S=np.einsum("zbn,n,b->z", aa, aph, aF),
                      phi=np.einsum("zbn,b->z", aa, aF), F=np.einsum("zbn,n,b->z", aa, aph, d_F), lam=np.einsum("zbn,n,b->z", aa, aph, 2.0 * kk))
    return out


def harmonics(g, A, centre, radii, heights=None, fields=("h",), n_az=16, kmax=4, motion=None, xp=True):
    """(c complex [n_out, n_rho, n_z, kmax + 1] in the twin's precision, S float64 [n_out, n_rho, n_z], bound of the same shape,
    status int32 [n_rho]); the rows of circles outside are NaN.  A [S_patch, V] Float64 in the reference layout."""
    T = _ty(xp)
    CT = np.clongdouble if xp else np.complex128
    fl, n_out = parse_fields(g, fields)
    radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    hs = [0.0] if heights is None else list(np.asarray(heights, dtype=np.float64).reshape(-1))
    K, nz, Zb = kmax + 1, len(hs), g.b_zDim
    status = circle_status(g, centre, radii)
    c = np.full((n_out, len(radii), nz, K), np.nan, dtype=CT)
    S, B = np.full((n_out, len(radii), nz), np.nan), np.full((n_out, len(radii), nz), np.nan)
    srcs = sorted({v for _, a, b in fl for v in (a, b) if v >= 0})
    Av = {v: A[:, v].reshape(g.b_zDim, g.K2, g.b_rDim).astype(T) for v in srcs}
    W = {v: (np.stack([E.vertical_weights(g, g.names[v], z, xp)[0] for z in hs]) if g.has_z else np.ones((1, 1), dtype=T)) for v in srcs}
    aW = {v: np.abs(W[v]).astype(np.float64) for v in srcs}
    ct, st = phase_table(n_az, xp)
    kj = (np.arange(K)[:, None] * np.arange(n_az)[None, :]) % n_az
    ek = (ct[kj] - 1j * st[kj]).astype(CT)                                    # [k, j] e^{-i k phi_j}
    ncol = Zb * g.K2
    d_phi = EPS * (2.0 * max(abs(g.xmin), abs(g.xmax)) / g.DX + 14.0)
    x0, y0 = T(centre[0]), T(centre[1])
    mo = None if motion is None else (T(motion[0]), T(motion[1]))
    tail = EPS * (CHUNK + 1 + -(-n_az // CHUNK) + Zb + 1 + 2)
    for i, rho in enumerate(radii):
        if status[i]:
            continue
        f = np.zeros((n_out, nz, n_az), dtype=T)
        Sj, Bj = np.zeros((n_out, nz, n_az)), np.zeros((n_out, nz, n_az))
        for j in range(n_az):
            x, y = x0 + T(rho) * ct[j], y0 + T(rho) * st[j]
            r = np.hypot(x, y)
            lam = T(0) if r == 0 else np.arctan2(y, x)
            if float(lam) <= -np.pi:
                lam = T(np.pi)
            rf = float(r)
            d_r = EPS * (4.0 * rho + 4.0 * rf)
            d_lam = 0.0 if rf == 0.0 else EPS * ((4.0 * rho + 2.0 * rf) / rf + 2.0 * np.pi)
            sums = _sample_sums(g, Av, r, lam, xp)
            val, Sv, Bv = {}, {}, {}
            for v in srcs:
                q = sums[v]
                val[v] = W[v] @ q["G"]                                         # [n_z]
                Sv[v] = aW[v] @ q["S"]
                Bv[v] = (EPS * (ncol + 6.0) + EPS) * Sv[v] + (d_phi + d_r / g.DX) * (aW[v] @ q["phi"]) + aW[v] @ q["F"] + d_lam * (aW[v] @ q["lam"])
            wre = np.cos(lam) * ct[j] + np.sin(lam) * st[j]
            wim = np.sin(lam) * ct[j] - np.cos(lam) * st[j]
            o = 0
            for kind, va, vb in fl:
                if kind == 0:
                    f[o, :, j], Sj[o, :, j], Bj[o, :, j] = val[va], Sv[va], Bv[va]
                    o += 1
                    continue
                f[o, :, j] = val[va] * wre - val[vb] * wim
                f[o + 1, :, j] = val[va] * wim + val[vb] * wre
                for t, (qa, qb) in enumerate(((abs(float(wre)), abs(float(wim))), (abs(float(wim)), abs(float(wre))))):
                    Sj[o + t, :, j] = qa * Sv[va] + qb * Sv[vb]
                    Bj[o + t, :, j] = Bv[va] + Bv[vb] + (7.0 * EPS + d_lam) * Sj[o + t, :, j]
                o += 2
        c[:, i] = np.einsum("ozj,kj->ozk", f.astype(CT), ek) / T(n_az)
        Sm = Sj.mean(axis=2)
        S[:, i] = Sm
        B[:, i] = Bj.mean(axis=2) + tail * Sm
        o = 0
        for kind, va, vb in fl:
            if kind == 1:
                B[o:o + 2, i] += EPS * Sm[o:o + 2]                               # the second product of the vertical step
                if mo is not None:
                    B[o:o + 2, i] += EPS * (abs(float(mo[0])) + abs(float(mo[1])))
                    if kmax >= 1:
                        c[o, i, :, 1] -= (mo[0] - 1j * mo[1]) / 2                    # eps_1 c_1 = cx - i cy
                        c[o + 1, i, :, 1] -= (mo[1] + 1j * mo[0]) / 2                # eps_1 c_1 = cy + i cx
            o += 1 + kind
    return c, S, B, status


def state_from_values(case, values):
    """A [S_patch, V] of the gridpoint values values(points) on the case's grid, through the oracle's forward transforms"""
    from tests import cases
    return np.array(cases.OracleModel(dict(case, ic=values)).A)


def cartesian_wind(p, U, V):
    """the grid's (radial, tangential) components of the Cartesian wind (U, V) at gridpoints p (columns r, lambda, ...)"""
    c, s = np.cos(p[:, 1]), np.sin(p[:, 1])
    return U * c + V * s, -U * s + V * c


def sample_radii(g, centre):
    """rho = 0, a circle through r = 0, one tangent to the outer edge, a duplicate, one outside, two ordinary ones"""
    d = float(np.hypot(centre[0], centre[1]))
    return np.array([0.0, d, 0.37 * (g.xmax - d), g.xmax - d, 0.81 * (g.xmax - d), 0.37 * (g.xmax - d), 1.02 * (g.xmax - d) + 0.3 * g.DX])


# ----------------------------------------------------------------------------- the read-only job, in a child process
def read_only_job(maker, kw, steps=6):
    """Two runs of `steps` steps of cases.<maker>(**kw); the second calls vortex_profile after every step: {state0, np10, state1,
    np11, tangential}.  The SX_* switches come from the environment of this process."""
    from tests import cases
    case = getattr(cases, maker)(**kw)
    out = {}
    for with_calls in (0, 1):
        hip = cases.HipModel(case)
        tile = hip.run.tiles[0]
        DX = (hip.gp.xmax - hip.gp.xmin) / hip.gp.num_cells
        for s in range(steps):
            hip.step()
            if with_calls:
                st0, np0 = tile.get_state(), tile.var_np1
                prof = hip.run.vortex_profile(("u", "v"), centre=(0.4 * DX, -0.3 * DX), radii=DX * np.arange(4),
                                              heights=[0.5 * (hip.gp.zmin + hip.gp.zmax)] if "Z" in hip.gp.geometry else None)
                st1, np1 = tile.get_state(), tile.var_np1
                out["same_state"] = np.array(bool(out.get("same_state", True)) and st0.tobytes() == st1.tobytes())
                out["same_np1"] = np.array(bool(out.get("same_np1", True)) and np0.tobytes() == np1.tobytes())
        out["state%d" % with_calls], out["np1%d" % with_calls] = tile.get_state(), tile.var_np1
        hip.run.close()
    out["tangential"] = prof.tangential
    return out


def read_only_in_child(tmp_path, maker, kw, overrides, timeout=300):
    """read_only_job in a fresh `python -m tests.vortex` with os.environ | overrides, as tests/child_run.py runs its jobs: one child,
    under a time limit; a child that dies on a signal or hangs ends the session - nothing more starts on the GPU."""
    import json
    import os
    import subprocess
    import sys
    import pytest
    from tests.child_run import ROOT, _tail
    path = os.path.join(str(tmp_path), "vortex_read_only_%s.npz" % "_".join(sorted(overrides)))
    cmd = [sys.executable, "-m", "tests.vortex", json.dumps([maker, kw]), path]
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
