"""TEST INFRASTRUCTURE - the numpy twin of sx_derive (include/scythe_hip.h).

values64: the mids by tests/distribution.py::program_values64 (the rule k_project is held to bitwise), then the operations one by one
in float64; the composites go through oracle_np.th_*, so no formula is restated here.  values_xp: the same in longdouble from the
same float64 inputs widened exactly.

bound = c u S per register and point, the rule tests/physics.py states:
  u = 2^-53.
  c is counted, not fitted: the longest chain of rounded operations to the register.  A mid counts its longest term (the power of r
  with its product: r 1, r r 2, 1 / r 2, 1 / (r r) 3; one per factor) plus one per term for the sum.  An exactly rounded operation counts 1; EXP, LOG,
  POW, ATAN2 count 2 (a library call within 1 ulp of its already rounded argument); AHYP 8 and TEMPERATURE 9 as in tests/physics.py's
  CHAIN; the other composites from their expressions in oracle_np: DRY_DENSITY 3 (exp, product), PRESSURE 4 (the three run-time products
  of the vapour part, the sum), VAPOR_PRESSURE 2, L_V 3, ESAT_BUCK 9 (Tc; Tc / d; b -; * Tc; / (Tc + c); exp 2; a *; fw4 *).  R, Z and
  REF are inputs: 0.
  S is the first-order condition sum: one-at-a-time relative perturbations of 2^-30 of every input (every plane the mids name, r, z,
  every constant, every reference entry read) and of every register's own result with the rest held - so that a difference such as
  theta - 300 sees the rounding of what it subtracts.

mask: the points at which a SELECT argument lies within its own bound of zero have no defined expected value.  MIN, MAX, ABS and
AHYP are continuous and need none."""
import numpy as np

from oracle import oracle_np as O
from scythe_jl_amd import _lib as L
from tests import distribution as D

XP = np.longdouble
U = 2.0 ** -53
DELTA = XP(2.0) ** -30
NAME = {v: k for k, v in L.FN.items()}
COST = dict(exp=2, log=2, pow=2, atan2=2, r=0, z=0, ref=0, ahyp=8, temperature=9, esat_buck=9, dry_density=3, pressure=4, vapor_pressure=2, l_v=3)
R_COST = {0: 0, 1: 1, 2: 2, -1: 2, -2: 3}


def _apply(fn, a, b, c):
    with np.errstate(all="ignore"):
        if fn == "add": return a + b
        if fn == "sub": return a - b
        if fn == "mul": return a * b
        if fn == "div": return a / b
        if fn == "neg": return -a
        if fn == "abs": return np.abs(a)
        if fn == "min": return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(b < a, b, a)))
        if fn == "max": return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(b > a, b, a)))
        if fn == "sqrt": return np.sqrt(a)
        if fn == "select": return np.where(a >= 0.0, b, c)
        if fn == "exp": return np.exp(a)
        if fn == "log": return np.log(a)
        if fn == "pow": return a ** b
        if fn == "atan2": return np.arctan2(a, b)
        if fn == "ahyp": return O.th_ahyp(a)
        if fn == "temperature": return O.th_temperature(a, b, c)
        if fn == "esat_buck": return O.th_sat_pressure_liquid_buck(a, b)
        if fn == "dry_density": return O.th_dry_density(a)
        if fn == "pressure": return O.th_pressure(a, b, c)
        if fn == "vapor_pressure": return O.th_vapor_pressure(a, b)
        if fn == "l_v": return O.th_L_v(a)
    raise ValueError(fn)


def _mid_xp(data, r, fp, o):
    """program_values64 in the dtype of its inputs"""
    with np.errstate(all="ignore"):
        rr = r * r
        pw = {1: r, 2: rr, -1: 1 / r, -2: 1 / rr}
        q = np.zeros(data.shape[0], dtype=data.dtype)
        for t in range(len(fp.coef)):
            if int(fp.terms[t, 0]) != o:
                continue
            p, nf = int(fp.terms[t, 1]), int(fp.terms[t, 2])
            x = np.full(data.shape[0], fp.coef[t], dtype=data.dtype)
            if p != 0:
                x = x * pw[p]
            for f in range(nf):
                x = x * data[:, fp.terms[t, 3 + f] - 1, fp.terms[t, 7 + f]]
            q = q + x
    return q


def _run(fp, data, r, z, ref, dtype, scale=None):
    """every register at every point, [n_regs, N] in dtype; scale: {key: factor} with key ("plane", var, slot), ("r",), ("z",),
    ("const", k), ("ref", profile, slot) or ("reg", k): that input, or that register's result, is multiplied by the factor"""
    scale = scale or {}
    data = np.asarray(data, dtype=np.float64)
    data = data[:, :, None] if data.ndim == 2 else data
    N = data.shape[0]
    r = np.asarray(r, dtype=np.float64)
    z = np.zeros(1) if z is None else np.asarray(z, dtype=np.float64)
    lev = np.arange(N) % len(z)
    exact = dtype == np.float64 and not scale
    regs = []
    if exact:
        regs = [D.program_values64(data, r, (fp.coef, fp.terms, fp.n_mid), o) for o in range(fp.n_mid)]
    else:
        d = data.astype(dtype)
        for key, fac in scale.items():
            if key[0] == "plane":
                d[:, key[1] - 1, key[2]] *= fac
        rx = r.astype(dtype) * scale.get(("r",), 1)
        regs = [_mid_xp(d, rx, fp, o) * scale.get(("reg", o), 1) for o in range(fp.n_mid)]
    consts = [dtype(c) * scale.get(("const", k), 1) for k, c in enumerate(fp.consts)]
    fetch = lambda x: regs[x] if x >= 0 else consts[-1 - x]
    for i, (fn, a, b, c) in enumerate(fp.ops):
        name = NAME[int(fn)]
        if name == "r":
            v = r.astype(dtype) * scale.get(("r",), 1)
        elif name == "z":
            v = z.astype(dtype)[lev] * scale.get(("z",), 1)
        elif name == "ref":
            v = np.asarray(ref, dtype=np.float64)[a, b].astype(dtype)[lev] * scale.get(("ref", int(a), int(b)), 1)
        else:
            na = L.FN_ARITY.get(name, 2)
            v = _apply(name, *[fetch(int(x)) if k < na else None for k, x in enumerate((a, b, c))])
        v = np.broadcast_to(np.asarray(v, dtype=dtype), (N,)) * scale.get(("reg", fp.n_mid + i), 1)
        regs.append(v)
    return np.array([np.broadcast_to(np.asarray(x, dtype=dtype), (N,)) for x in regs], dtype=dtype).reshape(len(regs), N)


def values64(fp, data, r, z=None, ref=None):
    """[n_regs, N] float64: what k_derive holds in every register, operation for operation"""
    return _run(fp, data, r, z, ref, np.float64)


def values_xp(fp, data, r, z=None, ref=None):
    return _run(fp, data, r, z, ref, XP)


def chain(fp):
    """[n_regs] c of every register"""
    c = []
    for o in range(fp.n_mid):
        rows = fp.terms[fp.terms[:, 0] == o]
        c.append(max([R_COST[int(q[1])] + int(q[2]) for q in rows], default=0) + len(rows))
    for fn, a, b, cc in fp.ops:
        name = NAME[int(fn)]
        na = L.FN_ARITY.get(name, 2)
        deps = [c[int(x)] for x in (a, b, cc)[:na] if x >= 0]
        c.append(COST.get(name, 1) + max(deps, default=0))
    return np.array(c)


def inputs(fp, has_z):
    """the keys of _run's scale for every input the program reads"""
    keys = {("plane", int(q[3 + f]), int(q[7 + f])) for q in fp.terms for f in range(int(q[2]))}
    keys |= {("const", k) for k in range(len(fp.consts))}
    if any(int(q[1]) != 0 for q in fp.terms) or any(NAME[int(q[0])] == "r" for q in fp.ops):
        keys.add(("r",))
    for fn, a, b, _ in fp.ops:
        if NAME[int(fn)] == "z" and has_z:
            keys.add(("z",))
        if NAME[int(fn)] == "ref":
            keys.add(("ref", int(a), int(b)))
    return sorted(keys)


def bound(fp, data, r, z=None, ref=None):
    """(truth [n_regs, N] longdouble, bound [n_regs, N] float64 = c u S)"""
    truth = _run(fp, data, r, z, ref, XP)
    S = np.zeros(truth.shape, dtype=XP)
    n_regs = truth.shape[0]
    with np.errstate(all="ignore"):
        for key in inputs(fp, z is not None) + [("reg", k) for k in range(n_regs)]:
            S += np.abs(_run(fp, data, r, z, ref, XP, {key: 1 + DELTA}) - truth) / DELTA
    return truth, (chain(fp)[:, None] * U * S).astype(np.float64)


def mask(fp, truth, bnd):
    """[N] bool: a SELECT argument of the point lies within its own bound of zero"""
    m = np.zeros(truth.shape[1], dtype=bool)
    for fn, a, _, _ in fp.ops:
        if NAME[int(fn)] == "select" and a >= 0:
            m |= np.abs(truth[int(a)]) <= bnd[int(a)]
    return m
