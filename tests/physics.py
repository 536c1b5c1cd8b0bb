"""The extended-precision twin of ONE sx_physics call (TEST INFRASTRUCTURE): plain numpy, longdouble, no GPU.

sx_physics reads `physical` and writes var_np1 (and, for the shallow-water sets, the diagnostic w into physical[:, 5, 0]):
the equation set's tendency, the explicit step (Euler at t = 1, AB2 at t = 2, AB3 from t = 3; the history restarts at t = 1),
then the semi-implicit adjustment and condensation_adjustment where the case has them.  Twin(case) computes the same from the
same Float64 bits, widened exactly, with every operation in longdouble: oracle_np.tendency / explicit_timestep /
Model._semiimplicit / condensation_adjustment follow the precision of their input, so no formula is stated here.

Twin.bound is c * u * S per point and variable: u = 2^-53, S the first-order condition sum  sum_i |x_i d(out)/d(x_i)|  over
everything the formula reads (every (variable, slot) plane, r, z, cos lambda, sin lambda, the parameters, the reference-state
profiles, the thermodynamic constants, the history entries, dt) and over the rounded exp / sqrt / pow results of the moist
thermodynamics that the sets subtract from one another (oracle_np.INTERMEDIATE: in rho_t - rhobar the reference density cancels
exactly, its rounding does not, so the inputs alone miss it by 10^3), taken by one-at-a-time relative perturbations of size 2^-30
of the twin itself.  Through a column operator the sum is level-separated, sum_j |M_ij| |dx_j| (not |sum_j M_ij dx_j|): the
twin records what each operator application is fed (oracle_np's col_ops hook), so one perturbed evaluation per input, with
the operators held at their unperturbed output, gives the input's pointwise effect and the deviation dx of each operator's
input; one evaluation per operator, its output shifted, gives the pointwise effect of that output on var_np1 and on the
inputs of the operators after it.  Chained with absolute values these are the level-separated sums (the triangle inequality
where an input reaches var_np1 on more than one path: never less than perturbing level by level, and nz times cheaper).

The entries of the column operators are inputs as well (sum_j |M_ij x_j| per operator, chained the same way), and the twin is
given the rounded operators of whatever it is compared with (semi_operators): a perturbation of dt or Pxi_bar leaves them alone.

c is counted, not fitted: CHAIN below, plus nz for every column operator on the path.

Data-dependent branches (Cd(U10), |w|, the min / max clamps of q_condensation, the whole-column clamp of
condensation_adjustment, ahyp, f_ice, autoconversion): oracle_np logs the quantity whose sign decides each; a point whose margin
is within c * u * (condition sum of the margin) of zero has no defined expected value and is masked - with its whole column where
the set has column operators.  Not logged: the max(q, 0) clamps of th_collection, th_f_ventilation, th_rain_evaporation and
th_sedimentation.  Each clamps a product of non-negative factors (or 1.6 + such a product), is continuous, and a flip moves the
result by no more than the margin itself - far inside the bound - while at q_r = 0 exactly both sides give 0."""
import functools

import numpy as np

from oracle import oracle_np as O
from tests import cases, linear_sw, rainfall

XP = np.longdouble
U = 2.0 ** -53
DELTA = XP(2.0) ** -30

SW_SETS = ("Oneway_ShallowWater_Slab", "Twoway_ShallowWater_Slab", "Oneway_ShallowWater_HeightResolvedBL")
THERMO_SETS = ("Euler_test", "rainfall_test")

# Depth of the longest chain of rounded operations from an input to var_np1, counted from the formulas (oracle_np.tendency,
# the same expressions as csrc/sx_physics.hip).  Common tail, the AB3 step: 23 e (1), 16 e1 and the difference (2), 5 e2 and the
# sum (3), ts / 12 (4), the product (5), u + (6).  exp / log / pow / sqrt count 2 (a correctly rounded sqrt and a libm call
# within 1 ulp of its already rounded argument).
STEP = 6
CHAIN = {
    # -(c0 u_r) + (K u_rr): product, sum
    "LinearAdvection1D": 2 + STEP,
    # K ((h_r / r) + h_rr + h_zz): quotient, two sums, product, the sum with the advection terms
    "LinearAdvectionRZ": 5 + STEP,
    # r r, h_ll / (r r), two sums, K (...), e +=
    "LinearAdvectionRL": 6 + STEP,
    "LinearAdvectionRLZ": 6 + STEP,
    # -H ((u / r) + u_r + (v_l / r)) is 4; K ((u_r / r) + u_rr + (u_ll / (r r))): r r, quotient, two sums, product, sum
    "LinearShallowWater1D": 3 + STEP,
    "LinearShallowWaterRL": 6 + STEP,
    # drag: ub^2 + vb^2 (2), sqrt (2), 0.78 (1), Cd U (1), ub (1), / Hb (1), then the six sums of e3;
    # w_: w is 4, |w| / 2 - w (2), (ug - ub) product, / Hb (2), sums.  Twoway: one more product and sum in e0
    "Oneway_ShallowWater_Slab": 14 + STEP,
    "Twoway_ShallowWater_Slab": 15 + STEP,
    # surface flux: sfcu (3), u10 (1), u10^2 + v10^2 (2), sqrt (2), Cd = 4.4e-4 sqrt(U10) (3), Cd U10 u10 (2): 13, then the
    # operator (+ nz), the six sums of e3: 19; interior flux: l (4), l^2 (1), S (4, in parallel), Kv (1), Kv ubz (1): shorter.
    # The matrix-core kernels multiply by 1 / r and (1 / r)^2 where the formula divides: + 2
    "Oneway_ShallowWater_HeightResolvedBL": 21 + STEP,
    # explicit: adv (3), K (u_rr + u_zz) (2), two sums: 7
    "LinearAcousticRZ": 7 + STEP,
    # q_v = ahyp (add 1, squares and sum 3, sqrt 2, two sums 2: 8); Cf (2); the exponent q_v Rv / Cf (2), pow (2), T_0 Tf rf qf (3):
    # 17; P_s (3); P_qv: log(Tk / T_0) (3), Cvv (1), two sums (2), P_s (1), sum (1): 28; pressure_gradient: product, two sums (3);
    # / rho_t (1); the sums of e[4] (3): 35
    "Euler_test": 35 + STEP,
    # Tk (17) -> sat_pressure (Tc 1, the exponent 4, exp 2, a (1), fw4 (1): 26) -> its dT (T1, T2: 6) -> dqsdT (4) -> Q_s (2) ->
    # q_cond = qss / (1 + Q_s) (2), the clamps, invtau (1): 41 -> s_cond: log(e / sat_e) (3), Rv (1), sum (1), q_cond (1): 47 ->
    # the sums of e[0] (3): 50
    "rainfall_test": 50 + STEP,
}
# semiimplicit_adjustment after the explicit step: star = x - (the AB3 sum of impdot: 6) - ts I (1) + ts 0.75 I1 (2): 9; the
# d/dz operator (+ nz), tau pxi (2), - star_w (1), the Helmholtz operator (+ nz), xi* - tau w_z (2): 14 + 2 nz
SEMI = 14
# condensation_adjustment on var_np1: Tk again (17), q_sat (26 + 2), Q_s (as above: 38), q_cond (3), s_condensation (6),
# s + tau_r (...) (2): 51
CONDENSATION = 51


def chain(case, nz):
    """(c, number of column operators on the longest path) of the case."""
    eq, semi = case["eq"], case.get("semiimplicit", False)
    c, nops = CHAIN[eq], 0
    if eq == "Oneway_ShallowWater_HeightResolvedBL":
        nops = 1
    if eq == "rainfall_test":
        nops = 1                      # the sedimentation flux's d/dz
        c += CONDENSATION
    if semi:
        nops += 2
        c += SEMI
    return c + nops * nz, nops


# ----------------------------------------------------------------------------- states
def base_coefficients(case):
    """The A coefficients of the case's initial condition (Float64 oracle), the amplitude every random state keeps."""
    g = cases.oracle_grid(case)
    m = O.Model(g, case["eq"], case["ts"], case["par"])
    pts = g.gridpoints()
    m.set_initial(case["ic"](pts.reshape(len(pts), -1)))
    return m.A


def state_coefficients(base, t, seed=7):
    """A different state per t: every coefficient of the initial condition times (1 + 0.2 N(0, 1)), seeded."""
    rng = np.random.default_rng([seed, t])
    return base * (1.0 + 0.2 * rng.standard_normal(base.shape))


def f32_slots(phys):
    """`physical` as storage = "f32" holds it: derivative slots rounded through float32, values kept."""
    out = phys.copy()
    out[:, :, 1:] = out[:, :, 1:].astype(np.float32).astype(np.float64)
    return out


# ----------------------------------------------------------------------------- column-operator hook
class _Ops:
    """tendency()'s col_ops.  record: apply and keep (input, output, |M|); frozen: return the recorded output and keep the
    input's deviation; poke k: as frozen, operator k returns its output + eps.

    Worked example, the HRBL set, whose tendency applies three operators in this order: 0 = Vint to the divergence (-> wb),
    1 = Vdz to the flux fu, 2 = Vdz to fv.  record (the base evaluation) leaves base = [(div, wb, |Vint|), (fu, VDu, |Vdz|),
    (fv, VDv, |Vdz|)], each [columns, nz].  "poke 0" returns wb + eps[0] and VDu, VDv as recorded: var_np1 moves by
    -ubz ts-weight eps[0] in ub (and likewise in vb), so D_out[0] = |d var_np1 / d wb| per point; no later operator is fed wb, so
    D_op[0][1] = D_op[0][2] = 0.  Then the plane ub_z is scaled by 1 + 2^-30 in "frozen": every operator returns its recorded
    output, var_np1 moves by the pointwise paths alone (-wb ubz), and dev = [0, d fu / 2^-30, d fv / 2^-30] holds how the operators'
    inputs moved.  The plane's share of S is |pointwise| + D_out[1] (|dev[1]| @ |Vdz|^T) + D_out[2] (|dev[2]| @ |Vdz|^T):
    sum_j |M_ij| |dx_j| per operator.  In the semi-implicit solve operator 3 (W) is fed operator 1's output (d/dz of xi*), and
    D_op[1][3] carries |dev| of one into the input of the other before |W| is applied."""

    def __init__(self):
        self.base, self.mode, self.k, self.dev, self.poke, self.eps = [], "record", 0, [], None, None

    def start(self, mode, poke=None):
        self.mode, self.k, self.dev, self.poke = mode, 0, [], poke

    def __call__(self, name, M, x):
        if self.mode == "record":
            y = x @ M.T
            self.base.append((x.copy(), y, np.abs(np.asarray(M, dtype=np.float64))))
            return y
        if self.mode == "plain":
            return x @ M.T
        i = self.k
        self.k += 1
        x0, y0, _ = self.base[i]
        self.dev.append(np.asarray((x - x0) / DELTA, dtype=np.float64))
        return y0 + self.eps[i] if self.poke == i else y0


def _rel(a, a0):
    """(a - a0) / DELTA as Float64, inf - inf (a margin that is infinite on both sides) taken as 0"""
    with np.errstate(invalid="ignore"):
        d = np.asarray((a - a0) / DELTA, dtype=np.float64)
    return np.nan_to_num(d, nan=0.0, posinf=0.0, neginf=0.0)


def semi_operators(case, device=False):
    """((W, X) at t = 1, (W, X) after) in Float64 of the case's semi-implicit column solve, or None: the bits the kernels read.
    The Helmholtz inverse is formed in 80-bit arithmetic at condition ~ nz^4, so two assemblies of it differ by ~1e-13 of the
    operator's norm, far above u: the twin and whatever it is compared with must hold the SAME rounded operators, as they hold the
    same `physical`.  device = True: the library's own (sx_semi_column_ops, what sx_create uploads); else the oracle's."""
    if not case.get("semiimplicit", False):
        return None
    g = cases.oracle_grid(case)
    pxi, ts, nz = case["par"]["Pxi_bar"], case["ts"], g.zDim
    out = []
    for tau in (0.5 * ts, 1.25 * ts):
        if device:
            import ctypes as C
            from scythe_jl_amd import _lib as L
            from scythe_jl_amd import model as M
            W, X = np.zeros((nz, nz)), np.zeros((nz, nz))
            bc = lambda d: L.BC[M.bc_name(d["w"], M._CHEB_BCS)]
            L.check(L.load().sx_semi_column_ops(C.c_double(g.zmin), C.c_double(g.zmax), nz, g.b_zDim, bc(g.BCB), bc(g.BCT),
                                                C.c_double(pxi), C.c_double(tau), W.ctypes.data_as(L.P_D), X.ctypes.data_as(L.P_D)))
            out.append((W, X))
        else:
            out.append(O.semi_matrices(g.cheb("w"), pxi, tau))
    return tuple(out)


class Twin:
    def __init__(self, case, pts=None, semi_ops=None):
        self.case, self.eq, self.semi = case, case["eq"], case.get("semiimplicit", False)
        self.g = g = cases.oracle_grid(case)
        if pts is None:
            pts = g.gridpoints()
        pts = np.asarray(pts, dtype=np.float64).reshape(g.tile_npoints(0, g.nc), -1)
        self.N, self.nz = len(pts), g.zDim
        self.pts = pts.astype(XP)
        self.trig = None
        if g.has_l:          # per column, as the library holds them: cos / sin of the Float64 angle, rounded to Float64
            lam = pts[:: self.nz, 1]
            self.trig = (np.cos(lam).astype(XP), np.sin(lam).astype(XP))
        self.sw = self.eq in SW_SETS
        self.model = O.Model(g, self.eq, case["ts"], case["par"], semiimplicit=self.semi, pxi_bar=case["par"].get("Pxi_bar", 0.0))
        self.model.semi_ops = semi_ops if semi_ops is not None else semi_operators(case)
        self.c, self.nops = chain(case, self.nz if g.has_z else 1)
        self.hist = None
        self._memo = {}

    # -- one evaluation
    def _inputs(self, phys):
        par = {k: XP(v) for k, v in self.case["par"].items() if k != "ref_state"}
        if "ref_state" in self.case["par"]:
            par["ref_state"] = {k: np.asarray(v, dtype=XP) for k, v in self.case["par"]["ref_state"].items()}
        X = dict(phys=np.asarray(phys, dtype=np.float64).astype(XP), pts=self.pts, trig=self.trig, par=par, ts=XP(self.case["ts"]),
                 TH={})
        X.update(self.hist)
        return X

    def _run(self, t, X, ops):
        saved = dict(O.TH)
        O.TH.update(X["TH"])
        O.BRANCHES = br = []
        self._site = 0

        def intermediate(x):
            self._site += 1
            return x * (XP(1) + DELTA) if self._site == X.get("site") else x
        O.INTERMEDIATE = intermediate
        try:
            E, I, ph = O.tendency(self.g, self.eq, X["par"], X["phys"].copy(), X["pts"], col_ops=ops, trig=X["trig"])
            np1, _, _ = O.explicit_timestep(t, X["ts"], ph[:, :, 0], E, X["e1"], X["e2"])
            if self.semi:
                m = self.model
                m.ts, m.pxi, m.col_ops = X["ts"], X["par"]["Pxi_bar"], ops
                m.hist[0] = dict(i1=X["i1"], i2=X["i2"])
                np1 = m._semiimplicit(0, t, np1, I)
            if self.eq == "rainfall_test":
                np1 = O.condensation_adjustment(np1, X["par"], self.nz)
        finally:
            O.BRANCHES = O.INTERMEDIATE = None
            O.TH.clear()
            O.TH.update(saved)
        out = np.concatenate([np1, ph[:, 5:6, 0]], axis=1) if self.sw else np1
        lifted = [np.repeat(b, self.N // b.size) if b.size != self.N else b.reshape(-1) for b in br]
        return out, E, I, (np.stack(lifted, axis=1) if lifted else np.zeros((self.N, 0), dtype=XP))

    # -- the three questions
    def _solve(self, phys, t, by_level=False):
        """by_level = True: the planes of `physical`, r and z are perturbed one LEVEL at a time through the live operators (the
        literal level-by-level sum, nz times the work) instead of once with the operators' inputs recorded; only
        tests/test_physics.py asks for it, to measure how much larger the chained sum is."""
        key = (t, np.asarray(phys).tobytes(), by_level)
        if self._memo.get("key") == key:
            return self._memo
        if t == 1 or self.hist is None:
            z = np.zeros((self.N, self.g.V), dtype=XP)
            self.hist = dict(e1=z, e2=z, i1=z, i2=z)
        X = self._inputs(phys)
        ops = _Ops()
        out0, E, I, br0 = self._run(t, X, ops)
        nout, nsites = out0.shape[1], self._site
        full0 = np.concatenate([out0, br0], axis=1)
        K = len(ops.base)
        ncol = self.N // self.nz
        col = lambda a: a.reshape(ncol, self.nz, -1)
        # the effect of each operator's output on the result and on the inputs of the operators after it
        ops.eps = [DELTA * (XP(np.abs(y).max()) or XP(1.0)) for _, y, _ in ops.base]
        D_out, D_op = [], []
        for k in range(K):
            ops.start("poke", k)
            o, _, _, b = self._run(t, X, ops)
            s = float(ops.eps[k] / DELTA)
            D_out.append(np.abs(_rel(np.concatenate([o, b], axis=1), full0)) / s)
            D_op.append([np.abs(d) / s for d in ops.dev])

        S = np.zeros(full0.shape)

        def array_input(Xp):
            ops.start("frozen")
            o, _, _, b = self._run(t, Xp, ops)
            tot = np.abs(_rel(np.concatenate([o, b], axis=1), full0))
            outs = []
            for k in range(K):
                a = np.abs(ops.dev[k])
                for m in range(k):
                    a = a + D_op[m][k] * outs[m]
                outs.append(a @ ops.base[k][2].T)
                tot = tot + D_out[k] * outs[k].reshape(self.N, 1)
            return tot

        def scalar_input(Xp):
            ops.start("plain")
            o, _, _, b = self._run(t, Xp, ops)
            return np.abs(_rel(np.concatenate([o, b], axis=1), full0))

        # the entries of the operators themselves, data the kernels read like any other: sum_j |M_ij x_j|
        for k in range(K):
            outs = []
            for m in range(K):
                a = np.zeros(ops.base[m][0].shape)
                for n in range(m):
                    a = a + D_op[n][m] * outs[n]
                outs.append(np.abs(np.asarray(ops.base[m][0], dtype=np.float64)) @ ops.base[m][2].T if m == k else a @ ops.base[m][2].T)
                if m >= k:
                    S += D_out[m] * outs[m].reshape(self.N, 1)

        up = XP(1) + DELTA
        level = np.arange(self.N) % self.nz
        groups = [level == j for j in range(self.nz)] if by_level else [slice(None)]
        one = scalar_input if by_level else array_input
        for v in range(self.g.V):
            for d in range(self.g.D):
                for sel in groups:
                    ph = X["phys"].copy()
                    ph[sel, v, d] *= up
                    S += one(dict(X, phys=ph))
        for j in range(self.pts.shape[1]):
            if self.g.has_l and j == 1:
                continue                          # lambda enters through cos / sin only
            for sel in groups:
                p = X["pts"].copy()
                p[sel, j] *= up
                S += one(dict(X, pts=p))
        if self.trig is not None:
            S += array_input(dict(X, trig=(self.trig[0] * up, self.trig[1])))
            S += array_input(dict(X, trig=(self.trig[0], self.trig[1] * up)))
        for name in ("e1", "e2") if t >= 3 else ("e1",) if t == 2 else ():
            S += array_input(dict(X, **{name: X[name] * up}))
        if self.semi:
            for name in ("i1", "i2") if t >= 3 else ("i1",) if t == 2 else ():
                for v in (self.g.vars["w"] - 1, self.g.vars["xi"] - 1):
                    h = X[name].copy()
                    h[:, v] *= up
                    S += array_input(dict(X, **{name: h}))
        for k, v in X["par"].items():
            if k == "ref_state":
                for name, prof in v.items():
                    for j in range(prof.shape[1]):
                        q = prof.copy()
                        q[:, j] *= up
                        S += array_input(dict(X, par=dict(X["par"], ref_state=dict(v, **{name: q}))))
            elif v != 0:
                S += scalar_input(dict(X, par=dict(X["par"], **{k: v * up})))
        S += scalar_input(dict(X, ts=X["ts"] * up))
        if self.eq in THERMO_SETS:
            for k, v in list(O.TH.items()):
                S += scalar_input(dict(X, TH={k: XP(v) * up}))

        for site in range(1, nsites + 1):       # the rounded exp / sqrt / pow results (oracle_np.INTERMEDIATE)
            S += array_input(dict(X, site=site))

        cu = self.c * U
        Sm, m0 = S[:, nout:], np.asarray(br0, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            near = ((np.abs(m0) <= cu * Sm) & (Sm > 0)).any(axis=1)
        if self.nops:
            near = np.repeat(near.reshape(ncol, self.nz).any(axis=1), self.nz)
        self._memo = dict(key=key, out=out0, bound=cu * S[:, :nout], mask=near, E=E, I=I, margins=m0)
        return self._memo

    def call(self, phys_f64, t):
        """(var_np1, w) in longdouble of one sx_physics(t) on phys_f64 [N, V, D]; w is None where the set has no diagnostic w.
        Advances the twin's own history (restarted at t = 1)."""
        r = self._solve(phys_f64, t)
        if self._memo.get("advanced") != r["key"]:
            h = self.hist
            self.hist = dict(e1=r["E"], e2=h["e1"], i1=r["I"] if r["I"] is not None else h["i1"], i2=h["i1"])
            self._memo["advanced"] = r["key"]
        V = self.g.V
        return r["out"][:, :V], (r["out"][:, V] if self.sw else None)

    def bound(self, phys_f64, t):
        """c u S [N, V (+ 1 for w)] of the same call; ask before the next call(..., t + 1)."""
        return self._solve(phys_f64, t)["bound"]

    def mask(self, phys_f64, t):
        """[N] True where a data-dependent branch is too close to call."""
        return self._solve(phys_f64, t)["mask"]

    def margins(self, phys_f64, t):
        """[N, branches] the quantity whose sign decides each data-dependent branch, in evaluation order (per-column ones
        repeated over the column).  condensation_adjustment's whole-column clamps are the last two: column_min, column_max."""
        return self._solve(phys_f64, t)["margins"]


# ----------------------------------------------------------------------------- the Float64 model, as a kernel would run it
class Float64Run:
    """oracle_np in Float64 for one sx_physics call after another, with its own history: stands in for a kernel in the CPU
    tests.  `mutate` names one deliberate error (tests/test_physics.py)."""

    def __init__(self, case, pts=None, mutate=None, semi_ops=None):
        self.case, self.eq, self.semi, self.mutate = case, case["eq"], case.get("semiimplicit", False), mutate
        self.g = g = cases.oracle_grid(case)
        p = g.gridpoints() if pts is None else pts
        self.pts = np.asarray(p, dtype=np.float64).reshape(g.tile_npoints(0, g.nc), -1)
        par = dict(case["par"])
        if mutate == "term":
            k = "Kh" if self.eq == "Oneway_ShallowWater_HeightResolvedBL" else "K"      # the diffusion term of every set
            par[k] = par[k] * (1.0 + 1.0e-9)
        self.par = par
        self.model = O.Model(g, self.eq, case["ts"], par, semiimplicit=self.semi, pxi_bar=par.get("Pxi_bar", 0.0))
        self.model.semi_ops = semi_ops if semi_ops is not None else semi_operators(case)
        if mutate == "semi":
            self.model.pxi = self.model.pxi * (1.0 + 1.0e-9)        # tau Pxi_bar of xi*_z inside semiimplicit_adjustment only
        self.e1 = self.e2 = None
        self.np1 = None

    def call(self, phys, t):
        g, ts = self.g, self.case["ts"]
        phys = np.array(phys, dtype=np.float64)
        if self.mutate == "f32":
            d = g.slots.index("r")
            phys[:, 0, d] = phys[:, 0, d].astype(np.float32)
        E, I, ph = O.tendency(g, self.eq, self.par, phys, self.pts)
        if t == 1:
            self.e1, self.e2 = np.zeros_like(E), np.zeros_like(E)
        e1, e2 = (self.e2, self.e1) if (self.mutate == "rotation" and t == 3) else (self.e1, self.e2)
        if self.mutate == "weight" and t >= 3:
            np1 = ph[:, :, 0] + ((ts / 12.0) * ((23.00000001 * E) - (16.0 * e1) + (5.0 * e2)))
        else:
            np1, _, _ = O.explicit_timestep(t, ts, ph[:, :, 0], E, e1, e2)
        self.e1, self.e2 = E.copy(), self.e1
        if self.semi:
            np1 = self.model._semiimplicit(0, t, np1, I)
        if self.eq == "rainfall_test":
            tau_r = O.RAIN_TAU_R
            try:
                if self.mutate == "condensation":
                    O.RAIN_TAU_R = tau_r * (1.0 + 1.0e-9)             # the time scale of condensation_adjustment
                np1 = O.condensation_adjustment(np1, self.par, g.zDim)
            finally:
                O.RAIN_TAU_R = tau_r
        if self.mutate == "stale" and self.np1 is not None:
            np1[-g.zDim:] = self.np1[-g.zDim:]
        self.np1 = np1
        return np1, (ph[:, 5, 0] if self.eq in SW_SETS else None)


def solve(twin, phys_by_t):
    """{t: (want [N, V (+ 1)], bound, mask, margins)} of the twin over t = 1..4, each t on its own `physical`"""
    out = {}
    for t in sorted(phys_by_t):
        ref, wref = twin.call(phys_by_t[t], t)
        want = ref if wref is None else np.concatenate([ref, wref[:, None]], axis=1)
        out[t] = (want, twin.bound(phys_by_t[t], t), twin.mask(phys_by_t[t], t), twin.margins(phys_by_t[t], t))
    return out


def ratios(solved_t, np1, w):
    """|err| / bound [N, V (+ 1)] of a result against the twin's (want, bound, mask), masked points set to 0.  A zero bound
    demands the twin's value exactly."""
    want, bound, mask = solved_t[:3]
    got = np.asarray(np1, dtype=XP) if w is None else np.concatenate([np.asarray(np1, dtype=XP), np.asarray(w, dtype=XP)[:, None]], axis=1)
    err = np.asarray(np.abs(got - want), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    q[mask] = 0.0
    return q


def check_clamp_mix(twin, solved):
    """rainfall_test: over t = 1..4 some columns take condensation_adjustment's whole-column clamp q_cond = -q_c (column_max, the
    last logged branch) and some keep q_cond - what rz_rain_mixed is for.  Returns the clamped columns per t of (column_min,
    column_max); column_min takes one side in every column of these states."""
    count = {t: tuple(int((s[3][:: twin.nz, k] < 0).sum()) for k in (-2, -1)) for t, s in solved.items()}
    ncol = twin.N // twin.nz
    hit = sum(c[1] for c in count.values())
    assert 0 < hit < ncol * len(count), "column_max clamps %d of %d columns over t = 1..4: not mixed" % (hit, ncol * len(count))
    return count


def worst(twin, q):
    """ring, column, level, variable and |err| / bound of the worst point"""
    p, v = np.unravel_index(int(np.argmax(q)), q.shape)
    g = twin.g
    colidx, lev = divmod(int(p), twin.nz)
    ring = int(np.searchsorted(g.ringstart, colidx, side="right") - 1)
    return "ring %d column %d level %d variable %d: |err| / bound = %.3g" % (ring, colidx, lev, v, q[p, v])


# ----------------------------------------------------------------------------- cases
def _hrbl(zDim, num_cells=5, ring_L=None):
    return cases.rlz_hrbl(num_cells=num_cells, zDim=zDim, ring_L=ring_L)


def make_case(maker, kw):
    mod = {"linear_sw": linear_sw, "rainfall": rainfall}.get(maker.split(".")[0], cases)
    return getattr(mod, maker.split(".")[-1])(**kw)


# id -> (maker, kwargs, storage, SX_* overrides of a child process or None, the timer names sx_physics must show, tails).
# tails: {"points" | "columns": unit of one workgroup, ...}: what sx_get_dims must NOT be a multiple of (and must exceed), so that
# every launch has more than one workgroup and a partial last one - k_phys_pointwise / k_phys_rain 256 points; k_phys_hrbl,
# k_semiimplicit and k_condensation 256 // nz columns; k_phys_hrbl_mfma 8 columns; k_semi_mfma 16 columns (launch_physics_t,
# launch_semi_mfma).  "full": the count is a multiple of the unit and cannot be otherwise - rings of 32 points give multiples of
# 32 columns, and the smallest native grid sx_create accepts (3 cells, 9 rings) has 2 * 9 * 12 = 216 = 27 * 8 columns; the partial
# last workgroup of k_phys_hrbl_mfma is covered by the native 5-cell cases (540 columns).
# The timer names cannot tell k_phys_hrbl from k_phys_hrbl_mfma nor k_semiimplicit from k_semi_mfma (launch_physics_t gives both
# of each pair one name): which of the two runs rests on the dispatch code (mfma_levels(nz), h->sw.wide, h->sw.semi_mfma, read
# at sx_create), not on the timers.
P, H, R, C, SI = "k_phys_pointwise", "k_phys_hrbl", "k_phys_rain", "k_condensation", "k_semiimplicit"
CASES = {
    # k_phys_pointwise: more than 256 points, not a multiple of 256
    "adv1d": ("r_bcs", dict(num_cells=100), "f64", None, (P,), {'points': 256}),
    "adv_rz": ("rz_advection", dict(num_cells=10, zDim=14), "f64", None, (P,), {'points': 256}),
    "adv_rl": ("rl_advection", dict(num_cells=4), "f64", None, (P,), {'points': 256}),
    "adv_rlz": ("rlz_advection", dict(num_cells=3, zDim=9), "f64", None, (P,), {'points': 256}),
    "slab_oneway": ("rl_slab", dict(num_cells=4), "f64", None, (P,), {'points': 256}),
    "slab_twoway": ("rl_slab", dict(num_cells=4, twoway=True), "f64", None, (P,), {'points': 256}),
    "lsw1d": ("linear_sw.r_case", dict(num_cells=100), "f64", None, (P,), {'points': 256}),
    "lsw_rl": ("linear_sw.rl_case", dict(num_cells=4), "f64", None, (P,), {'points': 256}),
    "acoustic": ("rz_semiimplicit", dict(num_cells=8, zDim=12), "f64", None, (P, SI), {'points': 256, 'semi columns': 16}),
    "euler": ("rz_euler", dict(num_cells=8, zDim=12, semiimplicit=False), "f64", None, (P,), {'points': 256}),
    # k_phys_hrbl (generic): 25 and 21 columns per workgroup
    "hrbl_z10": ("rlz_hrbl", dict(num_cells=3, zDim=10), "f64", None, (H,), {'columns': 25}),
    "hrbl_z12": ("rlz_hrbl", dict(num_cells=3, zDim=12), "f64", None, (H,), {'columns': 21}),
    # k_phys_hrbl_mfma, 8 columns per workgroup
    "hrbl_z32_native": ("rlz_hrbl", dict(num_cells=5, zDim=32), "f64", None, (H,), {'columns': 8}),
    "hrbl_z64_native": ("rlz_hrbl", dict(num_cells=5, zDim=64), "f64", None, (H,), {'columns': 8}),
    "hrbl_z32_uniform": ("rlz_hrbl", dict(num_cells=5, zDim=32, ring_L=32), "f64", None, (H,), {'columns': 8, 'full': True}),
    "hrbl_z64_uniform": ("rlz_hrbl", dict(num_cells=5, zDim=64, ring_L=32), "f64", None, (H,), {'columns': 8, 'full': True}),
    "hrbl_z128": ("rlz_hrbl", dict(num_cells=3, zDim=128), "f64", None, (H,), {'columns': 8, 'full': True}),
    "hrbl_z32_narrow": ("rlz_hrbl", dict(num_cells=5, zDim=32), "f64", {"SX_WIDE": 0}, (H,), {'columns': 8}),
    # fp32-stored derivative planes
    "adv_rlz_f32": ("rlz_advection", dict(num_cells=3, zDim=9), "f32", None, (P,), {'points': 256}),
    "hrbl_z32_f32": ("rlz_hrbl", dict(num_cells=5, zDim=32), "f32", None, (H,), {'columns': 8}),
    "rain_z12_f32": ("rainfall.rz_rain_mixed", dict(num_cells=9, zDim=12, semiimplicit=False), "f32", None, (R, C), {'points': 256, 'condensation columns': 21}),
    # k_phys_rain + k_condensation: 21, 18 and 16 columns per workgroup of k_condensation
    "rain_z12": ("rainfall.rz_rain_mixed", dict(num_cells=9, zDim=12, semiimplicit=False), "f64", None, (R, C), {'points': 256, 'condensation columns': 21}),
    "rain_z14": ("rainfall.rz_rain_mixed", dict(num_cells=7, zDim=14, semiimplicit=False), "f64", None, (R, C), {'points': 256, 'condensation columns': 18}),
    "rain_z16": ("rainfall.rz_rain_mixed", dict(num_cells=7, zDim=16, semiimplicit=False), "f64", None, (R, C), {'points': 256, 'condensation columns': 16}),
    "rain_z12_semi": ("rainfall.rz_rain_mixed", dict(num_cells=9, zDim=12, semiimplicit=True), "f64", None, (R, SI, C), {'points': 256, 'semi columns': 16, 'condensation columns': 21}),
    "rain_z14_semi": ("rainfall.rz_rain_mixed", dict(num_cells=7, zDim=14, semiimplicit=True), "f64", None, (R, SI, C), {'points': 256, 'semi columns': 16, 'condensation columns': 18}),
    "rain_z16_semi": ("rainfall.rz_rain_mixed", dict(num_cells=7, zDim=16, semiimplicit=True), "f64", None, (R, SI, C), {'points': 256, 'semi columns': 16, 'condensation columns': 16}),
    # k_semi_mfma (default) and k_semiimplicit (SX_SEMI_MFMA=0)
    "acoustic_z16": ("rz_semiimplicit", dict(num_cells=7, zDim=16), "f64", None, (P, SI), {'points': 256, 'semi columns': 16}),
    "acoustic_z32": ("rz_semiimplicit", dict(num_cells=7, zDim=32), "f64", None, (P, SI), {'points': 256, 'semi columns': 16}),
    "euler_z16": ("rz_euler", dict(num_cells=7, zDim=16), "f64", None, (P, SI), {'points': 256, 'semi columns': 16}),
    "euler_z32": ("rz_euler", dict(num_cells=7, zDim=32), "f64", None, (P, SI), {'points': 256, 'semi columns': 16}),
    "acoustic_z16_plain": ("rz_semiimplicit", dict(num_cells=7, zDim=16), "f64", {"SX_SEMI_MFMA": 0}, (P, SI), {'points': 256, 'semi columns': 16}),
    "acoustic_z32_plain": ("rz_semiimplicit", dict(num_cells=7, zDim=32), "f64", {"SX_SEMI_MFMA": 0}, (P, SI), {'points': 256, 'semi columns': 8}),
    "euler_z16_plain": ("rz_euler", dict(num_cells=7, zDim=16), "f64", {"SX_SEMI_MFMA": 0}, (P, SI), {'points': 256, 'semi columns': 16}),
    "euler_z32_plain": ("rz_euler", dict(num_cells=7, zDim=32), "f64", {"SX_SEMI_MFMA": 0}, (P, SI), {'points': 256, 'semi columns': 8}),
}

# k_semi_mfma / k_semiimplicit at the level counts where the launch changes: a second and a fourth K chunk of 64 levels, level
# counts one past a tile (33, 65, 129), the over-64 KB LDS branch and the second trip of the kernel's `kt += nw` loops (zDim > 128);
# 15 columns (one partial workgroup), 33 (two full and a partial one), 48 (three full).  The ids carry the launch as the library's
# plan reports it (cases.semi_launch_geometry).  15 columns do not fill a workgroup of 16, so these cases state the point count only
# (a whole number of 256-point workgroups at 256 levels and at 48 x 128).
SEMI_SHAPES = [
    # (maker, cells, zDim, SX_* overrides, tails)
    ("rz_semiimplicit", 5, 33, None, {'points': 256}),
    ("rz_semiimplicit", 11, 64, None, {'points': 256, 'semi columns': 16}),
    ("rz_semiimplicit", 5, 65, None, {'points': 256}),
    ("rz_semiimplicit", 16, 128, None, {'points': 256, 'semi columns': 16, 'full': True}),
    ("rz_semiimplicit", 5, 129, None, {'points': 256}),
    ("rz_semiimplicit", 5, 200, None, {'points': 256}),
    ("rz_semiimplicit", 5, 256, None, {'points': 256, 'full': True}),
    ("rz_semiimplicit", 5, 65, {"SX_SEMI_MFMA": 0}, {'points': 256}),
    ("rz_semiimplicit", 5, 200, {"SX_SEMI_MFMA": 0}, {'points': 256}),
    ("rz_euler", 5, 64, None, {'points': 256}),
    ("rz_euler", 5, 128, None, {'points': 256}),
]


def semi_id(maker, nc, nz, env):
    geo = cases.semi_launch_geometry(getattr(cases, maker)(num_cells=nc, zDim=nz), env)
    return "%s_n%dz%d-%s-wg%d-last%d-t%d-trips%d-kc%d-lds%d%s" % (
        maker[3:], nc, nz, geo["kernel"], geo["wgs"], geo["last"], geo["threads"], geo["trips"], geo["chunks"], geo["lds"],
        "-attr" if geo["attr"] else "")


SEMI_CASES = {semi_id(m, nc, nz, env): (m, dict(num_cells=nc, zDim=nz), "f64", env, (P, SI), tails) for m, nc, nz, env, tails in SEMI_SHAPES}
CASES.update(SEMI_CASES)

# one small case per equation set (the Float64 pin of tests/golden/physics_f64_pin.npz and the mutations of tests/test_physics.py)
PER_SET = ("adv1d", "adv_rz", "adv_rl", "adv_rlz", "slab_oneway", "slab_twoway", "lsw1d", "lsw_rl", "acoustic", "euler", "hrbl_z10",
           "rain_z12_semi")


def case_of(cid):
    maker, kw, storage, env, timers, _ = CASES[cid]
    return make_case(maker, kw), storage, env, timers


def check_tails(cid, n_points, n_columns):
    """Assert what CASES[cid] says of the launch shapes against the counts of sx_get_dims (or of the oracle's grid); returns
    the text of what was checked."""
    tails = CASES[cid][5]
    said = []
    for what, unit in tails.items():
        if what == "full":
            continue
        count = n_points if what == "points" else n_columns
        assert count > unit, "%s: %d %s do not fill one workgroup of %d" % (cid, count, what, unit)
        if tails.get("full"):
            assert count % unit == 0
        else:
            assert count % unit != 0, "%s: %d %s are a multiple of %d: no partial last workgroup" % (cid, count, what, unit)
        said.append("%d %s = %d x %d + %d" % (count, what, count // unit, unit, count % unit))
    assert said
    return ", ".join(said)


@functools.lru_cache(maxsize=None)
def solved_on_host(cid):
    """(case, twin, {t: physical}, solve(...)) with the oracle's inverse transform standing in for the device's"""
    case, storage, _, _ = case_of(cid)
    phys = {t: ph for t, (_, ph) in states(case, storage).items()}
    twin = Twin(case)
    return case, twin, phys, solve(twin, phys)


def states(case, storage="f64", ts=(1, 2, 3, 4)):
    """{t: (A coefficients, Float64 `physical` of the oracle's inverse transform)}: the CPU stand-in for what the device holds"""
    g = cases.oracle_grid(case)
    base = base_coefficients(case)
    out = {}
    for t in ts:
        A = state_coefficients(base, t)
        ph = g.inverse(A)
        out[t] = (A, f32_slots(ph) if storage == "f32" else ph)
    return out


# ----------------------------------------------------------------------------- the device side (GPU tests and their child processes)
def device_run(cid):
    """The helper of tests/test_gpu_physics.py: one tile, t = 1..4 with a different state each, every array the checks need.
    {"pts", "dims" (n_points, n_hpoints), "timers" (names), and per t: "phys%d" / "np1_before%d" / "np1_%d" / "phys_after%d"}"""
    import scythe_jl_amd as S
    case, storage, _, _ = case_of(cid)
    gp, mp = cases.hip_params(case, storage)
    tile = S.Grid(gp, mp)
    out = dict(pts=np.asarray(S.getGridpoints(tile)), dims=np.array([tile.N, int(tile.dims.n_hpoints)]))
    ops = semi_operators(case, device=True)
    if ops is not None:
        out["semi_ops"] = np.array(ops)           # [2 (t = 1, after)][2 (W, X)][nz][nz]
    base = base_coefficients(case)
    for t in (1, 2, 3, 4):
        tile.set_patch_spectral_a(state_coefficients(base, t))
        tile.tileTransform_()
        out["phys%d" % t] = tile.physical
        out["np1_before%d" % t] = tile.var_np1
        tile.enable_timers(True)          # around sx_physics alone: the transforms have timers too
        tile.physics(t)
        tile.enable_timers(False)
        out["np1_%d" % t] = tile.var_np1
        out["phys_after%d" % t] = tile.physical
    tm = tile.timers()
    out["timers"] = np.array(sorted(k for k, (ms, calls) in tm.items() if calls > 0))
    out["timer_calls"] = np.array([tm[k][1] for k in out["timers"]])
    tile.close()
    return out
