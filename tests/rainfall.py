"""rainfall_test (src/testModels.jl:387-585) for the tests: the warm-rain tendency and condensation_adjustment
(src/microphysics.jl:139-195) restated in numpy for the oracle twin, and the cases.

oracle/oracle_np.py knows only the sets it was written for and stays as it is.  `patch_oracle(monkeypatch)` wraps its module-level
`tendency`, which `Model.step` looks up as a global, and replaces its `Model` by `RainModel`, whose step runs the adjustment after
the explicit and the semi-implicit step, as the reference's rainfall_test does."""
import numpy as np

from oracle import oracle_np as O

SET = "rainfall_test"
VARS = {"s": 1, "xi": 2, "mu": 3, "u": 4, "w": 5, "mu_c": 6, "mu_r": 7, "qss": 8}
N_C, R_C = 100.0, 10.0                                  # src/testModels.jl:500-501
TAU_R = 0.25                                            # src/microphysics.jl:182
TH = O.TH
Cpd = TH["Cvd"] + TH["Rd"]                              # src/thermodynamics.jl:2-17
Eps = TH["Rd"] / TH["Rv"]


# ----------------------------------------------------------------------------- the thermodynamics oracle_np does not carry
def L_v(Tk):                                            # src/thermodynamics.jl:41-44
    return TH["L_v0"] + ((TH["Cpv"] - TH["Cl"]) * (Tk - TH["T_0"]))


def pressure(Tk, rho_d, q_v):                           # p of thermodynamic_tuple, :260-269
    return (0.01 * TH["Rd"] * Tk * rho_d) + (0.01 * TH["Rv"] * Tk * rho_d * q_v)


def vapor_pressure(p, q_v):                             # :89-94
    return (p * q_v) / (Eps + q_v)


def sat_pressure_liquid_buck(Tk, phPa):                 # :101-118
    Tc = Tk - 273.15
    A, B, C = 7.2e-4, 3.20e-6, 5.9e-10
    fw4 = 1.0 + A + (phPa * (B + (C * (Tc * Tc))))
    a, b, c, d = 6.1121, 18.729, 257.87, 227.3
    return fw4 * (a * np.exp((b - (Tc / d)) * Tc / (Tc + c)))


def sat_pressure_liquid_buck_dT(Tk, phPa):              # :120-142
    Tc = Tk - 273.15
    A, B, C = 7.2e-4, 3.20e-6, 5.9e-10
    fw4 = 1.0 + A + (phPa * (B + (C * (Tc * Tc))))
    d_fw4 = 2.0 * phPa * C * Tc
    a, b, c, d = 6.1121, 18.729, 257.87, 227.3
    ew4 = a * np.exp((b - (Tc / d)) * Tc / (Tc + c))
    T1 = (d * b - (2.0 * Tc)) * (d * (Tc + c)) - d * ((d * b * Tc) - (Tc * Tc))
    T2 = (d * (Tc + c)) * (d * (Tc + c))
    return ew4 * d_fw4 + fw4 * (ew4 * T1 / T2)


def q_sat_liquid(Tk, phPa):                             # :163-170
    ew = sat_pressure_liquid_buck(Tk, phPa)
    return Eps * ew / (phPa - ew)


def _cp(q_v, q_l):
    return Cpd + (q_v * TH["Cpv"]) + (q_l * TH["Cl"])


def _dqsdT(Tk, p, e_s):
    return sat_pressure_liquid_buck_dT(Tk, p) * Eps * p / ((p - e_s) * (p - e_s))


def Q_s_factor(Tk, p, q_v, q_l):                        # src/microphysics.jl:107-114
    e_s = sat_pressure_liquid_buck(Tk, p)
    return L_v(Tk) * _dqsdT(Tk, p, e_s) / _cp(q_v, q_l)


def dqsdp(Tk, p, rho_d, q_v, q_l):                      # :116-124
    e_s = sat_pressure_liquid_buck(Tk, p)
    return q_sat_liquid(Tk, p) / (100.0 * (p - e_s)) - (_dqsdT(Tk, p, e_s) / (rho_d * _cp(q_v, q_l)))


def vapor_diffusity(Tk, p):                             # :134-140
    return 0.211 * (Tk / 273.15) ** 1.94 * (1013.25 / p)


def invtau_condensation(Tk, p, N_c, r_c):               # :126-132
    return 4.0 * np.pi * vapor_diffusity(Tk, p) * N_c * (r_c * 1.0e-4)


def jl_min(x, y):
    """Julia's scalar min on Float64, elementwise: NaN propagates, -0.0 < 0.0."""
    x, y = np.broadcast_arrays(np.asarray(x, float), np.asarray(y, float))
    pick_y = (y < x) | (np.signbit(y) & ~np.signbit(x))
    return np.where(pick_y, np.where(np.isnan(x), x, y), np.where(np.isnan(y), y, x))


def jl_max(x, y):
    x, y = np.broadcast_arrays(np.asarray(x, float), np.asarray(y, float))
    pick_y = (y > x) | (~np.signbit(y) & np.signbit(x))
    return np.where(pick_y, np.where(np.isnan(x), x, y), np.where(np.isnan(y), y, x))


def q_condensation(qss, Tk, p, q_v, q_l, N_c, r_c):    # :84-93 (broadcast: scalar min / max)
    q_cond = qss / (1.0 + Q_s_factor(Tk, p, q_v, q_l))
    q_cond = jl_min(q_v, q_cond)
    q_cond = jl_max(-q_l, q_cond)
    return q_cond * invtau_condensation(Tk, p, N_c, r_c)


def s_condensation(q_cond, Tk, rho_d, q_v, q_l, p):    # :96-105
    Cm = (q_l * TH["Cl"]) / (TH["Cvd"] + (q_v * TH["Cvv"]) + (q_l * TH["Cl"]))
    e = vapor_pressure(p, q_v)
    sat_e = sat_pressure_liquid_buck(Tk, p)
    with np.errstate(divide="ignore", invalid="ignore"):
        return q_cond * (((-L_v(Tk) * Cm) / Tk) - (TH["Cl"] * np.log(Tk / TH["T_0"])) + (TH["Rv"] * np.log(e / sat_e)))


def autoconversion(q_c, rho_d):                         # :197-206
    q = 0.001 * (q_c - 0.001)
    return np.where(q < 0.0, 0.0, q)


def f_ice(Tk):                                          # :219-227
    return np.where(Tk < 273.15, 0.2 + 0.8 * (1.0 / np.cosh((273.15 - Tk) / 5.0)), 1.0)


def collection(q_c, q_r, rho_d, Tk):                    # :208-217
    q = 2.20 * q_c * q_r ** 0.875 * f_ice(Tk)
    return np.where(q < 0.0, 0.0, q)


def f_ventilation(q_r, rho_d, Tk):                      # :243-250
    f = 1.6 + 30.39 * (q_r * rho_d) ** 0.2046 * f_ice(Tk) ** 1.5
    return np.where(f < 0.0, 0.0, f)


def rain_evaporation(q_r, rho_d, Tk, p):                # :229-241
    rho_vs = sat_pressure_liquid_buck(Tk, p) / (TH["Rv"] * Tk)
    q = (f_ventilation(q_r, rho_d, Tk) * (q_r * rho_d) ** 0.525) / (1.0e4 * ((2.03 * rho_vs) + (3.337 / Tk)))
    return np.where(q < 0.0, 0.0, q)


def sedimentation(q_r, rho_d, Tk):                      # :252-261
    Vt = -14.164 * (q_r * rho_d) ** 0.1364 * (TH["rho_d0"] / rho_d) ** 0.5 * f_ice(Tk)
    return np.where(Vt < 0.0, 0.0, Vt)


def sedimentation_flux(grid, q_r, rho_d, Tk):
    """Vt_flux = CIx(q_r .* Vt) ./ rho_d through the mu_r column's filtered Chebyshev derivative (src/testModels.jl:521-528);
    zero for every finite state (the library drops it)."""
    nz = grid.zDim
    Vt = sedimentation(q_r, rho_d, Tk)
    col = (q_r * Vt).reshape(-1, nz)
    return (col @ grid.cheb("mu_r").Vdz.T).reshape(-1) / rho_d


def thermo_state(s, xi, mu, mu_c, mu_r, sbar, xibar, mubar):
    """thermodynamic_tuple of the totals plus q_c, q_r, q_l (src/testModels.jl:474-484, src/microphysics.jl:166-178)."""
    mu_total = mu + mubar
    q_v = O.th_ahyp(mu_total)
    rho_d = O.th_dry_density(xi + xibar)
    Tk = O.th_temperature(s + sbar, rho_d, q_v)
    q_c, q_r = O.th_ahyp(mu_c), O.th_ahyp(mu_r)
    return dict(mu_total=mu_total, q_v=q_v, rho_d=rho_d, Tk=Tk, p=pressure(Tk, rho_d, q_v), q_c=q_c, q_r=q_r, q_l=q_c + q_r)


def _levels(par, N, nz):
    rs, lev = par["ref_state"], np.arange(N) % nz
    return {k + suf: rs[k][lev, j] for k in ("sbar", "xibar", "mubar") for j, suf in enumerate(("", "_z", "_zz"))}


# ----------------------------------------------------------------------------- tendency
def rates(grid, par, phys):
    """Every microphysical rate of the tendency, [N] each: q_cond, s_cond, q_evap, qss_cond, q_auto, q_coll, Vt_flux."""
    return tendency(grid, SET, par, phys, None, full=True)[3]


def tendency(grid, eq, par, phys, pts, col_ops=None, full=False):
    """src/testModels.jl:387-570, term by term in the reference's order (the library's k_phys_pointwise-style k_phys_rain evaluates
    the same expressions, without the sedimentation flux)."""
    assert eq == SET
    N = phys.shape[0]
    P = lambda v, s: phys[:, v - 1, grid.slots.index(s)]
    K, Pxi_bar = par["K"], par["Pxi_bar"]
    R = _levels(par, N, grid.zDim)
    u, w = P(4, "u"), P(5, "u")
    T = thermo_state(P(1, "u"), P(2, "u"), P(3, "u"), P(6, "u"), P(7, "u"), R["sbar"], R["xibar"], R["mubar"])
    q_v, rho_d, Tk, p, q_c, q_r, q_l = (T[k] for k in ("q_v", "rho_d", "Tk", "p", "q_c", "q_r", "q_l"))
    rho_t = rho_d * (1.0 + (q_v + q_l))
    mu_factor = O.th_dmudq(T["mu_total"], q_v)
    qvp_x, qvp_z = P(3, "r") / mu_factor, P(3, "z") / mu_factor
    rhobar = O.th_dry_density(R["xibar"]) * (1.0 + O.th_ahyp(R["mubar"]))
    rho_p = rho_t - rhobar
    dpdx = O.th_pressure_gradient(Tk, rho_d, q_v, P(1, "r"), P(2, "r"), qvp_x)
    dpdz = O.th_pressure_gradient(Tk, rho_d, q_v, P(1, "z"), P(2, "z"), qvp_z)
    Cm = (q_l * TH["Cl"]) / (TH["Cvd"] + (q_v * TH["Cvv"]) + (q_l * TH["Cl"]))
    s_div = Cm * (TH["Rd"] + q_v * TH["Rv"]) * (P(4, "r") + P(5, "z"))
    qss = P(8, "u")
    q_cond = q_condensation(qss, Tk, p, q_v, q_l, N_C, R_C)
    s_cond = s_condensation(q_cond, Tk, rho_d, q_v, q_l, p)
    cloudtau = invtau_condensation(Tk, p, N_C, R_C)
    raintau = rain_evaporation(q_r, rho_d, Tk, p)
    q_evap = -qss * raintau
    qss_cond = dqsdp(Tk, p, rho_d, q_v, q_l) * ((u * dpdx) + (w * (dpdz - rhobar * TH["gravity"]))) - qss * (cloudtau + raintau)
    q_auto = autoconversion(q_c, rho_d)
    q_coll = collection(q_c, q_r, rho_d, Tk)
    Vt_flux = sedimentation_flux(grid, q_r, rho_d, Tk)
    adv = lambda v, bar_z=0.0: (-u * P(v, "r")) + (-w * (P(v, "z") + bar_z))
    dif = lambda v: K * (P(v, "rr") + P(v, "zz"))
    E = np.zeros((N, grid.V))
    I = np.zeros((N, grid.V))
    E[:, 0] = adv(1, R["sbar_z"]) + (s_cond + s_div) + dif(1)
    E[:, 1] = adv(2, R["xibar_z"]) + (-P(4, "r") - P(5, "z"))
    I[:, 1] = -P(5, "z")
    E[:, 2] = adv(3, R["mubar_z"]) + (mu_factor * (q_evap - q_cond)) + dif(3)
    I[:, 2] = q_v
    E[:, 3] = adv(4) + (-dpdx / rho_t) + dif(4)
    E[:, 4] = adv(5) + (((-TH["gravity"] * rho_p) - dpdz) / rho_t) + dif(5)
    I[:, 4] = -(Pxi_bar * P(2, "z"))
    E[:, 5] = adv(6) + (O.th_dmudq(P(6, "u"), q_c) * (q_cond - q_auto - q_coll)) + dif(6)
    E[:, 6] = adv(7) + (O.th_dmudq(P(7, "u"), q_r) * (q_auto + q_coll - q_evap - Vt_flux)) + dif(7)
    E[:, 7] = adv(8) + qss_cond
    I[:, 7] = qss
    if full:
        return E, I, phys, dict(q_cond=q_cond, s_cond=s_cond, q_evap=q_evap, qss_cond=qss_cond, q_auto=q_auto, q_coll=q_coll,
                                Vt_flux=Vt_flux)
    return E, I, phys


# ----------------------------------------------------------------------------- condensation_adjustment
def _isequal(a, b):
    return (np.isnan(a) & np.isnan(b)) | ((np.signbit(a) == np.signbit(b)) & (a == b))


def _isless(a, b):
    return (~np.isnan(a) & (np.isnan(b) | (np.signbit(a) & ~np.signbit(b)))) | (a < b)


def column_isless(a, b):
    """Julia's isless(a, b) of two vectors, per row of [ncol, nz]: cmp walks to the first index where !isequal and compares
    with isless there; equal vectors are not less."""
    diff = ~_isequal(a, b)
    first = np.argmax(diff, axis=1)
    rows = np.arange(a.shape[0])
    return diff.any(axis=1) & _isless(a[rows, first], b[rows, first])


def column_min(x, y):
    """Julia's min(x, y) = ifelse(isless(y, x), y, x) on vectors, per row: one of the two rows whole."""
    return np.where(column_isless(y, x)[:, None], y, x)


def column_max(x, y):
    """max(x, y) = ifelse(isless(y, x), x, y)"""
    return np.where(column_isless(y, x)[:, None], x, y)


def condensation_adjustment(np1, par, nz, elementwise=False):
    """src/microphysics.jl:139-195 on var_np1 [N, V] of one tile (whole columns, z fastest); returns the adjusted copy.
    elementwise=True clamps point by point instead - not the reference; only to show that a case tells the two apart."""
    out = np1.copy()
    R = _levels(par, np1.shape[0], nz)
    s, xi, mu, mu_c, mu_r, qss = (np1[:, v] for v in (0, 1, 2, 5, 6, 7))
    T = thermo_state(s, xi, mu, mu_c, mu_r, R["sbar"], R["xibar"], R["mubar"])
    q_v, Tk, p, q_c, q_l = T["q_v"], T["Tk"], T["p"], T["q_c"], T["q_l"]
    q_sat = q_sat_liquid(Tk, p)
    Q_s = Q_s_factor(Tk, p, q_v, q_l)
    q_cond = (q_v - q_sat - qss) / (1.0 + Q_s)
    if elementwise:
        q_cond = jl_max(-q_c, jl_min(q_v, q_cond))
    else:
        col = lambda a: a.reshape(-1, nz)
        q_cond = column_min(col(q_v), col(q_cond))
        q_cond = column_max(col(-q_c), q_cond).reshape(-1)
    out[:, 2] = mu - TAU_R * O.th_dmudq(T["mu_total"], q_v) * q_cond
    out[:, 5] = mu_c + TAU_R * O.th_dmudq(mu_c, q_c) * q_cond
    out[:, 0] = s + TAU_R * s_condensation(q_cond, Tk, T["rho_d"], q_v, q_l, p)
    return out


class RainModel(O.Model):
    """oracle_np.Model whose step runs condensation_adjustment after explicit_timestep and the semi-implicit adjustment
    (src/testModels.jl:572-580).  `elementwise = True` selects the point-by-point clamp (not the reference)."""
    elementwise = False

    def step(self):
        if self.eq != SET:
            return super().step()
        self.t += 1
        t, g = self.t, self.g
        shared = np.zeros((g.S_patch(), g.V))
        for i, (c0, n) in enumerate(self.tiles):
            phys = g.inverse(self.A, c0, n)
            pts = g.gridpoints(c0, n)
            pts = pts.reshape(len(pts), -1)
            E, I, phys = O.tendency(g, self.eq, self.par, phys, pts)
            hs = self.hist[i]
            if t == 1:
                hs["e1"] = np.zeros_like(E)
                hs["e2"] = np.zeros_like(E)
            unp1, hs["e1"], hs["e2"] = O.explicit_timestep(t, self.ts, phys[:, :, 0], E, hs["e1"], hs["e2"])
            if self.semi:
                unp1 = self._semiimplicit(i, t, unp1, I)
            unp1 = condensation_adjustment(unp1, self.par, g.zDim, self.elementwise)
            b = g.forward(unp1, c0, n)
            g.add_tile_to_shared(shared, b, c0, n, i == len(self.tiles) - 1)
        self.A = g.spline_transform(shared)


def patch_oracle(monkeypatch):
    """Route rainfall_test through `tendency` and `RainModel` above for the duration of one test."""
    original = O.tendency

    def wrapped(grid, eq, par, phys, pts, col_ops=None):
        if eq == SET:
            return tendency(grid, eq, par, phys, pts)
        return original(grid, eq, par, phys, pts, col_ops)
    monkeypatch.setattr(O, "tendency", wrapped)
    monkeypatch.setattr(O, "Model", RainModel)


# ----------------------------------------------------------------------------- cases (tests/cases.py dictionaries)
def reference_profiles(z, rh=0.97, rh_sfc=0.8, T0=300.0, lapse=6.5e-3, H=8.0e3):
    """A near-saturated sounding: T = T0 - lapse z, p = 1000 hPa exp(-z / H), q_v = RH q_sat(T, p) with RH from rh_sfc at the
    ground to rh aloft; as (sbar, xibar, mubar) through src/thermodynamics.jl's entropy / log_dry_density / bhyp."""
    import scythe_jl_amd.thermodynamics as ST
    Tk = T0 - lapse * z
    p = 1000.0 * np.exp(-z / H)
    q_v = (rh - (rh - rh_sfc) * np.exp(-z / 1.5e3)) * q_sat_liquid(Tk, p)
    e = vapor_pressure(p, q_v)
    rho_d = 100.0 * (p - e) / (TH["Rd"] * Tk)
    s = np.array([ST.entropy(float(a), float(b), float(c)) for a, b, c in zip(Tk, rho_d, q_v)])
    return dict(sbar=s, xibar=np.log(rho_d / TH["rho_d0"]), mubar=np.array([ST.bhyp(float(q)) for q in q_v]))


def ref_state(zmax, zDim, **kw):
    """[zDim, 3] value / d/dz / d2/dz2 per profile from the oracle's filtered Chebyshev operators, as cases.rz_euler does."""
    ch = O.Cheb(0.0, zmax, zDim, bdim=zDim)
    ref = {}
    for k, v in reference_profiles(ch.z, **kw).items():
        b = ch.CBm @ v
        ref[k] = np.stack([ch.M[0] @ b, ch.M[1] @ b, ch.M[2] @ b], axis=1)
    return ref


def rz_rain(num_cells=8, zDim=12, semiimplicit=True, ts=None, xmax=2.0e4, zmax=1.0e4, K=10.0, Pxi_bar=1.0e5, rh=1.02, rh_sfc=1.02,
            cloud_floor=5.0e-4, rain_floor=2.0e-5, qss_amp=4.0e-5):
    """rainfall_test about a near-saturated sounding: a warm, moist bubble; a cloud layer with q_c up to 2.5e-3 over a floor
    (autoconversion above 1e-3) and rain up to 1e-3 (collection, evaporation); qss of both signs; mu + mubar > 0 everywhere.

    The ground level decides condensation_adjustment's two clamps for the whole column.  The default sounding is slightly
    supersaturated at every level, so every column keeps the raw q_cond and condenses: the run stays smooth for tens of steps.
    With rh_sfc < 1 (subsaturated ground) every column takes q_cond = -q_c instead, and with rh_sfc = 1 and a large qss_amp the
    sign of qss at the ground picks the clamp column by column - the cases that tell the whole-column rule from a pointwise
    one.  Where a column keeps q_cond < -q_c, or the tendency's q_cond (clamped at -q_l, rain included) outruns the cloud,
    mu_c falls below zero and dmudq(mu_c, 0) = 1 - mu_c / q0 multiplies the next tendency by up to 10^3 - the reference's own
    behaviour, so such runs are kept short."""
    ref = ref_state(zmax, zDim, rh=rh, rh_sfc=rh_sfc)
    from scythe_jl_amd import thermodynamics as ST

    def ic(p):
        r, z = p[:, 0], p[:, 1]
        b = np.exp(-((r - 0.5 * xmax) / (0.2 * xmax)) ** 2 - ((z - 0.4 * zmax) / (0.2 * zmax)) ** 2)
        s_ = np.sin(np.pi * z / zmax)
        cloud = cloud_floor + 2.5e-3 * np.exp(-((r - 0.45 * xmax) / (0.3 * xmax)) ** 2 - ((z - 0.45 * zmax) / (0.2 * zmax)) ** 2)
        rain = rain_floor + 1.0e-3 * np.exp(-((r - 0.55 * xmax) / (0.3 * xmax)) ** 2 - ((z - 0.35 * zmax) / (0.25 * zmax)) ** 2)
        bh = np.vectorize(lambda q: ST.bhyp(float(q)))
        qss = qss_amp * (b * np.cos(2.0 * np.pi * r / xmax) + 0.25 * np.sin(3.0 * np.pi * z / zmax) +
                         0.5 * np.cos(3.0 * np.pi * r / xmax) * np.exp(-z / 1.0e3))
        return np.stack([0.5 * b, 1.0e-4 * b, 2.0e-4 * b, 0.5 * s_ * b, 0.2 * s_ * b, bh(cloud), bh(rain), qss], axis=1)
    grid = dict(geometry="RZ", xmin=0.0, xmax=xmax, num_cells=num_cells, zmin=0.0, zmax=zmax, zDim=zDim, b_zDim=zDim, vars=dict(VARS),
                BCB={"w": "R1T0"}, BCT={"w": "R1T0"})
    if ts is None:
        ts = 1.0 if semiimplicit else 0.1
    return dict(name="rz_rain", grid=grid, eq=SET, ts=ts, par=dict(K=K, Pxi_bar=Pxi_bar, ref_state=ref), ic=ic,
                semiimplicit=semiimplicit)


def rz_rain_mixed(**kw):
    """Saturated ground with qss of +-4e-4 there: the clamps differ from column to column (short runs only, see rz_rain)."""
    return rz_rain(**dict(dict(rh=0.97, rh_sfc=1.0, cloud_floor=2.0e-5, qss_amp=4.0e-4), **kw))
