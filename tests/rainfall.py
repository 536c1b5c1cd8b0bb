"""rainfall_test (src/testModels.jl:387-585) for the tests: the variable map and the cases.  The tendency and
condensation_adjustment (src/microphysics.jl:139-195) live in oracle/oracle_np.py with the other equation sets."""
import numpy as np

from oracle import oracle_np as O

VARS = {"s": 1, "xi": 2, "mu": 3, "u": 4, "w": 5, "mu_c": 6, "mu_r": 7, "qss": 8}


# ----------------------------------------------------------------------------- cases (tests/cases.py dictionaries)
def reference_profiles(z, rh=0.97, rh_sfc=0.8, T0=300.0, lapse=6.5e-3, H=8.0e3):
    """A near-saturated sounding: T = T0 - lapse z, p = 1000 hPa exp(-z / H), q_v = RH q_sat(T, p) with RH from rh_sfc at the
    ground to rh aloft; as (sbar, xibar, mubar) through src/thermodynamics.jl's entropy / log_dry_density / bhyp."""
    import scythe_jl_amd.thermodynamics as ST
    Tk = T0 - lapse * z
    p = 1000.0 * np.exp(-z / H)
    q_v = (rh - (rh - rh_sfc) * np.exp(-z / 1.5e3)) * O.th_q_sat_liquid(Tk, p)
    e = O.th_vapor_pressure(p, q_v)
    rho_d = 100.0 * (p - e) / (O.TH["Rd"] * Tk)
    s = np.array([ST.entropy(float(a), float(b), float(c)) for a, b, c in zip(Tk, rho_d, q_v)])
    return dict(sbar=s, xibar=np.log(rho_d / O.TH["rho_d0"]), mubar=np.array([ST.bhyp(float(q)) for q in q_v]))


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
    return dict(name="rz_rain", grid=grid, eq="rainfall_test", ts=ts, par=dict(K=K, Pxi_bar=Pxi_bar, ref_state=ref), ic=ic,
                semiimplicit=semiimplicit)


def rz_rain_mixed(**kw):
    """Saturated ground with qss of +-4e-4 there: the clamps differ from column to column (short runs only, see rz_rain)."""
    return rz_rain(**dict(dict(rh=0.97, rh_sfc=1.0, cloud_floor=2.0e-5, qss_amp=4.0e-4), **kw))
