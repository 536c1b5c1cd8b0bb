"""LinearShallowWater1D and LinearShallowWaterRL (src/shallowWaterModels.jl:235-298) for the tests: the variable maps, the cases
and the closed-form solutions the sets admit.  The tendency lives in oracle/oracle_np.py with the other equation sets."""
import numpy as np

SETS = ("LinearShallowWater1D", "LinearShallowWaterRL")
VARS_1D = {"h": 1, "u": 2}
VARS_RL = {"h": 1, "u": 2, "v": 3}


# ----------------------------------------------------------------------------- cases (tests/cases.py dictionaries)
def r_case(num_cells=24, bc="PERIODIC", g=2.0, H=0.5, K=0.02, ts=0.02):
    """R grid. PERIODIC on [-6, 6]; otherwise walls on [0, 12]: u R1T0 (no flow through), h R1T1 (no gradient)."""
    if bc == "PERIODIC":
        grid = dict(geometry="R", xmin=-6.0, xmax=6.0, num_cells=num_cells, vars=VARS_1D,
                    BCL={"h": "PERIODIC", "u": "PERIODIC"}, BCR={"h": "PERIODIC", "u": "PERIODIC"})
    else:
        grid = dict(geometry="R", xmin=0.0, xmax=12.0, num_cells=num_cells, vars=VARS_1D,
                    BCL={"h": "R1T1", "u": "R1T0"}, BCR={"h": "R1T1", "u": "R1T0"})
    x0, L = grid["xmin"], grid["xmax"] - grid["xmin"]

    def ic(p):
        s = (p[:, 0] - x0) / L
        h = np.exp(-((s - 0.4) / 0.12) ** 2) + 0.3 * np.cos(2.0 * np.pi * s)
        u = 0.5 * np.sin(2.0 * np.pi * s) * (1.0 if bc == "PERIODIC" else np.sin(np.pi * s))
        return np.stack([h, u], axis=1)
    return dict(name="lsw1d_" + bc, grid=grid, eq="LinearShallowWater1D", ts=ts, par=dict(g=g, K=K, H=H), ic=ic)


def rl_case(num_cells=8, ring_L=None, g=2.0, H=0.5, K=0.004, ts=0.005, xmax=10.0, bcl=None, bcr=None):
    """RL grid: h, u, v with radial structure and azimuthal wavenumbers 1, 2 and 3 in every variable."""
    def ic(p):
        r, l = p[:, 0], p[:, 1]
        s = r / xmax
        e = np.exp(-((r - 0.45 * xmax) / (0.2 * xmax)) ** 2)
        h = e * (1.0 + 0.4 * np.cos(l) * s + 0.25 * np.sin(2.0 * l + 0.3) * s * s) + 0.2 * s * s * np.cos(3.0 * l)
        u = 0.3 * e * np.sin(l + 0.2) * s + 0.1 * s * s * np.cos(2.0 * l)
        v = 0.2 * e * (1.0 + np.cos(3.0 * l - 0.5)) * s + 0.15 * s * np.sin(l)
        return np.stack([h, u, v], axis=1)
    grid = dict(geometry="RL", xmin=0.0, xmax=xmax, num_cells=num_cells, vars=VARS_RL, ring_L=ring_L)
    if bcl:
        grid["BCL"] = bcl
    if bcr:
        grid["BCR"] = bcr
    return dict(name="lswrl", grid=grid, eq="LinearShallowWaterRL", ts=ts, par=dict(g=g, K=K, H=H), ic=ic)


# ----------------------------------------------------------------------------- closed forms
def mode_1d(x, t, kap, g, H, K, h0=1.0 + 0.0j, u0=0.0j):
    """One Fourier mode exp(i kap x) of LinearShallowWater1D on a periodic line: d/dt [h^, u^] = M [h^, u^] with
    M = [[0, -i H kap], [-i g kap, -K kap^2]] (h_t = -H u_x, u_t = -g h_x + K u_xx), advanced with the matrix exponential."""
    from scipy.linalg import expm
    M = np.array([[0.0, -1j * H * kap], [-1j * g * kap, -K * kap * kap]])
    hh, uh = expm(M * t) @ np.array([h0, u0])
    ph = np.exp(1j * kap * x)
    return (hh * ph).real, (uh * ph).real


def bessel_gravity_mode(r, lam, t, m, kap, g, H):
    """K = 0: h = J_m(kap r) cos(m lam - w t), u = (g kap / w) J_m'(kap r) sin(m lam - w t), v = (g m / (w r)) J_m(kap r)
    cos(m lam - w t), w = kap sqrt(g H), solves LinearShallowWaterRL exactly (h_t = -H (u / r + u_r + v_l / r),
    u_t = -g h_r, v_t = -g h_l / r; Bessel's equation closes the first)."""
    from scipy.special import jv, jvp
    w = kap * np.sqrt(g * H)
    ph = m * lam - w * t
    J = jv(m, kap * r)
    return J * np.cos(ph), (g * kap / w) * jvp(m, kap * r) * np.sin(ph), (g * m / (w * r)) * J * np.cos(ph)
