"""Shared test cases: one description drives the CPU oracle (oracle/) and the HIP path (scythe.jl_amd)."""
import os
from unittest import mock

import numpy as np

from oracle import oracle_np as O
from oracle import oracle_c as OC

VARS6 = {"h": 1, "u": 2, "v": 3, "ub": 4, "vb": 5, "wb": 6}
BCL6 = {"h": "R1T1", "u": "R1T0", "v": "R1T0", "ub": "R1T0", "vb": "R1T0", "wb": "R1T1"}   # models/cha_bell2024
BCR6 = {"h": "R0", "u": "R1T1", "v": "R0", "ub": "R1T1", "vb": "R0", "wb": "R0"}
GEOM = {"R": 0, "RZ": 1, "RL": 2, "RLZ": 3}      # SX_GEOM_* (include/scythe_hip.h)
SW_PAR = dict(g=9.81, K=5000.0, Cd=2.4e-3, Hfree=2000.0, Hb=1000.0, f=5.0e-5, S1=1.0e-4, Kh=5000.0, Um=2.0, Vm=-1.0)


def _vortex(r):
    Rmax, V0 = 5.0e4, 50.0 / 5.0e4
    return np.where(r < Rmax, V0 * r, Rmax * Rmax * V0 / np.maximum(r, 1.0))


def kat_r(num_cells=100):
    """models/LinearAdvection1D.jl with the notebook's initial condition."""
    return dict(name="kat_r", grid=dict(geometry="R", xmin=-50.0, xmax=50.0, num_cells=num_cells, vars={"u": 1},
                                        BCL={"u": "PERIODIC"}, BCR={"u": "PERIODIC"}),
                eq="LinearAdvection1D", ts=0.05, par=dict(c_0=1.0, K=0.0),
                ic=lambda p: np.exp(-(p[:, 0] / 20.0) ** 2)[:, None])


def r_bcs(bcl="R1T0", bcr="R1T1", num_cells=24):
    return dict(name="r_%s_%s" % (bcl, bcr), grid=dict(geometry="R", xmin=0.0, xmax=12.0, num_cells=num_cells, vars={"u": 1},
                                                      BCL={"u": bcl}, BCR={"u": bcr}),
                eq="LinearAdvection1D", ts=0.01, par=dict(c_0=0.5, K=0.02),
                ic=lambda p: (np.sin(np.pi * p[:, 0] / 12.0) ** 2 * np.exp(-((p[:, 0] - 5.0) / 2.0) ** 2))[:, None])


def rz_advection(num_cells=10, zDim=14):
    def ic(p):
        r, z = p[:, 0], p[:, 1]
        b = np.exp(-((r - 5.0e3) / 2.0e3) ** 2 - ((z - 4.0e3) / 2.5e3) ** 2)
        return np.stack([b, 2.0 + 0.0 * r, 0.0 * r, 0.5 * np.sin(np.pi * z / 1.0e4)], axis=1)
    return dict(name="rz_adv", grid=dict(geometry="RZ", xmin=0.0, xmax=1.0e4, num_cells=num_cells, zmin=0.0, zmax=1.0e4,
                                         zDim=zDim, vars={"h": 1, "u": 2, "v": 3, "w": 4}, BCL={"h": "R1T1"},
                                         BCB={"w": "R1T0"}, BCT={"w": "R1T0"}),
                eq="LinearAdvectionRZ", ts=1.0, par=dict(K=20.0), ic=ic)


def rz_semiimplicit(num_cells=8, zDim=12):
    def ic(p):
        r, z = p[:, 0], p[:, 1]
        b = np.exp(-((r - 5.0e3) / 2.0e3) ** 2 - ((z - 5.0e3) / 2.0e3) ** 2)
        s = np.sin(np.pi * z / 1.0e4)
        return np.stack([b, 1.0e-3 * b, 0.5 * b, s * b, 0.5 * s * b], axis=1)
    return dict(name="rz_semi", grid=dict(geometry="RZ", xmin=0.0, xmax=1.0e4, num_cells=num_cells, zmin=0.0, zmax=1.0e4,
                                          zDim=zDim, b_zDim=zDim, vars={"s": 1, "xi": 2, "mu": 3, "u": 4, "w": 5},
                                          BCB={"w": "R1T0"}, BCT={"w": "R1T0"}),
                eq="LinearAcousticRZ", ts=2.0, par=dict(K=10.0, Pxi_bar=1.2e5), ic=ic, semiimplicit=True)


def rz_euler(num_cells=8, zDim=12, semiimplicit=True):
    """Euler_test (src/testModels.jl:100-215) about a stably stratified, slightly moist reference state.  The reference
    profiles are analytic; their derivative columns come from the ORACLE's Chebyshev operators (the same filtered
    CB -> CA -> CI / CIx / CIxx the reference applies, src/reference_state.jl:140-160) and are handed to both sides."""
    zmax = 1.0e4
    ch = O.Cheb(0.0, zmax, zDim, bdim=zDim)
    z = ch.z
    prof = dict(sbar=20.0 + 0.012 * z, xibar=-z / 8.5e3, mubar=0.5 * ((4e-3 * np.exp(-z / 2.5e3) + 1e-7) - 1e-14 / (4e-3 * np.exp(-z / 2.5e3) + 1e-7)))
    ref = {}
    for k, v in prof.items():
        b = ch.CBm @ v
        ref[k] = np.stack([ch.M[0] @ b, ch.M[1] @ b, ch.M[2] @ b], axis=1)

    def ic(p):
        r, zz = p[:, 0], p[:, 1]
        b = np.exp(-((r - 1.0e4) / 4.0e3) ** 2 - ((zz - 4.0e3) / 2.0e3) ** 2)
        s_ = np.sin(np.pi * zz / zmax)
        return np.stack([0.5 * b, 1.0e-4 * b, 2.0e-4 * b, 0.5 * s_ * b, 0.2 * s_ * b], axis=1)
    par = dict(K=10.0, Pxi_bar=1.0e5, ref_state=ref)
    return dict(name="rz_euler", grid=dict(geometry="RZ", xmin=0.0, xmax=2.0e4, num_cells=num_cells, zmin=0.0, zmax=zmax,
                                           zDim=zDim, b_zDim=zDim, vars={"s": 1, "xi": 2, "mu": 3, "u": 4, "w": 5},
                                           BCB={"w": "R1T0"}, BCT={"w": "R1T0"}),
                eq="Euler_test", ts=1.0, par=par, ic=ic, semiimplicit=semiimplicit)


def rl_advection(num_cells=8, ring_L=None):
    def ic(p):
        r, l = p[:, 0], p[:, 1]
        e = np.exp(-(r / 4.0) ** 2)
        return np.stack([e * (1 + (r / 4) ** 2 * np.cos(2 * l) + (r / 4) * np.sin(l)), 0.3 + 0 * r, 0.2 * r], axis=1)
    return dict(name="rl_adv", grid=dict(geometry="RL", xmin=0.0, xmax=10.0, num_cells=num_cells, vars={"h": 1, "u": 2, "v": 3},
                                         ring_L=ring_L),
                eq="LinearAdvectionRL", ts=0.01, par=dict(K=0.003), ic=ic)


def rl_slab(num_cells=8, twoway=False, ring_L=None):
    """models/cha_bell2024/*.jl boundary conditions and parameters on a small patch."""
    def ic(p):
        r, l = p[:, 0], p[:, 1]
        vb = _vortex(r)
        h = 100.0 * np.exp(-(r / 1.0e5) ** 2) * (1 + 0.1 * np.cos(2 * l))
        u = 0.5 * np.sin(l) * r / 3.0e5
        return np.stack([h, u, vb * (1 + 0.05 * np.cos(l)), 0.8 * u, 0.7 * vb, 0.0 * r], axis=1)
    return dict(name="rl_slab", grid=dict(geometry="RL", xmin=0.0, xmax=3.0e5, num_cells=num_cells, vars=VARS6, BCL=BCL6,
                                          BCR=BCR6, ring_L=ring_L),
                eq="Twoway_ShallowWater_Slab" if twoway else "Oneway_ShallowWater_Slab", ts=3.0, par=dict(SW_PAR), ic=ic)


def rlz_hrbl(num_cells=5, zDim=10, ring_L=None):
    def ic(p):
        r, l, z = p.T
        vb = _vortex(r)
        dec = 1.0 - np.exp(-(z + 50.0) / 300.0)
        h = 100.0 * np.exp(-(r / 1.0e5) ** 2) * (1 + 0.1 * np.cos(2 * l))
        u = 0.5 * np.sin(l) * r / 3.0e5
        return np.stack([h, u, vb * (1 + 0.05 * np.cos(l)), (u - 2.0 * r / 3.0e5) * dec, 0.7 * vb * dec, 0.0 * r], axis=1)
    return dict(name="rlz_hrbl", grid=dict(geometry="RLZ", xmin=0.0, xmax=3.0e5, num_cells=num_cells, vars=VARS6, BCL=BCL6,
                                           BCR=BCR6, zmin=0.0, zmax=2000.0, zDim=zDim, ring_L=ring_L),
                eq="Oneway_ShallowWater_HeightResolvedBL", ts=3.0, par=dict(SW_PAR), ic=ic)


def rlz_advection(num_cells=4, zDim=9, ring_L=None):
    def ic(p):
        r, l, z = p.T
        e = np.exp(-(r / 4.0) ** 2) * np.cos(0.4 * z)
        return np.stack([e * (1 + (r / 4) * np.sin(l)), 0.3 + 0 * r, 0.2 * r], axis=1)
    return dict(name="rlz_adv", grid=dict(geometry="RLZ", xmin=0.0, xmax=10.0, num_cells=num_cells, vars={"h": 1, "u": 2, "v": 3},
                                          zmin=0.0, zmax=3.0, zDim=zDim, ring_L=ring_L, BCB={"h": "R1T1"}),
                eq="LinearAdvectionRLZ", ts=0.01, par=dict(K=0.003), ic=ic)


def kat_in_geometry(geometry, ring_L=8, zDim=4):
    """The notebook's known answer (models/LinearAdvection1D.jl: u_t = -c_0 u_r, PERIODIC, 100 cells on [-50, 50], ts 0.05)
    posed on an RZ / RL / RLZ grid: LinearAdvectionRZ / RL / RLZ with K = 0, a unit radial wind and a field that does not
    depend on lambda or z integrate the same equation at every (lambda, z), so the notebook's printed values must come out at
    every ring point and level - the reference's only fixture, carried through the azimuthal and vertical transform paths."""
    nv = {"h": 1, "u": 2, "v": 3, "w": 4} if geometry == "RZ" else {"h": 1, "u": 2, "v": 3}
    grid = dict(geometry=geometry, xmin=-50.0, xmax=50.0, num_cells=100, vars=nv, BCL={k: "PERIODIC" for k in nv},
                BCR={k: "PERIODIC" for k in nv})
    if "Z" in geometry:
        grid.update(zmin=0.0, zmax=1.0, zDim=zDim)
    if "L" in geometry:
        grid.update(ring_L=ring_L)

    def ic(p):
        v = np.zeros((len(p), len(nv)))
        v[:, 0], v[:, 1] = np.exp(-(p[:, 0] / 20.0) ** 2), 1.0
        return v
    return dict(name="kat_" + geometry, grid=grid, eq="LinearAdvection" + geometry, ts=0.05, par=dict(K=0.0), ic=ic)


def kat_deviation(model, kat, steps=2000):
    """max relative deviation of the field from the notebook's printed values, over every ring point and level at those radii"""
    for _ in range(steps):
        model.step()
    ph = model.physical()
    r = model.pts[:, 0] if hasattr(model, "pts") else None
    if r is None:
        import scythe_jl_amd as S
        pts = np.concatenate([S.getGridpoints(g).reshape(g.N, -1) for g in model.run.tiles], axis=0)
        r = pts[:, 0]
    worst = 0.0
    for x, u in zip(kat["gridpoints"], kat["final_u"]):
        sel = np.abs(r - x) < 1e-9
        assert sel.any()
        worst = max(worst, np.abs(ph[sel, 0, 0] / u - 1.0).max())
    return worst


# ----------------------------------------------------------------------------- builders
def oracle_grid(case):
    g = dict(case["grid"])
    return O.Grid(g.pop("geometry"), g.pop("xmin"), g.pop("xmax"), g.pop("num_cells"), g.pop("vars"), **g)


def even_tiles(nc, n):
    sizes = [nc // n + (1 if t < nc % n else 0) for t in range(n)]
    out, c0 = [], 0
    for s in sizes:
        out.append((c0, s))
        c0 += s
    return out


class OracleModel:
    """C-oracle model (optionally split into tiles) started from the case's initial condition."""

    def __init__(self, case, tiles=None, numpy_twin=False, helmholtz="extended"):
        """helmholtz="lu" (numpy twin only): the reference's Float64 LU arithmetic for the semi-implicit column solve."""
        self.g = oracle_grid(case)
        if numpy_twin or helmholtz != "extended":
            self.m = O.Model(self.g, case["eq"], case["ts"], case["par"], tiles=tiles,
                             semiimplicit=case.get("semiimplicit", False), pxi_bar=case["par"].get("Pxi_bar", 0.0),
                             helmholtz=helmholtz)
        else:
            self.m = OC.ModelOracle(self.g, case["eq"], case["ts"], case["par"], tiles=tiles,
                                    semiimplicit=case.get("semiimplicit", False))
        pts = self.g.gridpoints()
        self.pts = pts.reshape(len(pts), -1)
        self.m.set_initial(case["ic"](self.pts))

    def step(self):
        self.m.step()

    def physical(self):
        return self.m.physical()

    @property
    def A(self):
        return self.m.A


def hip_params(case, storage="f64"):
    import scythe_jl_amd as S
    g = dict(case["grid"])
    ring_L = g.pop("ring_L", None)
    gp = S.GridParameters(ring_uniform_L=ring_L or 0, storage=storage, **g)
    par = dict(case["par"])
    rs = par.pop("ref_state", None)
    mp = S.ModelParameters(ts=case["ts"], equation_set=case["eq"], grid_params=gp, physical_params=par,
                           options={"semiimplicit": case.get("semiimplicit", False)})
    if rs is not None:
        mp.ref_state = S.ReferenceState(rs["sbar"], rs["xibar"], rs["mubar"], np.zeros_like(rs["sbar"]), par["Pxi_bar"])
    return gp, mp


class HipModel:
    """The product path: tiles are libscythe_hip handles, exchange on device buffers."""

    def __init__(self, case, num_tiles=1, device="cuda", exchange="a2a", storage="f64", impl="torch"):
        """impl="lib" (num_tiles > 1): the exchange runs inside libscythe_hip.so through its loopback transport (the RCCL
        path's buffers and offset tables, copies instead of sends); "torch": the Python-side stand-in (driver.Local*Exchange)."""
        import scythe_jl_amd as S
        self.gp, self.mp = hip_params(case, storage)
        self.run = S.ModelRun(self.mp, num_tiles=num_tiles, device=device, exchange=exchange, impl=impl)
        vals = []
        for g in self.run.tiles:
            pts = S.getGridpoints(g)
            vals.append(case["ic"](pts.reshape(len(pts), -1)))
        self.run.set_initial_conditions(vals)

    def step(self):
        self.run.step()

    def physical(self):
        return self.run.physical()

    @property
    def A(self):
        if self.run.exchange_kind in ("a2a", "iface"):
            return None          # no tile holds the whole patch in the transposed / interface-only solve
        return self.run.tiles[0].patchSpectral


def rel_err(a, b):
    """max over derivative slots of max|a-b| / max|b| (per-slot scale)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 3:
        return max(np.abs(a[:, :, d] - b[:, :, d]).max() / max(np.abs(b[:, :, d]).max(), 1e-300) for d in range(a.shape[2]))
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def rel_err_per_var(a, b):
    """max over (var, slot) of max|a-b| / scale[var, slot].

    scale = max|b[:, var, slot]|, floored at gain[slot] * max|b[:, var, 0]| where gain[slot] is the largest
    derivative-to-value ratio any variable shows in that slot: a derivative slot of a field that does not vary in
    that direction holds only rounding noise, and that noise is proportional to the field's own magnitude times the
    norm of the derivative operator."""
    worst = 0.0
    vmax = [np.abs(b[:, v, 0]).max() for v in range(a.shape[1])]
    for d in range(a.shape[2]):
        gain = max((np.abs(b[:, v, d]).max() / vmax[v]) for v in range(a.shape[1]) if vmax[v] > 0)
        for v in range(a.shape[1]):
            sc = max(np.abs(b[:, v, d]).max(), gain * vmax[v])
            diff = np.abs(a[:, v, d] - b[:, v, d]).max()
            if sc > 0:
                worst = max(worst, diff / sc)
            elif diff > 0:
                return np.inf
    return worst


# ----------------------------------------------------------------------------- splineTransform! (B -> A) references
def spline_columns(x, b_rDim):
    """[s_patch, V] patch array (reference layout: s = (z-mode * n_blocks + block) * b_rDim + node) -> [columns, b_rDim]:
    one row per (variable, z-mode, wavenumber block) right-hand side of the radial solve."""
    x = np.asarray(x)
    return np.transpose(x.reshape(b_rDim, -1, x.shape[1], order="F"), (2, 1, 0)).reshape(-1, b_rDim)


def rel_err_per_column(a, b, b_rDim):
    """Per spectral column of a [s_patch, V] patch array: max|a - b| over the column / max|b| over the same column.
    A column of b that is exactly zero demands an exactly zero column of a."""
    ca, cb = spline_columns(a, b_rDim), spline_columns(b, b_rDim)
    diff, sc = np.abs(ca - cb).max(axis=1), np.abs(cb).max(axis=1)
    return np.where(sc > 0, diff / np.where(sc > 0, sc, 1.0), np.where(diff > 0, np.inf, 0.0))


def dense_spline_transform(case, shared):
    """oracle_np.Grid.spline_transform (Spline1D.SA: the dense Cholesky factor of Gamma (P + eps_q Q) Gamma^T) with each
    boundary-condition class factored once and all its columns solved in one call - for grids with 10^4 - 10^5 columns."""
    g = oracle_grid(case)
    shared = np.asarray(shared)
    A = np.zeros_like(shared)
    nb = g.b_rDim
    for vi, v in enumerate(g.names):
        X = shared[:, vi].reshape(g.b_zDim, g.K2, nb)            # [z-mode, block, node]
        Y = np.zeros_like(X)
        for blocks in (slice(0, 1), slice(1, g.K2)):
            if blocks.start >= g.K2:
                continue
            spl = g.var_spline(v, blocks.start)
            rhs = X[:, blocks, :].reshape(-1, nb).T                  # [node, columns]
            y = np.linalg.solve(spl.cho, spl.G @ rhs)
            Y[:, blocks, :] = (spl.G.T @ np.linalg.solve(spl.cho.T, y)).T.reshape(g.b_zDim, -1, nb)
        A[:, vi] = Y.reshape(-1)
    return A


def pcr_launch_geometry(case, ngroups=None, r_force=0):
    """What launch_solve_pcr (scythe.jl_amd/csrc/sx_pcr.hip) picks for one launch over `ngroups` (variable, z-mode) groups
    (default: the whole patch), from the library's own plan: R columns per workgroup, threads per workgroup; and the column
    count of the last workgroup of the k = 0 run of a variable and of a group's k >= 1 run (== R: no partial segment), and
    whether the tables exist at all (nblk_max <= 1024; else the launch falls back to k_solve).  r_force: SX_PCR_R."""
    g, K2, _ = _handle_dims(case)
    nfree = {O.gamma_matrix(g.nc, bl, g.BCR[v]).shape[0] for v in g.names for bl in (g.BCL_k0[v], g.BCL[v])}
    nblk = max((n + 2) // 3 for n in nfree)
    ng = g.V * g.b_zDim if ngroups is None else ngroups
    _, (R, _, threads, *_) = launch_plan(PLAN_PCR, nblk, g.b_rDim, K2, ng, env={"SX_PCR_R": r_force} if r_force > 0 else None)
    last = lambda n: n - (n - 1) // R * R
    return dict(R=R, threads=threads, columns=ng * (K2 - 1 if K2 > 1 else 1), nblk=nblk, tail_k0=last(g.b_zDim),
                tail_k=last(K2 - 2) if K2 > 2 else None, tables=nblk <= 1024)


# ----------------------------------------------------------------------------- BASELINE.json configs at full size
from bench_configs import config2_literal     # noqa: E402,F401  (one definition for bench.py and the tests)


def config5_case():
    """SURVEY.md 8(d) config 5 at its full size: 341 cells -> 1023 rings x 512 azimuthal points x 128 levels, HRBL set
    (bench.py --workload rlz_1023x512x128)."""
    case = rlz_hrbl(num_cells=341, zDim=128, ring_L=512)
    case["ts"] = 0.02                    # bench.TS_OF: 0.3 m end spacing of the 128-level Chebyshev column
    return case


from bench_configs import config3_rz          # noqa: E402,F401


# ----------------------------------------------------------------------------- measured accuracy of derivative slots
def ring_points(g, rings):
    """Index array of the points (z fastest) of the listed patch rings inside a one-tile physical array."""
    return np.concatenate([np.arange(g.ringstart[r] * g.zDim, (g.ringstart[r] + g.L[r]) * g.zDim) for r in rings])


def slot_errors_vs_extended(g, phys, A, rings):
    """For each derivative slot: max over variables of  max|phys - truth| / scale  on the sampled rings, where `truth` is
    the inverse transform of the SAME Float64 coefficients A evaluated in extended precision (oracle_np.inverse_xp) and
    scale is rel_err_per_var's (slot scale floored by the operator gain times the variable's magnitude).
    This measures the rounding error of one implementation's tileTransform!; it does not depend on any other one."""
    pts = {r: ring_points(g, [r]) for r in rings}
    return slot_errors_vs_extended_rings(g, {r: phys[pts[r]] for r in rings}, A, rings)


def slot_errors_vs_extended_rings(g, ring_phys, A, rings):
    """slot_errors_vs_extended with the evaluated fields given ring by ring ({ring: [L * zDim, V, D]}) - for grids whose
    whole `physical` array is never formed on the host (config 5)."""
    truth = O.inverse_xp(g, A, rings)
    t = np.concatenate([truth[r] for r in rings], axis=0)
    a = np.concatenate([ring_phys[r] for r in rings], axis=0)
    t64 = np.asarray(t, dtype=np.float64)
    vmax = [max(np.abs(t64[:, v, 0]).max(), 1e-300) for v in range(a.shape[1])]
    out = np.zeros(a.shape[2])
    for d in range(a.shape[2]):
        gain = max(np.abs(t64[:, v, d]).max() / vmax[v] for v in range(a.shape[1]))
        for v in range(a.shape[1]):
            sc = max(np.abs(t64[:, v, d]).max(), gain * vmax[v], 1e-300)
            out[d] = max(out[d], float(np.abs(a[:, v, d].astype(O.XP) - t[:, v, d]).max()) / sc)
    return out


def report_slots(title, g, rows):
    print("\n%s - max error per derivative slot, relative to the slot's scale" % title)
    print("  %-44s" % "" + "".join("%10s" % s for s in g.slots))
    for name, e in rows:
        print("  %-44s" % name + "".join("%10.1e" % x for x in e))


def per_slot_errors(a, b):
    """rel_err_per_var slot by slot: out[d] = max over variables of max|a - b| / scale[var, d], with rel_err_per_var's scale
    (the slot's own magnitude, floored by the operator gain times the variable's magnitude: a derivative slot of a field
    that does not vary in that direction holds rounding noise only)."""
    vmax = [np.abs(b[:, v, 0]).max() for v in range(a.shape[1])]
    out = np.zeros(a.shape[2])
    for d in range(a.shape[2]):
        gain = max((np.abs(b[:, v, d]).max() / vmax[v]) for v in range(a.shape[1]) if vmax[v] > 0)
        for v in range(a.shape[1]):
            sc = max(np.abs(b[:, v, d]).max(), gain * vmax[v])
            diff = np.abs(a[:, v, d] - b[:, v, d]).max()
            if sc > 0:
                out[d] = max(out[d], diff / sc)
            elif diff > 0:
                out[d] = np.inf
    return out


def check_full(hip, orc, rings, title, orc_alt=None):
    """Parity at full size, in separately measured parts:
    (1) STATE: the A coefficients and the value slot of HIP and oracle agree to 1e-10 after the steps.
    (2) TRANSFORM ACCURACY (tests/py::slot_errors_vs_extended): each side's derivative slots against the
        extended-precision evaluation of ITS OWN coefficients on a sample of rings (innermost, middle, outermost = largest
        kmax).  Demanded: the HIP path is no less accurate than the fp64 oracle, err(HIP) <= 2 err(oracle) (+ 2e-15 for
        slots the oracle happens to hit exactly).
    (3) WHOLE GRID, slot by slot, HIP vs oracle.  The derivative operators amplify the last-bit differences of two fp64
        states by k, k^2 (azimuth) or N^2, N^4 (Chebyshev), so two CORRECT runs differ in those slots by far more than
        1e-10 of the slot's scale.  The noise floor is measured, not assumed: `orc_alt` is the same oracle with the patch
        split into two tiles (another summation order of the same arithmetic); HIP must be within 10 x that floor."""
    a, b = hip.physical(), orc.physical()
    assert np.isfinite(a).all()
    eA = rel_err(hip.A, orc.A)
    vals = max(np.abs(a[:, v, 0] - b[:, v, 0]).max() / np.abs(b[:, v, 0]).max()
               for v in range(b.shape[1]) if np.abs(b[:, v, 0]).max() > 0)
    g = orc.g
    e_hip = slot_errors_vs_extended(g, a, np.asarray(hip.A), rings)
    e_orc = slot_errors_vs_extended(g, b, np.asarray(orc.A), rings)
    d = per_slot_errors(a, b)
    rows = [("HIP vs extended precision (own A)", e_hip), ("fp64 oracle vs extended precision (own A)", e_orc),
            ("HIP vs fp64 oracle (whole grid)", d)]
    floor = None
    if orc_alt is not None:
        floor = per_slot_errors(orc_alt.physical(), b)
        rows.append(("oracle, 2 tiles vs 1 tile (fp64 noise floor)", floor))
    report_slots(title + " (A coefficients %.1e, values %.1e)" % (eA, vals), g, rows)
    assert eA < 1e-10 and vals < 1e-10, (eA, vals)
    assert (e_hip <= 2.0 * e_orc + 2e-15).all(), (e_hip, e_orc)
    if floor is not None:
        assert (d <= 10.0 * floor + 1e-12).all(), (d, floor)
    return e_hip, e_orc, d




# ----------------------------------------------------------------------------- launch geometry, asked of the library
PLAN_FORWARD, PLAN_ZINV, PLAN_PCR = 0, 1, 2      # include/scythe_hip.h
_UNSET = object()


def launch_plan(kind, *dims, env=_UNSET):
    """sx_launch_plan (host only): (kernel text, [out integers]) under the SX_* switches of os.environ as it is now, or, with
    `env`, under exactly the SX_* variables of that dict (None: no switch set) whatever the caller's environment holds."""
    import ctypes as C
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    if env is not _UNSET:
        scoped = {k: v for k, v in os.environ.items() if not k.startswith("SX_")}
        scoped.update((k, str(v)) for k, v in (env or {}).items())
        with mock.patch.dict(os.environ, scoped, clear=True):
            return launch_plan(kind, *dims)
    out, name = (C.c_int32 * 6)(), C.create_string_buffer(64)
    L.check(S.load().sx_launch_plan(kind, (C.c_int32 * len(dims))(*dims), out, name, len(name)))
    return name.value.decode(), list(out)


def _handle_dims(case, tile=None):
    """(K2 of the handle, tile cells, nz, Zb) as sx_create sets them: K2 = 2 (kDim + 1) with kDim the PATCH's largest kmax."""
    g = oracle_grid(case)
    ncells = g.nc if tile is None else tile[1]
    K2 = 2 * (g.kDim + 1) if g.has_l else 1
    return g, K2, ncells


def sb_launch_geometry(case, env=None, storage="f64", tile=None, v_cnt=None):
    """What launch_sb (scythe.jl_amd/csrc/sx_kernels.hip) launches for spectralTransform! on the tile (cell0, ncells) (default:
    the whole patch) with the switches in `env` (SX_SBW_MFMA, SX_SBW_PF, SX_SBW_T256, SX_SBW_SEG, SX_RZ_FUSED) and v_cnt
    variables in the window (default: all), from the library's own plan:
      kernel (with its template arguments), threads, bw (wavenumber blocks per workgroup), groups = ceil(K2 / bw) v_cnt,
      nseg, cps = max(ncells <= 64 ? 2 : 6, ceil(ncells / nseg)) cells per segment, segs = ceil(ncells / cps);
    and what follows from those inside the kernels: last = the last segment's cells, tail = K2 % bw, and for the matrix-core
    kernels MT = ceil(Zb / 16), mhalf = ceil(MT / 2) and nmt, the row tiles of each wave of a workgroup (k_sbw_mfma's mt0 /
    mt1 / nmt)."""
    g, K2, ncells = _handle_dims(case, tile)
    Zb = g.b_zDim if g.has_z else 1
    kernel, (threads, bw, groups, nseg, cps, segs) = launch_plan(PLAN_FORWARD, GEOM[g.geometry], g.zDim if g.has_z else 1, Zb, K2,
                                                                 g.V if v_cnt is None else v_cnt, ncells, storage == "f32x", env=env)
    if not kernel:
        return dict(kernel=None, refused="storage_f32 = 2", ncells=ncells, K2=K2)       # sx_create refuses the handle
    if kernel == "k_rz_forward":
        return dict(rz_forward_launch_geometry(case, tile, v_cnt), K2=K2)
    if kernel == "k_sb":
        return dict(kernel=kernel, threads=threads, ncells=ncells, K2=K2)
    if kernel == "k_sbz":
        return dict(kernel=kernel, threads=threads, ncells=ncells, K2=K2, bw=bw, tail=K2 % bw)
    out = dict(kernel=kernel, threads=threads, bw=bw, groups=groups, nseg=nseg, cps=cps, segs=segs,
               last=ncells - (segs - 1) * cps, tail=K2 % bw, ncells=ncells, K2=K2)
    if kernel.startswith("k_sbw_mfma"):
        MT = -(-Zb // 16)
        mhalf = (MT + 1) // 2
        nmt = []
        for wv in range(threads // 64):
            if bw == 64:
                nmt.append(mhalf if wv < 4 else MT - mhalf)
            else:
                mt0 = wv >> 1
                mt1 = mt0 + threads // 128
                nmt.append(0 if mt0 >= MT else 2 if mt1 < MT else 1)
        out.update(MT=MT, mhalf=mhalf, nmt=tuple(nmt))
    return out


def zinv_launch_geometry(case, env=None, storage="f64"):
    """What launch_zinv (sx_kernels.hip) launches for the vertical inverse into Az, from the library's own plan:
    k_colmat_mfma<MT = zDim / 16, OT, CT> at zDim 32 / 64 / 128 (CT from SX_ZINV_CT: 1, 2 or 4 at 128 levels, default 2; 2 at 64
    levels on request, else 1), k_colmat otherwise; grid.x = ceil(K2 / (64 CT)) and the tail K2 % (64 CT) of the last workgroup.
    None where no k_zinv runs (R / RL grids, fused RZ)."""
    g, K2, _ = _handle_dims(case)
    kernel, (ct, grid_x, *_) = launch_plan(PLAN_ZINV, GEOM[g.geometry], g.zDim if g.has_z else 1, K2, storage == "f32x", env=env)
    if not kernel:
        return None
    mfma = kernel != "k_colmat"
    return dict(kernel=kernel, MT=g.zDim // 16 if mfma else None, CT=ct, OT="float" if storage == "f32x" else "double",
                grid_x=grid_x, tail=K2 % (64 * ct), K2=K2)


PLAN_RZ_INVERSE, PLAN_RZ_FORWARD, PLAN_SEMI = 5, 6, 7


def _ceil(a, b):
    return -(-a // b)


def rz_inverse_launch_geometry(case, env=None, storage="f64", tile=None):
    """What launch_rz_inverse (scythe.jl_amd/csrc/sx_rz.hip) launches for tileTransform! on a fused RZ grid, from the library's
    own plan: kernel text, form ("nodes": 13 cells per workgroup, chunks of 32 coefficient rows; "rings": 16 rings, chunks of
    64), grid (x, y, z), LDS bytes, K chunks, attr (the over-64 KB dynamic-LDS attribute is set first); and what follows from
    those inside the kernels: last_x = cells (nodes form) or rings (ring-tile form) of the last workgroup along x, last_waves =
    waves of the last z-group that own a tile of 16 levels, tail_z = zDim % 16 and tail_k = b_zDim - (chunks - 1) rows of the
    last K chunk."""
    g, _, ncells = _handle_dims(case, tile)
    kernel, (gx, gy, gz, lds, chunks, attr) = launch_plan(PLAN_RZ_INVERSE, g.zDim, g.b_zDim, ncells, g.V, int(storage == "f32"), env=env)
    nodes = kernel.startswith("k_rz_inverse_nodes")
    per, rows, n = (13, 32, ncells) if nodes else (16, 64, 3 * ncells)
    return dict(kernel=kernel, form="nodes" if nodes else "rings", grid=(gx, gy, gz), lds=lds, chunks=chunks, attr=bool(attr),
                last_x=n - (gx - 1) * per, last_waves=_ceil(g.zDim, 16) - (gz - 1) * 4, tail_z=g.zDim % 16,
                tail_k=g.b_zDim - (chunks - 1) * rows, ncells=ncells, zDim=g.zDim, b_zDim=g.b_zDim)


def rz_forward_launch_geometry(case, tile=None, v_cnt=None):
    """What launch_rz_forward launches for spectralTransform! on a fused RZ grid, from the library's plan: grid (x: tiles of 16
    nodes, y: variables, z: groups of mt_per_wg tiles of 16 modes), mt_per_wg, K chunks of 64 levels, LDS bytes; last_x = nodes of
    the last node tile, tail_z = zDim - 64 (chunks - 1) levels of the last chunk, tail_m = b_zDim % 16."""
    g, _, ncells = _handle_dims(case, tile)
    kernel, (gx, gy, gz, mt, chunks, lds) = launch_plan(PLAN_RZ_FORWARD, g.zDim, g.b_zDim, ncells, g.V if v_cnt is None else v_cnt)
    return dict(kernel=kernel, grid=(gx, gy, gz), mt_per_wg=mt, chunks=chunks, lds=lds, last_x=ncells + 3 - (gx - 1) * 16,
                tail_z=g.zDim - 64 * (chunks - 1), tail_m=g.b_zDim % 16, ncells=ncells, zDim=g.zDim, b_zDim=g.b_zDim)


def semi_launch_geometry(case, env=None):
    """What the semi-implicit adjustment launches over the case's columns (one tile), from the library's plan: kernel
    (k_semi_mfma, or k_semiimplicit with SX_SEMI_MFMA=0), workgroups, threads, tiles = level tiles per wave trip, trips =
    ceil(ceil(zDim / 16) / tiles), K chunks of 64 levels, LDS bytes, attr; last = columns of the last workgroup."""
    g, _, ncells = _handle_dims(case)
    ncol = g.tile_npoints(0, ncells) // g.zDim
    kernel, (wgs, threads, tiles, chunks, lds, attr) = launch_plan(PLAN_SEMI, g.zDim, ncol, env=env)
    per = 16 if kernel == "k_semi_mfma" else max(1, 256 // g.zDim)
    return dict(kernel=kernel, wgs=wgs, threads=threads, tiles=tiles, trips=_ceil(_ceil(g.zDim, 16), tiles) if tiles else 0,
                chunks=chunks, lds=lds, attr=bool(attr), columns=ncol, last=ncol - (wgs - 1) * per, zDim=g.zDim)


def inverse_bound_ratio(phys, ref, scale, C, f32=False):
    """|phys - ref| / (C 2^-53 scale [+ 2^-24 |ref| on the derivative slots of fp32-stored planes]) per entry, [points, V, D] in
    Float64 (entries of zero bound: 0 where phys equals ref, else inf), and the index of the worst one."""
    err = np.abs(np.asarray(phys, dtype=O.XP) - ref)
    bound = O.XP(C) * O.XP(2.0 ** -53) * scale
    if f32:
        bound = bound.copy()
        bound[:, :, 1:] += O.XP(2.0 ** -24) * np.abs(ref[:, :, 1:])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    q = np.asarray(q, dtype=np.float64)
    return q, np.unravel_index(int(np.argmax(q)), q.shape)


def inverse_reference(case, A, tile=None, exact_offsets=True):
    """(ref, scale), each [tile points, V, D] longdouble: oracle_np.inverse_xp with its per-entry scale over every ring of the
    tile (RZ grids: a ring is one column), the basis weights at the exact Gauss offsets (what the library tabulates) unless
    exact_offsets = False (at the Float64 gridpoints, what the oracles evaluate)."""
    g, _, ncells = _handle_dims(case, tile)
    c0 = 0 if tile is None else tile[0]
    rings = list(g.tile_rings(c0, ncells))
    ref, sc = O.inverse_xp(g, A, rings, with_scale=True, exact_offsets=exact_offsets)
    return np.concatenate([ref[r] for r in rings], axis=0), np.concatenate([sc[r] for r in rings], axis=0)


def inverse_f64_tables(case, A, tile=None):
    """The fused RZ inverse as a plain Float64 evaluation from tables formed once in Float64, the way the library forms its own
    (basis weights bspline(3/2 + Gauss offset - j) / DX^d per ring of a cell, the oracle's once-rounded vertical operators):
    [tile points, V, D].  The stand-in for a kernel in the CPU check of the per-entry bound."""
    g, _, ncells = _handle_dims(case, tile)
    c0 = 0 if tile is None else tile[0]
    goff = np.array([-np.sqrt(3.0 / 5.0) / 2, 0.0, np.sqrt(3.0 / 5.0) / 2])
    phi = [np.stack([O.bspline((1.5 + goff[mu] - np.arange(4.0))[None, :], d)[0] * (1.0 / g.DX ** d) for mu in range(3)]) for d in range(3)]
    sl = {s: i for i, s in enumerate(g.slots)}
    out = np.zeros((3 * ncells * g.zDim, g.V, g.D))
    for vi, v in enumerate(g.names):
        M = g.cheb(v).M
        Av = A[:, vi].reshape(g.b_zDim, g.b_rDim)
        for i in range(3 * ncells):
            c = c0 + i // 3
            f = [Av[:, c:c + 4] @ phi[d][i % 3] for d in range(3)]
            pts = slice(i * g.zDim, (i + 1) * g.zDim)
            for name, val in (("u", M[0] @ f[0]), ("r", M[0] @ f[1]), ("rr", M[0] @ f[2]), ("z", M[1] @ f[0]), ("zz", M[2] @ f[0])):
                out[pts, vi, sl[name]] = val
    return out


def where_rz(g, idx, cell0=0):
    """(ring, level, variable, slot) text of an index into an RZ tile's [points, V, D] array"""
    return "ring %d level %d variable %d slot %s" % (3 * cell0 + idx[0] // g.zDim, idx[0] % g.zDim, idx[1], g.slots[idx[2]])


# every instantiation the two launchers can pick
SB_KERNELS = {"k_sb", "k_sbz", "k_rz_forward", "k_sbw<32, false>", "k_sbw<32, true>", "k_sbw<64, false>", "k_sbw<64, true>",
              "k_sbw<128, false>", "k_sbw_mfma<32>", "k_sbw_mfma<64>", "k_sbw_mfma<64, 32, 256>", "k_sbw_mfma<128, 32>",
              "k_sbw_mfma<32, 64, 512, float>", "k_sbw_mfma<64, 64, 512, float>", "k_sbw_mfma<64, 32, 256, float>",
              "k_sbw_mfma<128, 32, 512, float>"}
ZINV_KERNELS = {"k_colmat"} | {"k_colmat_mfma<%d, %s, %d>" % (mt, ot, ct) for ot in ("double", "float")
                               for mt, ct in ((2, 1), (4, 1), (4, 2), (8, 1), (8, 2), (8, 4))}
