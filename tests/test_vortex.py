"""sx_vortex_check (pure host helper) and the twin of tests/vortex.py where there is no GPU: the symbols, the circle rule, every
refusal that needs no device, the Float64 twin within the bound of the longdouble twin, and the three closed forms the GPU tests rest
on - checked on the twin here, so their inputs are known to satisfy them before a GPU sees them."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import cases
from tests import parcels as P
from tests import vortex as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"RL": lambda: cases.rl_advection(num_cells=6), "RLZ": lambda: cases.rlz_advection(num_cells=5, zDim=8),
         "HRBL": lambda: cases.rlz_hrbl(num_cells=6, zDim=10, ring_L=16)}
FIELDS = {"RL": ["h", ("wind", "u", "v")], "RLZ": ["h", ("wind", "u", "v")], "HRBL": ["h", ("wind", "ub", "wb"), ("wind", "u", "v")]}


def heights_of(g):
    return [g.zmin, g.zmin + 0.37 * (g.zmax - g.zmin), g.zmax] if g.has_z else None


def centre_of(g):
    return (0.21 * g.xmax, -0.13 * g.xmax)


def test_symbols_exported_and_declared():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    header = open(os.path.join(ROOT, "include", "scythe_hip.h")).read()
    for name in ("sx_vortex_harmonics", "sx_vortex_check"):
        assert hasattr(lib, name) and name in L.SYMBOLS
        assert "int %s(" % name in header
    assert "enum { SX_VORTEX_SCALAR = 0, SX_VORTEX_WIND = 1 };" in header
    assert "#define SX_ABI_VERSION 2" in header and lib.sx_abi_version() == 2
    assert S.default_vortex_n_az(7, 2) == 12 and S.default_vortex_n_az(8, 4) == 16 and S.default_vortex_n_az(3, 0) == 4


@pytest.mark.parametrize("centre", [(0.0, 0.0), (2.1, -1.3), (0.0, 4.0)])
def test_circle_rule(centre):
    """inside, tangent (rho formed as xmax - d and its two neighbours), outside; centre on and off the origin"""
    import scythe_jl_amd as S
    case = CASES["RL"]()
    g = cases.oracle_grid(case)
    gp, _ = cases.hip_params(case)
    d = float(np.hypot(*centre))
    t = g.xmax - d
    radii = np.array([0.0, d, 0.5 * t, t, np.nextafter(t, 0.0), np.nextafter(t, np.inf), t * (1 + 1e-12) + 1e-12, t + 0.1, 3 * g.xmax])
    n_out, status = S.vortex_check(gp, centre, radii, ["h", ("wind", "u", "v")], 16, 2)
    assert n_out == 3
    assert status.tolist() == V.circle_status(g, centre, radii).tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1]
    # a centre outside the tile: every circle leaves it
    assert S.vortex_check(gp, (g.xmax + 1.0, 0.0), [0.0, 0.5], ["h"], 16, 2)[1].tolist() == [1, 1]


def _raw_check(gp, centre, radii, n_az, kmax, fields, n_fields=None, null=()):
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    from scythe_jl_amd.model import grid_desc
    lib = S.load()
    d, keep = grid_desc(gp, 0, None)
    c0 = np.ascontiguousarray(centre, dtype=np.float64)
    r = np.ascontiguousarray(radii, dtype=np.float64)
    f = np.ascontiguousarray(fields, dtype=np.int32).reshape(-1, 3)
    st, n_out = np.full(max(len(r), 1), -9, dtype=np.int32), C.c_int32(-9)
    rc = lib.sx_vortex_check(C.byref(d), None if "centre" in null else c0.ctypes.data_as(L.P_D), None if "radii" in null else r.ctypes.data_as(L.P_D),
                             len(r), n_az, kmax, len(f) if n_fields is None else n_fields, None if "fields" in null else f.ctypes.data_as(L.P_I32),
                             C.byref(n_out), None if "status" in null else st.ctypes.data_as(L.P_I32))
    assert (st == -9).all() or rc == 0                      # a refusal writes nothing
    assert n_out.value == -9 or rc == 0
    return rc, lib.sx_last_error().decode()


def test_refusals():
    """everything sx_vortex_harmonics refuses of a call that needs no device, each with its message, and the twin's statement of it"""
    case = CASES["RLZ"]()
    g = cases.oracle_grid(case)
    gp, _ = cases.hip_params(case)
    ok = dict(centre=(1.0, 2.0), radii=[0.0, 1.0], n_az=16, kmax=2, fields=[[0, 1, 0], [1, 2, 3]])

    def refused(phrase, **kw):
        a = dict(ok, **{k: v for k, v in kw.items() if k in ok})
        rc, msg = _raw_check(gp, a["centre"], a["radii"], a["n_az"], a["kmax"], a["fields"], kw.get("n_fields"), kw.get("null", ()))
        assert rc != 0 and phrase in msg and msg.startswith("sx_vortex_check: "), (kw, msg)
        if "null" not in kw and "n_fields" not in kw:
            assert V.refusal(g, a["centre"], a["radii"], a["n_az"], a["kmax"], a["fields"]) in msg, (kw, msg)

    assert _raw_check(gp, **ok)[0] == 0 and V.refusal(g, **ok) is None
    refused("the centre is NaN or Inf", centre=(np.nan, 0.0))
    refused("the centre is NaN or Inf", centre=(0.0, np.inf))
    refused("radius 1 is NaN or Inf", radii=[0.0, np.nan])
    refused("radius 1 is negative", radii=[0.0, -1e-300])
    for n_az in (0, 3, 18, 4100):
        refused("n_az must be a multiple of 4 in 4 .. 4096", n_az=n_az)
    refused("kmax must be 0 .. 32 with 2 kmax < n_az", kmax=-1)
    refused("kmax must be 0 .. 32 with 2 kmax < n_az", kmax=8)
    refused("kmax must be 0 .. 32 with 2 kmax < n_az", kmax=33, n_az=128)
    refused("n_fields must be 1 .. 8", n_fields=0)
    refused("n_fields must be 1 .. 8", fields=[[0, 1, 0]] * 9)
    refused("field 1: kind must be SX_VORTEX_SCALAR or SX_VORTEX_WIND", fields=[[0, 1, 0], [2, 1, 1]])
    refused("field 0: var_a = 0 is 1-based and at most nvars", fields=[[0, 0, 0]])
    refused("field 0: var_a = 4 is 1-based and at most nvars", fields=[[1, 4, 1]])
    refused("field 0: var_b = 4 is 1-based and at most nvars", fields=[[1, 1, 4]])
    assert _raw_check(gp, **dict(ok, fields=[[0, 1, 99]]))[0] == 0           # a scalar field's var_b is ignored
    for null in ("centre", "radii", "status", "fields"):
        refused("null", null=(null,))
    assert _raw_check(gp, (0.0, 0.0), [], 16, 2, [[0, 1, 0]], null=("radii", "status"))[0] == 0      # n_rho == 0 needs neither
    # geometry, tiles
    for maker in (lambda: cases.rz_advection(num_cells=6, zDim=8), lambda: cases.r_bcs("R0", "R0", num_cells=8)):
        gq, _ = cases.hip_params(maker())
        rc, msg = _raw_check(gq, **dict(ok, fields=[[0, 1, 0]]))
        assert rc != 0 and "RL and RLZ grids only" in msg
    import scythe_jl_amd as S
    with pytest.raises(S.ScytheHipError, match="one-tile patches only"):
        S.vortex_check(gp, (0.0, 0.0), [1.0], ["h"], 16, 2, tile_cell0=0, tile_num_cells=3)
    # the LDS: 8 wind fields x kmax 32 x b_zDim
    big = [[1, 2, 3]] * 8
    rc, msg = _raw_check(gp, (0.0, 0.0), [1.0], 128, 32, big)
    need = 2 * (g.kDim + 1) + 2 * 32 * 33 * g.b_zDim + 2 * g.b_zDim
    assert rc != 0 and "do not fit the LDS" in msg and str(need) in msg and "b_zDim %d" % g.b_zDim in msg and "n_acc 32" in msg, msg
    assert V.refusal(g, (0.0, 0.0), [1.0], 128, 32, big) == "do not fit the LDS"
    with pytest.raises(ValueError, match="unknown variable"):
        S.vortex_check(gp, (0.0, 0.0), [1.0], ["nope"])
    with pytest.raises(ValueError, match="neither a variable nor"):
        S.vortex_check(gp, (0.0, 0.0), [1.0], [("wind", "u")])


@pytest.mark.parametrize("name", list(CASES))
def test_float64_twin_within_the_bound(name):
    g = cases.oracle_grid(CASES[name]())
    A = P.smooth_state(g, seed=3)
    cen = centre_of(g)
    radii = V.sample_radii(g, cen)
    for n_az, kmax in ((16, 2), (64, 0)):
        hi, S_abs, bound, status = V.harmonics(g, A, cen, radii, heights_of(g), FIELDS[name], n_az, kmax, motion=(0.3, -0.2), xp=True)
        lo, _, _, st2 = V.harmonics(g, A, cen, radii, heights_of(g), FIELDS[name], n_az, kmax, motion=(0.3, -0.2), xp=False)
        assert status.tolist() == st2.tolist() == [0, 0, 0, 0, 0, 0, 1]
        assert np.isnan(hi[:, 6]).all() and np.isnan(lo[:, 6]).all() and np.isnan(bound[:, 6]).all()
        live = status == 0
        ratio = np.abs(lo[:, live].astype(np.clongdouble) - hi[:, live]) / bound[:, live][..., None]
        print(name, n_az, kmax, "Float64 twin - longdouble twin over the bound: max %.4f" % float(ratio.max()))
        assert np.isfinite(np.asarray(hi[:, live], dtype=np.complex128)).all() and float(np.abs(hi[:, live]).max()) > 0
        assert (bound[:, live] > 0).all() and (bound[:, live] < 1e-9 * np.maximum(S_abs[:, live], 1e-300)).all()
        assert (ratio <= 1.0).all(), float(ratio.max())
        assert np.array_equal(hi[:, 2], hi[:, 5]) and lo[:, 2].tobytes() == lo[:, 5].tobytes()      # the duplicate radius


@pytest.mark.parametrize("name", ["RL", "RLZ"])
def test_sample_bound_is_the_parcels_bound(name):
    """At given Float64 (r, lambda, z) the per-sample sums of the twin are those of P.velocity(..., with_bound=True): S the same, and
    the bound's parts equal once P's vertical part d_w is replaced by u S (the rows are rounded once here) - so P's bound is the larger"""
    g = cases.oracle_grid(CASES[name]())
    A = P.smooth_state(g, seed=5)
    pts = P.interior_points(g, 6, seed=2)
    var = P.velocity_vars(g)
    vel, S_abs, bound = P.velocity(g, A, pts, var, xp=True, with_bound=True)
    d_phi = V.EPS * (2.0 * max(abs(g.xmin), abs(g.xmax)) / g.DX + 14.0)
    for i, p in enumerate(pts):
        Av = {v - 1: A[:, v - 1].reshape(g.b_zDim, g.K2, g.b_rDim).astype(V.XP) for v in var}
        sums = V._sample_sums(g, Av, V.XP(p[0]), V.XP(p[1]), True)
        for c, v in enumerate(var):
            W = V.E.vertical_weights(g, g.names[v - 1], p[-1], True)[0] if g.has_z else np.ones(1, dtype=V.XP)
            aW, q = np.abs(W).astype(np.float64), sums[v - 1]
            val, S1 = W @ q["G"], aW @ q["S"]
            mine = V.EPS * (g.b_zDim * g.K2 + 6.0 + 1.0) * S1 + d_phi * (aW @ q["phi"]) + aW @ q["F"]
            assert abs(float(val - vel[i, c])) <= 1e-17 * S1 and abs(S1 - S_abs[i, c]) <= 1e-12 * S1
            assert mine <= bound[i, c] * (1 + 1e-12) + V.EPS * S1                 # d_w >= u |w| whenever the grid has a vertical
            if not g.has_z:
                assert abs(mine - V.EPS * S1 - bound[i, c]) <= 1e-12 * bound[i, c]


# ----------------------------------------------------------------------------- the closed forms, on the twin alone
U0, V0, OMEGA, SIGMA = 0.7, -0.4, 0.25, 1.4
CENTRE = (1.3, -0.9)
RADII = np.array([0.0, 0.5, 1.5, 3.0, 4.5])


def uniform_flow_state():
    case = CASES["RL"]()
    return case, V.state_from_values(case, lambda p: np.stack([0.0 * p[:, 0], *V.cartesian_wind(p, U0, V0)], axis=1))


def solid_body_state():
    case = CASES["RL"]()
    return case, V.state_from_values(case, lambda p: np.stack([0.0 * p[:, 0], 0.0 * p[:, 0], OMEGA * p[:, 0]], axis=1))


def gaussian_state(num_cells=12):
    case = cases.rl_advection(num_cells=num_cells)

    def ic(p):
        x, y = p[:, 0] * np.cos(p[:, 1]), p[:, 0] * np.sin(p[:, 1])
        return np.stack([np.exp(-((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2) / (2 * SIGMA ** 2)), 0.0 * x, 0.0 * x], axis=1)
    return case, V.state_from_values(case, ic)


def uniform_flow_truth(kmax, n_rho, moved):
    """[2, n_rho, 1, kmax + 1]: radial eps_1 c_1 = U0 - i V0, tangential eps_1 c_1 = V0 + i U0, nothing else; all zero once the motion is out"""
    t = np.zeros((2, n_rho, 1, kmax + 1), dtype=np.complex128)
    if not moved:
        t[0, :, :, 1], t[1, :, :, 1] = (U0 - 1j * V0) / 2, (V0 + 1j * U0) / 2
    return t


def solid_body_truth(kmax, radii):
    """v = Omega r about the grid's centre seen from CENTRE: tangential c_0 = Omega rho, wave 1 the uniform flow Omega (-y0, x0)"""
    t = np.zeros((2, len(radii), 1, kmax + 1), dtype=np.complex128)
    Ux, Vy = -OMEGA * CENTRE[1], OMEGA * CENTRE[0]
    t[1, :, 0, 0] = OMEGA * radii
    t[0, :, :, 1], t[1, :, :, 1] = (Ux - 1j * Vy) / 2, (Vy + 1j * Ux) / 2
    return t


def test_uniform_flow_on_the_twin():
    case, A = uniform_flow_state()
    g = cases.oracle_grid(case)
    for motion in (None, (U0, V0)):
        c, _, bound, status = V.harmonics(g, A, CENTRE, RADII, None, [("wind", "u", "v")], 16, 3, motion=motion)
        err = np.abs(np.asarray(c, dtype=np.complex128) - uniform_flow_truth(3, len(RADII), motion is not None))
        print("uniform flow, motion", motion, ": twin - closed form max %.3e" % err.max())
        assert (status == 0).all() and err.max() <= 1e-12


def test_solid_body_on_the_twin():
    case, A = solid_body_state()
    g = cases.oracle_grid(case)
    c, _, bound, status = V.harmonics(g, A, CENTRE, RADII, None, [("wind", "u", "v")], 16, 3)
    err = np.abs(np.asarray(c, dtype=np.complex128) - solid_body_truth(3, RADII))
    print("solid body: twin - closed form max %.3e" % err.max())
    assert (status == 0).all() and err.max() <= 1e-12


def test_displaced_gaussian_on_the_twin():
    """about its own centre the Gaussian is wave 0 alone (to the truncation error of the grid); about the grid's it has a wave 1"""
    from tests import harmonics as H
    case, A = gaussian_state()
    g = cases.oracle_grid(case)
    radii = np.array([0.0, 0.7, 1.4, 2.1, 2.8])
    c, _, bound, status = V.harmonics(g, A, CENTRE, radii, None, ["h"], 32, 2)
    c = np.asarray(c[0, :, 0], dtype=np.complex128)
    err0 = np.abs(c[:, 0] - np.exp(-radii ** 2 / (2 * SIGMA ** 2)))
    own = H.harmonics(g, A, radii, None, all_k=True, xp=True)[:, 0, :, 0, 0]
    w1_vortex, w1_grid = float(np.abs(c[:, 1]).max()), float(np.abs(own[:, 1]).max())
    print("gaussian: c_0 - closed form max %.3e; wave 1 about the vortex %.3e, about the grid's centre %.3e" % (err0.max(), w1_vortex, w1_grid))
    assert err0.max() <= 2e-3 and np.abs(c[:, 1:]).max() <= 2e-3
    assert w1_grid >= 10 * w1_vortex
