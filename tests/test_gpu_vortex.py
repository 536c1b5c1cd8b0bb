"""sx_vortex_harmonics on the GPU against the twin of tests/vortex.py: the longdouble twin is the arbiter and the rounding bound is the
one derived there; the closed forms and their inputs are those tests/test_vortex.py has checked on the twin alone."""
import numpy as np
import pytest

from tests import cases
from tests import linear_sw as LS
from tests import parcels as P
from tests import vortex as V
from tests.test_vortex import (CASES, FIELDS, CENTRE, RADII, SIGMA, U0, V0, centre_of, heights_of, uniform_flow_state, solid_body_state,
                               gaussian_state, uniform_flow_truth, solid_body_truth)

pytestmark = pytest.mark.gpu


def _tile(case, A):
    import scythe_jl_amd as S
    gp, mp = cases.hip_params(case)
    tile = S.Grid(gp, mp)
    tile.set_patch_spectral_a(A)
    return tile


def _ratio(dev, truth, bound):
    return np.abs(dev.astype(np.clongdouble) - truth) / bound[..., None]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("n_az,kmax", [(16, 0), (16, 2), (16, 7), (64, 2)])
def test_twin(name, n_az, kmax):
    """seeded smooth state, scalar and wind fields together (on the HRBL case a wind pair that crosses vertical classes), radii with
    rho = 0, a circle through r = 0, one tangent to the outer edge, a duplicate and one outside; heights zmin, interior, zmax"""
    case = CASES[name]()
    g = cases.oracle_grid(case)
    A = P.smooth_state(g, seed=3)
    cen, hs = centre_of(g), heights_of(g)
    radii = V.sample_radii(g, cen)
    tile = _tile(case, A)
    tile.enable_timers(True)
    c, status = tile.vortex_harmonics(cen, radii, hs, FIELDS[name], n_az, kmax, motion=(0.3, -0.2))
    tm = tile.timers()
    assert tm["k_vortex_rings"][1] == 1 and tm["k_vortex_finish"][1] == 1
    truth, S_abs, bound, st = V.harmonics(g, A, cen, radii, hs, FIELDS[name], n_az, kmax, motion=(0.3, -0.2), xp=True)
    assert status.tolist() == st.tolist() == [0, 0, 0, 0, 0, 0, 1]
    live = status == 0
    assert np.isnan(c[:, ~live]).all()
    assert np.isfinite(c[:, live]).all() and (np.abs(c[:, live]).max(axis=(1, 2, 3)) > 0).all()
    ratio = _ratio(c[:, live], truth[:, live], bound[:, live])
    print("%s n_az %d kmax %d: |device - longdouble twin| / bound max %.4f" % (name, n_az, kmax, float(ratio.max())))
    assert (ratio <= 1.0).all(), float(ratio.max())
    assert c[:, 2].tobytes() == c[:, 5].tobytes()                                 # the duplicate radius
    n_src = len({v for f in FIELDS[name] for v in (f[1:] if isinstance(f, tuple) else (f,))})
    assert tile.kernel_bytes("k_vortex_rings") == 8.0 * 4 * g.b_zDim * g.K2 * n_src * n_az * int(live.sum())
    tile.close()


def _harmonics_abs(g, A, radii, hs, vi, kmax):
    """[n_r, n_z, kmax + 1]: the sum of absolute terms sum_zm |Wz| sum_node |phi| (|A_re| + |A_im|) of sx_harmonics' entry c_k"""
    a = np.abs(A[:, vi].reshape(g.b_zDim, g.K2, g.b_rDim))
    ak = np.concatenate([a[:, :1], a[:, 1::2] + a[:, 2::2]], axis=1)[:, :kmax + 1]                # [zm, k, node]
    W = (np.abs(np.stack([V.E.vertical_weights(g, g.names[vi], z, False)[0] for z in hs])) if g.has_z else np.ones((1, 1)))
    out = np.zeros((len(radii), W.shape[0], kmax + 1))
    for i, r in enumerate(radii):
        n0 = V.E.node0_of(g, r)
        out[i] = np.einsum("lz,zkn,n->lk", W, ak[:, :, n0:n0 + 4], np.abs(V.E.radial_weights(g, r, n0, False)[0]))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_centre_on_the_origin(name):
    """about the grid's own centre with the default n_az: a scalar's c_k are Grid.harmonics(all_k=True)'s, a wind field returns u's and
    v's harmonics unrotated; both within the sum of the two bounds.  That of an entry of sx_harmonics: weights rounded once (2 u), a
    4-node fma chain (4 u) and a sum b_zDim deep: u (b_zDim + 8) times the entry's sum of absolute terms."""
    case = CASES[name]()
    g = cases.oracle_grid(case)
    A = P.smooth_state(g, seed=7)
    hs, kmax = heights_of(g), 2
    radii = np.array([1e-3 * g.DX, 0.3 * g.xmax, g.DX, 0.77 * g.xmax, g.xmax])     # not rho = 0: there every sample is the pole at lambda = 0
    names = FIELDS[name][-1][1:]
    tile = _tile(case, A)
    c, status = tile.vortex_harmonics((0.0, 0.0), radii, hs, ["h", ("wind",) + names], kmax=kmax)
    assert (status == 0).all()
    ref = tile.harmonics(radii, hs, all_k=True)                                   # [ir, iz, k, v, s]
    _, S_abs, bound, _ = V.harmonics(g, A, (0.0, 0.0), radii, hs, ["h", ("wind",) + names], 4 * ((g.kDim + kmax) // 4 + 1), kmax, xp=True)
    for o, v in enumerate(("h",) + names):
        vi = g.names.index(v)
        tol = bound[o][..., None] + (g.b_zDim + 8) * V.EPS * _harmonics_abs(g, A, radii, hs, vi, kmax)
        err = np.abs(c[o] - ref[:, :, :kmax + 1, vi, 0])
        print("%s %s: |vortex - harmonics| / (sum of the bounds) max %.4f" % (name, v, float((err / tol).max())))
        assert (err <= tol).all()
    tile.close()


def test_uniform_flow():
    case, A = uniform_flow_state()
    g = cases.oracle_grid(case)
    tile = _tile(case, A)
    for motion in (None, (U0, V0)):
        c, status = tile.vortex_harmonics(CENTRE, RADII, None, [("wind", "u", "v")], 16, 3, motion=motion)
        twin, _, bound, _ = V.harmonics(g, A, CENTRE, RADII, None, [("wind", "u", "v")], 16, 3, motion=motion)
        truth = uniform_flow_truth(3, len(RADII), motion is not None)
        tol = bound[..., None] + np.abs(np.asarray(twin, dtype=np.complex128) - truth)
        err = np.abs(c - truth)
        print("uniform flow, motion %s: device - closed form max %.3e (allowed %.3e)" % (motion, err.max(), tol.max()))
        assert (status == 0).all() and (err <= tol).all()
    tile.close()


def test_solid_body_rotation():
    case, A = solid_body_state()
    g = cases.oracle_grid(case)
    tile = _tile(case, A)
    c, status = tile.vortex_harmonics(CENTRE, RADII, None, [("wind", "u", "v")], 16, 3)
    twin, _, bound, _ = V.harmonics(g, A, CENTRE, RADII, None, [("wind", "u", "v")], 16, 3)
    truth = solid_body_truth(3, RADII)
    tol = bound[..., None] + np.abs(np.asarray(twin, dtype=np.complex128) - truth)
    err = np.abs(c - truth)
    print("solid body: device - closed form max %.3e (allowed %.3e)" % (err.max(), tol.max()))
    assert (status == 0).all() and (err <= tol).all()
    tile.close()


def test_displaced_gaussian():
    case, A = gaussian_state()
    g = cases.oracle_grid(case)
    radii = np.array([0.0, 0.7, 1.4, 2.1, 2.8])
    tile = _tile(case, A)
    c, status = tile.vortex_harmonics(CENTRE, radii, None, ["h"], 32, 2)
    twin, _, bound, _ = V.harmonics(g, A, CENTRE, radii, None, ["h"], 32, 2)
    truth = np.zeros((1, len(radii), 1, 3), dtype=np.complex128)
    truth[0, :, 0, 0] = np.exp(-radii ** 2 / (2 * SIGMA ** 2))
    tol = bound[..., None] + np.abs(np.asarray(twin, dtype=np.complex128) - truth)
    assert (status == 0).all() and (np.abs(c - truth) <= tol).all()
    own = tile.harmonics(radii, None, all_k=True)[:, 0, :, 0, 0]
    w1_vortex, w1_grid = float(np.abs(c[0, :, 0, 1]).max()), float(np.abs(own[:, 1]).max())
    print("gaussian: wave 1 about the vortex %.3e, about the grid's centre %.3e; c_0 - closed form max %.3e"
          % (w1_vortex, w1_grid, float(np.abs(c - truth)[..., 0].max())))
    assert w1_grid >= 10 * w1_vortex
    tile.close()


def test_bitwise():
    """a circle's bytes alone, among others, duplicated and in a second call; an output's bytes whatever the other fields and their
    order; status and the NaN fill as vortex_check gives them; kernel_bytes; both timers count one call each"""
    import scythe_jl_amd as S
    case = CASES["HRBL"]()
    g = cases.oracle_grid(case)
    gp, _ = cases.hip_params(case)
    A = P.smooth_state(g, seed=9)
    cen, hs = centre_of(g), heights_of(g)
    radii = V.sample_radii(g, cen)
    tile = _tile(case, A)
    for n_az, kmax in ((16, 2), (64, 2)):
        full, status = tile.vortex_harmonics(cen, radii, hs, ["h", ("wind", "ub", "wb"), ("wind", "u", "v")], n_az, kmax)
        n_out, st = S.vortex_check(gp, cen, radii, ["h", ("wind", "ub", "wb"), ("wind", "u", "v")], n_az, kmax)
        assert n_out == 5 and status.tolist() == st.tolist() and np.isnan(full[:, st == 1]).all() and np.isfinite(full[:, st == 0]).all()
        again, _ = tile.vortex_harmonics(cen, radii, hs, ["h", ("wind", "ub", "wb"), ("wind", "u", "v")], n_az, kmax)
        assert again.tobytes() == full.tobytes()
        for i in (0, 1, 3):
            alone, s1 = tile.vortex_harmonics(cen, radii[i:i + 1], hs, ["h", ("wind", "ub", "wb"), ("wind", "u", "v")], n_az, kmax)
            assert s1.tolist() == [0] and alone[:, 0].tobytes() == full[:, i].tobytes()
        assert full[:, 2].tobytes() == full[:, 5].tobytes()
        rev, _ = tile.vortex_harmonics(cen, radii[::-1].copy(), hs, ["h", ("wind", "ub", "wb"), ("wind", "u", "v")], n_az, kmax)
        assert np.ascontiguousarray(rev[:, ::-1]).tobytes() == full.tobytes()
        # the fields: alone, reordered, with a source shared or not
        h_only, _ = tile.vortex_harmonics(cen, radii, hs, ["h"], n_az, kmax)
        assert h_only[0].tobytes() == full[0].tobytes()
        swapped, _ = tile.vortex_harmonics(cen, radii, hs, [("wind", "u", "v"), "wb", ("wind", "ub", "wb"), "h"], n_az, kmax)
        assert swapped[5].tobytes() == full[0].tobytes() and swapped[0:2].tobytes() == full[3:5].tobytes() and swapped[3:5].tobytes() == full[1:3].tobytes()
        live = int((st == 0).sum())
        assert tile.kernel_bytes("k_vortex_rings") == 8.0 * 4 * g.b_zDim * g.K2 * 5 * n_az * live
    tile.enable_timers(True)
    tile.vortex_harmonics(cen, radii, hs, ["h"], 16, 0)
    tm = tile.timers()
    assert tm["k_vortex_rings"][1] == 1 and tm["k_vortex_finish"][1] == 1 and tm["k_vortex_rings"][0] > 0
    assert tile.kernel_bytes("k_vortex_rings") == 8.0 * 4 * g.b_zDim * g.K2 * 1 * 16 * 6
    # every circle outside: no launch, NaN everywhere, zero bytes; no radii: nothing
    c, status = tile.vortex_harmonics((2 * g.xmax, 0.0), [0.0, 1.0], hs, ["h"], 16, 0)
    assert status.tolist() == [1, 1] and np.isnan(c).all() and tile.kernel_bytes("k_vortex_rings") == 0
    c, status = tile.vortex_harmonics(cen, [], hs, ["h"], 16, 0)
    assert c.shape == (1, 0, 3, 1) and status.shape == (0,)
    with pytest.raises(S.ScytheHipError, match="height 1: z = "):
        tile.vortex_harmonics(cen, radii, [0.0, g.zmax + 1.0], ["h"], 16, 0)
    with pytest.raises(S.ScytheHipError, match="the motion is NaN or Inf"):
        tile.vortex_harmonics(cen, radii, hs, [("wind", "u", "v")], 16, 1, motion=(np.nan, 0.0))
    tile.close()


@pytest.mark.parametrize("overrides", [{}, {"SX_DEFER_DIAG": 1}], ids=["default", "defer_diag"])
def test_reads_only(tmp_path, overrides):
    """a stepping HRBL model with vortex_profile called after every step is bitwise the model without the calls (fresh child process)"""
    out = V.read_only_in_child(tmp_path, "rlz_hrbl", dict(num_cells=6, zDim=10, ring_L=16), overrides)
    assert bool(out["same_state"]) and bool(out["same_np1"])
    assert out["state0"].tobytes() == out["state1"].tobytes() and out["np10"].tobytes() == out["np11"].tobytes()
    assert np.isfinite(out["tangential"]).all() and np.abs(out["tangential"]).max() > 0


def test_vortex_profile_end_to_end():
    """LinearShallowWaterRL, uniform 16-point rings, 12 cells: a vortex v = 2 v_m x / (1 + x^2), x = rho / r_m, about a displaced centre
    with a depression of h there.  The profile about locate's centre peaks at r_m to the spacing of the radii, and its wave 1 is
    below the one the grid-centred harmonics show."""
    vm, rm, cen = 1.5, 1.6, (0.9, -0.6)

    def ic(p):
        x, y = p[:, 0] * np.cos(p[:, 1]) - cen[0], p[:, 0] * np.sin(p[:, 1]) - cen[1]
        rho = np.hypot(x, y)
        s = 2.0 * vm / rm / (1.0 + (rho / rm) ** 2)                               # v_t / rho
        u, v = V.cartesian_wind(p, -s * y, s * x)
        return np.stack([-np.exp(-rho ** 2 / (2.0 * rm ** 2)), u, v], axis=1)
    hip = cases.HipModel(dict(LS.rl_case(num_cells=12, ring_L=16), ic=ic))
    run = hip.run
    radii = 0.2 * np.arange(1, 26)
    found = run.locate("h", "min")
    c0 = (found.pos[0] * np.cos(found.pos[1]), found.pos[0] * np.sin(found.pos[1]))
    assert found.status == 0 and np.hypot(c0[0] - cen[0], c0[1] - cen[1]) < 0.05
    prof = run.vortex_profile(radii=radii)
    assert (prof.status == 0).all() and np.allclose(prof.centre, c0)
    i = int(np.argmax(prof.tangential[:, 0]))
    rmw, vmax = run.radius_of_maximum_about(prof.centre, radii)
    print("radius of maximum wind about the centre: %.2f (set %.2f), v %.4f (set %.2f)" % (rmw, rm, vmax, vm))
    assert rmw == radii[i] and abs(rmw - rm) <= 0.2 and abs(vmax - vm) < 0.05 * vm
    own, _ = run.harmonics(radii, None, all_k=True)
    w1_grid = 2.0 * np.abs(own[:, 0, 1, 2, 0])                                    # the grid-centred wave 1 of v
    print("wave-1 amplitude of the tangential wind: about the vortex max %.3e, about the grid's centre max %.3e"
          % (prof.wave1[1].max(), w1_grid.max()))
    assert prof.wave1[1].max() < w1_grid.max() and prof.wave1.shape == (2, len(radii), 1)
    run.close()
