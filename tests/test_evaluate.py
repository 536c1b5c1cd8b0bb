"""sx_eval_basis and the host side of evaluation at arbitrary points, where there is no GPU: the twin (tests/evaluate.py) is pinned
to oracle_np.inverse_xp at the model's own gridpoints, and the library's weights are checked against the twin."""
import os

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import cases
from tests import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def _case(geom, ring_L=None):
    if geom == "R":
        return cases.r_bcs(num_cells=12)
    if geom == "RZ":
        return cases.rz_advection(num_cells=6, zDim=10)
    if geom == "RL":
        return cases.rl_slab(num_cells=6, ring_L=ring_L)
    return cases.rlz_advection(num_cells=4, zDim=9, ring_L=ring_L)


GEOMS = [("R", None), ("RZ", None), ("RL", None), ("RL", 16), ("RLZ", None), ("RLZ", 12)]


def test_symbols_exported_and_declared():
    import scythe_jl_amd as S
    lib = S.load()
    header = open(os.path.join(ROOT, "include", "scythe_hip.h")).read()
    for name in ("sx_evaluate", "sx_eval_basis"):
        assert hasattr(lib, name)
        assert "int %s(" % name in header
    assert "SX_EVAL_RING_K = 0, SX_EVAL_ALL_K = 1" in header
    assert "#define SX_ABI_VERSION 2" in header


@pytest.mark.parametrize("geom,ring_L", GEOMS)
def test_twin_matches_inverse_xp_at_own_gridpoints(geom, ring_L):
    """The longdouble twin at the Float64 gridpoints against inverse_xp, which takes the ring angles and the levels exactly: the two
    differ by the rounding of the coordinates alone, eps |coordinate| times the gain of one more derivative - at most kDim in
    lambda, and N^2 in z (Markov's inequality for a polynomial of degree N - 1)."""
    g = cases.oracle_grid(_case(geom, ring_L))
    A = np.random.default_rng(3).standard_normal((g.S_patch(), g.V))
    pts = g.gridpoints()
    pts = pts.reshape(len(pts), -1)
    rings = sorted({0, 1, g.rDim // 2, g.rDim - 1})
    truth = O.inverse_xp(g, A, rings)
    tol = 64 * EPS * (1 + g.kDim + g.zDim ** 2)
    for ring in rings:
        sel = np.arange(g.ringstart[ring] * g.zDim, (g.ringstart[ring] + g.L[ring]) * g.zDim)
        mine = E.evaluate(g, A, pts[sel], xp=True)
        e = E.slot_errors(mine, truth[ring])
        print(geom, ring_L, "ring", ring, "twin vs inverse_xp per slot", e, "tol", tol)
        assert (e <= tol).all(), (ring, e, tol)


def _special_points(g, cell0, ncells):
    lo, hi = E.tile_range(g, cell0, ncells)
    edges = g.xmin + np.arange(cell0 + 1, cell0 + ncells) * g.DX
    rings = O.mish_points(g.xmin, g.DX, cell0, ncells)
    rs = np.concatenate([[lo, hi], edges, rings, np.random.default_rng(1).uniform(lo, hi, 6)])
    zs = [0.0]
    if g.has_z:
        lev = g.cheb(g.names[0]).z
        zs = [g.zmin, g.zmax, lev[1], lev[len(lev) // 2], lev[-2], 0.37 * (g.zmax - g.zmin) + g.zmin]
    out = []
    for i, r in enumerate(rs):
        p = [r]
        if g.has_l:
            p.append([-1.3, 0.0, 2.0, 7.5][i % 4])
        if g.has_z:
            p.append(zs[i % len(zs)])
        out.append(p)
    return out


@pytest.mark.parametrize("geom,ring_L", GEOMS)
def test_eval_basis_matches_twin(geom, ring_L):
    import scythe_jl_amd as S
    case = _case(geom, ring_L)
    g = cases.oracle_grid(case)
    gp, _ = cases.hip_params(case)
    worst = 0.0
    for cell0, ncells in [(0, g.nc), (1, g.nc - 2)]:
        for p in _special_points(g, cell0, ncells):
            for v in g.names:
                for all_k in (False, True):
                    n0, wr, kc, wz = S.eval_basis(gp, v, p, all_k, cell0, ncells)
                    tn0, twr, tkc, twz = E.basis(g, v, p, all_k, cell0, ncells, xp=True)
                    _, fwr, _, fwz = E.basis(g, v, p, all_k, cell0, ncells, xp=False)
                    assert n0 == tn0 and kc == tkc, (p, n0, tn0, kc, tkc)
                    for w, t, f in ((wr, twr, fwr),) + (((wz, twz, fwz),) if wz is not None else ()):
                        for s in range(3):
                            mine = np.abs(w[s].astype(E.XP) - t[s]).max()
                            f64 = np.abs(f[s].astype(E.XP) - t[s]).max()
                            bound = max(10 * f64, 4 * EPS * np.abs(t[s]).max())
                            worst = max(worst, float(mine / max(bound, 1e-300)))
                            assert mine <= bound, (p, v, s, float(mine), float(f64))
    print(geom, ring_L, "worst |w - longdouble| / bound", worst)


@pytest.mark.parametrize("bcb,bct", [(b, t) for b in ("R0", "R1T0", "R1T1", "R1T2") for t in ("R0", "R1T0", "R1T1", "R1T2")])
def test_eval_basis_every_vertical_class(bcb, bct):
    """every (bcb, bct) class; at an exact level the weights are the rows of the collocation operators (d_Mz) to rounding"""
    import scythe_jl_amd as S
    case = cases.rz_advection(num_cells=4, zDim=12)
    case["grid"]["BCB"], case["grid"]["BCT"] = {"h": bcb}, {"h": bct}
    g = cases.oracle_grid(case)
    gp, _ = cases.hip_params(case)
    ch = g.cheb("h")
    for z in [g.zmin, g.zmax, ch.z[3], ch.z[7], 1234.5]:
        _, _, _, wz = S.eval_basis(gp, "h", [3.0e3, z])
        t = E.vertical_weights(g, "h", z, True)
        f = E.vertical_weights(g, "h", z, False)
        for s in range(3):
            bound = max(10 * np.abs(f[s].astype(E.XP) - t[s]).max(), 4 * EPS * np.abs(t[s]).max())
            assert np.abs(wz[s].astype(E.XP) - t[s]).max() <= bound, (z, s)
    for n in (0, 3, 7, g.zDim - 1):
        _, _, _, wz = S.eval_basis(gp, "h", [3.0e3, ch.z[n]])
        for s in range(3):
            # the level itself is rounded: eps |z| moves row s by at most N^2 of its scale (Markov)
            assert np.abs(wz[s] - ch.M[s][n]).max() <= 16 * EPS * g.zDim ** 2 * np.abs(ch.M[s]).max(), (n, s)


def test_kcap_on_every_ring_of_a_native_patch():
    import scythe_jl_amd as S
    case = cases.rl_advection(num_cells=30)
    g = cases.oracle_grid(case)
    gp, _ = cases.hip_params(case)
    rad = O.mish_points(g.xmin, g.DX, 0, g.nc)
    for i, r in enumerate(rad):
        _, _, kc, _ = S.eval_basis(gp, "h", [r, 0.5])
        assert kc == g.kmax[i] == i + 1, (i, r, kc)
        if i + 1 < len(rad):
            assert S.eval_basis(gp, "h", [0.5 * (r + rad[i + 1]), 0.5])[2] == g.kmax[i]
        assert S.eval_basis(gp, "h", [r, 0.5], True)[2] == g.kDim
    assert S.eval_basis(gp, "h", [g.xmin, 0.0])[2] == 1          # below the first ring: ring 1
    assert S.eval_basis(gp, "h", [g.xmax, 0.0])[2] == g.kmax[-1]
    # three tiles: the same radii give the same cap whatever tile is asked, and the shared edge is accepted by both neighbours
    edge = g.xmin + 10 * g.DX
    assert S.eval_basis(gp, "h", [edge, 0.0], False, 0, 10)[0] == 9
    assert S.eval_basis(gp, "h", [edge, 0.0], False, 10, 10)[0] == 10
    assert S.eval_basis(gp, "h", [edge, 0.0], False, 0, 10)[2] == S.eval_basis(gp, "h", [edge, 0.0], False, 10, 10)[2]


def test_eval_basis_refusals():
    import scythe_jl_amd as S
    case = cases.rlz_advection(num_cells=6, zDim=9)
    g = cases.oracle_grid(case)
    gp, _ = cases.hip_params(case)
    ok = [2.0, 1.0, 1.0]
    S.eval_basis(gp, "h", ok)
    for bad in ([g.xmax * (1 + 1e-12), 1.0, 1.0], [-1e-9, 1.0, 1.0], [2.0, 1.0, g.zmax + 1e-9], [2.0, 1.0, -1e-9],
                [np.nan, 1.0, 1.0], [2.0, np.inf, 1.0], [2.0, 1.0, np.nan]):
        with pytest.raises(S.ScytheHipError) as e:
            S.eval_basis(gp, "h", bad)
        assert str(e.value)
    # r of another tile
    with pytest.raises(S.ScytheHipError):
        S.eval_basis(gp, "h", [g.xmin + 4.5 * g.DX, 1.0, 1.0], False, 0, 3)
    S.eval_basis(gp, "h", [g.xmin + 3 * g.DX, 1.0, 1.0], False, 0, 3)
    S.eval_basis(gp, "h", ok)


def test_point_generators():
    import scythe_jl_amd as S
    gp, _ = cases.hip_params(cases.rlz_advection(num_cells=4, zDim=9))
    p = S.regular_gridpoints(gp, 5, 7, 3)
    assert p.shape == (5 * 7 * 3, 3)
    assert p[:, 0].min() == gp.xmin and p[:, 0].max() == gp.xmax
    assert p[:, 1].min() == 0.0 and p[:, 1].max() == 2 * np.pi
    assert p[:, 2].min() == gp.zmin and p[:, 2].max() == gp.zmax
    assert (p[:3, 0] == gp.xmin).all() and list(p[:3, 2]) == [gp.zmin, 0.5 * (gp.zmin + gp.zmax), gp.zmax]      # z fastest
    gr, _ = cases.hip_params(cases.r_bcs(num_cells=12))
    assert S.regular_gridpoints(gr, 9).shape == (9, 1)
    with pytest.raises(ValueError):
        S.regular_gridpoints(gp, 5)
    case = cases.rl_advection(num_cells=8)
    case["grid"]["xmin"] = 2.0
    gl, _ = cases.hip_params(case)
    pts, idx = S.cartesian_gridpoints(gl, 21, 17)
    x, y = np.meshgrid(np.linspace(-gl.xmax, gl.xmax, 21), np.linspace(-gl.xmax, gl.xmax, 17), indexing="ij")
    r = np.hypot(x, y).reshape(-1)
    inside = (r >= gl.xmin) & (r <= gl.xmax)
    assert 0 < inside.sum() < r.size                       # the corners and the hole are cut
    assert (idx == np.nonzero(inside)[0]).all() and pts.shape == (inside.sum(), 2)
    assert np.allclose(pts[:, 0] * np.cos(pts[:, 1]), x.reshape(-1)[idx], atol=1e-12)
    assert np.allclose(pts[:, 0] * np.sin(pts[:, 1]), y.reshape(-1)[idx], atol=1e-12)
    assert (pts[:, 1] >= 0).all() and (pts[:, 1] < 2 * np.pi).all()
    p3, i3 = S.cartesian_gridpoints(gp, 9, 9, 2)
    assert p3.shape[1] == 3 and len(i3) == len(p3) and set(p3[:, 2]) == {gp.zmin, gp.zmax}
    with pytest.raises(ValueError):
        S.cartesian_gridpoints(gr, 4, 4)


def test_writer_reuses_output_time_tag(tmp_path):
    """write_gridded_output with a stand-in run: the tag is output_time_tag's, the file sits beside physical_out_<tag>.csv"""
    import scythe_jl_amd as S
    from scythe_jl_amd import io
    gp, mp = cases.hip_params(cases.rl_advection(num_cells=8))
    mp.output_dir = str(tmp_path)

    class Run:
        def evaluate(self, p, all_k=False):
            v = np.arange(len(p) * 3 * 5, dtype=np.float64).reshape(len(p), 3, 5)
            return v, np.arange(len(p)) % 2 == 0

    pts, _ = S.cartesian_gridpoints(gp, 6, 6)
    for t in (0.3, 100.0, 1.0e6, 2.005):
        path = S.write_gridded_output(Run(), mp, t, pts)
        assert os.path.basename(path) == "gridded_out_%s.csv" % io.output_time_tag(t)
    with open(path) as f:
        header = f.readline().strip().split(",")
    assert header == ["r", "l"] + [n + s for s in ("", "_r", "_rr", "_l", "_ll") for n in ("h", "u", "v")]
    data = np.loadtxt(path, delimiter=",", skiprows=1, ndmin=2)
    assert data.shape == ((len(pts) + 1) // 2, 2 + 15)
    assert (data[:, :2] == pts[::2]).all()
