"""The twin of tests/extrema.py against tests/evaluate.py, and sx_newton_step (a pure host helper) against the twin's step."""
import ctypes as C

import numpy as np
import pytest

from tests import cases
from tests import evaluate as E
from tests import extrema as X

XP = X.XP
EPS = X.EPS


def _case(geom):
    if geom == "R":
        return cases.r_bcs(num_cells=24)
    if geom == "RZ":
        return cases.rz_advection(num_cells=10, zDim=14)
    if geom == "RL":
        return cases.rl_slab(num_cells=8)
    return cases.rlz_hrbl(num_cells=6, zDim=10, ring_L=16)


def _point(g, r, lam=0.7, zf=0.37):
    return np.array([r] + ([lam] if g.has_l else []) + ([g.zmin + zf * (g.zmax - g.zmin)] if g.has_z else []))


@pytest.mark.parametrize("geom", ["R", "RZ", "RL", "RLZ"])
def test_twin_derivatives(geom):
    """u, u_r, u_rr, u_l, u_ll, u_z, u_zz are evaluate's slots; the mixed ones are centred differences of evaluate's r and l slots"""
    g = cases.oracle_grid(_case(geom))
    A = np.random.default_rng(3).standard_normal((g.S_patch(), g.V))
    sl = {s: i for i, s in enumerate(g.slots)}
    var = g.V
    for r in (g.xmin + 0.3 * g.DX, g.xmin + 3.4 * g.DX, g.xmax - 0.45 * g.DX):          # the first cell next to xmin among them
        p = _point(g, r)
        d, S, B = X.derivatives(g, A, var, p, xp=True, with_bound=True)
        ev = E.evaluate(g, A, p[None, :], all_k=True, xp=True)[0, var - 1]
        direct = {"u": 0, "r": 1, "rr": 4, "l": 2, "ll": 7, "z": 3, "zz": 9}
        for s, m in direct.items():
            if s in sl:
                assert abs(d[m] - ev[sl[s]]) <= 64 * 2.0 ** -64 * S[m] * g.b_zDim * g.K2, (geom, r, s)
                assert B[m] > 0
        mixed = []
        if g.has_l:
            mixed.append((5, "r", 1, 1e-6))                                             # u_rl = d/dl of the r slot
        if g.has_z:
            mixed.append((6, "r", len(p) - 1, 1e-6 * (g.zmax - g.zmin)))                 # u_rz = d/dz of the r slot
        if g.has_l and g.has_z:
            mixed.append((8, "l", len(p) - 1, 1e-6 * (g.zmax - g.zmin)))                 # u_lz = d/dz of the l slot
        for m, slot, axis, h in mixed:
            hi, lo = p.copy(), p.copy()
            hi[axis] += h
            lo[axis] -= h
            e = E.evaluate(g, A, np.stack([hi, lo]), all_k=True, xp=True)[:, var - 1, sl[slot]]
            fd = (e[0] - e[1]) / (XP(hi[axis]) - XP(lo[axis]))
            # truncation h^2 / 6 x the third derivative: k^2 (lambda) or (pi zDim / Lz)^2 (z) of the derivative itself, generously
            scale = (g.kDim ** 2 if axis == 1 and g.has_l else (np.pi * g.zDim / (g.zmax - g.zmin)) ** 2) * S[m]
            assert S[m] > 0 and abs(d[m] - fd) <= h * h * scale + 2.0 ** -60 * S[m] / (h / max(abs(p[axis]), h)), (geom, r, X.NAMES[m])


MASKS = {"R": ["r"], "RZ": ["r", "z", "rz"], "RL": ["r", "l", "rl"], "RLZ": ["r", "l", "z", "rl", "rz", "lz", "rlz"]}


def _good_d(g, rng, r):
    """derivatives with a negative definite, well-conditioned Hessian in every coordinate system and a step well inside the caps"""
    Lz = (g.zmax - g.zmin) if g.has_z else 1.0
    sc = np.array([g.DX, 1.0 if not g.has_l else g.DX / max(r, g.DX), Lz])             # natural length of each native coordinate
    B = rng.standard_normal((3, 3)) * 0.2
    H = -(np.eye(3) + B @ B.T)
    H = H / np.outer(sc, sc)
    grad = rng.standard_normal(3) * 1e-3 / sc
    d = np.array([1.0, grad[0], grad[1], grad[2], H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]])
    if not g.has_l:
        d[[2, 5, 7, 8]] = 0.0
    if not g.has_z:
        d[[3, 6, 8, 9]] = 0.0
    return d


@pytest.mark.parametrize("geom", ["R", "RZ", "RL", "RLZ"])
def test_newton_step_against_twin(geom):
    import scythe_jl_amd as S
    case = _case(geom)
    gp, _ = cases.hip_params(case)
    g = cases.oracle_grid(case)
    rng = np.random.default_rng(8)
    n_bitwise = 0
    for free in MASKS[geom]:
        for r in (g.xmin + 0.3 * g.DX, g.xmin + 3.4 * g.DX):
            p = _point(g, r)
            d = _good_d(g, rng, r)
            mask = S.free_mask(gp, free)
            got, st = S.newton_step(gp, p, d, "max", free, 1e-9)
            info = {}
            want, wst = X.newton_step(g, 1, mask, 1e-9, p, d, np.float64, info)
            assert st == wst == -1, (geom, free, st, wst)
            if got.tobytes() == np.asarray(want, dtype=np.float64).tobytes():
                n_bitwise += 1
            # 4 ulp of the step (in the coordinates it is taken in; a lambda step seen from r: its arc)
            step = np.abs(np.asarray(info["step"], dtype=np.float64))
            tol_r = 4 * EPS * max(step[0], step[1] if "l" in free and "r" in free else 0.0, abs(r))
            assert abs(got[0] - float(want[0])) <= tol_r, (geom, free)
            if g.has_l:
                assert abs(got[1] - float(want[1])) <= 4 * EPS * max(np.pi, step[1]) + (tol_r / r if "r" in free and "l" in free else 0.0), (geom, free)
            if g.has_z:
                assert abs(got[-1] - float(want[-1])) <= 4 * EPS * max(step[2], abs(p[-1])), (geom, free)
            for c, name in enumerate(geom.lower()):
                if name not in free:
                    assert got[c] == p[c], (geom, free, name)                           # a frozen coordinate keeps its value
            # the longdouble twin agrees to the conditioning of the (well-conditioned) system
            wl, _ = X.newton_step(g, 1, mask, 1e-9, p, d, XP)
            assert np.abs(np.asarray(wl, dtype=np.float64) - got).max() <= 1e-12 * max(abs(r), g.DX)
    print("%s: %d of %d steps bitwise equal to the float64 twin" % (geom, n_bitwise, 2 * len(MASKS[geom])))
    assert n_bitwise >= 2 * sum(1 for f in MASKS[geom] if not ("r" in f and "l" in f))    # the same sequence where no trigonometry enters


def test_cartesian_pair_against_2x2_solve():
    """u = -1/2 (a dx^2 + 2 b dx dy + c dy^2) about (X0, Y0): Newton's step from anywhere lands on (X0, Y0); the native derivatives
    are written out by hand and the 2 x 2 system is solved by Cramer's rule in longdouble"""
    import scythe_jl_amd as S
    case = _case("RL")
    gp, _ = cases.hip_params(case)
    g = cases.oracle_grid(case)
    a, b, c = 2.0 / g.DX ** 2, 0.3 / g.DX ** 2, 1.5 / g.DX ** 2
    for (X0, Y0), (r, lam) in [((0.3 * g.DX, 0.1 * g.DX), (0.45 * g.DX, 2.1)), ((3.4 * g.DX, -0.2 * g.DX), (3.1 * g.DX, 0.1)),
                               ((-1.2 * g.DX, 0.4 * g.DX), (1.0 * g.DX, -3.0))]:
        cs, sn = np.cos(XP(lam)), np.sin(XP(lam))
        dx, dy = XP(r) * cs - XP(X0), XP(r) * sn - XP(Y0)
        uX, uY, uXX, uXY, uYY = -(a * dx + b * dy), -(b * dx + c * dy), XP(-a), XP(-b), XP(-c)
        rr = XP(r)
        d = [-(a * dx * dx + 2 * b * dx * dy + c * dy * dy) / 2,
             uX * cs + uY * sn, rr * (-uX * sn + uY * cs), 0,
             uXX * cs * cs + 2 * uXY * sn * cs + uYY * sn * sn,
             -sn * uX + cs * uY + rr * (-sn * cs * uXX + (cs * cs - sn * sn) * uXY + sn * cs * uYY), 0,
             -rr * (uX * cs + uY * sn) + rr * rr * (sn * sn * uXX - 2 * sn * cs * uXY + cs * cs * uYY), 0, 0]
        d64 = np.array([float(x) for x in d])
        got, st = S.newton_step(gp, [r, lam], d64, "max", "rl", 1e-9)
        assert st == -1
        gX, gY = XP(got[0]) * np.cos(XP(got[1])), XP(got[0]) * np.sin(XP(got[1]))
        # Cramer on the twin's Cartesian system
        gr, H = X.cartesian(d64, r, lam, XP)
        det = H[0, 0] * H[1, 1] - H[0, 1] * H[0, 1]
        sX, sY = -(gr[0] * H[1, 1] - gr[1] * H[0, 1]) / det, -(H[0, 0] * gr[1] - H[0, 1] * gr[0]) / det
        cond = float(np.linalg.cond(np.asarray(H[:2, :2], dtype=np.float64)))
        step = float(np.hypot(sX, sY))
        # the transform divides by r and cancels: its error is eps |d| / r^2-sized entries of H, i.e. eps cond (r / step-free) ... held to
        # 64 eps cond (step + r): the step's own 4 ulp, the transform's cancellation and the rounding of the d handed over
        tol = 64 * EPS * cond * (step + r)
        assert abs(gX - (XP(r) * cs + sX)) <= tol and abs(gY - (XP(r) * sn + sY)) <= tol
        assert abs(gX - XP(X0)) <= tol and abs(gY - XP(Y0)) <= tol, (float(gX - X0), float(gY - Y0), tol)
        assert -np.pi < got[1] <= np.pi


def test_newton_step_decisions():
    import scythe_jl_amd as S
    case = _case("RLZ")
    gp, _ = cases.hip_params(case)
    g = cases.oracle_grid(case)
    Lz = g.zmax - g.zmin
    rng = np.random.default_rng(2)
    r = 3.4 * g.DX
    p = _point(g, r)
    d = _good_d(g, rng, r)
    # wrong definiteness: 4, no step
    for want, dd in (("min", d), ("max", -d), ("any", d * 0.0)):
        got, st = S.newton_step(gp, p, dd, want, "rlz")
        assert st == 4 and got.tobytes() == p.tobytes()
    got, st = S.newton_step(gp, p, -d, "min", "rlz")
    assert st == -1
    got, st = S.newton_step(gp, p, d, "any", "rlz")
    assert st == -1
    # a step across xmax: 1, position = the last inside position
    pe = _point(g, g.xmax - 0.1 * g.DX)
    de = np.zeros(10)
    de[1], de[4] = 1.0 / g.DX, -1.0 / g.DX ** 2                                          # Newton step = +DX in r
    got, st = S.newton_step(gp, pe, de, "max", "r")
    assert st == 1 and got.tobytes() == pe.tobytes()
    # across zmax: 2
    pz = _point(g, r, zf=0.95)
    dz = np.zeros(10)
    dz[3], dz[9] = 1.0 / Lz, -10.0 / Lz ** 2                                             # +Lz / 10
    got, st = S.newton_step(gp, pz, dz, "max", "z")
    assert st == 2 and got.tobytes() == pz.tobytes()
    # the pole zone: 3 (r and lambda free only)
    pp = _point(g, 5e-7 * g.DX)
    got, st = S.newton_step(gp, pp, d, "max", "rlz")
    assert st == 3 and got.tobytes() == pp.tobytes()
    got, st = S.newton_step(gp, _point(g, 0.0), d, "max", "rl")
    assert st == 3
    got, st = S.newton_step(gp, pp, de, "max", "r")
    assert st == -1
    # a tiny step: 0, and the position after it
    dt = d.copy()
    dt[1:4] *= 1e-9
    got, st = S.newton_step(gp, p, dt, "max", "rlz", 1e-9)
    want, wst = X.newton_step(g, 1, 7, 1e-9, p, dt, XP)
    assert st == wst == 0 and np.abs(got - np.asarray(want, dtype=np.float64)).max() <= 1e-12 * r and got.tobytes() != p.tobytes()
    # free_mask == 0: 0 at once
    got, st = S.newton_step(gp, p, d, "max", 0)
    assert st == 0 and got.tobytes() == p.tobytes()
    # the caps scale the whole step by ONE factor: horizontal 40 DX, vertical 1.5 Lz asked for -> factor min(1 / 40, 1 / 12)
    dc = np.zeros(10)
    dc[1], dc[4], dc[3], dc[9] = 40.0 / g.DX, -1.0 / g.DX ** 2, 1.5 / Lz, -1.0 / Lz ** 2
    dc[7] = -1.0
    p0 = _point(g, r, zf=0.5)
    got, st = S.newton_step(gp, p0, dc, "max", "rz")
    assert st == -1
    assert abs((got[0] - p0[0]) - g.DX) <= 8 * EPS * r and abs((got[2] - p0[2]) - 1.5 * Lz / 40.0) <= 8 * EPS * Lz
    dc[1], dc[3] = 2.0 / g.DX, 1.5 / Lz                                                   # now the vertical cap binds: factor 1 / 12
    got, st = S.newton_step(gp, p0, dc, "max", "rz")
    assert abs((got[2] - p0[2]) - Lz / 8.0) <= 8 * EPS * Lz and abs((got[0] - p0[0]) - 2.0 * g.DX / 12.0) <= 8 * EPS * r
    # lambda wraps into (-pi, pi]
    pl = _point(g, r, lam=3.1)
    dl = np.zeros(10)
    dl[2], dl[7] = 0.1, -1.0                                                             # +0.1 in lambda: 3.2 -> 3.2 - 2 pi
    got, st = S.newton_step(gp, pl, dl, "max", "l")
    assert st == -1 and abs(got[1] - (3.2 - 2 * np.pi)) <= 8 * EPS * np.pi and -np.pi < got[1] <= np.pi
    # Cartesian: a step across the centre comes out with lambda on the other side, inside (-pi, pi]
    pc = _point(g, 0.2 * g.DX, lam=0.0, zf=0.5)
    dcart = np.zeros(10)
    dcart[1], dcart[4] = -0.5 / g.DX, -1.0 / g.DX ** 2                                   # u = -(X + 0.3 DX)^2 / (2 DX^2) along the ray
    dcart[7] = -pc[0] * dcart[1] - pc[0] ** 2 / g.DX ** 2                                # u_YY = -1 / DX^2
    got, st = S.newton_step(gp, pc, dcart, "max", "rl")
    assert st == -1 and abs(got[0] - 0.3 * g.DX) <= 1e-9 * g.DX and got[1] == np.pi


def test_newton_step_refusals():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    from scythe_jl_amd.model import grid_desc
    lib = L.load()
    gp_rlz, _ = cases.hip_params(_case("RLZ"))
    gp_r, _ = cases.hip_params(_case("R"))
    gp_rz, _ = cases.hip_params(_case("RZ"))
    d = np.zeros(10)
    d[4] = d[7] = d[9] = -1.0
    ok = np.array([1.0e5, 0.5, 500.0])

    def raw(gp, want, mask, tol, pos, dd, out=True, st=True):
        desc, keep = grid_desc(gp)
        new, s = np.full(3, -7.25), C.c_int32(-9)
        p = None if pos is None else np.ascontiguousarray(pos, dtype=np.float64)
        rc = lib.sx_newton_step(C.byref(desc) if gp is not None else None, want, mask, tol, None if p is None else p.ctypes.data_as(L.P_D),
                                None if dd is None else dd.ctypes.data_as(L.P_D), new.ctypes.data_as(L.P_D) if out else None,
                                C.byref(s) if st else None)
        return rc, new, s.value

    assert raw(gp_rlz, 1, 7, 1e-9, ok, d)[0] == 0
    bad = [("null pos", gp_rlz, 1, 7, 1e-9, None, d, True, True), ("null d", gp_rlz, 1, 7, 1e-9, ok, None, True, True),
           ("null new_pos", gp_rlz, 1, 7, 1e-9, ok, d, False, True), ("null status", gp_rlz, 1, 7, 1e-9, ok, d, True, False),
           ("want", gp_rlz, 2, 7, 1e-9, ok, d, True, True), ("want below", gp_rlz, -2, 7, 1e-9, ok, d, True, True),
           ("mask bit 8", gp_rlz, 1, 8, 1e-9, ok, d, True, True), ("l on R", gp_r, 1, 2, 1e-9, [5.0], d, True, True),
           ("z on R", gp_r, 1, 4, 1e-9, [5.0], d, True, True), ("l on RZ", gp_rz, 1, 3, 1e-9, [5.0e3, 4.0e3], d, True, True),
           ("tol nan", gp_rlz, 1, 7, float("nan"), ok, d, True, True), ("tol inf", gp_rlz, 1, 7, float("inf"), ok, d, True, True),
           ("r nan", gp_rlz, 1, 7, 1e-9, [float("nan"), 0.5, 500.0], d, True, True), ("r out", gp_rlz, 1, 7, 1e-9, [3.1e5, 0.5, 500.0], d, True, True),
           ("lambda inf", gp_rlz, 1, 7, 1e-9, [1e5, float("inf"), 500.0], d, True, True), ("z out", gp_rlz, 1, 7, 1e-9, [1e5, 0.5, 2000.5], d, True, True)]
    for what, gp, want, mask, tol, pos, dd, out, st in bad:
        rc, new, s = raw(gp, want, mask, tol, pos, dd, out, st)
        assert rc != 0 and lib.sx_last_error().decode(), what
        assert (new == -7.25).all() and s == -9, what
    desc, keep = grid_desc(gp_rlz)
    desc.abi_version = 1
    new, s = np.zeros(3), C.c_int32(0)
    assert lib.sx_newton_step(C.byref(desc), 1, 7, 1e-9, ok.ctypes.data_as(L.P_D), d.ctypes.data_as(L.P_D), new.ctypes.data_as(L.P_D), C.byref(s)) != 0
    assert lib.sx_newton_step(None, 1, 7, 1e-9, ok.ctypes.data_as(L.P_D), d.ctypes.data_as(L.P_D), new.ctypes.data_as(L.P_D), C.byref(s)) != 0
    with pytest.raises(ValueError):
        S.free_mask(gp_rlz, "rx")


def test_scan_twin_rules():
    """the twin's own tie, signed-zero and NaN rules on a hand-made field"""
    L, nz = np.array([2, 3]), 2
    q = np.array([[1.0, 5.0, -0.0, 5.0, 0.0, 2.0, -1.0, 2.0, -1.0, 5.0]])
    val, idx = X.scan(q, L, nz)
    assert idx[:, 0].tolist() == [6, 1] and val[:, 0].tolist() == [-1.0, 5.0]
    val, idx = X.scan(q, L, nz, "azimuth")
    assert idx[0, :, :, 0].tolist() == [[2, 1], [6, 5]] and idx[1, :, :, 0].tolist() == [[0, 1], [4, 9]]
    z = np.array([[0.0, -0.0, -0.0, 0.0]])
    val, idx = X.scan(z, np.array([2]), 2)
    assert idx[:, 0].tolist() == [0, 0] and not np.signbit(val[0, 0])
    q[0, 7] = np.nan
    val, idx = X.scan(q, L, nz)
    assert np.isnan(val).all() and idx[:, 0].tolist() == [7, 7]
    val, idx = X.scan(q, L, nz, "azimuth")
    assert np.isnan(val[:, 1, 1, 0]).all() and idx[:, 1, 1, 0].tolist() == [7, 7] and idx[0, 1, 0, 0] == 6


def test_packing(monkeypatch):
    """Grid.extrema hands its term list to pack_reduce_program exactly as Grid.reduce does: the packer is replaced by a recorder that
    stops the call before it reaches the library"""
    import scythe_jl_amd as S
    from scythe_jl_amd import model as M
    gp, _ = cases.hip_params(_case("RLZ"))
    terms = [(0, 1.0, 0, [("ub", ""), ("ub", "")]), (0, 1.0, 0, [("vb", ""), ("vb", "")]), (1, 2.0, -1, [("h", "l")])]

    class Stop(Exception):
        pass
    seen = []

    def recorder(patch, t):
        seen.append((patch, t))
        raise Stop()
    tile = S.Grid.__new__(S.Grid)                          # no handle: the packer is the first thing both methods call
    tile.patch_params = gp
    with monkeypatch.context() as mp:
        mp.setattr(M, "pack_reduce_program", recorder)
        for call in (lambda: S.Grid.reduce(tile, terms, "azimuth", "state"), lambda: S.Grid.extrema(tile, terms, "azimuth", "state")):
            with pytest.raises(Stop):
                call()
    assert len(seen) == 2 and seen[0][0] is gp and seen[1][0] is gp and seen[0][1] is terms and seen[1][1] is terms
    coef, packed, n_out = S.pack_reduce_program(gp, terms)
    assert n_out == 2 and packed.shape == (3, 11) and packed[2].tolist() == [1, -1, 1, 1, 0, 0, 0, 3, 0, 0, 0]
    assert S.reduce_planes(gp, terms).tolist() == [[4, 0], [5, 0], [1, 3]]
