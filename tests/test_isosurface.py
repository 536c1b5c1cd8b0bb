"""CPU-only: the host side of sx_isosurface (include/scythe_hip.h "isosurfaces") - the symbols, sx_column_series
against the twin of tests/isosurface.py, sx_isosurface_check with every refusal that needs no device, and the twin itself against
a closed form.

test_twin_converges_to_closed_form prints both errors; DESIGN.md 21, "Figures", holds them."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import isosurface as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XP = I.XP


def test_symbols():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    header = open(os.path.join(ROOT, "include", "scythe_hip.h")).read()
    for name in ("sx_isosurface", "sx_column_series", "sx_isosurface_check"):
        assert hasattr(lib, name) and name in L.SYMBOLS
        assert "int " + name + "(" in header
    assert callable(S.Grid.isosurface) and callable(S.ModelRun.height_where) and callable(S.ModelRun.on_surface)
    assert callable(S.isosurface_check) and callable(S.column_series) and callable(S.columns_of)


# ----------------------------------------------------------------------------- sx_column_series against the twin
@pytest.mark.parametrize("zDim", [8, 24, 25, 65])
def test_column_series_against_the_twin(zDim):
    """Random coefficients with a decaying tail; heights: random, every station (the oracle's levels), both ends.  All three
    outputs are BITWISE the float64 twin - the twin follows the helper operation for operation: the recurrence for T_n, products
    then sums in index order for Dc a, no fused multiply-add anywhere - and inside the derived bound of the longdouble twin
    (I.series_bound, I.coeff_bound)."""
    import scythe_jl_amd as S
    zmin, zmax = -250.0, 1750.0                                              # mid != 0: the x of a height is not exact
    rng = np.random.default_rng(zDim)
    a = rng.standard_normal(zDim) / (1.0 + np.arange(zDim)) ** 1.5
    Dc64, Dcx = I.dc_of(zDim, zmin, zmax, xp=False), I.dc_of(zDim, zmin, zmax, xp=True)
    a64 = [a, I.apply_dc(Dc64, a, False)]
    a64.append(I.apply_dc(Dc64, a64[1], False))
    ax = [a.astype(XP), Dcx @ a.astype(XP)]
    ax.append(Dcx @ ax[1])
    Dabs = np.abs(Dc64)
    bnd, aa, da = [], np.abs(a), np.zeros(zDim)
    for d in range(3):
        bnd.append(I.series_bound(zmin, zmax, aa, da))
        aa, da = I.coeff_bound(Dabs, aa, da)
    lev = np.cos(np.arange(zDim) * np.pi / (zDim - 1)) * (-0.5 * (zmax - zmin)) + 0.5 * (zmin + zmax)
    heights = np.concatenate([rng.uniform(zmin, zmax, 40), lev, [zmin, zmax]])
    worst = np.zeros(3)
    for z in heights:
        got = S.column_series(zmin, zmax, a, z)
        for d in range(3):
            assert got[d].tobytes() == np.float64(I.series(zmin, zmax, a64[d], z, xp=False)).tobytes(), (zDim, z, d)
            err = abs(float(XP(got[d]) - I.series(zmin, zmax, ax[d], z, xp=True)))
            worst[d] = max(worst[d], err / bnd[d])
            assert err <= bnd[d], (zDim, z, d, err, bnd[d])
    print("zDim %d: worst error / bound of value, d/dz, d2/dz2: %.3g %.3g %.3g" % (zDim, *worst))
    # a polynomial the series holds exactly: f = 3 + 2 x - x^2 in x = (z - mid) / (-half): a = (2.5, 1, -0.25)
    p = np.zeros(zDim)
    p[:3] = [2.5, 1.0, -0.25]
    mid, half = 0.5 * (zmin + zmax), 0.5 * (zmax - zmin)
    for z in (zmin, 300.0, zmax):
        x = (z - mid) / (-half)
        want = np.array([3.0 + 2.0 * x - x * x, (2.0 - 2.0 * x) / (-half), -2.0 / (half * half)])
        assert np.allclose(S.column_series(zmin, zmax, p, z), want, rtol=1e-12, atol=1e-15)


def test_column_series_refusals():
    import scythe_jl_amd as S
    a = np.ones(8)
    for kw, word in ((dict(zmin=0.0, zmax=0.0, a=a, z=0.0), "invalid"), (dict(zmin=0.0, zmax=1.0, a=np.ones(3), z=0.5), "invalid"),
                     (dict(zmin=0.0, zmax=1.0, a=a, z=1.5), "outside"), (dict(zmin=0.0, zmax=1.0, a=a, z=np.nan), "NaN")):
        with pytest.raises(S.ScytheHipError, match=word):
            S.column_series(**kw)
    lib = S.load()
    out = np.zeros(3)
    assert lib.sx_column_series(8, 0.0, 1.0, None, 0.5, out.ctypes.data_as(C.POINTER(C.c_double))) != 0 and b"null" in lib.sx_last_error()


# ----------------------------------------------------------------------------- sx_isosurface_check
def _patch(geometry, **over):
    import scythe_jl_amd as S
    kw = dict(geometry=geometry, xmin=0.0, xmax=10.0, num_cells=5, vars={"h": 1, "u": 2, "v": 3})
    if "L" in geometry:
        kw["ring_uniform_L"] = 8
    if "Z" in geometry:
        kw.update(zmin=0.0, zmax=3.0, zDim=8)
    kw.update(over)
    return S.GridParameters(**kw)


def test_check_counts_profiles_in_first_use_order():
    """a program that names every slot: u, z, zz share the profile (0, 0) of their variable; r, rr, l, ll take one each"""
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    for geometry, per_var in (("RZ", 3), ("RLZ", 5)):
        gp = _patch(geometry)
        slots = [s if s != "u" else "" for s in L.SLOTS[geometry]]
        every = [(0, 1.0, 0, [("h", s)]) for s in slots]
        assert S.isosurface_check(gp, every) == per_var
        assert S.isosurface_check(gp, every + [(1, 1.0, 0, [("u", "z")]), (2, 1.0, 0, [("u", "r"), ("h", "zz")])], carry=2) == per_var + 2
        assert S.isosurface_check(gp, [(0, 2.0, 2, [])]) == 0                # r^2: no plane, no profile
        # the order: the twin's plan numbers the same keys, first use first
        g = O.Grid(geometry, 0.0, 10.0, 5, {"h": 1, "u": 2, "v": 3}, zmin=0.0, zmax=3.0, zDim=8, **({"ring_L": 8} if "L" in geometry else {}))
        prog = [(0, 1.0, 0, [("u", "z"), ("h", "r")]), (0, 1.0, 0, [("h", "")]), (1, 1.0, 0, [("u", "")])]
        pl = I.plan(g, S.pack_reduce_program(gp, prog)[1])
        assert pl.keys == [(2, 0), (1, 1), (1, 0)] and pl.pprof == [0, 1, 2, 0] and pl.pz == [1, 0, 0, 0]
        assert S.isosurface_check(gp, prog, carry=1) == len(pl.keys)


def test_check_refusals_without_a_device():
    import scythe_jl_amd as S
    gp = _patch("RLZ")
    ok = [(0, 1.0, 0, [("h", "")])]
    assert S.isosurface_check(gp, ok) == 1
    for geometry in ("R", "RL"):
        with pytest.raises(S.ScytheHipError, match="no vertical"):
            S.isosurface_check(_patch(geometry), ok)
    with pytest.raises(S.ScytheHipError, match="n_carry"):
        S.isosurface_check(gp, ok, carry=9)
    with pytest.raises(S.ScytheHipError, match="n_carry"):
        S.isosurface_check(gp, ok, carry=-1)
    with pytest.raises(S.ScytheHipError, match="out = 1"):                   # a term whose out is above n_carry
        S.isosurface_check(gp, ok + [(1, 1.0, 0, [("u", "")])], carry=0)
    with pytest.raises(S.ScytheHipError, match="r_power"):
        S.isosurface_check(gp, [(0, 1.0, 3, [("h", "")])])
    with pytest.raises(S.ScytheHipError, match="var"):
        S.isosurface_check(gp, [(0, 1.0, 0, [(4, "")])])
    with pytest.raises(S.ScytheHipError, match="slot"):
        S.isosurface_check(_patch("RZ"), [(0, 1.0, 0, [(1, 5)])])
    with pytest.raises(S.ScytheHipError, match="more than 16"):
        S.isosurface_check(gp, [(0, 1.0, 0, [(v, s)]) for v in (1, 2, 3) for s in range(6)])
    # the tables of one column batch: 32 (kDim + 1) + 2304 <= 8192 doubles, so kDim <= 183; native rings of 62 cells reach 186
    with pytest.raises(S.ScytheHipError, match=r"32 \(kDim \+ 1\) \+ 2304 <= 8192"):
        S.isosurface_check(_patch("RLZ", num_cells=62, ring_uniform_L=0), ok)
    assert S.isosurface_check(_patch("RLZ", num_cells=61, ring_uniform_L=0), ok) == 1
    lib = S.load()
    n = C.c_int32(-5)
    assert lib.sx_isosurface_check(None, 0, None, 0, C.byref(n)) != 0 and b"null" in lib.sx_last_error() and n.value == -5


def test_columns_of():
    import scythe_jl_amd as S
    gp = _patch("RLZ")
    pts = S.regular_gridpoints(gp, 3, 4, 5)
    cols = S.columns_of(gp, pts)
    assert cols.shape == (12, 2) and np.array_equal(cols, pts[::5, :2])
    cpts, _ = S.cartesian_gridpoints(gp, 4, 4, 3)
    assert np.array_equal(S.columns_of(gp, cpts), cpts[::3, :2])
    with pytest.raises(ValueError):
        S.columns_of(_patch("RL"), pts)


# ----------------------------------------------------------------------------- the twin against a closed form
GAMMA, EPS2, B0, B_LEN, LEVEL = 2.0, 0.1, 1.5, 4.0, 4.0


def _b(r):
    """vanishes like r^2 at the centre, so that b cos 2 lambda is a smooth function of (x, y) there: with b(0) != 0 the wave-2 part
    is not single-valued at r = 0 and the spline's error near the centre is not fourth order (the ratio drops to 2.7)"""
    return B0 * (r / B_LEN) ** 2 * np.exp(-(r / B_LEN) ** 2)


def closed_form_case(nc, zDim=8):
    """f = Gamma z + b(r) (1 + eps cos 2 lambda) projected onto an RLZ grid (linear in z: the Chebyshev series holds it exactly)"""
    g = O.Grid("RLZ", 0.0, 10.0, nc, {"f": 1, "w": 2}, zmin=0.0, zmax=3.0, zDim=zDim, ring_L=16)
    pts = g.gridpoints()
    f = GAMMA * pts[:, 2] + _b(pts[:, 0]) * (1.0 + EPS2 * np.cos(2.0 * pts[:, 1]))
    return g, pts, np.stack([f, 0.5 * pts[:, 2] ** 2], axis=1)


def closed_form_columns():
    rng = np.random.default_rng(4)
    return np.stack([rng.uniform(0.3, 9.7, 24), rng.uniform(0.0, 2.0 * np.pi, 24)], axis=1)


def closed_form_height(cols):
    return (LEVEL - _b(cols[:, 0]) * (1.0 + EPS2 * np.cos(2.0 * cols[:, 1]))) / GAMMA


def _closed_form_error(nc):
    g, pts, vals = closed_form_case(nc)
    A = I.project(g, vals)
    cols = closed_form_columns()
    prog = (np.array([1.0]), np.array([[0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32), 1)
    res = I.isosurface(g, A, prog, [LEVEL], cols, max_cross=2, xp=True)
    assert (res.count == 1).all() and (res.dir[0] == 1).all() and (res.status == 0).all()
    return float(np.abs(res.height[0, 0] - closed_form_height(cols)).max())


def test_twin_converges_to_closed_form():
    """The surface f = c lies at z = (c - b(r) (1 + eps cos 2 lambda)) / Gamma exactly in z, so the error is the radial spline's:
    fourth order predicts 16 per halving of DX; more than 8 is asserted, from 10 to 20 cells, with b = 1.5 (r / 4)^2 exp(-(r / 4)^2)."""
    e10, e20 = _closed_form_error(10), _closed_form_error(20)
    print("closed form: |z - exact| max %.3e (10 cells), %.3e (20 cells), ratio %.1f" % (e10, e20, e10 / e20))
    assert e10 / e20 > 8.0


def test_selection_rules():
    h = np.full((3, 1, 4), np.nan)
    d = np.zeros((3, 1, 4), dtype=np.int32)
    h[:2, 0, 0], d[:2, 0, 0] = [1.0, 2.0], [1, -1]
    h[:3, 0, 1], d[:3, 0, 1] = [0.5, 1.5, 2.5], [-1, 1, -1]
    h[:1, 0, 2], d[:1, 0, 2] = [0.7], [-1]
    res = I.Result(h, d, None, None, None, None)
    assert np.array_equal(I.select(res, 0, "lowest"), [1.0, 0.5, 0.7, np.nan], equal_nan=True)
    assert np.array_equal(I.select(res, 0, "highest"), [2.0, 2.5, 0.7, np.nan], equal_nan=True)
    assert np.array_equal(I.select(res, 0, "lowest", rising=True), [1.0, 1.5, np.nan, np.nan], equal_nan=True)
    assert np.array_equal(I.select(res, 0, "highest", rising=False), [2.0, 2.5, 0.7, np.nan], equal_nan=True)
    from scythe_jl_amd import ModelRun
    for which, rising in (("lowest", None), ("highest", None), ("lowest", True), ("highest", False)):
        k = ModelRun._pick_height(res, which, rising)
        got = np.where(k >= 0, h[np.maximum(k, 0), 0, np.arange(4)], np.nan)
        assert np.array_equal(got, I.select(res, 0, which, rising), equal_nan=True)
