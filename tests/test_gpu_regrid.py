"""sx_regrid on the GPU: the values against the longdouble twin of tests/regrid.py within its derived bound, the destination's
coefficients as tests/test_gpu_project.py holds a companion's, the two closed forms re-centred, the bitwise guarantees, the columns
outside the source, and the ModelRun layer.  Shapes (tests/test_regrid.py::PAIRS) are the smallest that reach every path: an RLZ source
with native rings, 6 cells and zDim 10 (b_zDim 7: no multiple of 4 or 16) onto 9 cells with zDim 12 and other vertical classes - 1620
columns, so that source cells hold more than 16 columns and counts that are no multiple of 16, and the last tile of 16 is short; an RL
pair 6 -> 4 cells; an RZ and an R pair 5 -> 8 cells (the one-lane path)."""
import numpy as np
import pytest

from tests import cases
from tests import project as PJ
from tests import regrid as RG
from tests.test_regrid import OFFSET, PAIRS

pytestmark = pytest.mark.gpu

XP = RG.XP
VAR_SRC = {None: [1, 2, 3], "mixed": [3, 1, 3]}


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _field(p, geometry, seed=3):
    """smooth values [N, 3] at gridpoints p [N, n_coord]: a few radial, azimuthal and vertical scales per variable"""
    r = p[:, 0]
    lam = p[:, 1] if "L" in geometry else np.zeros(len(p))
    z = p[:, -1] if "Z" in geometry else np.zeros(len(p))
    out = []
    for v in range(3):
        a = np.exp(-((r - 1.0 - 0.5 * v) / 2.5) ** 2)
        out.append(a * (1.0 + 0.4 * (r / 3.0) * np.cos(lam - 0.3 * v) + 0.1 * (r / 3.0) ** 2 * np.sin(2 * lam)) * (1.0 + 0.3 * np.cos(0.9 * z + v)) + 0.05 * v)
    return np.stack(out, axis=1)


def _make(spec, values=True):
    import scythe_jl_amd as S
    gp, og = RG.oracle_pair(spec)
    tile = S.Grid(gp, None)
    if values:
        pts = S.getGridpoints(tile)
        tile.set_physical_values(_field(pts.reshape(len(pts), -1), gp.geometry))
        tile.spectralTransform_()
        tile.splineTransform_()
    return gp, og, tile


_SRC = {}


def _source(shape):
    """the source tile of a shape, made once and shared: (gp, oracle grid, tile, its A, its state)"""
    if shape not in _SRC:
        gp, og, tile = _make(PAIRS[shape][0])
        _SRC[shape] = (gp, og, tile, tile.patchSpectral, tile.get_state())
    return _SRC[shape]


def _levels(dst):
    import scythe_jl_amd as S
    pts = S.getGridpoints(dst)
    pts = pts.reshape(len(pts), -1)
    return pts[:max(dst.patch_params.zDim, 1), -1].copy() if "Z" in dst.patch_params.geometry else np.zeros(1)


def _existing_path(gp, vals):
    import scythe_jl_amd as S
    g = S.Grid(gp, None)
    g.set_physical_values(vals)
    g.spectralTransform_()
    g.splineTransform_()
    A = g.patchSpectral
    g.close()
    return A


@pytest.mark.parametrize("shape,centre,variables", [("RLZ", None, None), ("RLZ", OFFSET, "mixed"), ("RL", None, "mixed"), ("RL", OFFSET, None),
                                                    ("RZ", None, "mixed"), ("R", None, None)])
def test_values_and_coefficients(shape, centre, variables):
    import scythe_jl_amd as S
    gs, os_, src, A, _ = _source(shape)
    gd, od, dst = _make(PAIRS[shape][1], values=False)
    vs = VAR_SRC[variables]
    src.enable_timers(True)
    src.reset_timers()
    assert src.regrid(dst, centre, vs) == 0
    # 1. the values against the longdouble twin at the columns the library states, within the derived bound
    cols, ins = S.regrid_columns(gs, gd, centre)
    lev = _levels(dst)
    got = dst.var_np1
    want = RG.values(os_, A, vs, cols, ins, lev, xp=True)
    bound = RG.value_bound(os_, A, vs, cols, ins, lev)
    ratio = np.abs(got.astype(XP) - want) / bound
    print("%s %s %s: worst value at %.3g of its bound (%d columns, %d levels)" % (shape, centre, vs, float(ratio.max()), len(cols), len(lev)))
    assert got.shape == want.shape and float(ratio.max()) <= 1.0
    t = src.timers()
    assert t["k_regrid_levels"][1] == 1 and t["k_column_profiles"][1] == 1
    Zb, nz, ncls = os_.b_zDim, len(lev), (len({(os_.BCB[n], os_.BCT[n]) for n in os_.names}) if os_.has_z else 1)
    assert src.kernel_bytes("k_regrid_levels") == 8.0 * (3 * Zb * len(cols) + ncls * Zb * nz + 3 * dst.N) + 4.0 * len(cols)
    # 2. the coefficients: bitwise the existing forward chain fed the GPU's own values (whose repeatability is the premise), and within
    # tests/project.py's bar of the twins' coefficients of those values
    Ad = dst.patchSpectral
    E1, E2 = _existing_path(gd, got), _existing_path(gd, got)
    if _bits(E1) == _bits(E2):
        assert _bits(Ad) == _bits(E1), "%s: A against set_physical_values + transforms" % shape
    else:
        print("%s: the existing path does not repeat bitwise; held at the parity bar instead" % shape)
        assert np.max(np.abs(Ad - E1)) <= PJ.bar(E1)
    PJ.check_against_twins(Ad, RG.coefficients(od, got, xp=False), RG.coefficients(od, got, xp=True), "%s %s" % (shape, centre))
    dst.close()


@pytest.mark.parametrize("centre", [OFFSET, (-0.45, 0.15)])
def test_analytic_recentring(centre):
    """u = x and u = r^2 (R0 / R0 variables of the RL pair) regridded about (x0, y0), then evaluated at dst's gridpoints and at scattered
    points: x0 + r' cos l' and r'^2 + 2 r' (x0 cos l' + y0 sin l') + x0^2 + y0^2.  Both fields lie in either grid's spline and Fourier
    space, so what is left is the rounding of two forward chains and of evaluate: the project's parity bar, 1e-10 max|u|."""
    import scythe_jl_amd as S
    from tests import evaluate as EV
    spec_s, spec_d = (dict(s, vars={"x": 1, "rr": 2}) for s in PAIRS["RL"])
    gs, os_ = RG.oracle_pair(spec_s)
    src = S.Grid(gs, None)
    p = S.getGridpoints(src)
    src.set_physical_values(np.stack([p[:, 0] * np.cos(p[:, 1]), p[:, 0] ** 2], axis=1))
    src.spectralTransform_()
    src.splineTransform_()
    gd, od, dst = _make(spec_d, values=False)
    assert src.regrid(dst, centre) == 0
    x0, y0 = centre
    pts = np.concatenate([S.getGridpoints(dst), EV.scattered_points(od, 40, seed=5)])
    r, l = pts[:, 0], pts[:, 1]
    want = np.stack([x0 + r * np.cos(l), r * r + 2 * r * (x0 * np.cos(l) + y0 * np.sin(l)) + x0 * x0 + y0 * y0], axis=1)
    got = dst.evaluate(pts, all_k=True)[:, :, 0]
    err = np.abs(got - want).max(axis=0) / np.abs(want).max(axis=0)
    print("centre %s: u = x off by %.3g, u = r^2 by %.3g of max|u|" % (centre, err[0], err[1]))
    assert (err <= 1e-10).all()
    src.close()
    dst.close()


@pytest.mark.parametrize("shape,centre", [("RLZ", OFFSET), ("RL", OFFSET), ("RZ", None), ("R", None)])
def test_bitwise_guarantees(shape, centre):
    gs, os_, src, A, state = _source(shape)
    gd, od, dst = _make(PAIRS[shape][1], values=False)
    src.regrid(dst, centre, [1, 2, 3])
    first, firstA = dst.var_np1, dst.patchSpectral
    # two calls agree
    src.regrid(dst, centre, [1, 2, 3])
    assert _bits(dst.var_np1) == _bits(first) and _bits(dst.patchSpectral) == _bits(firstA)
    # one variable's result does not depend on what the other entries of var_src are
    src.regrid(dst, centre, [2, 2, 1])
    other = dst.var_np1
    assert _bits(other[:, 1]) == _bits(first[:, 1]) and _bits(other[:, 0]) == _bits(first[:, 1]) and _bits(other[:, 2]) == _bits(first[:, 0])
    # a column's values do not depend on the other columns: a destination with fewer cells of the same DX shares its cells' gridpoints
    spec = dict(PAIRS[shape][1])
    DX = (spec["xmax"] - spec["xmin"]) / spec["num_cells"]
    drop = 3 if shape == "RLZ" else 1
    spec.update(num_cells=spec["num_cells"] - drop, xmax=spec["xmax"] - drop * DX)
    g2, o2, small = _make(spec, values=False)
    src.regrid(small, centre, [1, 2, 3])
    assert small.N < dst.N and _bits(small.var_np1.T) == _bits(first[:small.N].T)
    # the source is unchanged
    assert _bits(src.get_state()) == _bits(state) and _bits(src.patchSpectral) == _bits(A)
    small.close()
    dst.close()


@pytest.mark.parametrize("shape", ["RLZ", "RL"])
def test_outside_columns(shape):
    import scythe_jl_amd as S
    centre = (2.5, 0.0)          # dst reaches r_s = 2.5 + 4.5 (RLZ) / 2.5 + 3 (RL) of the source's 6
    gs, os_, src, A, _ = _source(shape)
    if shape == "RL":            # the RL destination of 4 cells stays inside about this centre: one of 8 cells of the same DX pokes out
        spec = dict(PAIRS["RL"][1], num_cells=8, xmax=6.0)
    else:
        spec = dict(PAIRS[shape][1])
    gd, od, dst = _make(spec, values=False)
    nz = max(gd.zDim, 1)
    cols, ins = S.regrid_columns(gs, gd, centre)
    assert (ins == RG.inside(os_, cols[:, 0])).all() and 0 < int((~ins).sum()) < len(ins)
    # refused: nothing is written
    before = np.random.default_rng(1).standard_normal((dst.N, dst.V))
    dst.set_physical_values(before)
    with pytest.raises(S.ScytheHipError, match="SX_REGRID_REFUSE"):
        src.regrid(dst, centre)
    assert _bits(dst.var_np1) == _bits(before)
    with pytest.raises(S.ScytheHipError, match="fill"):
        src.regrid(dst, centre, outside="fill")
    with pytest.raises(S.ScytheHipError, match="fill"):
        src.regrid(dst, centre, outside="fill", fill=[0.0, np.nan, 0.0])
    assert _bits(dst.var_np1) == _bits(before)
    # filled
    fill = np.array([-1.5, 0.25, 7.0])
    assert src.regrid(dst, centre, outside="fill", fill=fill) == int((~ins).sum())
    got = dst.var_np1.reshape(len(cols), nz, 3)
    assert _bits(got[~ins]) == _bits(np.broadcast_to(fill, got[~ins].shape))
    lev = _levels(dst)
    want = RG.values(os_, A, [1, 2, 3], cols, ins, lev, fill=fill, xp=True).reshape(got.shape)
    bound = RG.value_bound(os_, A, [1, 2, 3], cols, ins, lev).reshape(got.shape)
    assert (np.abs(got.astype(XP) - want)[ins] <= bound[ins]).all()
    # the inside columns are bitwise what they are in a call where nothing is outside: the cells a smaller destination shares
    drop = 3 if shape == "RLZ" else 4           # to xmax = 3: r_s <= 5.5
    spec.update(num_cells=spec["num_cells"] - drop, xmax=spec["xmax"] - drop * (spec["xmax"] - spec["xmin"]) / spec["num_cells"])
    g2, o2, small = _make(spec, values=False)
    c2, i2 = S.regrid_columns(gs, g2, centre)
    assert i2.all() and src.regrid(small, centre) == 0
    assert _bits(small.var_np1.reshape(len(c2), nz, 3)) == _bits(got[:len(c2)])
    small.close()
    dst.close()


def test_model_run_regrid():
    """ModelRun.regrid, then three steps of LinearAdvectionRLZ on the new grid: finite, t carried, the first step taken as Euler (the
    state after it is bitwise that of a fresh run started from the regridded state)"""
    import dataclasses
    import scythe_jl_amd as S
    case = cases.rlz_advection(num_cells=6, zDim=10)
    hip = cases.HipModel(case)
    for _ in range(2):
        hip.step()
    run = hip.run
    gp_new = dataclasses.replace(hip.gp, num_cells=9, xmax=7.5, zDim=12, zmin=0.25, zmax=2.75, rDim=None, b_rDim=None, b_zDim=None,
                                 spectralIndexR=None, patchOffsetL=None, patchOffsetR=None)
    new = run.regrid(gp_new)
    assert new.t == run.t == 2 and new.n_outside == 0 and new.patch is gp_new
    assert np.isfinite(new.physical()).all()
    # a fresh run handed the same values takes its first step as Euler: the regridded run must agree bitwise
    fresh = S.ModelRun(dataclasses.replace(hip.mp, grid_params=gp_new), num_tiles=1, device="cuda")
    fresh.set_initial_conditions([new.tiles[0].var_np1])
    assert _bits(fresh.tiles[0].patchSpectral) == _bits(new.tiles[0].patchSpectral)
    for s in range(3):
        new.step()
        fresh.step()
        assert _bits(new.tiles[0].var_np1) == _bits(fresh.tiles[0].var_np1), "step %d after the regrid" % (s + 1)
    assert new.t == 5 and fresh.t == 3 and np.isfinite(new.tiles[0].var_np1).all()
    # attached parcels or statistics are not carried
    run.set_statistics([("max", [(1.0, 0, [("h", "")])])])
    with pytest.raises(ValueError, match="not carried"):
        run.regrid(gp_new)
    run.set_statistics([])
    fresh.close()
    new.close()
    run.close()


def test_recentre_brings_locate_to_the_axis():
    """recentre() on a shifted Gaussian depression: locate finds its centre, and in the re-centred run locate ends within the
    refinement's own tolerance of the new axis - the pole zone of 1e-6 DX (include/scythe_hip.h, sx_extremum_refine: where the
    refinement of a vortex centred on the pole ends).
    The case is one the grid can hold to that: (1) h has the conditions of a field that is regular at the pole (k = 0: R1T1, k >= 1:
    R1T0; with R0 the re-centred field is many-valued at r = 0 and the refinement finds no stationary point there); (2) the source's
    function is a piecewise cubic about ANOTHER axis, and the re-centred splines cannot hold the jumps of its third derivative (DX
    times the fourth derivative each): the minimum moves by c DX^3 f4 / f2 = 6 c (DX / s)^2 DX for a Gaussian of scale s, with c the
    spline-interpolation constant of order 0.01 to 0.1, so s = 400 DX keeps it below 4e-7 DX; (3) 24 cells, so that the step between
    the filled columns (one value per variable) and the field at the rim, which the spline solve carries inward at 0.27 per cell, is
    1e-13 at the axis.
    Measured on an MI355X: 1.9e-7 DX (status 3, the pole zone); with s = 200 DX 7.1e-7 DX, with s = 100 DX 2.6e-6 DX, with s = 2
    (5 DX) 1.4e-3 DX, and with 12 cells and s = 400 DX 1.8e-3 DX (the fill's step)."""
    import scythe_jl_amd as S
    case = cases.rlz_advection(num_cells=24, zDim=6)
    case["grid"].update(BCL={"h": "R1T0"}, BCL_k0={"h": "R1T1"})
    hip = cases.HipModel(case)
    run = hip.run
    DX = (hip.gp.xmax - hip.gp.xmin) / hip.gp.num_cells
    xc, yc, s = 1.1, 0.7, 400.0 * DX
    p = S.getGridpoints(run.tiles[0])
    x, y = p[:, 0] * np.cos(p[:, 1]), p[:, 0] * np.sin(p[:, 1])
    vals = np.stack([-np.exp(-((x - xc) ** 2 + (y - yc) ** 2) / s ** 2) * (1.0 + 0.1 * np.cos(0.4 * p[:, 2])), 0.3 + 0 * x, 0.2 + 0 * x], axis=1)
    run.set_initial_conditions([vals])
    loc = run.locate("h", "min")
    rec = run.recentre(var="h", want="min", outside="fill")
    assert rec.n_outside > 0 and rec.t == run.t and rec.patch is run.patch
    res = rec.locate("h", "min")
    print("centre located at r = %.6f (true %.6f) before; at r = %.3g DX, status %d, after" % (loc.pos[0], np.hypot(xc, yc), res.pos[0] / DX, res.status))
    assert abs(loc.pos[0] - np.hypot(xc, yc)) < 1e-2 * DX
    assert res.pos[0] <= 1e-6 * DX
    rec.close()
    run.close()
