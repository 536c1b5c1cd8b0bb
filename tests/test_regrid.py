"""sx_regrid's host side without a device: sx_regrid_columns against the column map written from its definition in longdouble, every
refusal of sx_regrid_check by message, and the pins of the numpy twin (tests/regrid.py): u = x and u = r^2 re-centred."""
import numpy as np
import pytest

from tests import project as PJ
from tests import regrid as RG

XP = RG.XP
U = 2.0 ** -52          # one ulp of a number in [1, 2)

VARS = {"h": 1, "u": 2, "v": 3}
SRC_Z = dict(zmin=0.0, zmax=3.0, zDim=10, BCB={"u": "R1T0", "v": "R1T1"}, BCT={"u": "R1T0"})
DST_Z = dict(zmin=0.5, zmax=2.5, zDim=12, BCB={"h": "R1T0"}, BCT={"v": "R1T1"})
# the shapes of tests/test_gpu_regrid.py
PAIRS = {
    "RLZ": (dict(geometry="RLZ", xmin=0.0, xmax=6.0, num_cells=6, vars=VARS, **SRC_Z), dict(geometry="RLZ", xmin=0.0, xmax=4.5, num_cells=9, vars=VARS, **DST_Z)),
    "RL": (dict(geometry="RL", xmin=0.0, xmax=6.0, num_cells=6, vars=VARS), dict(geometry="RL", xmin=0.0, xmax=3.0, num_cells=4, vars=VARS)),
    "RZ": (dict(geometry="RZ", xmin=0.0, xmax=5.0, num_cells=5, vars=VARS, **SRC_Z), dict(geometry="RZ", xmin=0.5, xmax=4.5, num_cells=8, vars=VARS, **DST_Z)),
    "R": (dict(geometry="R", xmin=0.0, xmax=5.0, num_cells=5, vars=VARS), dict(geometry="R", xmin=0.5, xmax=4.5, num_cells=8, vars=VARS)),
}
OFFSET = (0.3, -0.2)    # a fraction of DX = 1: dst (r <= 4.5 / 3) stays inside src (r_s <= 4.5 + 0.37 / 3.37 < 6)


def test_symbols():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    for name in ("sx_regrid", "sx_regrid_check", "sx_regrid_columns"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert L.REGRID_OUTSIDE == {"refuse": 0, "fill": 1}


@pytest.mark.parametrize("shape", ["RLZ", "RL"])
@pytest.mark.parametrize("centre", [OFFSET, (-0.45, 0.15), (1.25, 0.0)])
def test_columns_against_the_longdouble_map(shape, centre):
    """r_s within a relative 4 ulp, lambda_s within an absolute 4 ulp pi: hypot and atan2 are within 1 ulp each, with one rounding each
    in x and y"""
    import scythe_jl_amd as S
    (gs, os_), (gd, od) = (RG.oracle_pair(s) for s in PAIRS[shape])
    cols, ins = S.regrid_columns(gs, gd, centre)
    want = RG.column_map(od, centre)
    assert cols.shape == want.shape == (int(np.sum(od.L)), 2)
    dr = np.abs(cols[:, 0].astype(XP) - want[:, 0]) / want[:, 0]
    dl = np.abs(cols[:, 1].astype(XP) - want[:, 1])
    dl = np.minimum(dl, np.abs(dl - 2 * RG.O.PI_X))          # a column on the branch cut may come out at either end
    print("%s %s: r_s off by %.3g ulp, lambda_s by %.3g ulp pi" % (shape, centre, float(dr.max()) / U, float(dl.max()) / (U * np.pi)))
    assert float(dr.max()) <= 4 * U
    assert float(dl.max()) <= 4 * U * np.pi
    assert (ins == RG.inside(os_, cols[:, 0])).all() and ins.all()


@pytest.mark.parametrize("shape", list(PAIRS))
def test_identity_map_returns_the_gridpoints_bitwise(shape):
    import scythe_jl_amd as S
    (gs, os_), (gd, od) = (RG.oracle_pair(s) for s in PAIRS[shape])
    q, _ = RG.dst_columns(od)
    for centre in (None,) + (((0.0, 0.0), (-0.0, 0.0)) if od.has_l else ()):
        cols, ins = S.regrid_columns(gs, gd, centre)
        assert cols.shape == q.shape
        assert np.ascontiguousarray(cols.T).tobytes() == np.ascontiguousarray(q.T).tobytes(), (shape, centre)
        assert ins.all()


def test_inside_with_a_column_exactly_on_xmax():
    """dst's last ring radius, taken as src's xmax: that ring is inside (the ends count), and one ulp less of xmax puts it outside"""
    import scythe_jl_amd as S
    spec_s, spec_d = (dict(s) for s in PAIRS["RL"])
    gd, od = RG.oracle_pair(spec_d)
    r_last = float(RG.dst_columns(od)[0][-1, 0])
    for xmax, n_out in ((r_last, 0), (np.nextafter(r_last, 0.0), int(od.L[-1]))):
        spec_s["xmax"] = float(xmax)
        gs, os_ = RG.oracle_pair(spec_s)
        cols, ins = S.regrid_columns(gs, gd, None)
        assert (ins == RG.inside(os_, cols[:, 0])).all()
        assert int((~ins).sum()) == n_out and ins[:len(ins) - int(od.L[-1])].all()
    # about an offset centre the twin's rule on the returned doubles decides, column by column
    spec_s["xmax"] = 3.0
    gs, os_ = RG.oracle_pair(spec_s)
    cols, ins = S.regrid_columns(gs, gd, (0.4, 0.1))
    assert (ins == RG.inside(os_, cols[:, 0])).all() and 0 < int((~ins).sum()) < len(ins)


def test_check_refusals_without_a_device():
    import ctypes as C
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    from scythe_jl_amd.model import grid_desc
    P = {k: tuple(RG.oracle_pair(s)[0] for s in v) for k, v in PAIRS.items()}
    gs, gd = P["RLZ"]
    assert S.regrid_check(gs, gd) is None and S.regrid_check(gs, gd, OFFSET, ["h", "h", 3], "fill") is None
    for k in PAIRS:
        assert S.regrid_check(*P[k]) is None
    # one-tile patches
    lib = S.load()
    ds, k1 = grid_desc(gs, 0, 3)
    dd, k2 = grid_desc(gd)
    vs = (C.c_int32 * 3)(1, 2, 3)
    for a, b in ((ds, dd), (dd, ds)):
        assert lib.sx_regrid_check(C.byref(a), C.byref(b), None, vs, 0) == 1
        assert "one-tile" in lib.sx_last_error().decode()
    assert lib.sx_regrid_check(None, C.byref(dd), None, vs, 0) == 1 and "null" in lib.sx_last_error().decode()
    dd, k2 = grid_desc(gd)
    ds, k1 = grid_desc(gs)
    assert lib.sx_regrid_check(C.byref(ds), C.byref(dd), None, None, 0) == 1 and "null var_src" in lib.sx_last_error().decode()
    # geometry
    for a, b in (("RLZ", "RL"), ("RZ", "R"), ("RL", "R"), ("RZ", "RLZ")):
        with pytest.raises(S.ScytheHipError, match="geometries differ"):
            S.regrid_check(P[a][0], P[b][1])
    # the centre
    for k in ("R", "RZ"):
        with pytest.raises(S.ScytheHipError, match="RL / RLZ grids only"):
            S.regrid_check(*P[k], centre=(0.0, 0.0))
    for c in ((np.nan, 0.0), (0.0, np.inf)):
        with pytest.raises(S.ScytheHipError, match="centre is NaN or Inf"):
            S.regrid_check(gs, gd, c)
    # the variables
    for v in ([0, 1, 2], [1, 2, 4], [1, -1, 2]):
        with pytest.raises(S.ScytheHipError, match="not a variable of the source"):
            S.regrid_check(gs, gd, variables=v)
    with pytest.raises(S.ScytheHipError, match="SX_REGRID_REFUSE or SX_REGRID_FILL"):
        S.regrid_check(gs, gd, outside=2)
    # more than 2^20 columns: 90 cells of 4096-point rings
    big = RG.oracle_pair(dict(PAIRS["RL"][1], num_cells=90, ring_L=4096))[0]
    with pytest.raises(S.ScytheHipError, match="at most 1048576"):
        S.regrid_check(P["RL"][0], big)
    # the vertical extent, at either end
    for kw in (dict(zmin=-0.25), dict(zmax=3.5)):
        with pytest.raises(S.ScytheHipError, match="does not lie within"):
            S.regrid_check(gs, RG.oracle_pair(dict(PAIRS["RLZ"][1], **kw))[0])
    with pytest.raises(S.ScytheHipError, match="invalid vertical grid"):
        S.regrid_check(gs, RG.oracle_pair(dict(PAIRS["RLZ"][1], zDim=3))[0])
    # the tables of one column batch (tests/test_isosurface.py): native rings of 62 source cells reach kDim 186
    with pytest.raises(S.ScytheHipError, match=r"32 \(kDim \+ 1\) \+ 2304 <= 8192"):
        S.regrid_check(RG.oracle_pair(dict(PAIRS["RLZ"][0], num_cells=62))[0], gd)
    assert S.regrid_check(RG.oracle_pair(dict(PAIRS["RLZ"][0], num_cells=61))[0], gd) is None
    # a column outside: refused with SX_REGRID_REFUSE, accepted with SX_REGRID_FILL
    with pytest.raises(S.ScytheHipError, match=r"outside the source's \[xmin, xmax\]"):
        S.regrid_check(gs, gd, (2.5, 0.0))
    assert S.regrid_check(gs, gd, (2.5, 0.0), outside="fill") is None
    with pytest.raises(ValueError):
        S.regrid_check(gs, RG.oracle_pair(dict(PAIRS["RLZ"][1], vars={"h": 1, "q": 2}))[0])      # no variable q in the source


def _pin(field, closed, centre):
    """|twin - closed form| / bound over dst's gridpoints: the source holds `field` (an R0 / R0 variable of an RL grid) as the
    longdouble projection of its gridpoint values, the twin sums it at the columns sx_regrid_columns returns"""
    import scythe_jl_amd as S
    spec_s, spec_d = (dict(s, vars={"u": 1}) for s in PAIRS["RL"])
    (gs, os_), (gd, od) = RG.oracle_pair(spec_s), RG.oracle_pair(spec_d)
    p = os_.gridpoints()
    A = PJ.project_xp(os_, field(p[:, 0], p[:, 1])[:, None])
    cols, ins = S.regrid_columns(gs, gd, centre)
    assert ins.all()
    got = RG.values(os_, A, [1], cols, ins, np.zeros(1), xp=True)[:, 0]
    bound = RG.value_bound(os_, A, [1], cols, ins, np.zeros(1))[:, 0]
    q, _ = RG.dst_columns(od)
    want = closed(q[:, 0].astype(XP), q[:, 1].astype(XP), XP(centre[0]), XP(centre[1]))
    # the closed form is exact about the exact centre; the columns are the float64 map's: 4 ulp of r_s and of lambda_s move u = x
    # and u = r^2 by at most 4 ulp (|du/dr| + |du/dlambda|) = 4 ulp (r_s + 2 r_s^2), which is added to the twin's bound
    slack = 4 * U * (cols[:, 0] + 2 * cols[:, 0] ** 2)
    ratio = np.abs(got - want) / (bound + slack)
    return float(ratio.max())


@pytest.mark.parametrize("centre", [OFFSET, (-0.45, 0.15)])
def test_twin_pins_recentred_closed_forms(centre):
    """u = x becomes x0 + r' cos l', u = r^2 becomes r'^2 + 2 r' (x0 cos l' + y0 sin l') + x0^2 + y0^2 at dst's gridpoints (r', l'):
    both lie in the source's spline and Fourier space (tests/project.py), so the twin reproduces them to its own bound"""
    rx = _pin(lambda r, l: r * np.cos(l), lambda r, l, x0, y0: x0 + r * np.cos(l), centre)
    r2 = _pin(lambda r, l: r * r, lambda r, l, x0, y0: r * r + 2 * r * (x0 * np.cos(l) + y0 * np.sin(l)) + x0 * x0 + y0 * y0, centre)
    print("centre %s: u = x at %.3g of the bound, u = r^2 at %.3g" % (centre, rx, r2))
    assert rx <= 1.0 and r2 <= 1.0
