"""sx_antiderivative on the GPU against the twin of tests/antiderivative.py (longdouble: the arbiter; float64: the yardstick of the bar).

Shapes: the smallest at which the kernels can still go wrong - one column (R), a long running sum (37 cells), b_zDim 6 (below one
matrix-core K block multiple) and 27 (crosses a 16-row tile and a K pad) with one block per z-mode (the lane kernel), ragged native
rings with both boundary-condition classes in one wave, and uniform rings with 8 blocks per z-mode (lane kernel), 16 (one matrix-core
column tile, 96 columns: a second, partly filled workgroup of the radial kernel) and 32 with b_zDim 27 (two column tiles, two row tiles
with the edge in the second, K padded from 27 to 28)."""
import functools

import numpy as np
import pytest

from tests import antiderivative as AD
from tests import elliptic as EL
from tests import linear_sw

pytestmark = pytest.mark.gpu

VARS = {"f": 1, "g": 2, "s": 3}           # the source, a bystander, a spare variable with the companion's conditions
SHAPES = {
    "R4": dict(geometry="R", num_cells=4),
    "R37": dict(geometry="R", num_cells=37),
    "RZ5_9": dict(geometry="RZ", num_cells=5, zDim=9),
    "RZ5_40": dict(geometry="RZ", num_cells=5, zDim=40),
    "RL6": dict(geometry="RL", num_cells=6),
    "RL16": dict(geometry="RL", num_cells=12, ring_uniform_L=16),
    "RLZ8": dict(geometry="RLZ", num_cells=4, zDim=9, ring_uniform_L=8),
    "RLZ16": dict(geometry="RLZ", num_cells=6, zDim=9, ring_uniform_L=16),
    "RLZ32": dict(geometry="RLZ", num_cells=6, zDim=40, ring_uniform_L=32),
}
# the source's conditions, also given to the spare variable "s": both axes then carry their columns / rows one to one into "s"
BCS = dict(bcl="R1T0", bcl_k0="R1T1", bcr="R0", bcb="R1T1", bct="R0")
CASES = [("r", "low", False), ("r", "low", True), ("r", "high", False), ("r", "high", True), ("z", "low", False), ("z", "high", False)]


def _params(name, **over):
    import scythe_jl_amd as S
    one = lambda key: {"f": BCS[key], "s": BCS[key]}
    kw = dict(xmin=0.0, xmax=9.0, vars=dict(VARS), BCL=one("bcl"), BCL_k0=one("bcl_k0"), BCR=one("bcr"))
    kw.update(SHAPES[name])
    if "Z" in kw["geometry"]:
        kw.update(zmin=0.0, zmax=3.0, BCB=one("bcb"), BCT=one("bct"))
    kw.update(over)
    return S.GridParameters(**kw)


def _kdim(gp):
    if "L" not in gp.geometry:
        return 0
    rings = 3 * gp.num_cells
    return min(rings, gp.ring_uniform_L // 2 - 1) if gp.ring_uniform_L else rings


def _cases(gp):
    return [c for c in CASES if c[0] == "r" or "Z" in gp.geometry]


def _twin(grid, a, case, xp):
    axis, origin, wr = case
    if axis == "r":
        return AD.apply_radial(grid, a, origin, wr, BCS["bcl_k0"], BCS["bcl"], BCS["bcr"], 2.0, xp)
    return AD.apply_vertical(grid, a, origin, BCS["bcb"], BCS["bct"], xp)


def _bound(grid, a, case):
    """[Zb, K2ref]: the derived bound of every column (tests/antiderivative.py)"""
    axis, origin, wr = case
    out = np.zeros(a.shape[:2])
    for zm in range(a.shape[0]):
        for blk in range(a.shape[1]):
            if axis == "r":
                out[zm, blk] = AD.radial_bound(grid, a[zm, blk], origin, wr, BCS["bcl_k0"] if blk == 0 else BCS["bcl"], BCS["bcr"])
    if axis == "z":             # [K2ref, nb]: a vertical column is [Zb] at fixed (block, row)
        return AD.vertical_bound(grid, a.reshape(a.shape[0], -1), origin, BCS["bcb"], BCS["bct"]).reshape(a.shape[1:])
    return out


@functools.lru_cache(maxsize=None)
def _random_case(name):
    """parameters, random source coefficients, and per case the two twins and the bar: computed once, shared, left unchanged"""
    gp = _params(name)
    grid = AD.grid_of(gp, _kdim(gp))
    s_patch = grid["Zb"] * (2 * grid["kDim"] + 1) * (gp.num_cells + 3)
    A = np.random.default_rng(31).standard_normal((s_patch, len(VARS)))
    a = EL.to_blocks(grid, A[:, 0])
    twins = {}
    for case in _cases(gp):
        truth, f64 = _twin(grid, a, case, True), _twin(grid, a, case, False)
        if case[0] == "z":
            # a vertical column is [Zb] at fixed (block, row): errors relative to that column's largest coefficient
            err = lambda x, truth=truth: AD.column_error(np.moveaxis(np.asarray(x), 0, -1), np.moveaxis(truth, 0, -1))       # [K2ref, nb]
            bar = 10.0 * err(f64) + _bound(grid, a, case)
        else:
            err = lambda x, truth=truth: AD.column_error(x, truth)                                                             # [Zb, K2ref]
            bar = 10.0 * err(f64) + _bound(grid, a, case)
        twins[case] = (truth, err, bar, float(err(f64).max()))
    return gp, grid, A, twins


def _companion(gp, axis):
    import scythe_jl_amd as S
    return S.companion_grid(gp, name="F", **BCS)


@pytest.mark.parametrize("name", list(SHAPES))
def test_parity(name):
    """each axis x origin x weight, per column against the longdouble twin: max error relative to the column's largest coefficient
    <= 10 x the float64 twin's on the same input + the derived bound"""
    import scythe_jl_amd as S
    gp, grid, A, twins = _random_case(name)
    tile = S.Grid(gp, None)
    assert AD.grid_of(tile.patch_params, int(tile.dims.kDim)) == grid
    tile.set_patch_spectral_a(A)
    comp = _companion(gp, "r")
    for case, (truth, err, bar, e64) in twins.items():
        axis, origin, wr = case
        out = tile.antiderivative("f", axis, origin, wr, dst=comp)
        assert out is comp
        got = EL.to_blocks(grid, comp.patchSpectral[:, 0])
        assert np.isfinite(got).all()
        e = err(got)
        print("%s %s: worst column: GPU %.2e, float64 twin %.2e; largest GPU / bar %.3f" % (name, case, e.max(), e64, (e / bar).max()))
        assert (e <= bar).all(), (case, e.max(), (e / bar).max())
        assert tile.kernel_bytes("k_antiderivative_" + axis) > 0
    comp.close()
    tile.close()


@pytest.mark.parametrize("name", ["R4", "RZ5_40", "RL6", "RLZ16", "RLZ32"])
def test_bitwise_properties(name):
    """two calls agree bitwise; the same-handle call into the spare variable gives the same bits and leaves every other variable's A and
    the whole state blob's other parts as they were"""
    import scythe_jl_amd as S
    gp, grid, A, twins = _random_case(name)
    tile = S.Grid(gp, None)
    tile.set_patch_spectral_a(A)
    comp = _companion(gp, "r")
    for axis, origin, wr in twins:
        state = tile.get_state().tobytes()
        tile.antiderivative("f", axis, origin, wr, dst=comp)
        assert tile.get_state().tobytes() == state               # src is read only
        first = comp.patchSpectral.copy()
        comp.set_patch_spectral_a(np.full_like(first, 7.0))      # a second call rewrites every entry
        tile.antiderivative("f", axis, origin, wr, dst=comp)
        assert comp.patchSpectral.tobytes() == first.tobytes()
        tile.antiderivative("f", axis, origin, wr, dst=tile, var_dst="s")
        after = tile.patchSpectral
        assert after[:, 2].tobytes() == first[:, 0].tobytes()
        assert after[:, :2].tobytes() == np.asfortranarray(A[:, :2]).tobytes()
    comp.close()
    tile.close()


@pytest.mark.parametrize("name", ["R37", "RZ5_40", "RLZ32"])
def test_fundamental_theorem(name):
    """evaluate of dst's r slot (z slot) at off-grid points against w f from evaluate of src at the same points: within 10 x the
    residual the longdouble twin's coefficients leave at those points (the projection's own truncation), measured here"""
    import scythe_jl_amd as S
    gp, grid, A, twins = _random_case(name)
    tile = S.Grid(gp, None)
    # a smooth source: the projection's residual is then far above rounding, and the bar means something
    smooth = np.zeros_like(A)
    a = np.zeros((grid["Zb"], 2 * grid["kDim"] + 1, gp.num_cells + 3))
    nodes = gp.xmin + (np.arange(gp.num_cells + 3) - 1) * (gp.xmax - gp.xmin) / gp.num_cells
    a[0, 0] = np.cos(0.4 * nodes)
    if grid["Zb"] > 2:
        a[2, 0] = 0.3 * np.sin(0.3 * nodes)
    smooth[:, 0] = a.reshape(-1)
    tile.set_patch_spectral_a(smooth)
    rng = np.random.default_rng(7)
    n = 40
    cols = [rng.uniform(gp.xmin + 0.2, gp.xmax - 0.2, n)] + ([rng.uniform(0, 2 * np.pi, n)] if "L" in gp.geometry else []) + \
           ([rng.uniform(0.1, 2.9, n)] if "Z" in gp.geometry else [])
    pts = np.stack(cols, axis=1)
    f = tile.evaluate(pts, all_k=True)[:, 0, 0]
    # the destination is left free (R0) along the axis of integration, as the companion of dst=None is: F does not vanish at an end
    comps = {"r": S.companion_grid(gp, name="F", bcl="R0", bcl_k0="R0", bcr="R0", bcb=BCS["bcb"], bct=BCS["bct"]),
             "z": S.companion_grid(gp, name="F", bcl=BCS["bcl"], bcl_k0=BCS["bcl_k0"], bcr=BCS["bcr"], bcb="R0", bct="R0")}
    names = {"R": ("u", "r", "rr"), "RZ": ("u", "r", "rr", "z", "zz"), "RLZ": ("u", "r", "rr", "l", "ll", "z", "zz")}[gp.geometry]
    for axis, origin, wr in _cases(gp):
        comp = comps[axis]
        tile.antiderivative("f", axis, origin, wr, dst=comp)
        dF = comp.evaluate(pts, all_k=True)[:, 0, names.index(axis)]
        want = (pts[:, 0] if wr else 1.0) * f * (1.0 if origin == "low" else -1.0)
        # the twin's residual for this input: its longdouble coefficients loaded into the companion and sampled by the same evaluate
        truth = (AD.apply_radial(grid, a, origin, wr, "R0", "R0", "R0", 2.0, True) if axis == "r" else _twin(grid, a, (axis, origin, wr), True)).astype(np.float64)
        comp.set_patch_spectral_a(truth.reshape(-1, 1))
        res = np.abs(comp.evaluate(pts, all_k=True)[:, 0, names.index(axis)] - want).max()
        e = np.abs(dF - want).max()
        print("%s %s: max |dF - w f| %.3e, the twin's residual %.3e" % (name, (axis, origin, wr), e, res))
        assert e <= 10.0 * res
    for g in (comps["r"], comps["z"], tile):
        g.close()


@pytest.mark.parametrize("name", ["RZ5_40", "RLZ16"])
def test_commutation(name):
    """radial-then-vertical and vertical-then-radial give the same A within the sum of the two bars; every variable involved carries
    the source's conditions (BCS), so both orders apply the same CA and the same classes"""
    import scythe_jl_amd as S
    gp, grid, A, twins = _random_case(name)
    tile = S.Grid(gp, None)
    tile.set_patch_spectral_a(A)
    c1, c2 = _companion(gp, "r"), _companion(gp, "r")
    tile.antiderivative("f", "r", "low", True, dst=c1)
    c1.antiderivative("F", "z", "low", dst=tile, var_dst="s")
    rz = EL.to_blocks(grid, tile.patchSpectral[:, 2]).copy()
    tile.antiderivative("f", "z", "low", dst=c2)
    c2.antiderivative("F", "r", "low", True, dst=tile, var_dst="s")
    zr = EL.to_blocks(grid, tile.patchSpectral[:, 2])
    a = EL.to_blocks(grid, A[:, 0])
    truth = _twin(grid, _twin(grid, a, ("r", "low", True), True), ("z", "low", False), True)
    sc = np.abs(truth).max()
    bar = (twins[("r", "low", True)][2].max() + twins[("z", "low", False)][2].max()) * 2.0
    e = float(np.abs(rz - zr).max() / sc)
    print("%s: max |rz - zr| / max |F| %.3e, bar %.3e" % (name, e, bar))
    assert e <= bar
    for g in (c1, c2, tile):
        g.close()


def test_refusals():
    """every refusal that needs a handle; dst's A is what it was afterwards"""
    import scythe_jl_amd as S
    lib = S.load()
    base = lambda name="RLZ8", **over: _params(name, **dict(dict(num_cells=8), **over))      # 8 cells: a PERIODIC companion can be built at all
    gp = base()
    tile = S.Grid(gp, None)
    tile.set_patch_spectral_a(np.random.default_rng(3).standard_normal((int(tile.dims.s_patch), 3)))
    comp = _companion(gp, "r")
    comp.set_patch_spectral_a(np.full((int(comp.dims.s_patch), 1), 3.0))
    keep_comp, keep_tile = comp.patchSpectral.tobytes(), tile.patchSpectral.tobytes()

    def refused(match, src, dst, var="f", axis="r", weight_r=False, var_dst=1):
        keep = dst.patchSpectral.tobytes()
        with pytest.raises(S.ScytheHipError, match=match):
            src.antiderivative(var, axis, "low", weight_r, dst=dst, var_dst=var_dst)
        assert dst.patchSpectral.tobytes() == keep and comp.patchSpectral.tobytes() == keep_comp and tile.patchSpectral.tobytes() == keep_tile

    def raw(vs, axis, origin, weight, dst, vd, src=tile):
        rc = lib.sx_antiderivative(src._h if src is not None else None, vs, axis, origin, weight, dst._h if dst is not None else None, vd)
        assert rc != 0 and comp.patchSpectral.tobytes() == keep_comp and tile.patchSpectral.tobytes() == keep_tile
        return lib.sx_last_error().decode()

    assert "null handle" in raw(1, 0, 0, 0, None, 1) and "null handle" in raw(1, 0, 0, 0, comp, 1, src=None)
    assert "axis" in raw(1, 2, 0, 0, comp, 1) and "origin" in raw(1, 0, 2, 0, comp, 1) and "weight" in raw(1, 0, 0, 2, comp, 1)
    for vs, vd in ((0, 1), (4, 1), (1, 0), (1, 2)):
        assert "out of range" in raw(vs, 0, 0, 0, comp, vd)
    refused("destination variable is the source", tile, tile, "s", var_dst="s")
    refused("takes no weight", tile, comp, axis="z", weight_r=True)
    part = S.Grid(gp, None, 0, 3)
    refused("one-tile", part, comp)
    refused("one-tile", tile, part, var_dst="s")
    for over in (dict(geometry="RZ", ring_uniform_L=0), dict(xmin=0.5), dict(xmax=9.5), dict(num_cells=9), dict(ring_uniform_L=16), dict(ring_uniform_L=0),
                 dict(zDim=10, b_zDim=6), dict(b_zDim=5), dict(zmin=0.5), dict(zmax=3.5)):
        other = S.companion_grid(base(**over), name="F", **BCS)
        refused("grid differs", tile, other)
        other.close()
    rl = S.Grid(_params("RL16"), None)
    rlc = S.companion_grid(_params("RL16"), name="F", bcl=BCS["bcl"], bcl_k0=BCS["bcl_k0"], bcr=BCS["bcr"])
    with pytest.raises(S.ScytheHipError, match="RZ or RLZ"):
        rl.antiderivative("f", "z", dst=rlc)
    for bcs, axis, match in ((dict(BCS, bcl="PERIODIC", bcl_k0="PERIODIC", bcr="PERIODIC"), "r", "PERIODIC"), (dict(BCS, bcb="R0"), "r", "vertical boundary conditions differ"),
                             (dict(BCS, bct="R1T0"), "r", "vertical boundary conditions differ"), (dict(BCS, bcl="R0"), "z", "radial boundary conditions differ"),
                             (dict(BCS, bcl_k0="R0"), "z", "radial boundary conditions differ"), (dict(BCS, bcr="R1T0"), "z", "radial boundary conditions differ")):
        other = S.companion_grid(gp, name="F", **bcs)
        refused(match, tile, other, axis=axis)
        other.close()
    tile.antiderivative("f", "z", "high", dst=comp)             # after all that a good call still works
    assert comp.patchSpectral.tobytes() != keep_comp and np.isfinite(comp.patchSpectral).all()
    for g in (rl, rlc, part, comp, tile):
        g.close()


def test_inside_radius_against_the_domain_integral():
    """ModelRun.inside_radius at xmax times 2 pi is sx_reduce's integral of the same field over the disc (LinearShallowWaterRL, uniform 16,
    12 cells): the bar is 10 x the difference the float64 twin finds between the two from the same A, plus the rounding of the reduce
    (its points x eps); column_integral has no vertical to integrate on this grid and says so"""
    import scythe_jl_amd as S
    from tests import cases
    case = linear_sw.rl_case(num_cells=12, ring_L=16)
    gp, mp = cases.hip_params(case)
    run = S.ModelRun(mp, num_tiles=1, device="cuda")
    pts = S.getGridpoints(run.tiles[0])
    run.set_initial_conditions([case["ic"](pts)])
    for _ in range(2):
        run.step()
    tile = run.tiles[0]
    grid = AD.grid_of(gp, int(tile.dims.kDim))
    for v, name in enumerate(gp.var_names()):
        total = run.integrate([(0, 1.0, 0, [(name, "")])])[0]
        r, val = run.inside_radius(name, [gp.xmax])
        got = 2.0 * np.pi * val[0]
        # the float64 twin on the same input: F(xmax) of the k = 0 column from the A the device holds
        a = EL.to_blocks(grid, tile.patchSpectral[:, v])
        F = AD.radial(grid, a[0, 0], "low", True, "R0", "R0", gp.l_q, False)
        twin = 2.0 * np.pi * float(EL.basis(grid, np.array([gp.xmax]), 0, False)[0] @ F)
        scale = np.abs(run.integrate([(0, 1.0, 0, [(name, ""), (name, "")])])[0]) ** 0.5 * (np.pi * gp.xmax ** 2) ** 0.5
        bar = 10.0 * abs(twin - total) + len(pts) * np.finfo(float).eps * scale
        print("%s: 2 pi F(xmax) %.12e, integrate %.12e, float64 twin %.12e, bar %.3e" % (name, got, total, twin, bar))
        assert abs(got - total) <= bar
    with pytest.raises(S.ScytheHipError, match="RZ or RLZ"):
        run.column_integral(gp.var_names()[0])
    for g in run.tiles:
        g.close()


def test_column_integral_against_the_domain_integral():
    """ModelRun.column_integral (F(zmax) per column) times the radial quadrature against sx_reduce's integral over the domain
    (LinearAdvectionRZ).  The two differ by what F loses when its series is cut to b_zDim coefficients; the bar is 10 x the difference
    the float64 twin finds between the two from the same A, plus rounding (points x eps x the field's scale)"""
    import scythe_jl_amd as S
    from tests import cases
    case = cases.rz_advection()
    gp, mp = cases.hip_params(case)
    run = S.ModelRun(mp, num_tiles=1, device="cuda")
    pts = S.getGridpoints(run.tiles[0])
    run.set_initial_conditions([case["ic"](pts)])
    run.step()
    name = gp.var_names()[0]
    total = run.integrate([(0, 1.0, 0, [(name, "")])])[0]
    cols, val = run.column_integral(name)
    w_r, _, _ = S.reduce_weights(gp)
    got = float(np.dot(w_r, val))
    scale = np.abs(run.physical()[:, 0, 0]).max() * (gp.xmax - gp.xmin) * (gp.zmax - gp.zmin)
    # the float64 twin on the same input: F's truncated coefficients per node row, their series at the top (x = -1: T_k = (-1)^k, DCT-I
    # normalisation, free ends), the spline at the rings' radii, the same radial weights
    tile = run.tiles[0]
    grid = AD.grid_of(gp, 0)
    a = EL.to_blocks(grid, tile.patchSpectral[:, 0])[:, 0, :]
    bF = AD.vertical(grid, a, "low", "R0", "R0", False)
    k = np.arange(grid["Zb"])
    top = (np.where(k == 0, 1.0, 2.0) * (-1.0) ** k) @ bF
    twin = float(np.dot(w_r, EL.basis(grid, cols[:, 0], 0, False) @ top))
    bar = 10.0 * abs(twin - total) + len(pts) * np.finfo(float).eps * scale
    print("column_integral . w_r %.12e, integrate %.12e, float64 twin %.12e, bar %.3e" % (got, total, twin, bar))
    assert abs(got - total) <= bar
    for g in run.tiles:
        g.close()
