"""sx_elliptic_solve on the GPU against the dense twin of tests/elliptic.py (longdouble: the arbiter; float64: the yardstick of the bar).

Shapes: the smallest at which the kernel can still go wrong - 4 cells (7 patch rows: the 7-row window never fills), 5 and 37 cells, column
counts of 1, 6, 16, 38 and 48 (the tail guard of the one workgroup), 64 (uniform L = 64: exactly one full workgroup) and 96 (RLZ16: a
second, partly filled workgroup), k = 0 and k >= 1 classes with different ranks in one wave, b_zDim 6."""
import functools

import numpy as np
import pytest

from tests import elliptic as EL
from tests import linear_sw

pytestmark = pytest.mark.gpu

VARS = {"u": 1, "v": 2, "f": 3, "s": 4}           # two wind components, a scalar, a spare variable with the companion's conditions
SHAPES = {
    "R4": dict(geometry="R", num_cells=4),
    "R37": dict(geometry="R", num_cells=37),
    "RZ5": dict(geometry="RZ", num_cells=5, zDim=8),
    "RL6": dict(geometry="RL", num_cells=6),
    "RL16": dict(geometry="RL", num_cells=12, ring_uniform_L=16),
    "RLZ8": dict(geometry="RLZ", num_cells=5, zDim=8, ring_uniform_L=8),
    "RL64": dict(geometry="RL", num_cells=40, ring_uniform_L=64),
    "RLZ16": dict(geometry="RLZ", num_cells=5, zDim=8, ring_uniform_L=16),
}
BCS = dict(bcl="R1T0", bcl_k0="R1T1", bcr="R1T0")      # companion_grid's defaults, also given to the spare variable "s"


def _params(name, **over):
    import scythe_jl_amd as S
    kw = dict(xmin=0.0, xmax=9.0, vars=dict(VARS), BCL={"s": BCS["bcl"]}, BCL_k0={"s": BCS["bcl_k0"]}, BCR={"s": BCS["bcr"]})
    kw.update(SHAPES[name])
    if "Z" in kw["geometry"]:
        kw.update(zmin=0.0, zmax=3.0)
    kw.update(over)
    return S.GridParameters(**kw)


def _twin_grid(tile):
    return EL.grid_of(tile.patch_params, int(tile.dims.kDim))


def _kinds(gp):
    return ("field", "vorticity", "divergence") if "L" in gp.geometry else ("field",)


def _rhs(kind):
    return ("field", "f") if kind == "field" else (kind, "u", "v")


ALPHA = {"field": 0.37, "vorticity": 0.0, "divergence": 0.37}


@functools.lru_cache(maxsize=None)
def _random_case(name):
    """parameters, random source coefficients and the two twins per rhs kind: computed once, shared, left unchanged"""
    import scythe_jl_amd as S
    gp = _params(name)
    kDim = 0
    if "L" in gp.geometry:
        rings = 3 * gp.num_cells
        kDim = min(rings, gp.ring_uniform_L // 2 - 1) if gp.ring_uniform_L else rings
    grid = EL.grid_of(gp, kDim)
    s_patch = grid["Zb"] * (2 * kDim + 1) * (gp.num_cells + 3)
    A = np.random.default_rng(29).standard_normal((s_patch, len(VARS)))
    twins = {}
    for kind in _kinds(gp):
        a, b = (A[:, 2], None) if kind == "field" else (A[:, 0], A[:, 1])
        blk = lambda x: None if x is None else EL.to_blocks(grid, x)
        twins[kind] = tuple(EL.invert(grid, kind, blk(a), blk(b), ALPHA[kind], BCS["bcl_k0"], BCS["bcl"], BCS["bcr"], xp) for xp in (True, False))
    return gp, grid, A, twins


@pytest.mark.parametrize("name", list(SHAPES))
def test_parity(name):
    """per wavenumber: error against the longdouble twin <= 10 x the float64 twin's error on the same input (max norm, relative to the
    column's largest coefficient)"""
    import scythe_jl_amd as S
    gp, grid, A, twins = _random_case(name)
    tile = S.Grid(gp, None)
    assert _twin_grid(tile) == grid
    tile.set_patch_spectral_a(A)
    comp = S.companion_grid(gp, **BCS)
    for kind in _kinds(gp):
        truth, f64 = twins[kind]
        out = tile.invert(_rhs(kind), ALPHA[kind], into=comp)
        assert out is comp
        got = EL.to_blocks(grid, comp.patchSpectral[:, 0])
        assert np.isfinite(got).all()
        e_new, e_f64 = EL.per_k_error(grid, got, truth), EL.per_k_error(grid, f64, truth)
        print("%s %s alpha=%g: worst over k: GPU %.2e, float64 twin %.2e; largest GPU / (10 x float64 twin) %.3f at k = %d"
              % (name, kind, ALPHA[kind], e_new.max(), e_f64.max(), (e_new / (10 * e_f64)).max(), int(np.argmax(e_new / (10 * e_f64)))))
        assert (e_new <= 10.0 * e_f64).all(), (kind, e_new, e_f64)
        assert tile.kernel_bytes("k_elliptic") > 0
    # the cached companion of into=None carries the same conditions: the same bits
    auto = tile.invert(_rhs("field"), ALPHA["field"])
    tile.invert(_rhs("field"), ALPHA["field"], into=comp)
    assert auto is not comp and auto.patchSpectral.tobytes() == comp.patchSpectral.tobytes()
    comp.close()
    tile.close()


@pytest.mark.parametrize("name", ["R4", "RZ5", "RL6", "RL64", "RLZ16"])
def test_bitwise_properties(name):
    import scythe_jl_amd as S
    gp, grid, A, twins = _random_case(name)
    tile = S.Grid(gp, None)
    tile.set_patch_spectral_a(A)
    comp = S.companion_grid(gp, **BCS)
    for kind in _kinds(gp):
        tile.invert(_rhs(kind), ALPHA[kind], into=comp)
        first = comp.patchSpectral.copy()
        comp.set_patch_spectral_a(np.full_like(first, 7.0))             # a second call rewrites every entry
        tile.invert(_rhs(kind), ALPHA[kind], into=comp)
        assert comp.patchSpectral.tobytes() == first.tobytes()
        # the same-handle solve into the spare variable: the same bits, and the other variables' A as they were
        tile.invert(_rhs(kind), ALPHA[kind], into=tile, var="s")
        after = tile.patchSpectral
        assert after[:, 3].tobytes() == first[:, 0].tobytes()
        assert after[:, :3].tobytes() == np.asfortranarray(A[:, :3]).tobytes()
    comp.close()
    tile.close()


def _lsw_run(ring_L=16, num_cells=12):
    import scythe_jl_amd as S
    from tests import cases
    case = linear_sw.rl_case(num_cells=num_cells, ring_L=ring_L)
    gp, mp = cases.hip_params(case)
    run = S.ModelRun(mp, num_tiles=1, device="cuda")
    pts = S.getGridpoints(run.tiles[0])
    run.set_initial_conditions([case["ic"](pts)])
    return run, gp


def test_nothing_else_moves():
    """the model state of both handles is bitwise what it was, and the next step gives what it gives without the call"""
    import scythe_jl_amd as S
    run, gp = _lsw_run()
    ref, _ = _lsw_run()
    for r in (run, ref):
        for _ in range(3):
            r.step()
    tile = run.tiles[0]
    tile.set_parcels(np.array([[2.0, 0.3], [5.5, 4.0]]), ("u", "v"))
    tile.advance_parcels(0.01)
    tile.tileTransform_()
    comp = S.companion_grid(gp)
    comp.set_physical_values(np.linspace(0.0, 1.0, comp.N)[:, None])
    snap = lambda g: (g.get_state().tobytes(), g.physical.tobytes(), g.var_np1.tobytes(), g.patchSpectral.tobytes(), g.spectral.tobytes(),
                      tuple(x.tobytes() for x in g.parcels()))
    before_src, before_dst = snap(tile), snap(comp)
    psi = run.streamfunction(into=comp)
    chi = run.velocity_potential()
    assert psi is comp and chi is not comp
    assert snap(tile) == before_src
    after_dst = snap(comp)
    assert after_dst[1:3] == before_dst[1:3] and after_dst[4:] == before_dst[4:]       # all but its A (and the state blob that holds it)
    assert after_dst[3] != before_dst[3]
    tile.set_parcels(np.zeros((0, 2)), ("u", "v"))
    for r in (run, ref):
        r.step()
    assert run.tiles[0].patchSpectral.tobytes() == ref.tiles[0].patchSpectral.tobytes()
    assert run.tiles[0].var_np1.tobytes() == ref.tiles[0].var_np1.tobytes()
    assert run.physical().tobytes() == ref.physical().tobytes()
    comp.close()
    for r in (run, ref):
        for g in r.tiles:
            g.close()


def test_refusals():
    """every refusal of the issue's list that needs a handle; dst's A is what it was afterwards"""
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    gp = _params("RL16")
    tile = S.Grid(gp, None)
    A = np.random.default_rng(3).standard_normal((int(tile.dims.s_patch), 4))
    tile.set_patch_spectral_a(A)
    comp = S.companion_grid(gp, **BCS)
    comp.set_patch_spectral_a(np.full((int(comp.dims.s_patch), 1), 3.0))
    keep_comp, keep_tile = comp.patchSpectral.tobytes(), tile.patchSpectral.tobytes()

    def refused(match, src, rhs, into, var=1, alpha=0.0):
        keep_into = into.patchSpectral.tobytes()
        with pytest.raises(S.ScytheHipError, match=match):
            src.invert(rhs, alpha, into=into, var=var)
        assert into.patchSpectral.tobytes() == keep_into
        assert comp.patchSpectral.tobytes() == keep_comp and tile.patchSpectral.tobytes() == keep_tile

    def raw(kind, va, vb, alpha, dst, vd, src=tile):
        rc = lib.sx_elliptic_solve(src._h if src is not None else None, kind, va, vb, alpha, dst._h if dst is not None else None, vd)
        assert rc != 0
        assert comp.patchSpectral.tobytes() == keep_comp and tile.patchSpectral.tobytes() == keep_tile
        return lib.sx_last_error().decode()

    assert "null handle" in raw(0, 3, 0, 0.0, None, 1) and "null handle" in raw(0, 3, 0, 0.0, comp, 1, src=None)
    assert "rhs_kind" in raw(3, 1, 2, 0.0, comp, 1) and "rhs_kind" in raw(-1, 1, 2, 0.0, comp, 1)
    for va, vb, vd in ((0, 2, 1), (5, 2, 1), (1, 0, 1), (1, 5, 1), (1, 2, 0), (1, 2, 2)):
        assert "out of range" in raw(1, va, vb, 0.0, comp, vd)
    assert "out of range" in raw(0, 5, 0, 0.0, comp, 1)
    refused("destination variable is a source", tile, ("vorticity", "u", "v"), tile, "u")
    refused("destination variable is a source", tile, ("divergence", "u", "s"), tile, "s")
    refused("destination variable is a source", tile, ("field", "s"), tile, "s")
    for alpha in (-1.0, float("nan"), float("inf")):
        refused("alpha must be finite", tile, ("field", "f"), comp, 1, alpha)
    # vorticity / divergence on a grid without an azimuth
    rgp = _params("R37")
    rt, rc = S.Grid(rgp, None), S.companion_grid(rgp, **BCS)
    for kind in ("vorticity", "divergence"):
        with pytest.raises(S.ScytheHipError, match="RL or RLZ"):
            rt.invert((kind, "u", "v"), 0.0, into=rc)
    # one-tile patches only, on either side
    part = S.Grid(gp, None, 0, 6)
    refused("one-tile", part, ("field", "f"), comp)
    refused("one-tile", tile, ("field", "f"), part, "s")
    # a destination on another grid: geometry, xmin, xmax, num_cells, ring table (and with it kDim), zDim, b_zDim, zmin, zmax
    others = [rgp, _params("RL16", xmin=0.5), _params("RL16", xmax=9.5), _params("RL16", num_cells=13), _params("RL16", ring_uniform_L=32),
              _params("RL16", ring_uniform_L=0)]
    for ogp in others:
        other = S.companion_grid(ogp, **BCS)
        refused("grid differs", tile, ("field", "f"), other)
        other.close()
    zgp = _params("RLZ8")
    zt = S.Grid(zgp, None)
    for over in (dict(zDim=9, b_zDim=6), dict(b_zDim=5), dict(zmin=0.5), dict(zmax=3.5)):
        other = S.companion_grid(_params("RLZ8", **over), **BCS)
        with pytest.raises(S.ScytheHipError, match="grid differs"):
            zt.invert(("field", "f"), 0.37, into=other)
        other.close()
    # a source variable whose vertical conditions differ from the destination's
    other = S.companion_grid(zgp, bcb="R1T0", **BCS)
    with pytest.raises(S.ScytheHipError, match="vertical boundary conditions"):
        zt.invert(("field", "f"), 0.37, into=other)
    other.close()
    zt.close()
    # the destination variable's radial conditions: PERIODIC, singular, not zero at the centre
    for bcs, match in ((dict(bcl="PERIODIC", bcl_k0="PERIODIC", bcr="PERIODIC"), "PERIODIC"),
                       (dict(bcl="R1T0", bcl_k0="R1T1", bcr="R1T1"), "singular"), (dict(bcl="R1T1", bcl_k0="R1T1", bcr="R1T0"), "vanish at r = 0")):
        other = S.companion_grid(gp, **bcs)
        refused(match, tile, ("field", "f"), other)
        other.close()
    # after all that a good call still works
    tile.invert(("vorticity", "u", "v"), 0.0, into=comp)
    assert comp.patchSpectral.tobytes() != keep_comp and np.isfinite(comp.patchSpectral).all()
    for g in (rt, rc, part, comp, tile):
        g.close()


def test_end_to_end_streamfunction():
    """u = -psi0_lambda / r, v = psi0_r of psi0 = J_2(kappa r) cos 2 lambda, kappa R a zero of J_2: streamfunction() returns psi0 to within
    2 x the error the float64 twin makes from the same wind coefficients, and the velocity potential of this non-divergent wind stays
    below that error."""
    import scythe_jl_amd as S
    from scipy.special import jn_zeros, jv, jvp
    run, gp = _lsw_run()
    tile = run.tiles[0]
    pts = S.getGridpoints(tile)
    r, lam = pts[:, 0], pts[:, 1]
    kap = jn_zeros(2, 1)[0] / gp.xmax
    psi0 = jv(2, kap * r) * np.cos(2 * lam)
    u = 2.0 * jv(2, kap * r) / r * np.sin(2 * lam)
    v = kap * jvp(2, kap * r) * np.cos(2 * lam)
    run.set_initial_conditions([np.stack([0.0 * r, u, v], axis=1)])
    psi = run.streamfunction()
    got = psi.evaluate(pts, all_k=True)[:, 0, 0]            # every wavenumber at every radius: the first ring alone has kmax = 1
    # the float64 twin on the same input: the A coefficients of u and v the device holds
    grid = _twin_grid(tile)
    A = tile.patchSpectral
    a64 = EL.invert(grid, "vorticity", EL.to_blocks(grid, A[:, 1]), EL.to_blocks(grid, A[:, 2]), 0.0, "R1T1", "R1T0", "R1T0", xp=False)
    e_twin = np.abs(EL.field(grid, a64, r, lam, xp=False) - psi0).max()
    e_gpu = np.abs(got - psi0).max()
    chi = run.velocity_potential(into=S.companion_grid(gp))
    e_chi = np.abs(chi.evaluate(pts, all_k=True)[:, 0, 0]).max()
    print("streamfunction: max error %.3e (float64 twin %.3e); max |velocity potential| %.3e; max |psi0| %.3f" % (e_gpu, e_twin, e_chi, np.abs(psi0).max()))
    assert e_gpu <= 2.0 * e_twin
    assert e_chi <= e_twin
    chi.close()
    tile.close()
