"""sx_project on the GPU: the values k_project writes bitwise against program_values64, the companion's coefficients bitwise against
the existing path (set_physical_values + spectralTransform_ + splineTransform_) and within the parity bar of the numpy twins of
tests/project.py, a truncating destination, the compositions (ModelRun.project, antiderivative(var=terms), invert(rhs=terms)), the
bystanders, repeatability and the refusals.  Shapes are the smallest at which the kernel can go wrong: fewer points than a wave, an
odd point count (the 8-byte form), zDim that does not divide a workgroup, lanes that straddle two columns (odd zDim, even N), rings
shorter than a stride, several workgroups, fp32-stored derivative slots."""

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import antiderivative as AD
from tests import cases
from tests import elliptic as EL
from tests import project as PJ
from tests.test_project import limit_program

pytestmark = pytest.mark.gpu

VARS = {"h": 1, "u": 2, "v": 3}
Z9, Z40 = dict(zmin=0.0, zmax=3.0, zDim=9), dict(zmin=0.0, zmax=3.0, zDim=40)
SHAPES = {
    "R4": dict(geometry="R", num_cells=4),                          # 12 points, less than a wave
    "R37": dict(geometry="R", num_cells=37),                        # 111 points: odd, one point per lane
    "RZ5_9": dict(geometry="RZ", num_cells=5, **Z9),                # 135 points, odd
    "RZ5_40": dict(geometry="RZ", num_cells=5, **Z40),
    "RL6": dict(geometry="RL", num_cells=6),                        # native ragged rings
    "RL16": dict(geometry="RL", num_cells=12, ring_L=16),
    "RLZ8": dict(geometry="RLZ", num_cells=4, ring_L=8, **Z9),      # 864 points, zDim 9: a lane's two points straddle columns
    "RLZ64": dict(geometry="RLZ", num_cells=4, ring_L=64, **Z40),   # 30720 points: several workgroups
    "RLZ8-f32": dict(geometry="RLZ", num_cells=4, ring_L=8, storage="f32", **Z9),
}
R0 = dict(bcl="R0", bcl_k0="R0", bcr="R0", bcb="R0", bct="R0")


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _grids(shape):
    """(GridParameters, oracle Grid) of a shape: no Gauss point sits at r = 0, so 1 / r is finite; three variables, free conditions"""
    import scythe_jl_amd as S
    g = dict(SHAPES[shape])
    storage, ring_L = g.pop("storage", "f64"), g.pop("ring_L", None)
    g.update(xmin=0.0, xmax=10.0, vars=dict(VARS))
    return S.GridParameters(ring_uniform_L=ring_L or 0, storage=storage, **g), O.Grid(g.pop("geometry"), g.pop("xmin"), g.pop("xmax"), g.pop("num_cells"), g.pop("vars"), ring_L=ring_L, **g)


def _source(shape, source, seed=7):
    """a tile holding random values, and what a program reads of it: `physical` as stored, or var_np1"""
    import scythe_jl_amd as S
    gp, og = _grids(shape)
    tile = S.Grid(gp, None)
    pts = S.getGridpoints(tile)
    vals = np.random.default_rng(seed).standard_normal((tile.N, tile.V))
    tile.set_physical_values(vals)
    tile.spectralTransform_()
    tile.splineTransform_()
    tile.tileTransform_()
    return gp, og, tile, pts.reshape(len(pts), -1)[:, 0], (tile.physical if source == "physical" else tile.var_np1)


def _program(gp, kind, source):
    """(terms for Grid.project, packed program, companion names, var_dst)"""
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L_
    if kind == "limits":
        prog, _ = limit_program(11, 3, len(L_.SLOTS[gp.geometry]), source=source)
        terms = [(int(q[0]), float(c), int(q[1]), [(int(q[3 + f]), int(q[7 + f])) for f in range(q[2])]) for c, q in zip(prog[0], prog[1])]
        return terms, prog, ["f%d" % o for o in range(16)], None
    fp = S.field_programs(S.ModelParameters(grid_params=gp))
    if source == "state":          # var_np1 holds no derivatives: the parts of the two programs that need none
        outs = [[t for t in fp["vorticity"] if all(s == "" for _, s in t[2])] or [(1.0, 0, [("v", "")])], fp["kinetic_energy"]]
    else:
        outs = [fp["vorticity"], fp["kinetic_energy"]]
    terms = S.program_of_outputs(outs)
    return terms, S.pack_reduce_program(gp, terms), ["ke", "zeta"], (2, 1)


def _existing_path(gp, names, want, b_zDim=None):
    """A of a companion fed the same values through set_physical_values, spectralTransform_(), splineTransform_()"""
    import scythe_jl_amd as S
    par = S.companion_params(gp, names=names, **R0)
    if b_zDim:
        par.b_zDim = b_zDim
    g = S.Grid(par, None)
    g.set_physical_values(want)
    g.spectralTransform_()
    g.splineTransform_()
    A = g.patchSpectral
    g.close()
    return A


@pytest.mark.parametrize("source", ["physical", "state"])
@pytest.mark.parametrize("kind", ["limits", "wind"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_values_transform_and_twin(shape, kind, source):
    import scythe_jl_amd as S
    gp, og, tile, r, data = _source(shape, source)
    terms, prog, names, var_dst = _program(gp, kind, source)
    dst = S.companion_grid(gp, names=names, **R0)
    tile.enable_timers(True)
    assert tile.project(terms, dst, source, var_dst) is dst
    # 1. values, bitwise (fp32 storage: from the stored values, which `physical` returns widened)
    want = PJ.values(data, r, prog, var_dst)
    got = dst.var_np1
    assert _bits(got.T) == _bits(want.T), "%s %s %s: var_np1 of the companion" % (shape, kind, source)
    assert tile.timers()["k_project"][1] == 1
    planes = S.reduce_planes(gp, terms, source)
    assert tile.kernel_bytes("k_project") == sum(4.0 if gp.storage == "f32" and s else 8.0 for _, s in planes) * tile.N + 8.0 * len(names) * tile.N
    # 2. transform, bitwise against the existing path, whose own repeatability is the premise
    A = dst.patchSpectral
    E1, E2 = _existing_path(gp, names, want), _existing_path(gp, names, want)
    premise = _bits(E1) == _bits(E2)
    if premise:
        assert _bits(A) == _bits(E1), "%s %s %s: A against set_physical_values + transforms" % (shape, kind, source)
    else:
        print("%s: the existing path does not repeat bitwise; held at the parity bar instead" % shape)
        assert np.max(np.abs(A - E1)) <= PJ.bar(E1)
    # 3. the twins
    odst = PJ.companion(og, names)
    PJ.check_against_twins(A, PJ.project64(odst, want), PJ.project_xp(odst, want), "%s %s %s" % (shape, kind, source))
    dst.close()
    tile.close()


def test_truncating_destination():
    """a destination with a smaller b_zDim (kDim follows from the ring table, which must agree): truncated as the destination says"""
    import scythe_jl_amd as S
    gp, og, tile, r, data = _source("RLZ8", "physical")
    terms, prog, names, var_dst = _program(gp, "wind", "physical")
    par = S.companion_params(gp, names=names, **R0)
    par.b_zDim = 4
    assert par.b_zDim < gp.b_zDim
    dst = S.Grid(par, None)
    tile.project(terms, dst, "physical", var_dst)
    want = PJ.values(data, r, prog, var_dst)
    A = dst.patchSpectral
    odst = PJ.companion(og, names, b_zDim=4)
    assert A.shape == (odst.S_patch(), 2)
    PJ.check_against_twins(A, PJ.project64(odst, want), PJ.project_xp(odst, want), "RLZ8 into b_zDim 4")
    assert _bits(A) == _bits(_existing_path(gp, names, want, b_zDim=4))
    dst.close()
    tile.close()


def _within_bar(got, want, what):
    b = 1e-10 * float(np.max(np.abs(want)))
    d = float(np.max(np.abs(np.asarray(got) - np.asarray(want))))
    print("%s: %.3g of the bar" % (what, d / b))
    assert d <= b, (what, d, b)


def test_composition_modelrun_project():
    """ModelRun.project({"ke": ...}, transform=True): the companion's radial-derivative slot against the twin's inverse of its own A"""
    import scythe_jl_amd as S
    hip = cases.HipModel(cases.rl_slab(num_cells=6))
    hip.step()
    fp = S.field_programs(hip.mp)
    comp = hip.run.project({"ke": fp["kinetic_energy"]}, transform=True)
    assert comp is hip.run.project({"ke": fp["kinetic_energy"]}) and comp.patch_params.var_names() == ["ke"]
    tile = hip.run.tiles[0]
    data, r = tile.physical, S.getGridpoints(tile)[:, 0]
    og = cases.oracle_grid(cases.rl_slab(num_cells=6))
    odst = PJ.companion(og, ["ke"])
    prog = S.pack_reduce_program(hip.gp, S.program_of_outputs([fp["kinetic_energy"]]))
    A64 = PJ.project64(odst, PJ.values(data, r, prog))
    _within_bar(comp.patchSpectral, A64, "ModelRun.project: A")
    comp.tileTransform_()
    _within_bar(comp.physical[:, 0, 1], odst.inverse(A64)[:, 0, 1], "ModelRun.project: d/dr of the kinetic energy")
    hip.run.close()


def test_composition_antiderivative_and_invert():
    """antiderivative(var=<divergence terms>, axis="z") against project -> tests/antiderivative.py, invert(rhs=<terms>) against
    project -> tests/elliptic.py"""
    import scythe_jl_amd as S
    gp, og, tile, r, data = _source("RLZ8", "physical")
    fp = S.field_programs(S.ModelParameters(grid_params=gp))
    odst = PJ.companion(og, ["f"])
    grid = AD.grid_of(gp, int(tile.dims.kDim))
    for name in ("divergence", "vorticity"):
        prog = S.pack_reduce_program(gp, S.program_of_outputs([fp[name]]))
        a = EL.to_blocks(grid, PJ.project64(odst, PJ.values(data, r, prog))[:, 0])
        if name == "divergence":
            F = tile.antiderivative(fp[name], axis="z")
            _within_bar(EL.to_blocks(grid, F.patchSpectral[:, 0]), AD.apply_vertical(grid, a, "low", "R0", "R0", False), "w from the divergence")
        else:
            psi = tile.invert(fp[name])
            _within_bar(EL.to_blocks(grid, psi.patchSpectral[:, 0]), EL.invert(grid, "field", a, None, 0.0, "R1T1", "R1T0", "R1T0", False),
                        "streamfunction from a program")
    tile.close()


def test_bystanders():
    """the source stays bitwise as it is with parcels and a statistics set attached, and a stepped run does not notice the calls"""
    import scythe_jl_amd as S
    case = cases.rl_slab(num_cells=6)
    fp = S.field_programs(S.ModelParameters(grid_params=cases.hip_params(case)[0]))
    outs = {"zeta": fp["vorticity"], "ke": fp["kinetic_energy"]}
    plain, busy = cases.HipModel(case), cases.HipModel(case)
    tile = busy.run.tiles[0]
    busy.run.set_parcels(np.array([[1.0e5, 0.3], [2.0e5, 2.0]]), ("u", "v"))
    busy.run.set_statistics([("max", [(1.0, 0, [("u", "")])])], "state")
    plain.run.set_parcels(np.array([[1.0e5, 0.3], [2.0e5, 2.0]]), ("u", "v"))
    plain.run.set_statistics([("max", [(1.0, 0, [("u", "")])])], "state")
    for _ in range(3):
        plain.step()
        busy.step()
        tile.tileTransform_()
        before = (tile.get_state(), tile.physical, tile.patchSpectral, tile.var_np1, tile.spectral, tile.get_parcel_state(), tile.get_statistics_state())
        busy.run.project(outs, source="physical")
        busy.run.project({"ke": fp["kinetic_energy"]}, source="state")
        after = (tile.get_state(), tile.physical, tile.patchSpectral, tile.var_np1, tile.spectral, tile.get_parcel_state(), tile.get_statistics_state())
        assert _bits(*before) == _bits(*after)
    assert _bits(plain.run.tiles[0].get_state(), plain.physical()) == _bits(tile.get_state(), busy.physical())
    assert _bits(*plain.run.parcels()) == _bits(*busy.run.parcels())
    plain.run.close()
    busy.run.close()


def test_repeatable_and_independent_of_other_outputs():
    import scythe_jl_amd as S
    gp, og, tile, r, data = _source("RLZ64", "physical")
    fp = S.field_programs(S.ModelParameters(grid_params=gp))
    two = S.companion_grid(gp, names=["zeta", "ke"], **R0)
    terms = S.program_of_outputs([fp["vorticity"], fp["kinetic_energy"]])
    A1 = tile.project(terms, two).patchSpectral
    two.set_physical_values(np.zeros((two.N, 2)))
    A2 = tile.project(terms, two).patchSpectral
    assert _bits(A1) == _bits(A2)
    other = tile.project(S.program_of_outputs([fp["divergence"], fp["vorticity"]]), two).patchSpectral
    one = S.companion_grid(gp, names=["zeta"], **R0)
    alone = tile.project(S.program_of_outputs([fp["vorticity"]]), one).patchSpectral
    assert _bits(A1[:, 0]) == _bits(other[:, 1]) == _bits(alone[:, 0])
    for g in (one, two, tile):
        g.close()


def test_refusals_leave_the_destination_as_it_is():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    gp, og, tile, r, data = _source("RL6", "physical")
    dst = S.companion_grid(gp, names=["a", "b"], **R0)
    ok = [(0, 1.0, 0, [("u", "r")]), (1, 1.0, -1, [("v", "")])]
    A0 = tile.project(ok, dst).patchSpectral
    state0 = (A0, dst.var_np1, dst.spectral)

    def refused(match, src=tile, terms=ok, into=dst, **kw):
        with pytest.raises(S.ScytheHipError, match=match):
            src.project(terms, into, **kw)
        assert _bits(dst.patchSpectral, dst.var_np1, dst.spectral) == _bits(*state0), match
    three = S.Grid(gp, None)
    refused("the destination is the source", src=three, terms=ok + [(2, 1.0, 0, [("h", "")])], into=three)
    case = cases.rl_advection(num_cells=6)
    model = S.Grid(*cases.hip_params(case))
    refused("has an equation set", terms=ok + [(2, 1.0, 0, [("h", "")])], into=model)
    part = S.Grid(gp, None, 0, 3)
    refused("one-tile", src=part)
    gp2, _ = _grids("RL16")
    wide = S.Grid(gp2, None)
    refused("differs from the source's in num_cells", src=wide)
    refused("not the destination's number of variables", terms=ok[:1])
    refused("not a permutation", var_dst=(1, 1))
    refused("SX_REDUCE_STATE holds the values only", source="state")
    refused("output 0 has no term", terms=ok[1:])
    lib = S.load()
    coef, packed, n_out = S.pack_reduce_program(gp, ok)
    vd = np.array([1, 2], dtype=np.int32)
    P = lambda a: a.ctypes.data_as(L.P_I32)
    assert lib.sx_project(None, 0, 2, coef.ctypes.data_as(L.P_D), P(packed), 2, dst._h, P(vd)) == 1 and b"null handle" in lib.sx_last_error()
    assert lib.sx_project(tile._h, 0, 2, coef.ctypes.data_as(L.P_D), P(packed), 2, None, P(vd)) == 1 and b"null handle" in lib.sx_last_error()
    assert lib.sx_project(tile._h, 0, 2, None, P(packed), 2, dst._h, P(vd)) == 1 and b"null coef" in lib.sx_last_error()
    assert lib.sx_project(tile._h, 0, 2, coef.ctypes.data_as(L.P_D), None, 2, dst._h, P(vd)) == 1 and b"null terms" in lib.sx_last_error()
    assert lib.sx_project(tile._h, 0, 2, coef.ctypes.data_as(L.P_D), P(packed), 2, dst._h, None) == 1 and b"null var_dst" in lib.sx_last_error()
    assert _bits(dst.patchSpectral, dst.var_np1, dst.spectral) == _bits(*state0)
    for g in (three, model, part, wide, dst, tile):
        g.close()
