"""The fused RZ inverse transform (csrc/sx_rz.hip: k_rz_inverse_nodes, k_rz_inverse) entry by entry against extended precision,
at every launch shape of launch_rz_inverse and through both masks.

Every ring, level, variable and slot of `physical` is held to

    |phys_hip - phys_xp| <= C_INV 2^-53 scale        (+ 2^-24 |phys_xp| on the derivative slots of fp32-stored planes)

with phys_xp and scale from oracle_np.inverse_xp(..., with_scale=True): the same chain in longdouble, and the same chain over
absolute values, sum_zm |M_sz[z, zm]| sum_j |phi_d[ring, j]| |A[node + j, v, zm]|.  One statement for both kernels, every slot and
every shape; the ids name the launch as the library's own plan reports it (cases.rz_inverse_launch_geometry) and
tests/test_rz_reference.py proves on the host that the lists reach every branch of the launcher.

C_INV = b_zDim + 14, counted, not fitted.  Along the path of any term there are: the basis weight, formed in Float64 from its
definition (the argument 3/2 + offset - j: 2 roundings, the cubic: 4, the scale 1 / DX^d: 3 - 9 in all), its product with A and
the three radial sums (4), the once-rounded entry of the vertical operator (1), and the vertical product and sums (b_zDim).
The reference takes the basis weights at the exact Gauss offsets (inverse_xp(..., exact_offsets=True)), which is what the library
tabulates once per grid.  tests/test_rz_reference.py asserts on the CPU that a plain Float64 evaluation from Float64 tables
(cases.inverse_f64_tables) stays inside the bound at every shape and tile below - worst c per slot (u, r, rr, z, zz) 3.4 / 3.0 /
2.7 / 3.8 / 4.4, whatever the cell count - and that the bound catches a swapped level, a neighbour's weights, a dropped mode and
a single entry moved by 8 C_INV 2^-53 scale.
The two fp64 oracles (oracle_np Grid.inverse, the C oracle) do NOT stay inside b_zDim + 14 on grids of many cells: they evaluate
the B-spline at (r - x_node) / DX from the Float64 gridpoint r, three roundings of (r / DX) 2^-53 each in the argument, which
grows with the cell index and has nothing to do with the transform's arithmetic.  Worst c per slot against this reference:

    cells (shape)        u      r      rr     z      zz        (oracle_np; the C oracle is within 1.5 of it everywhere)
    5   (all levels)     4.0    8.2    7.2    5.4    5.5
    12 .. 14            20.5   44.6   44.0   26.1   31.3
    26, 27              36.4  112.0   65.5   39.0   51.2
    40  (tile 27..39)   44.3   95.6   79.8   56.6   68.9

tests/test_rz_reference.py holds them to b_zDim + 14 + 5 x the patch's cells (4.3 per cell measured) and records the table.
MI355X, worst c over all cases: see DESIGN.md section 2.

The mask test reads `physical` after sx_advance, which include/scythe_hip.h leaves unspecified in general; on the fused RZ path
the planes the equation set asks for are final after the step's inverse transform and every other plane is untouched, and that
is what it pins."""
import numpy as np
import pytest

from tests import cases, physics
from tests.child_run import forward_inputs, make_case



def c_inv(case):
    """b_zDim + 14: the roundings along the path of one term (module docstring)"""
    return cases.oracle_grid(case).b_zDim + 14

# (cells, zDim, b_zDim or None for the default)
_CELLS = [(4, 9, None), (12, 9, None), (13, 9, None), (14, 9, None), (26, 9, None), (27, 9, None)]
_LEVELS = [(5, 16, 16), (5, 17, 17), (5, 64, 43), (5, 65, 43), (5, 128, 86), (5, 129, 86), (5, 256, 100)]
_CHUNKS = [(5, 40, 31), (5, 40, 32), (5, 40, 33), (5, 72, 64), (5, 72, 65)]
_RINGS = [(5, 72, 63), (5, 72, 64), (5, 72, 65), (14, 17, 17), (5, 136, 136)]       # SX_RZ_INV=0; the last: over 64 KB of LDS
_F32 = [(14, 17, 17), (5, 65, 43)]
RING_ENV = {"SX_RZ_INV": "0"}
# (shape, per-handle switches, storage)
INV_CASES = ([(s, {}, "f64") for s in _CELLS + _LEVELS + _CHUNKS] + [(s, RING_ENV, "f64") for s in _RINGS]
             + [(s, env, "f32") for s in _F32 for env in ({}, RING_ENV)])

# sx_advance: the equation set's mask.  (maker, kwargs, switches)
ADV_SHAPE = dict(num_cells=14, zDim=17)
ADV_CASES = [("rz_advection", ADV_SHAPE, {}), ("rz_semiimplicit", ADV_SHAPE, {}), ("rz_euler", ADV_SHAPE, {}),
             ("rainfall.rz_rain_mixed", ADV_SHAPE, {}), ("rz_advection", ADV_SHAPE, RING_ENV)]

# a patch of 40 cells in 3 tiles (14, 13, 13 cells): cell0 != 0
TILE_SPEC = ["rz_advection", {"num_cells": 40, "zDim": 20}, {}]
TILES = 3


def inv_case(shape):
    nc, nz, b = shape
    return make_case(["rz_advection", {"num_cells": nc, "zDim": nz}, {"b_zDim": b} if b else {}])


def inv_id_of(geo, storage="f64"):
    k = geo["kernel"].replace("<double>", "").replace("<float>", "-f32")
    return "%s%s-n%dz%db%d-g%dx%dx%d-lastx%d-lastw%d-kc%d-tailk%d-lds%d%s" % (
        k, "" if storage == "f64" or "f32" in k else "-f32", geo["ncells"], geo["zDim"], geo["b_zDim"], *geo["grid"], geo["last_x"],
        geo["last_waves"], geo["chunks"], geo["tail_k"], geo["lds"], "-attr" if geo["attr"] else "")


def _inv_id(shape, env, storage):
    return inv_id_of(cases.rz_inverse_launch_geometry(inv_case(shape), env or None, storage), storage)


def adv_case(maker, kw):
    return physics.make_case(maker, kw)


def slot_masks(case):
    """Per-variable bit masks of the planes sx_advance's inverse transform produces, from the library (sx_equation_slot_masks)."""
    import ctypes as C
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    g = cases.oracle_grid(case)
    lib = S.load()
    out = (C.c_int32 * g.V)()
    L.check(lib.sx_equation_slot_masks(lib.sx_equation_set_id(case["eq"].encode()), cases.GEOM[g.geometry], g.V, out))
    return list(out)


def ops_pass_width(mask, g):
    """NB of rz_ops_pass<NB> for a variable's mask: the vertical operators it needs (value for u / r / rr, d/dz, d2/dz2); 0: the
    early return of a variable with an empty mask."""
    sl = {s: 1 << i for i, s in enumerate(g.slots)}
    return int(bool(mask & (sl["u"] | sl["r"] | sl["rr"]))) + int(bool(mask & sl["z"])) + int(bool(mask & sl["zz"]))


def check_inverse(case, A, phys, storage, label, tile=None, planes=None):
    """Every entry (or, with `planes` [V, D] bool, every entry of those planes) against the bound; prints the worst c = |err| /
    (2^-53 scale) after the fp32 allowance, the case's C_INV and where it is."""
    g = cases.oracle_grid(case)
    ref, scale = cases.inverse_reference(case, A, tile)
    assert phys.shape == ref.shape and np.isfinite(phys).all()
    q, idx = cases.inverse_bound_ratio(phys, ref, scale, 1.0, f32=storage == "f32")
    if planes is not None:
        q = np.where(planes[None, :, :], q, 0.0)
        idx = np.unravel_index(int(np.argmax(q)), q.shape)
    where = cases.where_rz(g, idx, tile[0] if tile else 0)
    print("\n%s: worst c = %.2f of C_INV = %d at %s" % (label, q[idx], c_inv(case), where))
    assert q[idx] <= c_inv(case), (label, q[idx], where)
    return float(q[idx])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,env,storage", INV_CASES, ids=[_inv_id(*c) for c in INV_CASES])
def test_inverse_against_extended_precision(monkeypatch, shape, env, storage):
    """Random A -> sx_tile_transform (the full mask: rz_ops_pass<3>, rz_pass<3>) -> every entry of `physical`."""
    import scythe_jl_amd as S
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = inv_case(shape)
    g = S.Grid(*cases.hip_params(case, storage))
    _, A = forward_inputs(g.N, g.V, int(g.dims.s_patch))
    g.set_patch_spectral_a(A)
    g.tileTransform_()
    phys = g.physical
    g.close()
    if storage == "f32":
        assert (phys[:, :, 1:].astype(np.float32).astype(np.float64) == phys[:, :, 1:]).all()
    check_inverse(case, A, phys, storage, _inv_id(shape, env, storage))


@pytest.mark.gpu
@pytest.mark.parametrize("maker,kw,env", ADV_CASES, ids=["%s-%s" % (m.split(".")[-1], "rings" if e else "nodes") for m, _, e in ADV_CASES])
def test_inverse_of_sx_advance_writes_the_planes_of_the_mask_and_no_other(monkeypatch, maker, kw, env):
    """A = a1, sx_tile_transform: P1.  A = a2, sx_advance(1): the planes the equation set's mask names (asked of the library) hold
    the inverse transform of a2 within the bound, every other plane is P1 bit for bit - rz_ops_pass<1> / <2> / <3> and "no plane nobody asked for" (no RZ
    equation set has a variable with an empty mask, so the kernels' early return for one runs in no test).  This reads `physical` after sx_advance, which the
    header leaves unspecified in general; on the fused RZ path the requested planes are final, and that is what this pins."""
    import scythe_jl_amd as S
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = adv_case(maker, kw)
    og = cases.oracle_grid(case)
    masks = slot_masks(case)
    planes = np.array([[bool(m >> d & 1) for d in range(og.D)] for m in masks])
    base = physics.base_coefficients(case)
    a1, a2 = physics.state_coefficients(base, 1), physics.state_coefficients(base, 2)
    g = S.Grid(*cases.hip_params(case))
    g.set_patch_spectral_a(a1)
    g.tileTransform_()
    p1 = g.physical
    g.set_patch_spectral_a(a2)
    g.advance(1)
    p2 = g.physical
    g.close()
    geo = cases.rz_inverse_launch_geometry(case, env or None)
    label = "%s %s NB per variable %s" % (case["eq"], inv_id_of(geo), [ops_pass_width(m, og) for m in masks])
    check_inverse(case, a1, p1, "f64", label + " (full mask, a1)")
    check_inverse(case, a2, p2, "f64", label + " (set's mask, a2)", planes=planes)
    assert planes.any() and not planes.all()
    assert (p2[:, ~planes].view(np.int64) == p1[:, ~planes].view(np.int64)).all(), "sx_advance wrote a plane outside the mask"
    ref2, _ = cases.inverse_reference(case, a2)
    moved = np.asarray(ref2, dtype=np.float64)[:, planes] != p1[:, planes]
    assert ((p2[:, planes] != p1[:, planes]) | ~moved).all(), "a requested plane kept its old values"


@pytest.mark.gpu
def test_inverse_of_each_tile():
    """40 cells in 3 tiles (14, 13, 13 cells, cell0 = 0, 14, 27): each tile's `physical` against inverse_xp of its own rings."""
    import scythe_jl_amd as S
    case = make_case(TILE_SPEC)
    gp, mp = cases.hip_params(case)
    og = cases.oracle_grid(case)
    A = np.random.default_rng(31).standard_normal((og.S_patch(), og.V))
    for t, (c0, n) in enumerate(cases.even_tiles(case["grid"]["num_cells"], TILES)):
        g = S.Grid(gp, mp, tile_cell0=c0, tile_num_cells=n, tile_num=t)
        g.set_patch_spectral_a(A)
        g.tileTransform_()
        phys = g.physical
        g.close()
        geo = cases.rz_inverse_launch_geometry(case, tile=(c0, n))
        check_inverse(case, A, phys, "f64", "tile %d (cells %d..%d) %s" % (t, c0, c0 + n - 1, inv_id_of(geo)), tile=(c0, n))
