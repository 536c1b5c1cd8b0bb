"""The references of tests/test_gpu_rz.py and of the fused-RZ and semi-implicit cases of tests/test_gpu_forward.py and
tests/physics.py, checked without a GPU.

(1) The three launch plans (sx_launch_plan: SX_PLAN_RZ_INVERSE, SX_PLAN_RZ_FORWARD, SX_PLAN_SEMI) against the arithmetic stated in
    include/scythe_hip.h, for every case.  (2) Together the case lists reach every branch of the three launchers, and every switch
    case changes the launch it is about.  (3) The bound of tests/test_gpu_rz.py, |phys - phys_xp| <= (b_zDim + 14) 2^-53 scale, holds for
    a plain Float64 evaluation from Float64 tables at every inverse shape and tile, the two fp64 oracles are within their
    gridpoint term of it (worst ratio per slot: that file's docstring), and the forward bound of
    tests/test_forward_reference.py holds for the oracle's forward at every new forward shape: asserted.  (4) The bound bites:
    four deliberate errors are each caught and reported at the right (ring, level, variable, slot)."""
import numpy as np
import pytest

from oracle import oracle_c as OC
from oracle import oracle_np as O
from tests import cases, physics
from tests import test_gpu_forward as F
from tests import test_gpu_rz as R
from tests.child_run import forward_inputs, make_case
from tests.test_forward_reference import C_ORACLE

ceil = lambda a, b: -(-a // b)
RZ_FWD = [c for c in F.FWD_CASES if c[0].startswith("rz-fused")]


# ----------------------------------------------------------------------------- (1) plans against the header's arithmetic
@pytest.mark.parametrize("shape,env,storage", R.INV_CASES, ids=[R._inv_id(*c) for c in R.INV_CASES])
def test_rz_inverse_plan(shape, env, storage):
    nc, nz, _ = shape
    case = R.inv_case(shape)
    b, V = cases.oracle_grid(case).b_zDim, 4
    geo = cases.rz_inverse_launch_geometry(case, env or None, storage)
    ldsn = 8 * (16 * ceil(b, 32) * 32 + 3 * 16 * 65 + 3 * 39 * 4)
    nodes = not env and ldsn <= 65536
    st = "float" if storage == "f32" else "double"
    assert geo["kernel"] == ("k_rz_inverse_nodes<%s>" if nodes else "k_rz_inverse<%s>") % st
    gz = ceil(ceil(nz, 16), 4)
    if nodes:
        assert (geo["grid"], geo["lds"], geo["chunks"], geo["attr"]) == ((ceil(nc, 13), V, gz), ldsn, ceil(b, 32), False)
    else:
        lds = 8 * 3 * 16 * ceil(b, 64) * 64
        assert (geo["grid"], geo["lds"], geo["chunks"], geo["attr"]) == ((ceil(3 * nc, 16), V, gz), lds, ceil(b, 64), lds > 65536)
    assert 1 <= geo["last_x"] <= (13 if nodes else 16) and 1 <= geo["last_waves"] <= 4


def test_rz_inverse_plan_falls_back_where_the_nodes_form_does_not_fit():
    """The nodes form needs 8 (16 Zp + 3588) bytes: 64 KB are passed at Zp = 288, which b_zDim <= 256 never reaches - the default
    takes the nodes form at every size the kernels accept, and only SX_RZ_INV=0 reaches the ring-tile form."""
    for b in (129, 200, 256):
        kernel, out = cases.launch_plan(cases.PLAN_RZ_INVERSE, 256, b, 5, 4, 0, env=None)
        assert kernel == "k_rz_inverse_nodes<double>" and out[3] <= 65536 and out[5] == 0
        kernel, out = cases.launch_plan(cases.PLAN_RZ_INVERSE, 256, b, 5, 4, 0, env=R.RING_ENV)
        assert kernel == "k_rz_inverse<double>" and out[3] == 8 * 3 * 16 * ceil(b, 64) * 64 and out[5] == 1


@pytest.mark.parametrize("name,spec,env,storage", RZ_FWD, ids=[F._fwd_id(*c) for c in RZ_FWD])
def test_rz_forward_plan(name, spec, env, storage):
    case = make_case(spec)
    g = cases.oracle_grid(case)
    geo = cases.rz_forward_launch_geometry(case)
    nmt = ceil(g.b_zDim, 16)
    mt = min(nmt, 4)
    assert geo["kernel"] == "k_rz_forward" == cases.sb_launch_geometry(case)["kernel"]
    assert geo["grid"] == (ceil(g.nc + 3, 16), g.V, ceil(nmt, mt)) and geo["mt_per_wg"] == mt
    assert (geo["chunks"], geo["lds"]) == (ceil(g.zDim, 64), 8 * (16 * 64 * ceil(g.zDim, 64) + 19 * 3 * 4))
    assert cases.rz_forward_launch_geometry(case, v_cnt=1)["grid"][1] == 1


@pytest.mark.parametrize("cid", list(physics.SEMI_CASES))
def test_semi_plan(cid):
    case, _, env, _ = physics.case_of(cid)
    g = cases.oracle_grid(case)
    nz, ncol = g.zDim, 3 * g.nc
    geo = cases.semi_launch_geometry(case, env)
    if env:
        cpb = max(1, 256 // nz)
        assert geo == dict(kernel="k_semiimplicit", wgs=ceil(ncol, cpb), threads=cpb * nz, tiles=0, trips=0, chunks=0, lds=8 * 3 * cpb * nz,
                           attr=False, columns=ncol, last=ncol - (ceil(ncol, cpb) - 1) * cpb, zDim=nz)
    else:
        tiles, lds = min(8, ceil(nz, 16)), 8 * 4 * 16 * 64 * ceil(nz, 64)
        assert geo == dict(kernel="k_semi_mfma", wgs=ceil(ncol, 16), threads=64 * tiles, tiles=tiles, trips=ceil(ceil(nz, 16), tiles),
                           chunks=ceil(nz, 64), lds=lds, attr=lds > 65536, columns=ncol, last=ncol - (ceil(ncol, 16) - 1) * 16, zDim=nz)


def test_plans_refuse_what_the_kernels_do_not_take():
    import scythe_jl_amd as S
    for kind, dims in ((cases.PLAN_RZ_INVERSE, (257, 100, 5, 4, 0)), (cases.PLAN_RZ_FORWARD, (20, 21, 5, 4)), (cases.PLAN_SEMI, (0, 15)),
                       (8, (1, 1, 1, 1))):
        with pytest.raises(S.ScytheHipError):
            cases.launch_plan(kind, *dims)


# ----------------------------------------------------------------------------- (2) coverage
def test_the_cases_reach_every_launcher_branch():
    inv = [cases.rz_inverse_launch_geometry(R.inv_case(s), e or None, st) for s, e, st in R.INV_CASES]
    assert {g_["kernel"] for g_ in inv} == {"k_rz_inverse_nodes<double>", "k_rz_inverse_nodes<float>", "k_rz_inverse<double>", "k_rz_inverse<float>"}
    assert any(g_["attr"] and g_["form"] == "rings" for g_ in inv) and not all(g_["attr"] for g_ in inv if g_["form"] == "rings")
    nodes = [g_ for g_ in inv if g_["form"] == "nodes"]
    assert {g_["grid"][0] for g_ in nodes} >= {1, 2, 3}
    assert {g_["last_x"] for g_ in nodes if g_["grid"][0] > 1} >= {1, 13}
    assert {g_["grid"][2] for g_ in nodes} >= {1, 2, 4}
    assert any(g_["grid"][2] > 1 and g_["last_waves"] == 1 for g_ in nodes) and any(g_["grid"][2] > 1 and g_["last_waves"] == 1 for g_ in inv if g_["form"] == "rings")
    assert {g_["chunks"] for g_ in nodes} >= {1, 2, 3, 4} and {g_["chunks"] for g_ in inv if g_["form"] == "rings"} >= {1, 2, 3}
    assert {g_["tail_k"] for g_ in nodes} >= {1, 31, 32} and {g_["tail_k"] for g_ in inv if g_["form"] == "rings"} >= {1, 63, 64}
    # the masks of sx_advance: rz_ops_pass<1>, <2>, <3> and a variable that returns early, in the nodes form; the ring-tile form too
    widths = {}
    for maker, kw, env in R.ADV_CASES:
        case = R.adv_case(maker, kw)
        og = cases.oracle_grid(case)
        geo = cases.rz_inverse_launch_geometry(case, env or None)
        assert geo["grid"][0] >= 2
        widths.setdefault(geo["form"], set()).update(R.ops_pass_width(m, og) for m in R.slot_masks(case))
    assert widths["nodes"] >= {1, 2, 3}, widths
    assert "rings" in widths and len(widths["rings"]) >= 2
    # The early return of a variable with an EMPTY mask cannot be launched: the library's four RZ equation sets (these) read at least
    # the value of every variable, and sx_tile_transform asks for everything.  Should a set gain such a variable, this fails and
    # the mask test of tests/test_gpu_rz.py needs a case for it (it already demands that the variable's planes stay bit for bit).
    assert 0 not in widths["nodes"] | widths["rings"]
    # forward: three node tiles, a second group of mode tiles, a second and a fourth K chunk; tiles of a patch
    fwd = [cases.rz_forward_launch_geometry(make_case(spec)) for _, spec, _, _ in RZ_FWD]
    assert max(g_["grid"][0] for g_ in fwd) >= 3 and max(g_["grid"][2] for g_ in fwd) >= 2
    assert {g_["last_x"] for g_ in fwd if g_["grid"][0] > 1} >= {1, 16} and {g_["chunks"] for g_ in fwd} >= {1, 2, 4}
    tiles = [t for n, spec, t in F.TILE_CASES if cases.sb_launch_geometry(make_case(spec))["kernel"] == "k_rz_forward"]
    assert tiles == [3] and make_case(R.TILE_SPEC)["grid"]["num_cells"] == 40 and R.TILES == 3
    # semi-implicit: one and two wave trips, 1, 2 and 4 K chunks, the over-64 KB branch, partial and full last workgroups, both kernels
    semi = [cases.semi_launch_geometry(physics.case_of(c)[0], physics.case_of(c)[2]) for c in physics.SEMI_CASES]
    mf = [g_ for g_ in semi if g_["kernel"] == "k_semi_mfma"]
    assert {g_["trips"] for g_ in mf} == {1, 2} and {g_["chunks"] for g_ in mf} >= {1, 2, 4}
    assert {g_["attr"] for g_ in mf} == {False, True} and {g_["last"] for g_ in mf} >= {1, 15, 16} and {g_["wgs"] for g_ in mf} >= {1, 3}
    assert sum(g_["kernel"] == "k_semiimplicit" for g_ in semi) == 2


def test_the_switch_cases_change_the_launch():
    for s, env, st in R.INV_CASES:
        if env:
            a, b = (cases.rz_inverse_launch_geometry(R.inv_case(s), e, st) for e in (None, env))
            assert a["form"] == "nodes" and b["form"] == "rings" and a["kernel"] != b["kernel"]
    for cid in physics.SEMI_CASES:
        case, _, env, _ = physics.case_of(cid)
        if env:
            assert cases.semi_launch_geometry(case, None)["kernel"] == "k_semi_mfma"
            assert cases.semi_launch_geometry(case, env)["kernel"] == "k_semiimplicit"


# ----------------------------------------------------------------------------- (3) the fp64 oracles inside the bound
INV_SHAPES = sorted({s for s, _, _ in R.INV_CASES}, key=lambda s: (s[1], s[0], s[2] or 0))


@pytest.fixture(scope="module")
def references():
    """{shape: (case, A, ref, scale)}, computed once"""
    out = {}
    for s in INV_SHAPES:
        case = R.inv_case(s)
        g = cases.oracle_grid(case)
        _, A = forward_inputs(g.tile_npoints(0, g.nc), g.V, g.S_patch())
        out[s] = (case, A) + cases.inverse_reference(case, A)
    return out


def test_scale_bounds_the_reference_and_is_not_loose(references):
    for case, A, ref, scale in references.values():
        assert ref.dtype == O.XP and (scale >= np.abs(ref)).all() and (scale > 0).all()
        assert float(np.median(np.abs(ref) / scale)) > 1e-3


ORACLE_PER_CELL = 5       # the oracles' basis weights from the Float64 gridpoint: 3 roundings of (r / DX) 2^-53 in the argument


def _held(case, A, ref, scale, tile=None):
    """The Float64 table evaluation inside C_INV (and inside it with fp32-stored planes); both oracles inside C_INV + 5 x cells."""
    g = cases.oracle_grid(case)
    C = R.c_inv(case)
    c0, n = tile if tile else (0, g.nc)
    tab = cases.inverse_f64_tables(case, A, tile)
    q, idx = cases.inverse_bound_ratio(tab, ref, scale, 1.0)
    print("\n%-9s C_INV = %3d  worst c per slot %s" % ("tables", C, " ".join("%5.1f" % x for x in q.max(axis=(0, 1)))))
    assert q[idx] <= C, (q[idx], cases.where_rz(g, idx, c0))
    assert cases.inverse_bound_ratio(physics.f32_slots(tab), ref, scale, C, f32=True)[0].max() <= 1.0
    for name, phys in (("oracle_np", g.inverse(A, c0, n)), ("C oracle", OC.TileOracle(g, c0, n).inverse(A))):
        q, idx = cases.inverse_bound_ratio(phys, ref, scale, 1.0)
        print("%-9s cells %3d   worst c per slot %s" % (name, g.nc, " ".join("%5.1f" % x for x in q.max(axis=(0, 1)))))
        assert q[idx] <= C + ORACLE_PER_CELL * g.nc, (name, q[idx], cases.where_rz(g, idx, c0))


@pytest.mark.parametrize("shape", INV_SHAPES, ids=["n%dz%db%s" % s for s in INV_SHAPES])
def test_fp64_evaluations_are_inside_the_inverse_bound(references, shape):
    _held(*references[shape])


def test_fp64_evaluations_are_inside_the_inverse_bound_on_each_tile():
    case = make_case(R.TILE_SPEC)
    g = cases.oracle_grid(case)
    A = np.random.default_rng(31).standard_normal((g.S_patch(), g.V))
    ref, scale = cases.inverse_reference(case, A)
    p0 = 0
    for c0, n in cases.even_tiles(g.nc, R.TILES):
        r, s = cases.inverse_reference(case, A, (c0, n))
        N = g.tile_npoints(c0, n)
        assert (r == ref[p0:p0 + N]).all() and (s == scale[p0:p0 + N]).all()
        _held(case, A, r, s, (c0, n))
        p0 += N


@pytest.mark.parametrize("name,spec,env,storage", RZ_FWD, ids=[F._fwd_id(*c) for c in RZ_FWD])
def test_the_oracle_forward_is_inside_the_forward_bound(name, spec, env, storage):
    g = cases.oracle_grid(make_case(spec))
    vals, _ = forward_inputs(g.tile_npoints(0, g.nc), g.V, g.S_patch())
    B, S = O.forward_xp(g, vals)
    c = float((np.abs(g.forward(vals).astype(O.XP) - B) / S).max() / O.XP(2.0 ** -53))
    print("\n%s: oracle forward worst c = %.1f" % (name, c))
    assert c <= C_ORACLE, c


# ----------------------------------------------------------------------------- (4) the bound bites
MUT_SHAPE = (14, 17, 17)
RING, LEVEL, VAR = 19, 5, 2


def _mutated(kind, case, A, ref, scale):
    """(phys, (ring, level, variable, slot) or None where any slot of the point may be the worst)"""
    g = cases.oracle_grid(case)
    nz = g.zDim
    phys = np.asarray(ref, dtype=np.float64).copy()
    p = RING * nz + LEVEL
    if kind == "entry":
        d = g.slots.index("rr")
        phys[p, VAR, d] += float(8 * R.c_inv(case) * O.XP(2.0 ** -53) * scale[p, VAR, d])
        return phys, (RING, LEVEL, VAR, "rr")
    if kind == "levels":
        q = RING * nz + LEVEL + 1
        phys[[p, q]] = phys[[q, p]]
        return phys, (RING, (LEVEL, LEVEL + 1), None, None)
    if kind == "weights":         # ring RING evaluated with the basis weights of ring RING + 1 (the same cell: the same four nodes)
        assert RING // 3 == (RING + 1) // 3
        other = O.inverse_xp(g, A, [RING + 1], exact_offsets=True)[RING + 1]
        phys[RING * nz:(RING + 1) * nz] = np.asarray(other, dtype=np.float64)
        return phys, (RING, None, None, None)
    if kind == "mode":            # the last Chebyshev mode dropped for one variable
        A2 = A.copy()
        A2.reshape(g.b_zDim, g.K2, g.b_rDim, g.V)[g.b_zDim - 1, :, :, VAR] = 0.0
        ref2, _ = cases.inverse_reference(case, A2)
        return np.asarray(ref2, dtype=np.float64), (None, None, VAR, None)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["entry", "levels", "weights", "mode"])
def test_the_inverse_bound_catches(references, kind):
    case, A, ref, scale = references[MUT_SHAPE]
    g = cases.oracle_grid(case)
    clean, _ = cases.inverse_bound_ratio(np.asarray(ref, dtype=np.float64), ref, scale, R.c_inv(case))
    assert clean.max() <= 1.0
    phys, want = _mutated(kind, case, A, ref, scale)
    q, idx = cases.inverse_bound_ratio(phys, ref, scale, R.c_inv(case))
    bad = np.argwhere(q > 1.0)
    assert len(bad), "%s stays inside the bound (worst ratio %.3g)" % (kind, q.max())
    ring, level, var, slot = want
    got = (idx[0] // g.zDim, idx[0] % g.zDim, idx[1], g.slots[idx[2]])
    text = cases.where_rz(g, idx)
    assert text == "ring %d level %d variable %d slot %s" % got
    if ring is not None:
        assert set(bad[:, 0] // g.zDim) == {ring}, text
    if isinstance(level, tuple):
        assert set(bad[:, 0] % g.zDim) == set(level), text
    elif level is not None:
        assert got[1] == level and len(bad) == 1, text
    if var is not None:
        assert set(bad[:, 1]) == {var}, text
    if slot is not None:
        assert got[3] == slot
    if kind == "weights":         # every level of the ring is off, in the radial-derivative slots at least
        assert set(bad[:, 0] % g.zDim) == set(range(g.zDim))
    if kind == "mode":            # every ring is off
        assert set(bad[:, 0] // g.zDim) == set(range(g.rDim))
