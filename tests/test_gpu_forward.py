"""spectralTransform! (values -> B) and the vertical inverse (A -> Az) at every launch shape of launch_sb and launch_zinv.

launch_sb (csrc/sx_kernels.hip) picks k_sb (no z), k_sbz (zDim not 32 / 64 / 128), k_sbw<NZ, PREFETCH> or one of the matrix-core
k_sbw_mfma instantiations (fp64 or fp32-stored ring spectra), then cuts the patch into segments of cps cells with a 3-cell warm-up,
the last segment owning the 3 trailing nodes; inside k_sbw_mfma the rows are split into row tiles per wave.  launch_zinv picks
k_colmat_mfma<MT, OT, CT> or k_colmat.  Every case id names that launch as cases.sb_launch_geometry / zinv_launch_geometry
report it (the library's own launch plans, sx_launch_plan, pinned by tests/test_forward_reference.py), and
test_the_cases_reach_every_launcher_branch checks on the host that the list covers every instantiation.

B is compared entry by entry with oracle_np.forward_xp, the same operation in extended precision, which also returns each entry's
condition scale (the chain of sums over absolute values): |B_hip - B_xp| <= C_B 2^-53 scale.  C_B is fixed once for every kernel:
an fp64 evaluation in any summation order stays within n u scale for its n terms per stage (up to zDim + L + 12 here), and a
correct kernel measures well below C_B (the worst c per kernel is printed).  A wrong row tile, a lost warm-up cell or a missing
trailing node leaves an entry O(1) of its scale off.  f32x stores the ring spectra as fp32: the bar widens by the rounding of
those, 2^-24 scale.  The A coefficients after the solve are checked per column against the fp64 oracle's solve of that B."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import cases
from tests.child_run import forward_inputs, make_case, run_in_child

C_B = 32                  # |B_hip - B_xp| <= C_B * 2^-53 * scale, every kernel (MI355X: <= 3.3 on random values, 11 on model fields)
TOL_A = 1e-12             # per column, A vs the fp64 oracle's solve of the same B
TOL = 1e-10               # A coefficients and values after 3 steps vs the C oracle (fp64)
F32_SLOT = 4 * 2.0 ** -24       # f32x: fp32-stored Az and derivative planes, on top of the fp64 bar of check_full
F32_MODEL = 1e-5          # f32x: A coefficients and values after 3 steps vs the C oracle


def _z(nz, b, nc=4, L=16, maker="rlz_advection"):
    return [maker, {"num_cells": nc, "zDim": nz, "ring_L": L}, {"b_zDim": b}]


def rz_fwd_id(geo):
    """Name fragment of one launch_rz_forward launch, from the library's plan (cases.rz_forward_launch_geometry)."""
    return "n%dz%db%d-g%dx%dx%d-lastx%d-mt%d-kc%d-tailz%d-tailm%d" % (
        geo["ncells"], geo["zDim"], geo["b_zDim"], *geo["grid"], geo["last_x"], geo["mt_per_wg"], geo["chunks"], geo["tail_z"], geo["tail_m"])


def _rz_fused(nc, nz, b):
    spec = ["rz_advection", {"num_cells": nc, "zDim": nz}, {"b_zDim": b} if b else {}]
    return ("rz-fused-" + rz_fwd_id(cases.rz_forward_launch_geometry(make_case(spec))), spec, {}, "f64")


# (name, spec, per-handle switches, storage): spec as tests/child_run.make_case takes it
FWD_CASES = (
    [("z32b%d" % b, _z(32, b), {}, "f64") for b in (16, 17, 22, 32)]
    + [("z32b%d-valu" % b, _z(32, b), {"SX_SBW_MFMA": "0"}, "f64") for b in (17, 32)]
    + [("z32b%d-valu-pf" % b, _z(32, b), {"SX_SBW_MFMA": "0", "SX_SBW_PF": "1"}, "f64") for b in (17, 32)]
    + [("z64b%d" % b, _z(64, b), {}, "f64") for b in (43, 48, 49, 64)]
    # b_zDim <= zDim (sx_create), so at 32 / 64 levels the VALU kernels run only with SX_SBW_MFMA=0
    + [("z64b43-valu", _z(64, 43), {"SX_SBW_MFMA": "0"}, "f64"), ("z64b64-valu-pf", _z(64, 64), {"SX_SBW_MFMA": "0", "SX_SBW_PF": "1"}, "f64")]
    + [("z128b%d" % b, _z(128, b), {}, "f64") for b in (80, 86, 96, 97, 128)]
    + [("z128b86-L64x7", _z(128, 86, nc=7, L=64), {}, "f64")]                 # K2 44: two column groups of 32, the second 12 wide
    # the generic k_sbz: zDim not 32 / 64 / 128, b_zDim not a multiple of 4
    + [("z%db%d" % (nz, b), _z(nz, b), {}, "f64") for nz, b in ((16, 11), (20, 13), (33, 23))]
    # K2 tails: 16-point rings above (K2 16 < bw); a 3-cell patch of 64-point rings (kmax 9: K2 20); 512-point rings (K2 68)
    + [("z64b43-L64x3", _z(64, 43, nc=3, L=64), {}, "f64"), ("z32b22-L512x11", _z(32, 22, nc=11, L=512), {}, "f64")]
    # segmentation: cps 2 (< the 3-cell warm-up) up to 64 cells, 6 above; last segments of 1 cell at 3, 5, 7 and 65
    + [("z32b22-n%d" % n, _z(32, 22, nc=n), {}, "f64") for n in (3, 5, 7, 64, 65, 66)]
    # f32x: fp32-stored ring spectra
    + [("f32x-z%db%d" % (nz, b), _z(nz, b), {}, "f32x") for nz, b in ((32, 22), (64, 43), (128, 86))]
    # other geometries: RL (k_sb), fused RZ (k_rz_forward), and RZ through the general path (k_sbw_mfma with K2 = 1)
    + [("rl-L16", ["rl_advection", {"num_cells": 6, "ring_L": 16}, {}], {}, "f64"),
       ("rz-fused", ["rz_advection", {"num_cells": 7, "zDim": 20}, {}], {}, "f64"),
       ("rz-general", ["rz_advection", {"num_cells": 7, "zDim": 32}, {"b_zDim": 21}], {"SX_RZ_FUSED": "0"}, "f64")]
    # k_rz_forward beyond one node tile, one K chunk and one mode group: 16 / 17 and 32 / 33 nodes (the 19-cell weight window, both
    # halves of 8 nodes, zero weights outside the tile), a second chunk of 64 levels, a second group of 4 mode tiles, 4 chunks
    + [_rz_fused(nc, nz, b)
       for nc, nz, b in ((13, 20, None), (14, 20, None), (29, 20, None), (30, 20, None), (7, 64, 64), (7, 65, 65), (7, 128, 80), (5, 256, 100))]
)

# tiles of a patch: each tile's B against forward_xp of its own points
TILE_CASES = [("native-z32b22-2tiles", _z(32, 22, nc=10, L=None), 2), ("z64b43-L32-3tiles", _z(64, 43, nc=12, L=32), 3),
              # fused RZ: tiles of 14, 13 and 13 cells, cell0 != 0, weight windows that reach outside the tile on both sides
              ("rz-fused-z20-3tiles", ["rz_advection", {"num_cells": 40, "zDim": 20}, {}], 3)]

# SX_DEFER_DIAG=1 (one-tile HRBL on the FFT path): a step covers the prognostic variables (v_cnt = V - 1); reading B then
# brings the diagnostic one up to date (v_lo = V - 1, v_cnt = 1)
DEFER_SPEC = ["rlz_hrbl", {"num_cells": 6, "zDim": 64, "ring_L": 32}, {}]

# vertical inverse at the b_zDim boundaries of launch_sb's kernel choice, k_colmat at 20 levels, and two column groups (K2 68)
ZINV_SHAPES = [(32, b, 4, 16) for b in (16, 17, 22, 32)] + [(64, b, 4, 16) for b in (43, 48, 49, 64)] + \
              [(128, b, 4, 16) for b in (80, 86, 96, 97, 128)] + [(20, 13, 4, 16), (32, 22, 11, 512)]


def _f32x_ok(nz, b):
    """sx_create accepts storage_f32 = 2 only where the matrix-core B kernel exists."""
    return nz in (32, 64, 128) and (b <= 64 if nz <= 64 else b <= 96)


ZINV_CASES = [(nz, b, nc, L, st) for nz, b, nc, L in ZINV_SHAPES for st in ("f64", "f32x") if st == "f64" or nz in (32, 64, 128)]


def _compact(kernel):
    return kernel.replace(", ", ",").replace(" ", "")


def sb_id(geo):
    """Test id fragment of one launch_sb launch."""
    if "bw" not in geo:
        return _compact(geo["kernel"]) + "-K2_%d" % geo["K2"]
    if geo["kernel"] == "k_sbz":
        return "k_sbz-K2_%d-tail%d" % (geo["K2"], geo["tail"])
    s = "%s-t%d-bw%d-nseg%d-cps%d-segs%d-last%d-tail%d" % (_compact(geo["kernel"]), geo["threads"], geo["bw"], geo["nseg"],
                                                            geo["cps"], geo["segs"], geo["last"], geo["tail"])
    if "MT" in geo:
        s += "-MT%d-mhalf%d-nmt%s" % (geo["MT"], geo["mhalf"], "".join(map(str, geo["nmt"])))
    return s


def zinv_id(geo):
    return "none" if geo is None else "%s-gx%d-tail%d" % (_compact(geo["kernel"]), geo["grid_x"], geo["tail"])


def _fwd_id(name, spec, env, storage):
    return name + "-" + sb_id(cases.sb_launch_geometry(make_case(spec), env, storage))


# ----------------------------------------------------------------------------- process-wide switches (child processes)
# SX_ZINV_CT and SX_SBW_SEG / SX_SBW_T256 are read once per process; each child sets one value of each and runs these shapes
SWITCH_SPECS = [_z(128, 86, nc=10), _z(128, 86, nc=10) + ["f32x"], _z(64, 43, nc=10), _z(64, 43, nc=10) + ["f32x"],
                _z(32, 22, nc=10)]
SWITCH_ENVS = [{"SX_ZINV_CT": "1", "SX_SBW_SEG": "1"}, {"SX_ZINV_CT": "2", "SX_SBW_SEG": "3"},
               {"SX_ZINV_CT": "4", "SX_SBW_SEG": "4"}]                   # SEG 4 at 10 cells: cps 3, a last segment of 1 cell
T256_SPECS = [_z(64, 49), _z(64, 64), _z(64, 43) + ["f32x"]]
T256_ENV = {"SX_SBW_T256": "0"}


def _storage(spec):
    return spec[3] if len(spec) > 3 else "f64"


def _switch_id(env, specs):
    parts = ["%s=%s" % kv for kv in sorted(env.items())]
    for spec in specs:
        case, st = make_case(spec), _storage(spec)
        sb = cases.sb_launch_geometry(case, env, st)
        parts.append("z%d%s:%s:zinv=%s" % (case["grid"]["zDim"], "f32x" if st == "f32x" else "",
                                           sb_id(sb), zinv_id(cases.zinv_launch_geometry(case, env, st))))
    return "|".join(parts)


# ----------------------------------------------------------------------------- host checks (no GPU)
def test_the_cases_reach_every_launcher_branch():
    """Every instantiation launch_sb and launch_zinv can pick is launched by at least one case of this file, and every switch
    case changes the launch it is about (a default would prove nothing)."""
    sb, zi = set(), set()
    for _, spec, env, st in FWD_CASES:
        sb.add(cases.sb_launch_geometry(make_case(spec), env, st)["kernel"])
    for _, spec, _n in TILE_CASES:
        sb.add(cases.sb_launch_geometry(make_case(spec))["kernel"])
    for nz, b, nc, L, st in ZINV_CASES:
        zi.add(cases.zinv_launch_geometry(make_case(_z(nz, b, nc, L)), None, st)["kernel"])
    for env, specs in [(e, SWITCH_SPECS) for e in SWITCH_ENVS] + [(T256_ENV, T256_SPECS)]:
        for spec in specs:
            case, st = make_case(spec), _storage(spec)
            sb.add(cases.sb_launch_geometry(case, env, st)["kernel"])
            zi.add(cases.zinv_launch_geometry(case, env, st)["kernel"])
    assert sb == cases.SB_KERNELS, (cases.SB_KERNELS - sb, sb - cases.SB_KERNELS)
    assert zi == cases.ZINV_KERNELS, (cases.ZINV_KERNELS - zi, zi - cases.ZINV_KERNELS)
    # the switches really change the launch
    for env in SWITCH_ENVS:
        ct, seg = int(env["SX_ZINV_CT"]), int(env["SX_SBW_SEG"])
        for spec in SWITCH_SPECS:
            case, st = make_case(spec), _storage(spec)
            assert cases.sb_launch_geometry(case, env, st)["nseg"] == seg
            z = cases.zinv_launch_geometry(case, env, st)
            nz = case["grid"]["zDim"]
            assert z["CT"] == (ct if nz == 128 else 2 if nz == 64 and ct == 2 else 1)
    assert cases.sb_launch_geometry(make_case(SWITCH_SPECS[2]), SWITCH_ENVS[2])["last"] == 1
    for spec in T256_SPECS:
        case, st = make_case(spec), _storage(spec)
        assert cases.sb_launch_geometry(case, None, st)["threads"] == 256
        assert cases.sb_launch_geometry(case, T256_ENV, st)["threads"] == 512
    # the geometry this file exists for: short segments, 1-cell last segments, K2 tails, partial last row tiles
    geos = [cases.sb_launch_geometry(make_case(spec), env, st) for _, spec, env, st in FWD_CASES]
    assert any(g_.get("last") == 1 for g_ in geos) and any(g_.get("cps", 9) < 3 for g_ in geos)
    assert any(g_.get("cps", 0) >= 6 for g_ in geos) and any(g_.get("tail", 0) not in (0, g_.get("K2")) for g_ in geos)
    assert {g_["MT"] for g_ in geos if "MT" in g_} == {1, 2, 3, 4, 5, 6}            # every row-tile count, partial last tiles


# ----------------------------------------------------------------------------- GPU checks
def _b_errors(og, vals, B, storage, cell0=0, ncells=None):
    """max over entries of |B - B_xp| / (2^-53 scale), after the f32x allowance; entries of zero scale must be exactly zero."""
    Bx, Sx = O.forward_xp(og, vals, cell0, ncells)
    assert B.shape == Bx.shape, (B.shape, Bx.shape)
    assert np.isfinite(B).all()
    zero = Sx == 0
    assert not np.any(B[zero]), "entries outside every ring's wavenumbers must be zero"
    d = np.abs(B.astype(O.XP) - Bx)
    if storage == "f32x":
        d = np.maximum(d - O.XP(2.0 ** -24) * Sx, 0)
    c = np.where(zero, 0, d / np.where(zero, 1, Sx)) / O.XP(2.0 ** -53)
    return float(c.max()), np.unravel_index(int(c.argmax()), c.shape)


def _where(og, idx, ncells):
    nbt, K2t = ncells + 3, og.tile_K2(0, ncells)
    return "var %d z-mode %d block %d node %d" % (idx[1], idx[0] // nbt // K2t, (idx[0] // nbt) % K2t, idx[0] % nbt)


def _check_b(case, vals, B, storage, label, cell0=0, ncells=None):
    og = cases.oracle_grid(case)
    n = og.nc if ncells is None else ncells
    c, idx = _b_errors(og, vals, B, storage, cell0, n)
    print("\n%s: worst c = %.2f at %s" % (label, c, _where(og, idx, n)))
    assert c <= C_B, (label, c, _where(og, idx, n))


def _check_a(case, B, A):
    """A after splineTransform! vs the fp64 oracle's dense solve of the same B (one tile: tile layout == patch layout)."""
    nb = case["grid"]["num_cells"] + 3
    ref = cases.dense_spline_transform(case, B)
    e = cases.rel_err_per_column(A, ref, nb)
    assert np.isfinite(A).all() and e.max() <= TOL_A, ("A per column", int(e.argmax()), e.max())


def _rings(og):
    return sorted({0, og.rDim // 2, og.rDim - 1})


def _check_inverse(case, A, phys, storage, label):
    og = cases.oracle_grid(case)
    rings = _rings(og)
    e_hip = cases.slot_errors_vs_extended(og, phys, A, rings)
    e_orc = cases.slot_errors_vs_extended(og, og.inverse(A), A, rings)
    cases.report_slots(label, og, [("HIP vs extended precision", e_hip), ("fp64 oracle vs extended precision", e_orc)])
    if storage == "f32x":
        assert (e_hip <= 2.0 * e_orc + F32_SLOT).all(), (e_hip, e_orc)
        assert e_hip.max() > 1e-12, "the fp32 intermediates were not in the path"
    else:
        assert (e_hip <= 2.0 * e_orc + 2e-15).all(), (e_hip, e_orc)


@pytest.mark.gpu
@pytest.mark.parametrize("name,spec,env,storage", FWD_CASES, ids=[_fwd_id(*c) for c in FWD_CASES])
def test_forward_projection_against_extended_precision(monkeypatch, name, spec, env, storage):
    """Random values -> spectralTransform! -> B entry by entry against forward_xp; then splineTransform! -> A per column against
    the oracle's solve of that B."""
    import scythe_jl_amd as S
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = make_case(spec)
    g = S.Grid(*cases.hip_params(case, storage))
    vals, _ = forward_inputs(g.N, g.V, int(g.dims.s_patch))
    g.set_physical_values(vals)
    g.spectralTransform_()
    B = g.spectral
    g.splineTransform_()
    A = g.patchSpectral
    g.close()
    _check_b(case, vals, B, storage, _fwd_id(name, spec, env, storage))
    _check_a(case, B, A)


@pytest.mark.gpu
@pytest.mark.parametrize("name,spec,ntiles", TILE_CASES, ids=[n for n, _, _ in TILE_CASES])
def test_forward_projection_of_each_tile(name, spec, ntiles):
    """Each tile of a patch split into 2 / 3 tiles: its B against forward_xp of its own points (tile-level K2, cell offset)."""
    import scythe_jl_amd as S
    case = make_case(spec)
    gp, mp = cases.hip_params(case)
    for t, (c0, n) in enumerate(cases.even_tiles(case["grid"]["num_cells"], ntiles)):
        g = S.Grid(gp, mp, tile_cell0=c0, tile_num_cells=n, tile_num=t)
        vals = np.random.default_rng(20 + t).standard_normal((g.N, g.V))
        g.set_physical_values(vals)
        g.spectralTransform_()
        B = g.spectral
        g.close()
        geo = cases.sb_launch_geometry(case, tile=(c0, n))
        shape = sb_id(geo) + ("-" + rz_fwd_id(geo) if geo["kernel"] == "k_rz_forward" else "")
        _check_b(case, vals, B, "f64", "%s tile %d (cells %d..%d) %s" % (name, t, c0, c0 + n - 1, shape), c0, n)


@pytest.mark.gpu
def test_forward_projection_with_the_deferred_diagnostic_variable(monkeypatch):
    """SX_DEFER_DIAG=1: the step's forward path covers variables 0..V-2 (v_cnt = V - 1: fewer column groups, other segments), and
    reading B runs it for variable V-1 alone (v_lo = V - 1).  After one step, B of all variables against forward_xp of var_np1,
    the values the step transformed."""
    case = make_case(DEFER_SPEC)
    monkeypatch.setenv("SX_DEFER_DIAG", "1")
    hip = cases.HipModel(case)
    hip.step()
    t = hip.run.tiles[0]
    vals = t.var_np1
    B = t.spectral
    hip.run.close()
    V = len(case["grid"]["vars"])
    ids = "%s | %s" % (sb_id(cases.sb_launch_geometry(case, v_cnt=V - 1)), sb_id(cases.sb_launch_geometry(case, v_cnt=1)))
    _check_b(case, vals, B, "f64", "SX_DEFER_DIAG=1 " + ids)


def _zinv_id(c):
    nz, b, nc, L, st = c
    case = make_case(_z(nz, b, nc, L))
    ok = st == "f64" or _f32x_ok(nz, b)
    return "z%db%d-L%dx%d-%s-%s" % (nz, b, L, nc, st, zinv_id(cases.zinv_launch_geometry(case, None, st)) if ok else "refused")


@pytest.mark.gpu
@pytest.mark.parametrize("nz,b,nc,L,storage", ZINV_CASES, ids=[_zinv_id(c) for c in ZINV_CASES])
def test_vertical_inverse_and_three_steps(nz, b, nc, L, storage):
    """tileTransform! of random A: derivative slots on sampled rings against inverse_xp, no less accurate than the fp64 oracle
    (check_full's rule: HIP <= 2 x oracle + 2e-15; f32x: + 4 x 2^-24 for the fp32-stored Az and planes).  Then 3 model steps
    against the C oracle: A coefficients and values within 1e-10 (f32x 1e-5).  An f32x shape that sx_create refuses must be refused with its message."""
    import scythe_jl_amd as S
    case = make_case(_z(nz, b, nc, L))
    if storage == "f32x" and not _f32x_ok(nz, b):
        with pytest.raises(S.ScytheHipError, match="storage_f32 = 2"):
            S.Grid(*cases.hip_params(case, storage))
        return
    g = S.Grid(*cases.hip_params(case, storage))
    _, A = forward_inputs(g.N, g.V, int(g.dims.s_patch))
    g.set_patch_spectral_a(A)
    g.tileTransform_()
    phys = g.physical
    g.close()
    _check_inverse(case, A, phys, storage, _zinv_id((nz, b, nc, L, storage)))
    # the state after 3 steps, as check_full compares it: A coefficients and the value slot (derivative slots amplify the last-bit
    # differences of two correct fp64 states by up to zDim^4; their accuracy is what the slot check above measures)
    hip, orc = cases.HipModel(case, storage=storage), cases.OracleModel(case)
    for _ in range(3):
        hip.step()
        orc.step()
    a, o = hip.physical(), orc.physical()
    eA, eu = cases.rel_err(hip.A, orc.A), cases.rel_err_per_var(a[:, :, :1], o[:, :, :1])
    hip.run.close()
    print("3 steps vs oracle: A %.2e, values %.2e" % (eA, eu))
    assert np.isfinite(a).all()
    assert max(eA, eu) < (F32_MODEL if storage == "f32x" else TOL), (eA, eu)


def _check_forward_job(specs, got, label):
    for i, spec in enumerate(specs):
        case, st = make_case(spec), _storage(spec)
        og = cases.oracle_grid(case)
        vals, A = forward_inputs(og.tile_npoints(0, og.nc), og.V, og.S_patch())
        _check_b(case, vals, got["b%d" % i], st, "%s case %d" % (label, i))
        _check_a(case, got["b%d" % i], got["a%d" % i])
        _check_inverse(case, A, got["phys%d" % i], st, "%s case %d" % (label, i))


@pytest.mark.gpu
@pytest.mark.parametrize("env", SWITCH_ENVS, ids=[_switch_id(e, SWITCH_SPECS) for e in SWITCH_ENVS])
def test_process_wide_column_tiles_and_segments(tmp_path, env):
    """SX_ZINV_CT (column tiles per wave of the vertical inverse: 1 / 2 / 4 at 128 levels, 2 at 64 on request) and SX_SBW_SEG
    (segments per column group) in a fresh child: B, A and the derivative slots against the extended-precision references."""
    got = run_in_child(tmp_path, {"kind": "forward", "cases": SWITCH_SPECS}, env)
    _check_forward_job(SWITCH_SPECS, got, _switch_id(env, SWITCH_SPECS))


@pytest.mark.gpu
def test_process_wide_512_thread_sbw(tmp_path):
    """SX_SBW_T256=0 at zDim 64: k_sbw_mfma<64> (512 threads, 64 blocks, waves 0-3 own the first mhalf row tiles, waves 4-7 the
    rest) at b_zDim 49 and 64, and its fp32 form; the same references as above."""
    got = run_in_child(tmp_path, {"kind": "forward", "cases": T256_SPECS}, T256_ENV)
    _check_forward_job(T256_SPECS, got, _switch_id(T256_ENV, T256_SPECS))
