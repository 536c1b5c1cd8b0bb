"""sx_derive on the GPU: the values k_derive writes bitwise against the float64 twin of tests/derive.py for programs of exactly rounded
operations and within the counted bound of the longdouble twin for every operation and for the thermodynamic programs, the
companion's coefficients bitwise against the existing path, the same arithmetic as the model, the bystanders, a refused call, the
compositions (freezing_level, minimum_pressure, crossings of the derived speed against wind_radii) and the bookkeeping.  Shapes are tests/test_gpu_project.py's."""
import numpy as np
import pytest

from tests import cases
from tests import derive as DV
from tests import project as PJ
from tests.test_derive import assert_physical, euler_state, every_operation, exact_programs
from tests.test_gpu_project import R0, SHAPES, _bits, _existing_path, _source, _within_bar

pytestmark = pytest.mark.gpu

EULER = {"euler8_12": dict(num_cells=8, zDim=12), "euler3_9": dict(num_cells=3, zDim=9)}      # 288 points; 81 points, odd


def _held(got, fp, data, r, z, ref, what, outs=None):
    """|got - values_xp| <= bound for every output, off the masked points (at most 1 % of the case); prints the worst ratio"""
    truth, bnd = DV.bound(fp, data, r, z, ref)
    keep = ~DV.mask(fp, truth, bnd)
    assert keep.mean() >= 0.99, (what, keep.mean())
    for v, k in enumerate(fp.reg_dst):
        err = np.abs(got[:, v] - truth[k]).astype(np.float64)[keep]
        b = bnd[k][keep]
        nan = np.isnan(truth[k].astype(np.float64))[keep]
        assert np.array_equal(np.isnan(got[:, v][keep]), nan), (what, fp.names[v])
        ratio = np.max(np.where(nan, 0.0, np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))), initial=0.0)
        print("%s %s: worst |got - xp| / bound = %.3g" % (what, fp.names[v], ratio))
        assert ratio <= 1.0, (what, fp.names[v], ratio)
    return truth


def _coords(tile, gp):
    import scythe_jl_amd as S
    pts = S.getGridpoints(tile)
    pts = pts.reshape(len(pts), -1)
    return pts[:, 0], (pts[:gp.zDim, -1] if "Z" in gp.geometry else None)


@pytest.mark.parametrize("source", ["physical", "state"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_values_and_transform(shape, source):
    import scythe_jl_amd as S
    gp, og, tile, r, data = _source(shape, source)
    _, z = _coords(tile, gp)
    tile.enable_timers(True)
    # 1. exactly rounded operations: bitwise, NaN and Inf included (random normal data: radicands and denominators near zero)
    outs = exact_programs(gp)
    fp = S.pack_function_program(gp, outs)
    dst = S.companion_grid(gp, names=list(outs), **R0)
    assert tile.derive(fp, dst, source) is dst
    want = DV.values64(fp, data, r, z)[fp.reg_dst].T
    got = dst.var_np1
    assert _bits(got.T) == _bits(want.T), "%s %s: var_np1 of the companion" % (shape, source)
    # 6. one launch per call, and the bytes of the formula
    assert tile.timers()["k_derive"][1] == 1
    planes = sorted({(int(q[3 + f]), int(q[7 + f])) for q in fp.terms for f in range(int(q[2]))})
    assert tile.kernel_bytes("k_derive") == sum(4.0 if gp.storage == "f32" and s else 8.0 for _, s in planes) * tile.N + 8.0 * len(outs) * tile.N
    # 2. transform, bitwise against the existing path, whose own repeatability is the premise (finite values only reach it)
    fin = S.pack_function_program(gp, {"speed": outs["speed"], "sel": outs["sel"]})
    two = S.companion_grid(gp, names=["speed", "sel"], **R0)
    A = tile.derive(fin, two, source).patchSpectral
    wf = DV.values64(fin, data, r, z)[fin.reg_dst].T
    assert np.isfinite(wf).all() and _bits(two.var_np1.T) == _bits(wf.T)
    E1, E2 = _existing_path(gp, ["speed", "sel"], wf), _existing_path(gp, ["speed", "sel"], wf)
    if _bits(E1) == _bits(E2):
        assert _bits(A) == _bits(E1), "%s %s: A against set_physical_values + transforms" % (shape, source)
    else:
        print("%s: the existing path does not repeat bitwise; held at the parity bar instead" % shape)
        assert np.max(np.abs(A - E1)) <= PJ.bar(E1)
    # 1b. every operation once (no reference state here: REF and the composites run on the Euler cases), within the bound
    ev = S.pack_function_program(gp, every_operation(("h", "u", "v"), z is not None))
    many = S.companion_grid(gp, names=ev.names, **R0)
    _held(tile.derive(ev, many, source).var_np1, ev, data, r, z, None, "%s %s" % (shape, source))
    for g in (dst, two, many, tile):
        g.close()


def _euler(name):
    """an Euler_test tile holding the perturbed state, and what the programs read of it"""
    import scythe_jl_amd as S
    case = cases.rz_euler(**EULER[name])
    gp, mp = cases.hip_params(case)
    pts, vals, ref = euler_state(case)
    tile = S.Grid(gp, mp)
    tile.set_physical_values(vals)
    tile.spectralTransform_()
    tile.splineTransform_()
    tile.tileTransform_()
    return case, gp, mp, tile, ref


@pytest.mark.parametrize("source", ["physical", "state"])
@pytest.mark.parametrize("name", list(EULER))
def test_thermodynamic_programs(name, source):
    """every thermo_programs output (nine in one call; theta_e, which fills a program by itself, in a second) and every operation with
    REF and the composites, within the bound; T and p are the model's arithmetic; repeatable; independent of the other outputs"""
    import scythe_jl_amd as S
    case, gp, mp, tile, ref = _euler(name)
    r, z = _coords(tile, gp)
    data = tile.physical if source == "physical" else tile.var_np1
    tp = S.thermo_programs(mp)
    nine = {k: tp[k] for k in tp if k != "theta_e"}
    results = {}
    for outs in (nine, {"theta_e": tp["theta_e"]}, every_operation(("s", "xi", "mu"), True, tp)):
        fp = S.pack_function_program(gp, outs)
        dst = S.companion_grid(gp, names=fp.names, **R0)
        got = tile.derive(fp, dst, source).var_np1
        truth = _held(got, fp, data, r, z, ref, "%s %s" % (name, source))
        if "T" in outs:
            assert_physical(truth[fp.reg_dst[fp.names.index("T")]], truth[fp.reg_dst[fp.names.index("p")]])
        results[tuple(outs)] = (got, dst.patchSpectral)
        # two calls agree bitwise
        dst.set_physical_values(np.zeros_like(got))
        again = tile.derive(fp, dst, source)
        assert _bits(again.var_np1, again.patchSpectral) == _bits(*results[tuple(outs)])
        dst.close()
    # one output alone and among nine: bitwise the same values and coefficients
    got9, A9 = results[tuple(nine)]
    for k in ("T", "p"):
        one = S.companion_grid(gp, names=[k], **R0)
        tile.derive({k: tp[k]}, one, source)
        j = list(nine).index(k)
        assert _bits(one.var_np1[:, 0], one.patchSpectral[:, 0]) == _bits(got9[:, j], A9[:, j]), k
        one.close()
    tile.close()


def test_bystanders_and_a_refused_call():
    """the source stays bitwise as it is and a stepped run does not notice the calls; a refused call leaves the destination alone"""
    import scythe_jl_amd as S
    case = cases.rz_euler(**EULER["euler8_12"])
    plain, busy = cases.HipModel(case), cases.HipModel(case)
    tile = busy.run.tiles[0]
    tp = S.thermo_programs(busy.mp)
    for _ in range(3):
        plain.step()
        busy.step()
        tile.tileTransform_()
        before = (tile.get_state(), tile.physical, tile.patchSpectral, tile.var_np1, tile.spectral)
        comp = busy.run.derive({k: tp[k] for k in ("T", "p", "theta")})
        busy.run.derive({"T": tp["T"]}, source="state")
        assert _bits(*before) == _bits(tile.get_state(), tile.physical, tile.patchSpectral, tile.var_np1, tile.spectral)
    assert _bits(plain.run.tiles[0].get_state(), plain.physical()) == _bits(tile.get_state(), busy.physical())
    state0 = (comp.patchSpectral, comp.var_np1, comp.spectral)

    def refused(match, program, into=comp, src=tile, **kw):
        with pytest.raises(S.ScytheHipError, match=match):
            src.derive(program, into, **kw)
        assert _bits(comp.patchSpectral, comp.var_np1, comp.spectral) == _bits(*state0), match
    three = {k: tp[k] for k in ("T", "p", "theta")}
    refused("the destination is the source", {k: tp["T"] for k in "abcde"}, into=tile)
    with pytest.raises(ValueError, match="1 outputs for the 3 variables"):
        tile.derive({"T": tp["T"]}, comp)
    refused("SX_REDUCE_STATE holds the values only", {"a": ("sqrt", [(1.0, 0, [("s", "r")])]), "b": "r", "c": "z"}, source="state")
    other = S.Grid(S.GridParameters(geometry="RZ", xmin=0.0, xmax=2.0e4, num_cells=8, zmin=0.0, zmax=1.0e4, zDim=12, b_zDim=12,
                                    vars={"s": 1, "xi": 2, "mu": 3}), None)
    refused("the source has no reference state", three, src=other)
    other.close()
    plain.run.close()
    busy.run.close()


@pytest.mark.parametrize("eq", ["Euler_test", "rainfall_test"])
def test_freezing_level_and_minimum_pressure(eq):
    """agreement with the same quantity formed on the host, at the parity bar: height_where on a companion filled with the twin's T,
    and the minimum of the twin's p.  The Euler case stays below 273.15 K throughout, so its entropy profile is raised by 40 J / (kg K)
    here (about 15 K): every column then has a freezing level.  The rainfall case (300 K at the ground) has one as it is."""
    import scythe_jl_amd as S
    from tests import rainfall
    if eq == "Euler_test":
        case = cases.rz_euler(**EULER["euler8_12"])
        case["par"]["ref_state"]["sbar"][:, 0] += 40.0
    else:
        case = rainfall.rz_rain(num_cells=8, zDim=12)
    hip = cases.HipModel(case)
    hip.step()
    tile, gp = hip.run.tiles[0], hip.gp
    columns = np.linspace(1.0e3, 1.9e4, 7).reshape(-1, 1)
    got = hip.run.freezing_level(columns)
    p_min, where = hip.run.minimum_pressure()
    r, z = _coords(tile, gp)
    rs = case["par"]["ref_state"]
    ref = np.stack([rs[k].T for k in ("sbar", "xibar", "mubar")])
    tp = S.thermo_programs(hip.mp)
    fp = S.pack_function_program(gp, {"T": tp["T"], "p": tp["p"]})
    twin = DV.values64(fp, tile.physical, r, z, ref)[fp.reg_dst]
    host = S.companion_grid(gp, names=["T"], **R0)
    host.set_physical_values(twin[0][:, None])
    host.spectralTransform_()
    host.splineTransform_()
    want = hip.run.height_where([(0, 1.0, 0, [("T", "")])], 273.15, columns, grid=host)
    assert np.isfinite(want).all() and np.array_equal(np.isnan(got), np.isnan(want))
    _within_bar(got, want, "freezing_level")
    k = int(np.argmin(twin[1]))
    _within_bar(p_min, twin[1][k], "minimum_pressure")
    pts = S.getGridpoints(tile)
    at = int(np.nonzero((pts == where).all(axis=1))[0][0])
    assert abs(twin[1][at] - twin[1][k]) <= 1e-10 * twin[1][k]          # columns mirrored about the bell tie up to rounding
    host.close()
    hip.run.close()


def test_crossings_of_the_derived_speed_against_wind_radii():
    """crossings of the derived `speed` companion at a threshold against wind_radii's radii for the same threshold, on the slab set.
    wind_radii brackets the root of u^2 + v^2 - threshold^2 summed from the coefficients of u and v; the companion holds the
    projection of sqrt(u^2 + v^2) at the gridpoints, whose root differs by the projection's error between rings.  Both brackets are
    tol DX wide, far below that, so the two are compared at the ring spacing: the largest gap between neighbouring rings."""
    import scythe_jl_amd as S
    hip = cases.HipModel(cases.rl_slab(num_cells=6))
    hip.step()
    thr, n = 20.0, 16
    wr = hip.run.wind_radii("u", "v", [thr], n_azimuths=n, quadrants=False)
    comp = hip.run.derive({"speed": S.function_programs(hip.mp)["speed"]})
    res = comp.crossings([(0, 1.0, 0, [("speed", "")])], [thr], wr.azimuths[:, None], max_cross=16)
    falling = np.where(res.dir[:, 0, :] == -1, res.radius[:, 0, :], -np.inf).max(axis=0)
    got = np.where(np.isfinite(falling), falling, np.nan)
    rings = np.unique(S.getGridpoints(hip.run.tiles[0])[:, 0])
    spacing = float(np.diff(rings).max())
    print("wind radii %s\nfrom the derived speed %s\nworst difference %.3g of the ring spacing %.4g"
          % (np.array2string(wr.radii[0], precision=1), np.array2string(got, precision=1), float(np.nanmax(np.abs(got - wr.radii[0])) / spacing), spacing))
    assert not np.isnan(wr.radii[0]).any() and not np.isnan(got).any()
    assert np.all(np.abs(got - wr.radii[0]) <= spacing)
    hip.run.close()
