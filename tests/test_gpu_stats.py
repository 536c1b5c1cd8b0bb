"""sx_stats_* on the GPU against the twin of tests/stats.py: MAX, MIN, their times and DURATION bitwise, SUM within the bound derived
there; the order rules, independence of tiling and of the other outputs, "reads only", the set driven by ModelRun.step() (both
schedules, graph replay, checkpoints, cadence), refusals and lifecycle, and the two conveniences.  Shapes are the smallest with
every index path: an odd zDim (one point per lane), an even one (two), zDim that does not divide 256, rings shorter than a wave,
a ring of two pieces, more than one workgroup."""

import numpy as np
import pytest

from tests import cases
from tests import stats as ST
from tests.test_stats import SAMPLES

pytestmark = pytest.mark.gpu

# (maker, its arguments, storage): R 12 cells; RZ 9 x 12 levels; RL 9 cells, native rings; RL with a ring of two pieces (8448 points
# are 33 strides of 256); RLZ 9 x 10 native; RLZ 9 x 9 native (odd zDim: the one-point-per-lane kernel); RLZ 6 x 32 x 32 uniform; f32
SHAPES = {
    "R": ("r_bcs", dict(num_cells=12), "f64"),
    "RZ": ("rz_advection", dict(num_cells=9, zDim=12), "f64"),
    "RL": ("rl_slab", dict(num_cells=9), "f64"),
    "RL-long": ("rl_advection", dict(num_cells=3, ring_L=8448), "f64"),
    "RLZ": ("rlz_hrbl", dict(num_cells=9, zDim=10), "f64"),
    "RLZ-odd": ("rlz_advection", dict(num_cells=9, zDim=9), "f64"),
    "RLZ-uniform": ("rlz_hrbl", dict(num_cells=6, zDim=32, ring_L=32), "f64"),
    "RLZ-f32": ("rlz_hrbl", dict(num_cells=6, zDim=32, ring_L=32), "f32"),
}


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _tile(shape, cell0=0, ncells=None):
    import scythe_jl_amd as S
    maker, kw, storage = SHAPES[shape]
    case = getattr(cases, maker)(**kw)
    gp, mp = cases.hip_params(case, storage)
    tile = S.Grid(gp, mp, cell0, ncells) if ncells else S.Grid(gp, mp)
    pts = S.getGridpoints(tile)
    return gp, tile, pts.reshape(len(pts), -1)


def _outputs(V, source, thr):
    """one output per op: an r^p term, a 4-factor term and an nf = 0 term among them; with source physical a derivative slot (r)"""
    s = 1 if source == "physical" else 0
    v2 = min(2, V)
    return [("sum", [(2.0, 1, [(1, 0)]), (0.5, 0, [(1, 0), (v2, s), (1, 0), (v2, 0)])]),
            ("max", [(1.0, 2, [(v2, 0)]), (-0.25, 0, [])]),
            ("min", [(1.0, 0, [(1, s)]), (3.0, -1, [(V, 0)])]),
            ("duration", [(1.0, 0, [(V, 0)])], thr)]


def _install(tile, vals, source):
    """the state of one sample; returns what the program reads"""
    tile.set_physical_values(vals)
    if source == "state":
        return vals
    tile.spectralTransform_()
    tile.splineTransform_()
    tile.tileTransform_()
    return tile.physical


def _against_twin(tile, gp, r, outputs, source, datas, what, varied=True):
    import scythe_jl_amd as S
    coef, packed, n_out, op, thr = S.pack_statistics(gp, outputs)
    ops = [o[0] for o in outputs]
    st = tile.statistics()
    samples = [(d, t, w) for d, (t, w) in zip(datas, SAMPLES)]
    twins = ST.run((coef, packed, n_out), ops, [o[2] if len(o) > 2 else None for o in outputs], samples, r)
    ratio = 0.0
    for o, (name, tw) in enumerate(zip(ops, twins)):
        if name == "sum":
            ratio = max(ratio, ST.check_sum(st.value[:, o], tw, "%s output %d" % (what, o)))
            assert np.isnan(st.time[:, o]).all()
        elif name == "duration":
            ST.check_bitwise(st.value[:, o], tw.result(), "%s duration" % what)
            ST.check_bitwise(st.value[:, o], tw.duration_exact(), "%s duration, exact" % what)
        else:
            ST.check_bitwise(st.value[:, o], tw.value, "%s %s" % (what, name))
            ST.check_bitwise(st.time[:, o], tw.time, "%s %s time" % (what, name))
            assert not varied or len(np.unique(tw.time)) > 1, what          # the extremum is not everywhere set by one sample
    hi, lo = ST.elapsed([w for _, w in SAMPLES])
    assert st.samples == len(SAMPLES) and st.elapsed == hi + lo and st.elapsed_lo == lo
    assert st.t_first == SAMPLES[0][0] and st.t_last == SAMPLES[-1][0]
    print("%s: largest |SUM - longdouble twin| / derived bound = %.3f" % (what, ratio))
    return st, twins


# the two-piece ring is there for the kernel's walk over the pieces: the source does not change that walk
@pytest.mark.parametrize("shape,source", [(sh, so) for sh in SHAPES for so in ("state", "physical") if (sh, so) != ("RL-long", "physical")])
def test_against_twin(shape, source):
    gp, tile, pts = _tile(shape)
    rng = np.random.default_rng(41)
    vals = [rng.standard_normal((tile.N, tile.V)) for _ in SAMPLES]
    first = _install(tile, vals[0], source)
    thr = float(first[5, tile.V - 1] if first.ndim == 2 else first[5, tile.V - 1, 0])      # hit exactly, by sample 0 at point 5
    outputs = _outputs(tile.V, source, thr)
    tile.set_statistics(outputs, source)
    tile.enable_timers(True)
    datas = []
    for v, (t, w) in zip(vals, SAMPLES):
        datas.append(_install(tile, v, source))
        tile.accumulate_statistics(t, w)
    st, twins = _against_twin(tile, gp, pts[:, 0], outputs, source, datas, "%s %s" % (shape, source))
    assert tile.timers()["k_stats"][1] == len(SAMPLES)
    # bytes of a sample: the planes named x N x their element size + n_out x N x 32
    planes = {(1, 0), (min(2, tile.V), 0), (tile.V, 0)} | ({(min(2, tile.V), 1), (1, 1)} if source == "physical" else set())
    plane_bytes = sum(4.0 if SHAPES[shape][2] == "f32" and s else 8.0 for _, s in planes) * tile.N
    assert tile.kernel_bytes("k_stats") == plane_bytes + 4 * tile.N * 32.0
    # the stored pair stays a pair: the blob holds (hi, lo) whose fold is the value returned
    blob = tile.get_statistics_state()
    raw = blob[-2 * 4 * tile.N:].reshape(4, 2, tile.N)
    assert _bits(raw[0, 0] + raw[0, 1]) == _bits(st.value[:, 0]) and _bits(raw[0, 1]) == _bits(st.residual[:, 0])
    assert _bits(raw[1, 0], raw[1, 1]) == _bits(st.value[:, 1], st.time[:, 1])
    tile.close()


@pytest.mark.parametrize("tiles", [1, 3])
@pytest.mark.parametrize("shape", ["RL", "RLZ"])
def test_against_twin_after_model_steps(shape, tiles):
    """1 and 3 tiles of a stepped model, both sources: every tile accumulates its own points"""
    maker, kw, storage = SHAPES[shape]
    hip = cases.HipModel(getattr(cases, maker)(**kw), num_tiles=tiles, exchange="gather", impl="lib" if tiles > 1 else "torch")
    import scythe_jl_amd as S
    for source in ("state", "physical"):
        datas = {i: [] for i in range(len(hip.run.tiles))}
        outs = None
        for k, (t, w) in enumerate(SAMPLES):
            hip.step()
            for i, tile in enumerate(hip.run.tiles):
                if source == "physical":
                    tile.tileTransform_()
                d = tile.physical if source == "physical" else tile.var_np1
                if k == 0:
                    outs = outs or _outputs(tile.V, source, float(d.reshape(len(d), tile.V, -1)[5, tile.V - 1, 0]))
                    tile.set_statistics(outs, source)
                datas[i].append(d)
                tile.accumulate_statistics(t, w)
        for i, tile in enumerate(hip.run.tiles):
            pts = S.getGridpoints(tile)
            _against_twin(tile, hip.gp, pts.reshape(len(pts), -1)[:, 0], outs, source, datas[i], "%s %d tiles, tile %d, %s" % (shape, tiles, i, source),
                          varied=False)
    hip.run.close()


def test_order_rules():
    gp, tile, pts = _tile("RLZ")
    N = tile.N
    A, B, Cn = 7, N // 2 + 1, N - 3
    times = (1.0, 2.0, 3.0, 4.0)
    rng = np.random.default_rng(43)
    vals = [rng.standard_normal((N, tile.V)) for _ in times]
    for k in range(4):
        vals[k][A, 0] = 50.0 if k in (0, 2) else -50.0 if k == 1 else 0.0      # the largest twice, the smallest once
        vals[k][B, 0] = -0.0 if k % 2 == 0 else 0.0                             # -0.0 then +0.0: a tie
    vals[1][Cn, 0] = np.nan                                                      # a NaN in sample 2 of 4
    outputs = [("max", [(1.0, 0, [(1, 0)])]), ("min", [(1.0, 0, [(1, 0)])]), ("sum", [(1.0, 0, [(1, 0)])]), ("duration", [(1.0, 0, [(1, 0)])], 0.0)]
    tile.set_statistics(outputs, "state")
    empty = tile.statistics()
    assert empty.samples == 0 and np.isnan(empty.value[:, :2]).all() and np.isnan(empty.time[:, :2]).all() and (empty.value[:, 2:] == 0).all()
    assert np.isnan(empty.t_first) and np.isnan(empty.t_last) and empty.elapsed == 0.0
    for v, t in zip(vals, times):
        tile.set_physical_values(v)
        tile.accumulate_statistics(t, 1.0)
    st = tile.statistics()
    import scythe_jl_amd as S
    coef, packed, n_out, _, _ = S.pack_statistics(gp, outputs)
    twins = ST.run((coef, packed, n_out), ["max", "min", "sum", "duration"], [None, None, None, 0.0], [(v, t, 1.0) for v, t in zip(vals, times)], pts[:, 0])
    for o in (0, 1):
        ST.check_bitwise(st.value[:, o], twins[o].value, "order rules, output %d" % o)
        ST.check_bitwise(st.time[:, o], twins[o].time, "order rules, time %d" % o)
    assert st.value[A, 0] == 50.0 and st.time[A, 0] == 1.0 and st.value[A, 1] == -50.0 and st.time[A, 1] == 2.0
    assert st.value[B, 0] == 0.0 and st.time[B, 0] == 1.0 and st.value[B, 1] == 0.0 and st.time[B, 1] == 1.0
    nan = np.isnan(st.value[:, 0])
    assert nan[Cn] and nan.sum() == 1 and st.time[Cn, 0] == 2.0 and np.isnan(st.value[Cn, 1]) and st.time[Cn, 1] == 2.0
    assert np.isnan(st.value[Cn, 2]) and np.isnan(st.value[:, 2]).sum() == 1          # SUM is NaN there, and only there
    ST.check_sum(st.value[:, 2], twins[2], "order rules, sum")
    ST.check_bitwise(st.value[:, 3], twins[3].result(), "order rules, duration")
    assert st.value[Cn, 3] == float(sum(vals[k][Cn, 0] >= 0.0 for k in (0, 2, 3)))    # the NaN sample is not counted
    assert st.value[B, 3] == 4.0                                                       # -0.0 >= 0.0
    tile.close()


def test_independent_of_tiling_and_of_other_outputs():
    import scythe_jl_amd as S
    gp, one, pts = _tile("RLZ")
    rng = np.random.default_rng(47)
    vals = [rng.standard_normal((one.N, one.V)) for _ in SAMPLES]
    outputs = _outputs(one.V, "state", float(vals[0][5, one.V - 1]))

    def run(tile, lo, hi, outs):
        tile.set_statistics(outs, "state")
        for v, (t, w) in zip(vals, SAMPLES):
            tile.set_physical_values(v[lo:hi])
            tile.accumulate_statistics(t, w)
        return tile.statistics()
    whole = run(one, 0, one.N, outputs)
    lay = S.PatchLayout(gp, 3)
    parts, off = [], 0
    for c0, n in zip(lay.cell0, lay.ncells):
        _, tile, _ = _tile("RLZ", c0, n)
        parts.append(run(tile, off, off + tile.N, outputs))
        off += tile.N
        tile.close()
    assert off == one.N
    cat = S.Statistics.concatenate(parts)
    assert _bits(cat.value, cat.time, cat.residual) == _bits(whole.value, whole.time, whole.residual)
    # one output alone against the same output inside a set of 16
    names = ["sum", "max", "min", "duration"]
    many = [(names[o % 4], [(1.0 + o, 0, [(1 + o % one.V, 0)]), (0.5, 1, [(1, 0), (one.V, 0)])]) + ((0.1,) if o % 4 == 3 else ()) for o in range(16)]
    full = run(one, 0, one.N, many)
    for o in (0, 5, 10, 15):
        alone = run(one, 0, one.N, [many[o]])
        assert _bits(alone.value[:, 0], alone.time[:, 0], alone.residual[:, 0]) == _bits(full.value[:, o], full.time[:, o], full.residual[:, o]), o
    one.close()


def test_reads_only():
    hip = cases.HipModel(cases.rl_advection(num_cells=6))
    run, tile = hip.run, hip.run.tiles[0]
    run.set_parcels(np.array([[1.0, 0.5], [4.0, -2.5]]), ("u", "v"))
    for _ in range(2):
        run.step()
    tile.tileTransform_()

    def snapshot():
        return _bits(tile.physical, tile.var_np1, tile.get_state(), tile.patchSpectral, *tile.parcels(), tile.get_parcel_state())
    before = snapshot()
    for source in ("state", "physical"):
        tile.set_statistics(_outputs(tile.V, source, 0.1), source)
        tile.accumulate_statistics(0.0, 0.0)
        tile.accumulate_statistics(1.0, 0.5)
        assert tile.statistics().samples == 2
    assert snapshot() == before
    run.close()


# ---- with the model ---------------------------------------------------------------------------------------------------------------
MODELS = {"RL": lambda: cases.rl_advection(num_cells=6), "HRBL": lambda: cases.rlz_hrbl(num_cells=8, zDim=32, ring_L=32)}


def _model_outputs(case):
    names = list(case["grid"]["vars"])
    u, v = names[1], names[2]
    return [("max", [(1.0, 0, [(u, ""), (u, "")]), (1.0, 0, [(v, ""), (v, "")])]), ("sum", [(1.0, 0, [(names[0], "")])]),
            ("min", [(1.0, 0, [(names[0], "")])]), ("duration", [(1.0, 0, [(v, "")])], 0.5)]


def _model_run(model, source=None, steps=6, every=1, checkpoint=None, resume=None, manual=False):
    """source None: no set.  manual: no set either; returns var_np1 after every step (and the initial one) for the twin"""
    case = MODELS[model]()
    hip = cases.HipModel(case)
    run, tile = hip.run, hip.run.tiles[0]
    seq = [tile.var_np1] if manual else None
    if resume is not None:
        run.load_checkpoint(resume)
    elif source is not None:
        run.set_statistics(_model_outputs(case), source, every=every)
    while run.t < steps:
        run.step()
        if manual:
            seq.append(tile.var_np1)
        if checkpoint is not None and run.t == 3:
            run.save_checkpoint(checkpoint)
    out = dict(A=run.patch_spectral(), state=tile.get_state(), np1=tile.var_np1, seq=seq, ts=run.model.ts, gp=hip.gp,
               stats=run.statistics() if run._stats else None, blob=tile.get_statistics_state(),
               r=run.gridpoints()[:, 0].copy(), case=case)
    run.close()
    return out


def _check_model_stats(st, ref, every):
    import scythe_jl_amd as S
    outputs = _model_outputs(ref["case"])
    coef, packed, n_out, _, _ = S.pack_statistics(ref["gp"], outputs)
    ts = ref["ts"]
    samples = [(ref["seq"][0], 0.0, 0.0)] + [(ref["seq"][t], t * ts, every * ts) for t in range(every, len(ref["seq"]), every)]
    twins = ST.run((coef, packed, n_out), [o[0] for o in outputs], [None, None, None, 0.5], samples, ref["r"])
    ST.check_bitwise(st.value[:, 0], twins[0].value, "swath")
    ST.check_bitwise(st.time[:, 0], twins[0].time, "swath time")
    ST.check_sum(st.value[:, 1], twins[1], "sum")
    ST.check_bitwise(st.value[:, 2], twins[2].value, "min")
    ST.check_bitwise(st.time[:, 2], twins[2].time, "min time")
    ST.check_bitwise(st.value[:, 3], twins[3].duration_exact(), "duration")
    hi, lo = ST.elapsed([w for _, _, w in samples])
    assert st.samples == len(samples) and st.elapsed == hi + lo and st.t_first == 0.0 and st.t_last == samples[-1][1]


@pytest.mark.parametrize("model,env", [("RL", {"SX_OVERLAP": "0"}), ("RL", {"SX_OVERLAP": "1"}), ("HRBL", {"SX_OVERLAP": "0"}),
                                       ("HRBL", {"SX_OVERLAP": "1"}), ("RL", {"SX_GRAPH": "1"})])
def test_with_the_model(model, env, monkeypatch, tmp_path):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ck = str(tmp_path / "ck.npz")
    plain = _model_run(model, manual=True)
    auto = _model_run(model, "state", checkpoint=ck)
    phys = _model_run(model, "physical")
    # the model does not see the set
    assert _bits(plain["A"], plain["state"], plain["np1"]) == _bits(auto["A"], auto["state"], auto["np1"])
    assert _bits(plain["A"], plain["state"], plain["np1"]) == _bits(phys["A"], phys["state"], phys["np1"])
    assert plain["stats"] is None and plain["blob"] is None
    # step, var_np1, twin
    _check_model_stats(auto["stats"], plain, 1)
    assert phys["stats"].samples == 7
    # a run resumed from the checkpoint of step 3 ends where the uninterrupted one does
    resumed = _model_run(model, resume=ck)
    assert _bits(resumed["blob"]) == _bits(auto["blob"]) and _bits(resumed["A"], resumed["state"]) == _bits(auto["A"], auto["state"])
    assert resumed["stats"].samples == 7
    # every = 2: samples at steps 2, 4 and 6 with weight 2 ts (and the initial one with weight 0)
    two = _model_run(model, "state", every=2)
    _check_model_stats(two["stats"], plain, 2)
    assert two["stats"].samples == 4


def test_with_the_model_launch_counts(monkeypatch):
    """nothing but k_stats is added to the step, and without a set nothing at all"""
    def counts(source):
        case = MODELS["HRBL"]()
        hip = cases.HipModel(case)
        if source:
            hip.run.set_statistics(_model_outputs(case), source, include_initial=False)
        hip.run.tiles[0].enable_timers(True)
        for _ in range(3):
            hip.run.step()
        c = {k: v[1] for k, v in hip.run.tiles[0].timers().items()}
        hip.run.close()
        return c
    c0, c1 = counts(None), counts("state")
    assert "k_stats" not in c0 and c1.pop("k_stats") == 3 and c1 == c0


def test_three_tile_run_and_csv(tmp_path):
    import scythe_jl_amd as S
    case = cases.rl_advection(num_cells=9)
    res = {}
    for tiles in (1, 3):
        hip = cases.HipModel(case, num_tiles=tiles, exchange="gather", impl="lib" if tiles > 1 else "torch")
        hip.mp.output_dir = str(tmp_path)
        hip.run.set_statistics(_model_outputs(case), "state")
        for _ in range(3):
            hip.step()
        st = hip.run.statistics()
        assert st.value.shape == (len(hip.run.gridpoints()), 4) and st.samples == 4
        path = S.write_statistics(hip.run, 3 * hip.mp.ts, names=["swath", "h_total", "h_min", "v_duration"])
        header = open(path).readline().strip().split(",")
        assert header == ["r", "l", "swath", "swath_time", "h_total", "h_min", "h_min_time", "v_duration"]
        data = np.loadtxt(path, delimiter=",", skiprows=1)
        assert _bits(data[:, :2]) == _bits(hip.run.gridpoints()) and _bits(data[:, 2], data[:, 3], data[:, 4]) == _bits(st.value[:, 0], st.time[:, 0], st.value[:, 1])
        hip.run.reset_statistics()
        assert hip.run.statistics().samples == 0
        res[tiles] = st
        hip.run.close()
    # the tiled run's state differs from the one-tile run's in the last bits (another solve): the statistics agree to that
    assert np.allclose(res[1].value[:, :3], res[3].value[:, :3], rtol=1e-9, atol=1e-12) and res[1].elapsed == res[3].elapsed


# ---- refusals and lifecycle -------------------------------------------------------------------------------------------------------
def test_refusals_and_lifecycle():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    gp, tile, pts = _tile("RZ")
    N, V = tile.N, tile.V
    rng = np.random.default_rng(53)
    tile.set_physical_values(rng.standard_normal((N, V)))
    tile.enable_timers(True)
    # no set: accumulate and reset succeed and launch nothing; get is refused
    tile.accumulate_statistics(0.0, 1.0)
    tile.reset_statistics()
    assert "k_stats" not in tile.timers() and tile.describe_statistics() is None and tile.get_statistics_state() is None
    out, info = np.full((N, 2, 2), 7.0, order="F"), np.full(5, 7.0)
    assert tile._lib.sx_stats_get(tile._h, out.ctypes.data_as(L.P_D), info.ctypes.data_as(L.P_D)) != 0
    assert b"no statistics set" in tile._lib.sx_last_error() and (out == 7.0).all() and (info == 7.0).all()
    with pytest.raises(S.ScytheHipError, match="no statistics set"):
        tile.statistics()
    good = [("max", [(1.0, 0, [(1, 0)])]), ("duration", [(1.0, 0, [(2, 0)])], 0.25)]
    tile.set_statistics(good, "state")
    assert tile.describe_statistics() == ("state", ["max", "duration"], [None, 0.25])
    tile.accumulate_statistics(1.0, 0.5)
    before = _bits(tile.get_statistics_state())
    coef, packed, n_out, op, thr = S.pack_statistics(gp, good)
    pd, pi = lambda a: a.ctypes.data_as(L.P_D), lambda a: a.ctypes.data_as(L.P_I32)

    def refused(what, *args):
        assert tile._lib.sx_stats_set(tile._h, *args) != 0
        assert what in tile._lib.sx_last_error().decode(), tile._lib.sx_last_error()
        assert _bits(tile.get_statistics_state()) == before
    refused("null coef", 1, len(coef), None, pi(packed), n_out, pi(op), pd(thr))
    refused("null terms", 1, len(coef), pd(coef), None, n_out, pi(op), pd(thr))
    refused("null op", 1, len(coef), pd(coef), pi(packed), n_out, None, pd(thr))
    refused("null threshold", 1, len(coef), pd(coef), pi(packed), n_out, pi(op), None)
    refused("none of SX_STAT", 1, len(coef), pd(coef), pi(packed), n_out, pi(np.array([1, 4], dtype=np.int32)), pd(thr))
    refused("NaN or Inf", 1, len(coef), pd(coef), pi(packed), n_out, pi(op), pd(np.array([0.0, np.inf])))
    refused("source must be", 2, len(coef), pd(coef), pi(packed), n_out, pi(op), pd(thr))
    refused("n_out must be", 1, len(coef), pd(coef), pi(packed), 17, pi(op), pd(thr))
    bad = packed.copy()
    bad[0, 7] = 1                                    # a derivative slot with the source state
    refused("slot 0", 1, len(coef), pd(coef), pi(bad), n_out, pi(op), pd(thr))
    for t, w, what in ((np.nan, 1.0, "time is NaN or Inf"), (1.0, np.inf, "weight is NaN or Inf")):
        with pytest.raises(S.ScytheHipError, match=what):
            tile.accumulate_statistics(t, w)
    assert _bits(tile.get_statistics_state()) == before and tile.timers()["k_stats"][1] == 1
    # bytes: 2 planes of 8 bytes + 2 outputs x 32
    assert tile.kernel_bytes("k_stats") == 2 * 8.0 * N + 2 * 32.0 * N
    # a negative weight is allowed
    tile.accumulate_statistics(2.0, -0.25)
    assert tile.statistics().elapsed == 0.25 and tile.statistics().samples == 2
    # the blob: back into this handle, refused on another grid size and when damaged
    blob = tile.get_statistics_state()
    _, other, _ = _tile("R")
    for b, what in ((blob, "does not belong"), (blob[:-1], "does not belong")):
        with pytest.raises(S.ScytheHipError, match=what):
            (other if b is blob else tile).set_statistics_state(b)
    assert other.describe_statistics() is None
    other.close()
    broken = blob.copy()
    broken[0] = 1.0
    with pytest.raises(S.ScytheHipError, match="does not belong"):
        tile.set_statistics_state(broken)
    tile.reset_statistics()
    st = tile.statistics()
    assert st.samples == 0 and np.isnan(st.value[:, 0]).all() and (st.value[:, 1] == 0).all() and tile.describe_statistics()[1] == ["max", "duration"]
    tile.set_statistics_state(blob)
    assert _bits(tile.get_statistics_state()) == _bits(blob) and tile.statistics().samples == 2
    # a new set replaces the old one; n_out = 0 frees it
    tile.set_statistics([("sum", [(1.0, 0, [(1, 0)])])], "state")
    assert tile.describe_statistics()[1] == ["sum"] and tile.statistics().samples == 0
    tile.set_statistics([])
    assert tile.describe_statistics() is None and tile.get_statistics_state() is None
    calls = tile.timers()["k_stats"][1]
    tile.accumulate_statistics(3.0, 1.0)
    assert tile.timers()["k_stats"][1] == calls
    tile.close()


# ---- conveniences -----------------------------------------------------------------------------------------------------------------
def test_wind_swath_and_accumulated():
    hip = cases.HipModel(cases.rl_advection(num_cells=6))
    run, tile = hip.run, hip.run.tiles[0]
    r = run.gridpoints()[:, 0]
    omega, amps, ts = 0.25, (1.0, 3.0, 2.0, 3.0), run.model.ts

    def state(a):
        v = np.zeros((tile.N, 3))
        v[:, 0], v[:, 2] = 1.5, a * omega * r           # h constant; a solid-body vortex of amplitude a
        return v
    tile.set_physical_values(state(amps[0]))
    sw = run.wind_swath("u", "v")                        # attaches the set and takes the state as it stands
    assert sw.samples == 1 and _bits(sw.speed) == _bits(np.sqrt((amps[0] * omega * r) ** 2)) and (sw.time == 0.0).all()
    for k, a in enumerate(amps[1:], start=1):            # the test scales the vortex between samples
        tile.set_physical_values(state(a))
        run._sample_statistics(k * ts, ts)
    sw = run.wind_swath("u", "v")
    assert sw.samples == 4 and _bits(sw.speed) == _bits(np.sqrt((3.0 * omega * r) ** 2))
    assert (sw.time == 1 * ts).all()                     # the largest sample, and the first of the two that reach it
    total, elapsed = run.accumulated("h")                # replaces the swath set; no initial sample
    assert elapsed == 0.0 and (total == 0.0).all()
    for k in range(1, 4):
        run._sample_statistics(k * ts, ts)
    total, elapsed = run.accumulated("h")
    hi, lo = ST.elapsed([ts] * 3)
    assert elapsed == hi + lo and np.abs(total - 1.5 * 3 * ts).max() <= 1.5 * 3 * ts * 2.0 ** -52
    assert np.abs(run.statistics().mean(0) - 1.5).max() <= 1.5 * 2.0 ** -51
    run.close()
