"""The twin of tests/stats.py against hand-worked sequences, and the Python layer of the statistics set where there is no GPU: the
symbols, the packing and its refusals, the CSV writer's header.  The weights the GPU tests use are checked here to have subset
sums that longdouble and exact arithmetic round to the same double (what makes DURATION a bitwise check)."""
import itertools
import math
import os

import numpy as np
import pytest

from tests import stats as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

# 5 samples, unequal weights, one of them 0 (the "extrema only" sample): (time, weight)
SAMPLES = ((0.0, 0.0), (0.3, 0.3), (1.0, 0.7), (2.1, 1.1), (2.55, 0.45))


def _feed(op, seq, thr=None):
    """seq: [(q [N], time, weight)]"""
    tw = ST.Twin(op, len(seq[0][0]), thr)
    for q, t, w in seq:
        tw.add(np.array(q, dtype=np.float64), t, w)
    return tw


def test_symbols_exported_and_declared():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    header = open(os.path.join(ROOT, "include", "scythe_hip.h")).read()
    for name in ("sx_stats_set", "sx_stats_reset", "sx_stats_accumulate", "sx_stats_get", "sx_stats_describe", "sx_stats_state_size",
                 "sx_stats_get_state", "sx_stats_set_state"):
        assert hasattr(lib, name) and name in L.SYMBOLS
        assert "int %s(" % name in header
    assert "enum { SX_STAT_SUM = 0, SX_STAT_MAX = 1, SX_STAT_MIN = 2, SX_STAT_DURATION = 3 };" in header
    assert L.STAT_OP == {"sum": 0, "max": 1, "min": 2, "duration": 3}
    assert "statistics of field programs over time" in header
    for name in ("Statistics", "pack_statistics", "write_statistics", "statistics_header", "Swath"):
        assert hasattr(S, name)
    for name in ("set_statistics", "accumulate_statistics", "reset_statistics", "statistics", "get_statistics_state", "set_statistics_state"):
        assert hasattr(S.Grid, name)
    for name in ("set_statistics", "statistics", "reset_statistics", "wind_swath", "accumulated"):
        assert hasattr(S.ModelRun, name)


def test_twin_extrema_by_hand():
    # point 0: a tie keeps the first time; point 1: -0.0 then +0.0 is a tie (the stored bits stay -0.0); point 2: a NaN in the second
    # sample stays, with ITS time; point 3: NaN first stays although numbers follow; point 4: strictly increasing
    seq = [([1.0, -0.0, 5.0, NAN, 1.0], 10.0, 1.0),
           ([1.0, 0.0, NAN, 7.0, 2.0], 20.0, 0.0),
           ([0.5, -1.0, 9.0, 8.0, 3.0], 30.0, 2.0)]
    mx, mn = _feed("max", seq), _feed("min", seq)
    ST.check_bitwise(mx.value, [1.0, -0.0, NAN, NAN, 3.0], "max")
    ST.check_bitwise(mx.time, [10.0, 10.0, 20.0, 10.0, 30.0], "max time")
    ST.check_bitwise(mn.value, [0.5, -1.0, NAN, NAN, 1.0], "min")
    ST.check_bitwise(mn.time, [30.0, 30.0, 20.0, 10.0, 10.0], "min time")
    assert mx.samples == 3
    empty = ST.Twin("max", 2)
    assert empty.samples == 0 and np.isnan(empty.value).all() and np.isnan(empty.time).all()


def test_twin_sum_and_duration_by_hand():
    # weights 1, 0 (skipped), 2; the threshold 2.0 is hit exactly in sample 1 of point 1 and counted; a NaN is not counted
    seq = [([1.0, 2.0, NAN], 0.0, 1.0), ([100.0, 100.0, 100.0], 1.0, 0.0), ([3.0, 1.5, 4.0], 2.0, 2.0)]
    sm, du = _feed("sum", seq), _feed("duration", seq, thr=2.0)
    assert sm.result()[0] == 7.0 and sm.result()[1] == 5.0 and np.isnan(sm.result()[2])
    assert list(sm.S_abs[:2]) == [7.0, 5.0]
    assert list(du.result()) == [2.0, 1.0, 2.0] and list(du.duration_exact()) == [2.0, 1.0, 2.0]
    assert sm.samples == 3 and du.samples == 3
    # the bound: u S_abs and a second-order term that grows with n (n + 1)
    b1, b5 = float(ST.sum_bound(1.0, 1)), float(ST.sum_bound(1.0, 5))
    assert ST.U < b1 < b5 < 1.01 * ST.U
    hi, lo = ST.elapsed([0.1] * 10)
    assert hi + lo == math.fsum([0.1] * 10) and lo != 0.0


def test_gpu_weights_make_duration_bitwise():
    """every subset sum of the GPU tests' weights, in the order of the samples: longdouble rounded once == the exact sum rounded once"""
    w = [x for _, x in SAMPLES if x != 0.0]
    for k in range(len(w) + 1):
        for sub in itertools.combinations(range(len(w)), k):
            ld = ST.XP(0)
            for j in sub:
                ld = ld + ST.XP(w[j])
            assert float(ld) == math.fsum(w[j] for j in sub), sub
    assert sum(1 for _, x in SAMPLES if x == 0.0) == 1 and len({x for _, x in SAMPLES}) == len(SAMPLES)


def _patch():
    import scythe_jl_amd as S
    return S.GridParameters(geometry="RLZ", xmin=0.0, xmax=10.0, num_cells=4, zmin=0.0, zmax=1.0, zDim=8, vars={"h": 1, "u": 2, "v": 3})


def test_packing():
    import scythe_jl_amd as S
    gp = _patch()
    sq = [(1.0, 0, [("u", ""), ("u", "")]), (1.0, 0, [("v", ""), ("v", "")])]
    coef, packed, n_out, op, thr = S.pack_statistics(gp, [("max", sq), ("sum", [(7, 2.0, -1, [("h", "r")])]), ("duration", sq, 33.0 ** 2)])
    assert n_out == 3 and list(op) == [1, 0, 3] and list(thr) == [0.0, 0.0, 33.0 ** 2]
    assert list(coef) == [1.0, 1.0, 2.0, 1.0, 1.0]
    assert list(packed[:, 0]) == [0, 0, 1, 2, 2]                    # a term's own `out` (7) gives way to the entry's index
    assert list(packed[2]) == [1, -1, 1, 1, 0, 0, 0, 1, 0, 0, 0]
    # a Program plus ops
    prog = S.Program([(0, 1.0, 0, [("h", "")]), (1, 1.0, 0, [("u", "")])], ["h", "u"])
    c2, p2, n2, o2, t2 = S.pack_statistics(gp, prog, ops=["min", ("duration", 0.5)])
    assert n2 == 2 and list(o2) == [2, 3] and list(t2) == [0.0, 0.5] and list(p2[:, 0]) == [0, 1]
    # no outputs: what removes a set
    assert S.pack_statistics(gp, [])[2] == 0
    for bad, what in (([("median", sq)], "none of"), ([("duration", sq)], "threshold"), ([("max", sq, 1.0)], "threshold"),
                      ([("max",)], "no \\(op, terms"), ([("max", [(1.0, 0, [("q", "")])])], "unknown variable"),
                      ([("max", [(1.0, 0, [("u", "zzz")])])], "no slot")):
        with pytest.raises(ValueError, match=what):
            S.pack_statistics(gp, bad)
    with pytest.raises(ValueError, match="ops names"):
        S.pack_statistics(gp, prog, ops=["min"])


def test_statistics_object_and_header():
    import scythe_jl_amd as S
    out = np.zeros((3, 2, 2), order="F")
    out[:, 0, 0], out[:, 0, 1] = [6.0, 3.0, 0.0], [1e-17, 0.0, 0.0]
    out[:, 1, 0], out[:, 1, 1] = [2.0, NAN, 5.0], [0.3, 0.3, 1.0]
    st = S.Statistics.from_raw(out, np.array([4.0, 3.0, 0.0, 0.0, 2.55]), ["sum", "max"])
    assert st.samples == 4 and st.elapsed == 3.0 and st.t_first == 0.0 and st.t_last == 2.55
    assert np.isnan(st.time[:, 0]).all() and list(st.time[:, 1]) == [0.3, 0.3, 1.0] and st.residual[0, 0] == 1e-17
    assert list(st.mean(0)) == [2.0, 1.0, 0.0]
    with pytest.raises(ValueError, match="not a 'sum'"):
        st.mean(1)
    both = S.Statistics.concatenate([st, st])
    assert both.value.shape == (6, 2) and both.samples == 4
    assert S.statistics_header("RLZ", ["max", "sum", "min", "duration"]) == ["r", "l", "z", "max0", "max0_time", "sum1", "min2", "min2_time", "duration3"]
    assert S.statistics_header("R", ["max"], ["vmax"]) == ["r", "vmax", "vmax_time"]
    with pytest.raises(ValueError, match="names"):
        S.statistics_header("R", ["max"], ["a", "b"])
