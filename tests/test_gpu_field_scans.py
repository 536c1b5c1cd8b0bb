"""The five entry points that evaluate a field program at every gridpoint (reduce, extrema, distribution, statistics, project) share
one scan table per handle - the work list and the quadrature weights (csrc/sx_redprog.hpp) - made by whichever of them a handle sees
first and extended with the weights when reduce or distribution first asks for them.  Whichever comes first, and in whichever order
the others follow, every result has the same bytes; a second round on the same handle repeats the first; and a handle that has used
all five closes cleanly, after which a new handle on the same grid gives the same bytes again.

In the forward order reduce makes the table with its weights before extrema and statistics use it; in the reverse order statistics
makes and uses it without weights and distribution adds them before extrema runs; the third handle starts with extrema, before any
weights exist.  The grids cover ring pieces and the flat walk, two points
per lane and one (RL has no vertical), native and uniform rings and both storage types, on one tile and on three.  project takes
one-tile patches only: with three tiles it is left out.  A tile has at least 3 cells, so the f32 grid has 9 cells where it is split
in three (6 on one tile: the shape the other f32 tests use)."""
import numpy as np
import pytest

from tests import cases
from tests import reduce as R

pytestmark = pytest.mark.gpu

# (maker, its arguments, storage)
GRIDS = {
    "R": ("r_bcs", dict(num_cells=12), "f64"),
    "RZ": ("rz_advection", dict(num_cells=9, zDim=12), "f64"),
    "RL": ("rl_slab", dict(num_cells=9), "f64"),
    "RLZ": ("rlz_hrbl", dict(num_cells=9, zDim=10, ring_L=16), "f64"),
    "RLZ-f32": ("rlz_hrbl", dict(num_cells=6, zDim=32, ring_L=32), "f32"),
}
EDGES = np.array([-1.0e3, -1.0, -1.0e-3, 0.0, 1.0e-3, 1.0, 1.0e3])
OPS = ["sum", "max", "min", "duration", "sum"]


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _calls(g, with_project):
    """(name, function of a tile -> bytes), in the forward order"""
    progs = {"physical": R.random_program(g, 11), "state": R.random_program(g, 13, source="state")}
    hists = {"physical": R.random_program(g, 11, n_out=4), "state": R.random_program(g, 13, n_out=4, source="state")}

    def reduce(t):
        return _bytes(*[t.reduce(p, kind, s) for s, p in progs.items() for kind in ("domain", "azimuth")])

    def extrema(t):
        return _bytes(*[a for s, p in progs.items() for kind in ("domain", "azimuth") for a in t.extrema(p, kind, s)])

    def distribution(t):
        out = []
        for s, p in hists.items():
            for kind in ("domain", "level"):
                d = t.distribution(p, EDGES, kind, s)
                out += [d.count, d.sums]
        return _bytes(*out)

    def statistics(t):
        out = []
        for s, p in progs.items():
            outputs = [(OPS[o], [(c, pw, f) for oo, c, pw, f in p if oo == o]) + ((0.0,) if OPS[o] == "duration" else ()) for o in range(5)]
            t.set_statistics(outputs, s)
            t.accumulate_statistics(1.0, 0.5)
            t.accumulate_statistics(2.0, 1.5)
            st = t.statistics()
            out += [st.value, st.time, t.get_statistics_state()]
        t.set_statistics([])
        return _bytes(*out)

    def project(t):
        out = []
        for s, p in progs.items():
            comp = t.project(p, t.project_companion(["a", "b", "c", "d", "e"]), s)
            out += [comp.var_np1, comp.spectral]
        return _bytes(*out)

    calls = [("reduce", reduce), ("extrema", extrema), ("distribution", distribution), ("statistics", statistics)]
    return calls + ([("project", project)] if with_project else [])


def _case(name, tiles):
    maker, kw, _ = GRIDS[name]
    return getattr(cases, maker)(**dict(kw, num_cells=max(kw["num_cells"], 3 * tiles)))


def _model(name, tiles):
    hip = cases.HipModel(_case(name, tiles), num_tiles=tiles, exchange="gather", storage=GRIDS[name][2], impl="lib" if tiles > 1 else "torch")
    for _ in range(2):
        hip.step()
    for tile in hip.run.tiles:
        tile.tileTransform_()
    return hip


def _run(hip, calls):
    """name -> the bytes of every tile's result"""
    return {k: b"".join(f(tile) for tile in hip.run.tiles) for k, f in calls}


@pytest.mark.parametrize("tiles", [1, 3])
@pytest.mark.parametrize("name", list(GRIDS))
def test_any_order_same_bytes(name, tiles):
    calls = _calls(cases.oracle_grid(_case(name, tiles)), tiles == 1)
    first, second = _model(name, tiles), _model(name, tiles)
    got1, got2 = _run(first, calls), _run(second, calls[::-1])
    for k, _ in calls:
        print("%s, %d tiles, %s: %d result bytes" % (name, tiles, k, len(got1[k])))
        assert len(got1[k]) > 0 and any(got1[k]), k
        assert got1[k] == got2[k], k
    again1, again2 = _run(first, calls), _run(second, calls)        # the second round, on the second handle in the other order than its first
    for k, _ in calls:
        assert again1[k] == got1[k] and again2[k] == got1[k], k
    first.run.close()                                               # with all five states and the table made
    second.run.close()
    third = _model(name, tiles)
    got3 = _run(third, calls[1:] + calls[:1])                       # extrema as the first a handle ever sees
    for k, _ in calls:
        assert got3[k] == got1[k], k
    third.run.close()
