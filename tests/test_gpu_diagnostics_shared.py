"""The five device diagnostics (evaluate, reduce, harmonics, spectrum, parcels) keep their per-handle state in one place and build it
lazily, partly from one another's: the vertical classes belong to evaluate's state and are used by harmonics, spectrum and parcels.
Whichever diagnostic a handle sees first, and in whichever order the others follow, every result has the same bytes; kernel_bytes
of the call's kernel, read straight after the call (it counts the last call), is positive and the same; and a handle closes cleanly
with any subset of the states made.

Two grids: RLZ with two vertical classes, one height tile and b_zDim = 7 (no multiple of 4), and RL, which has no vertical (no
class, b_zDim 1).  A dozen points and radii, three heights, two pairs, one two-term program, four parcels."""
import numpy as np
import pytest

from tests import cases
from tests import evaluate as E
from tests import harmonics as H

pytestmark = pytest.mark.gpu

GRIDS = {"RLZ": lambda: cases.rlz_hrbl(num_cells=6, zDim=10, ring_L=16), "RL": lambda: cases.rl_slab(num_cells=8)}


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _calls(g):
    """(name, function of a tile, the call's kernel), in the order of the first handle"""
    pts = E.scattered_points(g, 12, seed=31)
    radii = H.sample_radii(g, 12, seed=33)
    heights = np.array([g.zmin, 0.37 * (g.zmax - g.zmin) + g.zmin, g.zmax]) if g.has_z else None
    slots = H.grid_slots(g)
    pairs = [(("h", "u"), ("h", "u")), (("u", "r"), ("v", "u"))]
    program = [(0, 1.0, 1, [("h", ""), ("h", "")]), (0, -0.5, 0, [("u", ""), ("v", "")])]
    parcels = E.scattered_points(g, 4, seed=35)
    parcels[:, 0] = g.xmin + (g.xmax - g.xmin) * np.array([0.2, 0.4, 0.6, 0.8])
    velocity = ("u", "v", "wb") if g.has_z else ("u", "v")

    def run_parcels(tile):
        tile.set_parcels(parcels, velocity)
        tile.advance_parcels(0.5)
        return _bytes(*tile.parcels())

    return [("spectrum", lambda t: _bytes(t.spectrum(pairs, "ring"), t.spectrum(pairs, "domain")), "k_spectrum"),
            ("parcels", run_parcels, "k_parcels"),
            ("harmonics", lambda t: _bytes(t.harmonics(radii, heights, False, slots)), "k_harmonics"),
            ("reduce", lambda t: _bytes(t.reduce(program, "domain", "state"), t.reduce(program, "azimuth", "state")), "k_reduce"),
            ("evaluate", lambda t: _bytes(t.evaluate(pts)), "k_evaluate"),
            ("band", lambda t: _bytes(t.evaluate(pts, k_band=(1, 2))), "k_evaluate")]


def _run(tile, calls):
    """name -> (result bytes, kernel_bytes of the call's kernel after the call)"""
    return {k: (f(tile), tile.kernel_bytes(kern)) for k, f, kern in calls}


@pytest.mark.parametrize("name", list(GRIDS))
def test_any_order_same_bytes(name):
    import scythe_jl_amd as S
    case = GRIDS[name]()
    gp, mp = cases.hip_params(case)
    g = cases.oracle_grid(case)
    A = np.random.default_rng(7).standard_normal((g.S_patch(), g.V))
    calls = _calls(g)

    def handle():
        tile = S.Grid(gp, mp)
        tile.set_patch_spectral_a(A)
        tile.set_physical_values(np.random.default_rng(11).standard_normal((tile.N, g.V)))      # var_np1: what reduce(source="state") reads
        return tile

    first, second = handle(), handle()
    got1, got2 = _run(first, calls), _run(second, calls[::-1])
    for k, _, kern in calls:
        print("%s %s: %d result bytes, kernel_bytes(%s) %g" % (name, k, len(got1[k][0]), kern, got1[k][1]))
        assert len(got1[k][0]) > 0 and any(got1[k][0]), k
        assert got1[k][0] == got2[k][0], k
        assert got1[k][1] > 0 and got1[k][1] == got2[k][1], k
    first.close()
    second.close()
    third = handle()                                        # harmonics as the first diagnostic a handle ever sees
    assert _run(third, calls[2:3])["harmonics"] == got1["harmonics"]
    third.close()
