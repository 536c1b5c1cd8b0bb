"""sx_spectrum where there is no GPU: the symbols, the pair validator (sx_spectrum_check), and the twin (tests/spectrum.py) pinned to
the oracle by Parseval: the sum over k of a spectrum is the azimuthal mean of the product, because every ring table has
2 kmax[ring] < L[ring]."""
import dataclasses
import os

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import cases
from tests import harmonics as H
from tests import reduce as R
from tests import spectrum as SP
from tests.test_evaluate import _case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XP = O.XP
GEOMS = [("RL", None), ("RL", 16), ("RLZ", None), ("RLZ", 12)]          # tests/test_harmonics.py::GEOMS


def test_symbols_exported_and_declared():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    header = open(os.path.join(ROOT, "include", "scythe_hip.h")).read()
    julia = open(os.path.join(ROOT, "julia", "hipTile.jl")).read()
    for name in ("sx_spectrum", "sx_spectrum_check"):
        assert hasattr(lib, name) and name in L.SYMBOLS
        assert "int %s(" % name in header
    assert "enum { SX_SPEC_RING = 0, SX_SPEC_DOMAIN = 1 };" in header and L.SPEC_KIND == {"ring": 0, "domain": 1}
    assert ":sx_spectrum, libsx" in julia
    assert "#define SX_ABI_VERSION 2" in header and lib.sx_abi_version() == 2
    assert callable(S.spectrum_check) and hasattr(S.Grid, "spectrum") and hasattr(S.ModelRun, "spectrum")


def test_spectrum_check_refusals():
    import ctypes as C
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    from scythe_jl_amd.model import grid_desc
    lib = S.load()
    gp, _ = cases.hip_params(cases.rlz_hrbl(num_cells=9, zDim=10))
    gp_rl, _ = cases.hip_params(cases.rl_slab(num_cells=9))
    V = len(gp.vars)
    name = next(iter(gp.vars))

    def raw(patch, n, pairs):
        d, keep = grid_desc(patch)
        q = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
        rc = lib.sx_spectrum_check(C.byref(d), n, None if q is None else q.ctypes.data_as(L.P_I32))
        return rc, lib.sx_last_error().decode()

    good = [[1, 0, 2, 4]]
    assert raw(gp, 1, good)[0] == 0
    assert raw(gp, 0, None)[0] == 0                                            # no pairs: nothing to refuse
    S.spectrum_check(gp, [((name, "u"), (name, "zz")), ((1, 1), (V, 2))])
    S.spectrum_check(gp, [((1, "u"), (1, "u"))] * 16)
    S.spectrum_check(gp_rl, [((1, "u"), (2, "rr"))])
    bad = [(gp, 1, None), (gp, -1, good), (gp, 17, [[1, 0, 1, 0]] * 17), (gp, 1, [[0, 0, 1, 0]]), (gp, 1, [[1, 0, V + 1, 0]]),
           (gp, 1, [[1, -1, 1, 0]]), (gp, 1, [[1, 0, 1, 5]]), (gp_rl, 1, [[1, 3, 1, 0]]), (gp_rl, 1, [[1, 0, 1, 4]])]
    for patch, n, pairs in bad:
        rc, msg = raw(patch, n, pairs)
        assert rc != 0 and msg, (n, pairs)
    tall = dataclasses.replace(gp, zDim=200, b_zDim=130)
    rc, msg = raw(tall, 1, good)
    assert rc != 0 and "128" in msg
    assert raw(dataclasses.replace(gp, zDim=200, b_zDim=128), 1, good)[0] == 0
    assert raw(dataclasses.replace(gp, zDim=256, b_zDim=None), 1, good)[0] != 0         # the default b_zDim of 256 levels is 171
    with pytest.raises(L.ScytheHipError):
        S.spectrum_check(gp_rl, [((1, "u"), (1, "z"))])
    with pytest.raises(ValueError):
        S.spectrum_check(gp, [((1, "u"), (1, "l"))])                           # lambda derivatives are i k c_k: no slot of a spectrum
    with pytest.raises(ValueError):
        S.spectrum_check(gp, [(("nope", "u"), (1, "u"))])


@pytest.mark.parametrize("geom,ring_L", GEOMS)
def test_parseval_in_the_twin(geom, ring_L):
    """sum_k of the longdouble twin against the oracle, for every legal slot pair of two variables: per ring, the w_z-weighted level
    sum of the azimuthal mean of the product of inverse_xp's ring values; for the domain, tests/reduce.py::reduce of the one-term
    programs on the same values.  Bound 32 2^-53 S_abs (tests/reduce.py::BOUND)."""
    g = cases.oracle_grid(_case(geom, ring_L))
    A = np.random.default_rng(3).standard_normal((g.S_patch(), g.V))
    pairs = SP.all_pairs(g)
    q = SP.resolve(g, pairs)
    slots = H.grid_slots(g)
    assert len(pairs) == len(slots) * (2 * len(slots) + 1)
    ring, ring_abs, dom, dom_abs = SP.spectrum(g, A, pairs, xp=True)
    assert ring.shape == (g.kDim + 1, g.rDim, len(pairs)) and dom.shape == (g.kDim + 1, len(pairs))
    rings = list(range(g.rDim))
    phys = O.inverse_xp(g, A, rings)
    _, _, w_z = R.weights(g)
    worst = 0.0
    for i in rings:
        L, km = int(g.L[i]), int(g.kmax[i])
        assert 2 * km < L
        assert (ring[km + 1:, i] == 0).all() and np.abs(ring[km, i]).max() > 0
        u = phys[i].reshape(L, g.zDim, g.V, g.D)
        for p, (va, sa, vb, sb) in enumerate(q):
            fa, fb = u[:, :, va - 1, g.slots.index(slots[sa])], u[:, :, vb - 1, g.slots.index(slots[sb])]
            mean = ((fa * fb).sum(axis=0) / XP(L) * w_z).sum()
            err, lim = abs(ring[:, i, p].sum() - mean), XP(R.BOUND) * ring_abs[:, i, p].sum()
            worst = max(worst, float(err / lim))
            assert err <= lim, (i, pairs[p], float(err / lim))
    print("%s ring_L=%s: sum_k ring spectrum vs the oracle's weighted azimuthal mean, worst ratio to 32 ulp S_abs %.3g" % (geom, ring_L, worst))
    data = np.concatenate([phys[i] for i in rings], axis=0)
    truth, _ = R.reduce(g, data, g.gridpoints(), SP.product_program(g, pairs), "domain")
    err, lim = np.abs(dom.sum(axis=0) - truth), XP(R.BOUND) * dom_abs.sum(axis=0)
    print("%s ring_L=%s: sum_k domain spectrum vs reduce of the products, worst ratio to 32 ulp S_abs %.3g" % (geom, ring_L, float((err / lim).max())))
    assert (err <= lim).all(), (err / lim).max()
