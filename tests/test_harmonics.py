"""sx_harmonics / sx_evaluate_band where there is no GPU: the symbols, and the twin (tests/harmonics.py) pinned to the Fourier
definition of the harmonics on the rings of the grid and to the band identity."""
import os

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import cases
from tests import evaluate as E
from tests import harmonics as H
from tests.test_evaluate import _case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
GEOMS = [("RL", None), ("RL", 16), ("RLZ", None), ("RLZ", 12)]


def test_symbols_exported_and_declared():
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib as L
    lib = S.load()
    header = open(os.path.join(ROOT, "include", "scythe_hip.h")).read()
    for name in ("sx_harmonics", "sx_evaluate_band"):
        assert hasattr(lib, name) and name in L.SYMBOLS
        assert "int %s(" % name in header
    assert "#define SX_ABI_VERSION 2" in header and lib.sx_abi_version() == 2


@pytest.mark.parametrize("geom,ring_L", GEOMS)
def test_twin_is_the_ring_dft(geom, ring_L):
    """The longdouble twin at the Float64 ring radii and levels against (1 / L) sum_j u_j e^{-i k lambda_j} of inverse_xp's ring
    values, with the exact ring angles on both sides: the two differ by the rounding of the r and z coordinates alone (the argument
    of test_twin_matches_inverse_xp_at_own_gridpoints; no lambda enters), so 64 eps (1 + zDim^2) of the slot's scale."""
    g = cases.oracle_grid(_case(geom, ring_L))
    A = np.random.default_rng(3).standard_normal((g.S_patch(), g.V))
    rings = sorted({0, 1, g.rDim // 2, g.rDim - 1})
    truth = O.inverse_xp(g, A, rings)
    rad = O.mish_points(g.xmin, g.DX, 0, g.nc)
    lev = g.cheb(g.names[0]).z if g.has_z else None
    slots = H.grid_slots(g)
    sl = [g.slots.index(s) for s in slots]
    tol = 64 * EPS * (1 + g.zDim ** 2)
    for ring in rings:
        L, km = int(g.L[ring]), int(g.kmax[ring])
        assert km < L / 2
        c = H.harmonics(g, A, [rad[ring]], lev, slots=slots, xp=True)[0]              # [iz, k, v, s]
        u = truth[ring].reshape(L, g.zDim, g.V, g.D)[:, :, :, sl]                     # [lambda, z, v, s]
        d = H.ring_dft(u, H.ring_angles_xp(g, ring))                                  # [k, z, v, s]
        for si, s in enumerate(slots):
            mine, ref = c[:, :km + 1, :, si].transpose(1, 0, 2), d[:km + 1, :, :, si]
            e = H.rel_err(mine, ref)
            print(geom, ring_L, "ring", ring, "slot", s, "twin vs ring DFT", e, "tol", tol)
            assert e <= tol, (ring, s, e, tol)
        assert (c[:, km + 1:] == 0).all()                                             # above the ring's kmax: exact zeros
        if km < g.kDim:
            assert np.abs(H.harmonics(g, A, [rad[ring]], lev, all_k=True, xp=True)[0][:, km + 1:]).max() > 0


@pytest.mark.parametrize("geom,ring_L", GEOMS)
def test_band_identity_in_the_twin(geom, ring_L):
    """evaluate restricted to [k, k] is eps_k Re(c_k e^{i k lambda}) in every slot, and the bands add up to the whole"""
    g = cases.oracle_grid(_case(geom, ring_L))
    A = np.random.default_rng(4).standard_normal((g.S_patch(), g.V))
    pts = E.scattered_points(g, 40, seed=11)
    slots = H.grid_slots(g)
    for all_k in (False, True):
        total = 0
        for k in range(g.kDim + 1):
            band = H.evaluate_band(g, A, pts, k, k, all_k, xp=True)
            total = total + band
            c = np.stack([H.harmonics(g, A, [p[0]], [p[-1]] if g.has_z else None, all_k, slots, xp=True)[0, 0, k] for p in pts])
            rec = H.from_harmonic(g, c, k, pts[:, 1], xp=True)
            for d in range(g.D):
                scale = max(float(np.abs(band[:, :, d]).max()), 1e-300)
                assert float(np.abs(band[:, :, d] - rec[:, :, d]).max()) <= 64 * EPS * scale or float(np.abs(rec[:, :, d]).max()) == 0, (k, d)
        full = E.evaluate(g, A, pts, all_k, xp=True)
        assert (E.slot_errors(total, full) <= 64 * EPS * (1 + g.kDim)).all()
