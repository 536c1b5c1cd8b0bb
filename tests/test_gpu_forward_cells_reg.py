"""k_fl_forward_cells at 256-point rings: the transform's four radix-4 passes in registers (SX_FFT_REG=1, the default) against the passes
through LDS (SX_FFT_REG=0), the ring-spectra pair (SX_SBW_MFMA=2) and the two CPU oracles.

Every case runs with SX_SBW_MFMA=3, so that these small grids take the pair.  The rule is tests/test_gpu_forward_cells.py::_check's:
per variable |B_cells - B_rings| / max|B| <= 10 x the spread between the numpy and the C oracle, and the error against numpy is at most
2 x the ring-spectra pair's.  The right-hand side of the first bound is fixed by the two oracles alone; _oracles() asserts that it is
not zero for the seed used (seed 5: 1.1e-16 .. 6.6e-16 over the three cases' variables).

The single-wavenumber cases feed cos(k lambda + phi) on every ring whose truncation holds k: B may have energy in that wavenumber's
columns only, and there it must be the numpy oracle's.  A wrong digit reversal after the register passes, or a wrong mirror bin
L - k in the untangling, moves the energy to another column or changes its amplitude, which a smooth field hides behind its own decay."""
import numpy as np
import pytest

from oracle import oracle_c as OC
from tests import cases
from tests import test_gpu_forward_cells as fc

SEED = 5
CASES = {
    "hrbl-7x32": dict(nc=7, nz=32, nvars=6),       # rings with kmax < 64: lanes that own no wavenumber of the ring
    "hrbl-12x32": dict(nc=12, nz=32, nvars=6),     # at least two segments: edge partials
    "one-7x64": dict(nc=7, nz=64, nvars=1),        # one variable, b_zDim below zDim
}
_ORACLES = {}
_OG44 = None       # oracle grid of the single-wavenumber cases, built once


def _case(name):
    c = CASES[name]
    return fc._case(256, c["nc"], c["nz"], nvars=c["nvars"])


def _oracles(name, vals):
    """numpy and C oracle of the case's B, computed once and shared; the oracle spread must not be zero."""
    if name not in _ORACLES:
        og = cases.oracle_grid(_case(name))
        Bnp, Bc = og.forward(vals, 0, og.nc), OC.TileOracle(og, 0, None).forward(vals)
        for v in range(Bnp.shape[1]):
            assert np.abs(Bnp[:, v] - Bc[:, v]).max() > 0.0, (name, v, "oracle spread is zero: choose another seed")
        _ORACLES[name] = (og, vals.copy())
    og, v0 = _ORACLES[name]
    assert np.array_equal(v0, vals)
    return og


def _run(monkeypatch, case, reg, cells=True, vals=None):
    monkeypatch.setenv("SX_FFT_REG", "1" if reg else "0")
    vals, B, alloc = fc._b(monkeypatch, case, cells, vals, seed=SEED)
    assert (alloc[0] == 0) == cells
    return vals, B


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_register_passes_against_the_ring_spectra_pair_and_the_oracles(monkeypatch, name):
    case = _case(name)
    og0 = cases.oracle_grid(case)
    if name == "hrbl-12x32":
        assert fc._plan(case)[1]["segs"] >= 2, fc._plan(case)
    if name == "one-7x64":
        assert og0.b_zDim < og0.zDim
    if name == "hrbl-7x32":
        assert int(og0.kmax.max()) < 64
    assert fc._plan(case)[0] == "k_fl_forward_cells<8>"
    vals, B1 = _run(monkeypatch, case, True)
    _, B1b = _run(monkeypatch, case, True, vals=vals)
    _, B0 = _run(monkeypatch, case, False, vals=vals)
    _, B0b = _run(monkeypatch, case, False, vals=vals)
    _, Br = _run(monkeypatch, case, True, cells=False, vals=vals)
    og = _oracles(name, vals)
    print("%s: max|B(reg) - B(lds)| / max|B| %.2e" % (name, np.abs(B1 - B0).max() / np.abs(B0).max()))
    assert np.array_equal(B1, B1b), "SX_FFT_REG=1 is not repeatable"
    assert np.array_equal(B0, B0b), "SX_FFT_REG=0 is not repeatable"
    assert not np.array_equal(B1, B0), "SX_FFT_REG=1 gave the bits of the LDS passes: the register passes did not run"
    fc._check(name + " SX_FFT_REG=1", og, vals, B1, Br)
    fc._check(name + " SX_FFT_REG=0", og, vals, B0, Br)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 63, 64, 126, 127])
def test_a_single_wavenumber_stays_in_its_columns(monkeypatch, k):
    """One variable, 44 cells x 32 levels: rings 1..132, kmax = min(ring, 127), so every k of the list has rings that hold it."""
    import scythe_jl_amd as S
    nc, nz, L = 44, 32, 256
    case = fc._case(L, nc, nz, nvars=1)
    monkeypatch.setenv("SX_SBW_MFMA", "3")
    monkeypatch.setenv("SX_FFT_REG", "1")
    assert fc._plan(case)[0] == "k_fl_forward_cells<8>"
    g = S.Grid(*cases.hip_params(case))
    pts = np.asarray(S.getGridpoints(g)).reshape(-1, 3)
    ring = np.arange(len(pts)) // (L * nz)
    kmax = np.minimum(ring + 1, L // 2 - 1)
    assert len(pts) == 3 * nc * L * nz and (kmax >= k).any()
    l = (np.arange(len(pts)) // nz) % L                                  # lambda = 2 pi l / L; k l reduced mod L, so that the input
    assert np.allclose(pts[:, 1], 2.0 * np.pi * l / L)                   # itself carries no k ulp of phase error
    f = np.cos(2.0 * np.pi * ((k * l) % L) / L + 0.7) * (1.0 + pts[:, 0] / 3.0e5) * (1.0 + 0.3 * pts[:, 2] / 2000.0)
    g.set_physical_values(np.where(kmax >= k, f, 0.0)[:, None])
    g.spectralTransform_()
    B = np.asarray(g.spectral)
    g.close()
    nbt = nc + 3
    K2t = 1 + 2 * (L // 2 - 1)
    col = np.abs(B[:, 0].reshape(-1, K2t, nbt)).max(axis=(0, 2))        # [block]: 0 is k = 0, 2 k - 1 and 2 k are wavenumber k
    own = [0] if k == 0 else [2 * k - 1, 2 * k]
    peak = col[own].max()
    rest = np.delete(col, own).max()
    print("k %d: peak %.3e, largest other column %.3e (%.2e of the peak)" % (k, peak, rest, rest / peak))
    assert np.isfinite(B).all() and peak > 0.0
    assert rest <= 1e-13 * peak, (k, peak, rest)
    # the wavenumber's own columns against the numpy oracle: a mirror bin L - k read wrongly but from an empty place would halve the
    # peak and mix the two packed levels without moving energy to another column.  Same bound: rounding of a 256-point fp64 transform
    # and of sums over at most 12 rings per node is a few 1e-16 of the peak.
    global _OG44
    if _OG44 is None:
        _OG44 = cases.oracle_grid(case)
    Bnp = _OG44.forward(np.where(kmax >= k, f, 0.0)[:, None], 0, nc)
    assert Bnp.shape == B.shape
    err = np.abs(B - Bnp).max()
    print("k %d: max|B - B_numpy| %.3e (%.2e of the peak)" % (k, err, err / peak))
    assert err <= 1e-13 * peak, (k, peak, err)
