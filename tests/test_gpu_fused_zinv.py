"""-m gpu: the vertical inverse inside the node FFT kernel (the default where fft_fused_zinv holds, sx_fft.hip) against the pair it
replaces (SX_FUSE_ZINV=0: k_zinv writes Az for every node, the node FFT kernel reads it back), through the public step API.

Nothing promises that the two forms sum the b_zDim vertical modes in the same order, so the demand is closeness, not bit-identity
(measured on an MI355X: with the register passes every case below came out bit-identical - k_zinv's matrix-core kernel takes the K
steps in the same order; with SX_FFT_REG=0 against the pair on the register passes: var_np1 5e-15, A 1e-15, slots 4e-15 .. 2e-12
under floors of 1e-14 .. 2e-11).  The bars are check_full's (tests/cases.py), nothing new:
  (1) state - var_np1, the A coefficients, the value slot of `physical` - within 1e-10;
  (2) every slot of `physical` after tileTransform! within 10 x floor + 1e-12, floor = the spread per_slot_errors measures between two
      fp64 oracles of the same case and steps (the C oracle on one tile and split into two: another summation order of the same
      arithmetic, check_full's `orc_alt`).  Each floor is computed once per shape and shared.
The fused kernel needs the node-space path, which exists at 32 / 64 / 128 levels only (mfma_levels): at 16 levels no handle qualifies,
both runs take the same kernels, and those cases demand bit-identity and equal k_zinv traffic instead."""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu
STEPS = 3
_floor = {}


def _case(L, cells, levels, b_zDim=None):
    case = cases.rlz_hrbl(num_cells=cells, zDim=levels, ring_L=L)
    if b_zDim is not None:
        case["grid"]["b_zDim"] = b_zDim
    return case


def _noise_floor(key):
    """per-slot spread of two fp64 oracles after STEPS steps, once per shape"""
    if key not in _floor:
        case = _case(*key)
        one, two = cases.OracleModel(case), cases.OracleModel(case, tiles=cases.even_tiles(key[1], 2))
        for _ in range(STEPS):
            one.step()
            two.step()
        _floor[key] = cases.per_slot_errors(two.physical(), one.physical())
    return _floor[key]


def _run(case, monkeypatch, env):
    """STEPS steps under the switches `env` -> var_np1, A, physical after tileTransform!, (k_zinv, k_node_fft) bytes of the last step"""
    for k in ("SX_FUSE_ZINV", "SX_OVERLAP", "SX_FFT_REG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = cases.HipModel(case)
    for _ in range(STEPS):
        m.step()
    tile = m.run.tiles[0]
    nbytes = (tile.kernel_bytes("k_zinv"), tile.kernel_bytes("k_node_fft"))
    return tile.var_np1, np.asarray(m.A), m.physical(), nbytes


def _check_close(key, fused, pair):
    (np1_f, A_f, ph_f, by_f), (np1_p, A_p, ph_p, by_p) = fused, pair
    assert np.isfinite(ph_f).all() and np.abs(ph_f[:, :, 0]).max() > 0
    # the fused form is what ran: k_zinv serves the inner rings' nodes only, and the node kernel reads A rows, not Az
    assert by_f[0] < by_p[0] and by_f[1] != by_p[1], (by_f, by_p)
    e_np1 = max(cases.rel_err(np1_f[:, v], np1_p[:, v]) for v in range(np1_p.shape[1]) if np.abs(np1_p[:, v]).max() > 0)
    e_A = cases.rel_err(A_f, A_p)
    e_val = max(cases.rel_err(ph_f[:, v, 0], ph_p[:, v, 0]) for v in range(ph_p.shape[1]) if np.abs(ph_p[:, v, 0]).max() > 0)
    d, floor = cases.per_slot_errors(ph_f, ph_p), _noise_floor(key)
    print("%s: var_np1 %.1e  A %.1e  values %.1e\n  slots fused vs pair %s\n  oracle floor        %s"
          % (key, e_np1, e_A, e_val, " ".join("%.1e" % x for x in d), " ".join("%.1e" % x for x in floor)))
    assert e_np1 < 1e-10 and e_A < 1e-10 and e_val < 1e-10, (e_np1, e_A, e_val)
    assert (d <= 10.0 * floor + 1e-12).all(), (d, floor)


# (ring length, cells, levels, b_zDim).  256 points: the register passes behind the slab; node units = cells + 3 - 42 = 6, 8 and 9: one
# partial group of 8, exactly one group, one group + 1 (the guard of fused_unit_of on both sides); 2 and 4 level chunks; b_zDim 11: a
# partial K step.  64 points: the LDS-pass fused form, units = cells + 3 - 10 = 6.
SHAPES = [(256, 45, 32, None), (256, 47, 32, None), (256, 48, 64, None), (256, 45, 32, 11), (64, 13, 32, None)]


@pytest.mark.parametrize("key", SHAPES, ids=lambda k: "L%d-c%d-z%d-b%s" % k)
def test_fused_vertical_inverse_equals_the_zinv_pair(monkeypatch, key):
    case = _case(*key)
    _check_close(key, _run(case, monkeypatch, {}), _run(case, monkeypatch, {"SX_FUSE_ZINV": "0"}))


def test_fused_vertical_inverse_through_the_lds_passes_at_256_points(monkeypatch):
    """SX_FFT_REG=0 keeps the fused prologue in front of fft_inplace"""
    key = SHAPES[0]
    case = _case(*key)
    _check_close(key, _run(case, monkeypatch, {"SX_FFT_REG": "0"}), _run(case, monkeypatch, {"SX_FUSE_ZINV": "0"}))


def test_fused_vertical_inverse_in_plain_grid_order_gives_the_same_bits(monkeypatch):
    """SX_FUSE_ZINV=2 only changes which workgroup takes which (chunk, node)"""
    case = _case(*SHAPES[2])
    a, b = _run(case, monkeypatch, {}), _run(case, monkeypatch, {"SX_FUSE_ZINV": "2"})
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)


def test_fused_vertical_inverse_on_two_streams_gives_the_same_bits(monkeypatch):
    """SX_OVERLAP=1 (the inner-ring chain on a second stream) against the one-stream run, both fused"""
    case = _case(*SHAPES[0])
    a, b = _run(case, monkeypatch, {"SX_OVERLAP": "1"}), _run(case, monkeypatch, {})
    assert a[3][0] == b[3][0]
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("key", [(256, 45, 16, None), (64, 13, 16, None)], ids=lambda k: "L%d-c%d-z%d-b%s" % k)
def test_at_16_levels_no_handle_qualifies_and_the_switch_changes_nothing(monkeypatch, key):
    case = _case(*key)
    a, b = _run(case, monkeypatch, {}), _run(case, monkeypatch, {"SX_FUSE_ZINV": "0"})
    assert a[3] == b[3]
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
