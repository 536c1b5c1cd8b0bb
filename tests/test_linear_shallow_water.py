"""CPU-only: LinearShallowWater1D and LinearShallowWaterRL (src/shallowWaterModels.jl:235-298) through the host side of the library -
the equation-set names, the parameter table's three mirrors (C header, Python, Julia), and the numpy restatement of the two sets
(oracle/oracle_np.py) on the oracle twin against the closed-form periodic 1D mode, with the parameters the Python mirror packs for
sx_create."""
import os
import re

import numpy as np
import pytest

from tests import cases
from tests import linear_sw as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_equation_set_ids_of_the_linear_shallow_water_sets():
    import scythe_jl_amd as S
    lib = S.load()
    assert lib.sx_equation_set_id(b"LinearShallowWater1D") == 9
    assert lib.sx_equation_set_id(b"LinearShallowWaterRL") == 10
    # never advanced by the reference (no explicit_timestep call, src/shallowWaterModels.jl:300-344): still refused
    assert lib.sx_equation_set_id(b"ShallowWaterRL") == -1


def _header_params():
    src = open(os.path.join(ROOT, "include", "scythe_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"enum\s*\{\s*(SX_P_G\s*=\s*0[^}]*)\}", src).group(1)
    names = [n.strip().split("=")[0].strip() for n in body.split(",") if n.strip()]
    assert names[-1] == "SX_NPARAMS"
    return names[:-1]


def _julia_params(path):
    src = open(path).read()
    return re.findall(r":(\w+)", re.search(r"^const SX_PARAMS = \(([^)]*)\)", src, flags=re.M).group(1))


def test_parameter_table_is_the_same_in_the_header_python_and_julia():
    from scythe_jl_amd import _lib
    header = _header_params()
    assert header[-1] == "SX_P_H" and len(header) == 13
    norm = lambda s: s.upper().replace("_", "")
    assert [norm(h[len("SX_P_"):]) for h in header] == [norm(p) for p in _lib.PARAM_ORDER]
    assert _julia_params(os.path.join(ROOT, "julia", "hipTile.jl")) == _lib.PARAM_ORDER
    assert _julia_params(os.path.join(ROOT, "INTEGRATION.md")) == _lib.PARAM_ORDER


def test_python_mirror_packs_the_mean_depth():
    """model_desc (the sx_model_desc the Python mirror hands to sx_create) carries :H at SX_P_H and accepts the new names."""
    import scythe_jl_amd as S
    from scythe_jl_amd import _lib
    from scythe_jl_amd.model import model_desc
    for eq, geometry, nv in (("LinearShallowWater1D", "R", LS.VARS_1D), ("LinearShallowWaterRL", "RL", LS.VARS_RL)):
        gp = S.GridParameters(geometry=geometry, xmin=0.0, xmax=1.0, num_cells=10, vars=nv)
        mp = S.ModelParameters(ts=1.0, equation_set=eq, grid_params=gp, physical_params={":g": 9.81, ":K": 3.0, ":H": 250.0})
        m, keep = model_desc(mp, gp)
        assert m.equation_set == {"LinearShallowWater1D": 9, "LinearShallowWaterRL": 10}[eq]
        par = list(keep["par"])
        assert len(par) == 13 and par[_lib.PARAM_ORDER.index("H")] == 250.0 and par[0] == 9.81 and par[1] == 3.0
    gp = S.GridParameters(geometry="RL", xmin=0.0, xmax=1.0, num_cells=10, vars=LS.VARS_RL)
    with pytest.raises(ValueError, match="not defined"):
        model_desc(S.ModelParameters(ts=1.0, equation_set="ShallowWaterRL", grid_params=gp), gp)


def _packed_params(case):
    """The physical parameters as sx_create receives them (scythe_jl_amd.model.model_desc), read back by name."""
    from scythe_jl_amd import _lib
    from scythe_jl_amd.model import model_desc
    gp, mp = cases.hip_params(case)
    _, keep = model_desc(mp, gp)
    return dict(zip(_lib.PARAM_ORDER, list(keep["par"])))


def periodic_mode_error(num_cells, ts, steps, K, m=2, g=2.0, H=0.5):
    """Oracle twin (numpy restatement of LinearShallowWater1D) on the PERIODIC line [-6, 6], started from the right-moving
    gravity wave h = cos(kap x), u = sqrt(g / H) cos(kap x); error of h and of u / sqrt(g / H) against tests/linear_sw.py::mode_1d."""
    kap = 2.0 * np.pi * m / 12.0
    u0 = np.sqrt(g / H) + 0.0j
    keep = {}

    def ic(p):
        keep["x"] = p[:, 0]
        return np.stack(LS.mode_1d(p[:, 0], 0.0, kap, g, H, K, 1.0, u0), axis=1)
    case = LS.r_case(num_cells=num_cells, K=K, ts=ts, g=g, H=H)
    case["ic"] = ic
    case["par"] = _packed_params(case)
    assert (case["par"]["g"], case["par"]["K"], case["par"]["H"]) == (g, K, H)
    orc = cases.OracleModel(case, numpy_twin=True)
    for _ in range(steps):
        orc.step()
    ph = orc.physical()
    h, u = LS.mode_1d(keep["x"], ts * steps, kap, g, H, K, 1.0, u0)
    h0, _ = LS.mode_1d(keep["x"], 0.0, kap, g, H, K, 1.0, u0)
    return max(np.abs(ph[:, 0, 0] - h).max(), np.abs(ph[:, 1, 0] - u).max() / abs(u0)), np.abs(h - h0).max()


@pytest.mark.parametrize("K", [0.0, 0.05])
def test_numpy_restatement_follows_the_exact_periodic_mode(K):
    """24 cells, 150 steps of 0.02: the wave (c = sqrt(g H) = 1, wavelength 6) travels half a wavelength, h changes by ~2;
    the twin stays within 3.3e-3 of the 2 x 2 matrix-exponential solution (the spline's truncation error at kap DX = 0.52) -
    a wrong sign, a swapped g / H or a missing term is an O(1) difference."""
    err, change = periodic_mode_error(24, 0.02, 150, K)
    print("\nLinearShallowWater1D twin, K = %g: h changed by %.2f, error %.2e" % (K, change, err))
    assert change > 1.8 and err < 1e-2
