"""Host-side mirror of the reference's interface for the spectral-transform time-stepping path.

Names, argument meaning and error behaviour follow the reference (Julia); `!` is spelled with a trailing
underscore.  Every object that computes anything is a thin wrapper over a libscythe_hip handle.

  GridParameters      src/spectralGrid.jl:20-45 (vestige of the live Springsteel definition)
  ModelParameters     src/Scythe.jl:8-21
  createGrid          src/spectralGrid.jl:63-94
  ModelTile           src/semiimplicit.jl:18-42
  createModelTile     src/semiimplicit.jl:44-124
  advanceTimestep     src/semiimplicit.jl:301-332
"""
import collections
import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from . import _lib as L


# ----------------------------------------------------------------------------- boundary-condition namespaces
class CubicBSpline:
    """Boundary-condition tags (Dicts in the reference: CubicBSpline.R0 etc., models/*.jl)."""
    mubar = 3
    R0 = {"R0": 0}
    R1T0 = {"α1": -4.0, "β1": -1.0}
    R1T1 = {"α1": 0.0, "β1": 1.0}
    R1T2 = {"α1": 2.0, "β1": -1.0}
    R2T10 = {"β1": 1.0, "β2": -0.5}
    R2T20 = {"β1": -1.0, "β2": 0.0}
    R3 = {"R3": 0}
    PERIODIC = {"PERIODIC": 0}


class Chebyshev:
    R0 = {"R0": 0}
    R1T0 = {"α0": 0.0}
    R1T1 = {"α1": 0.0}
    R1T2 = {"α2": 0.0}


_SPLINE_BCS = [(CubicBSpline.R0, "R0"), (CubicBSpline.R1T0, "R1T0"), (CubicBSpline.R1T1, "R1T1"),
               (CubicBSpline.R1T2, "R1T2"), (CubicBSpline.R2T10, "R2T10"), (CubicBSpline.R2T20, "R2T20"),
               (CubicBSpline.R3, "R3"), (CubicBSpline.PERIODIC, "PERIODIC")]
_CHEB_BCS = [(Chebyshev.R0, "R0"), (Chebyshev.R1T0, "R1T0"), (Chebyshev.R1T1, "R1T1"), (Chebyshev.R1T2, "R1T2")]


def bc_name(bc, table=_SPLINE_BCS):
    """Dict tag (or plain string) -> canonical BC name."""
    if isinstance(bc, str):
        if bc not in L.BC:
            raise ValueError("Unknown boundary condition %r" % (bc,))
        return bc
    for d, name in table:
        if bc == d:
            return name
    raise ValueError("Unknown boundary condition %r" % (bc,))


def _default_b_zDim(zDim):
    return int(min(zDim, math.floor(((2 * zDim) - 1) / 3) + 1)) if zDim > 0 else 0


# ----------------------------------------------------------------------------- parameters
@dataclass
class GridParameters:
    geometry: str = "R"
    xmin: float = 0.0
    xmax: float = 0.0
    num_cells: int = 0
    rDim: Optional[int] = None
    b_rDim: Optional[int] = None
    l_q: float = 2.0
    BCL: Dict = field(default_factory=dict)
    BCR: Dict = field(default_factory=dict)
    lDim: int = 0
    b_lDim: int = 0
    zmin: float = 0.0
    zmax: float = 0.0
    zDim: int = 0
    b_zDim: Optional[int] = None
    BCB: Dict = field(default_factory=dict)
    BCT: Dict = field(default_factory=dict)
    vars: Dict = field(default_factory=lambda: {"u": 1})
    spectralIndexL: int = 1
    spectralIndexR: Optional[int] = None
    patchOffsetL: Optional[int] = None
    patchOffsetR: Optional[int] = None
    tile_num: int = 0
    # extensions (not in the reference): uniform ring table and a separate k = 0 inner BC
    ring_uniform_L: int = 0
    BCL_k0: Optional[Dict] = None
    storage: str = "f64"       # "f32": derivative slots of `physical` stored as fp32; "f32x": also the spectral transform
                               # intermediates (sx_grid_desc.storage_f32 = 1 / 2)

    def __post_init__(self):
        if self.rDim is None:
            self.rDim = self.num_cells * CubicBSpline.mubar
        if self.b_rDim is None:
            self.b_rDim = self.num_cells + 3
        if self.b_zDim is None:
            self.b_zDim = _default_b_zDim(self.zDim)
        if self.spectralIndexR is None:
            self.spectralIndexR = self.spectralIndexL + self.b_rDim - 1
        if self.patchOffsetL is None:
            self.patchOffsetL = (self.spectralIndexL - 1) * 3
        if self.patchOffsetR is None:
            self.patchOffsetR = self.patchOffsetL + self.rDim

    def var_names(self):
        return [n for n, _ in sorted(self.vars.items(), key=lambda kv: kv[1])]


@dataclass
class ModelParameters:
    ts: float = 0.0
    integration_time: float = 1.0
    output_interval: float = 1.0
    equation_set: str = "LinearAdvection1D"
    initial_conditions: str = "ic.csv"
    output_dir: str = "./output/"
    ref_state_file: str = ""
    grid_params: GridParameters = None
    physical_params: Dict = field(default_factory=dict)
    options: Dict = field(default_factory=lambda: {"semiimplicit": False, "exact_reference_state": False})
    ref_state: object = None       # ReferenceState; built from ref_state_file when the equation set needs one and this is None


# ----------------------------------------------------------------------------- descriptors
def _i32(values):
    return (C.c_int32 * len(values))(*values)


def grid_desc(patch: GridParameters, tile_cell0=0, tile_num_cells=None, tile_num=0):
    """Flatten patch GridParameters (+ tile range) into the C descriptor. Returns (desc, keepalive)."""
    if patch.geometry not in L.GEOM:
        raise ValueError("Unknown geometry")          # DomainError(0, "Unknown geometry") src/spectralGrid.jl:90
    names = patch.var_names()
    d = L.GridDesc()
    keep = {}
    get = lambda dct, n, table: L.BC[bc_name((dct or {}).get(n, "R0"), table)]
    keep["bcl"] = _i32([get(patch.BCL, n, _SPLINE_BCS) for n in names])
    keep["bcr"] = _i32([get(patch.BCR, n, _SPLINE_BCS) for n in names])
    k0 = patch.BCL_k0 if patch.BCL_k0 is not None else patch.BCL
    keep["bcl0"] = _i32([get({**(patch.BCL or {}), **(k0 or {})}, n, _SPLINE_BCS) for n in names])
    keep["bcb"] = _i32([get(patch.BCB, n, _CHEB_BCS) for n in names])
    keep["bct"] = _i32([get(patch.BCT, n, _CHEB_BCS) for n in names])
    d.abi_version, d.geometry = L.SX_ABI_VERSION, L.GEOM[patch.geometry]
    d.xmin, d.xmax, d.num_cells, d.l_q, d.nvars = patch.xmin, patch.xmax, patch.num_cells, patch.l_q, len(names)
    d.bcl, d.bcl_k0, d.bcr = keep["bcl"], keep["bcl0"], keep["bcr"]
    d.zmin, d.zmax, d.zDim, d.b_zDim = patch.zmin, patch.zmax, patch.zDim, patch.b_zDim or 0
    d.bcb, d.bct = keep["bcb"], keep["bct"]
    d.ring_uniform_L = patch.ring_uniform_L
    d.tile_cell0 = tile_cell0
    d.tile_num_cells = patch.num_cells if tile_num_cells is None else tile_num_cells
    d.tile_num = tile_num
    if patch.storage not in ("f64", "f32", "f32x"):
        raise ValueError("GridParameters.storage must be 'f64', 'f32' or 'f32x'")
    d.storage_f32 = {"f64": 0, "f32": 1, "f32x": 2}[patch.storage]
    return d, keep


RAINFALL_VARS = {"s": 1, "xi": 2, "mu": 3, "u": 4, "w": 5, "mu_c": 6, "mu_r": 7, "qss": 8}


def model_desc(model: Optional[ModelParameters], patch: GridParameters):
    m = L.ModelDesc()
    keep = {}
    lib = L.load()
    if model is None:
        m.ts, m.equation_set, m.semiimplicit = 0.0, 99, 0
        keep["par"] = (C.c_double * len(L.PARAM_ORDER))()
    else:
        eq = lib.sx_equation_set_id(model.equation_set.encode())
        if eq < 0:
            # getfield(Scythe, Symbol(...)) raises UndefVarError for an unknown name (src/semiimplicit.jl:359-361)
            raise ValueError("equation set %r is not defined on the HIP path" % model.equation_set)
        pp = {(k if isinstance(k, str) else str(k)).lstrip(":"): v for k, v in model.physical_params.items()}
        opts = {str(k).lstrip(":"): v for k, v in (model.options or {}).items()}
        if model.equation_set == "rainfall_test" and patch.vars != RAINFALL_VARS:
            # its tendency reads the variables by position (src/testModels.jl:404-450), condensation_adjustment by name
            # (src/microphysics.jl:142-165): any other mapping would mix the two
            raise ValueError("rainfall_test needs grid_params.vars = %r" % (RAINFALL_VARS,))
        if model.equation_set in ("Euler_test", "rainfall_test"):
            # createModelTile builds mtile.ref_state from model.ref_state_file (src/semiimplicit.jl:44-124)
            if model.ref_state is None:
                from . import reference_state as RS
                build = RS.exact_reference_state if opts.get("exact_reference_state", False) else RS.interpolate_reference_file
                model.ref_state = build(model)
            keep["ref"] = model.ref_state.packed()
            m.ref_state = keep["ref"].ctypes.data_as(L.P_D)
            pp.setdefault("Pxi_bar", model.ref_state.Pxi_bar)
        keep["par"] = (C.c_double * len(L.PARAM_ORDER))(*[float(pp.get(k, 0.0)) for k in L.PARAM_ORDER])
        m.ts, m.equation_set = model.ts, eq
        m.semiimplicit = int(bool(opts.get("semiimplicit", False)))
    m.params = keep["par"]
    m.w_index = patch.vars.get("w", 0)
    m.xi_index = patch.vars.get("xi", 0)
    m.col_var = patch.vars.get("h", 0)
    return m, keep


def calcTileSizes(patch: GridParameters, num_tiles: int):
    """calcTileSizes(patch, n) -> 5 x n matrix: xmin, xmax, num_cells, spectralIndexL, gridpoints
    (src/semiimplicit.jl:141-144, 157-168)."""
    d, keep = grid_desc(patch)
    out = np.zeros((5, num_tiles), order="F")
    L.check(L.load().sx_calc_tile_sizes(C.byref(d), num_tiles, out.ctypes.data_as(L.P_D)))
    return out


# ----------------------------------------------------------------------------- grid / tile objects
class Grid:
    """A tile (or the whole patch) resident on the GPU: createGrid(GridParameters) + the ModelTile state."""

    def __init__(self, patch: GridParameters, model: Optional[ModelParameters] = None, tile_cell0=0,
                 tile_num_cells=None, tile_num=0):
        lib = L.load()
        self.patch_params = patch
        self.model = model
        gd, k1 = grid_desc(patch, tile_cell0, tile_num_cells, tile_num)
        md, k2 = model_desc(model, patch)
        h = C.c_void_p()
        L.check(lib.sx_create(C.byref(gd), C.byref(md), C.byref(h)))
        self._h = h
        self._lib = lib
        dims = L.Dims()
        L.check(lib.sx_get_dims(h, C.byref(dims)))
        self.dims = dims
        self.cell0 = tile_cell0
        self.ncells = patch.num_cells if tile_num_cells is None else tile_num_cells
        DX = (patch.xmax - patch.xmin) / patch.num_cells
        self.params = GridParameters(
            geometry=patch.geometry, xmin=patch.xmin + tile_cell0 * DX, xmax=patch.xmin + (tile_cell0 + self.ncells) * DX,
            num_cells=self.ncells, l_q=patch.l_q, BCL={k: CubicBSpline.R0 for k in patch.vars},
            BCR={k: CubicBSpline.R0 for k in patch.vars}, lDim=int(dims.n_hpoints) if "L" in patch.geometry else 0,
            zmin=patch.zmin, zmax=patch.zmax, zDim=patch.zDim, b_zDim=patch.b_zDim, BCB=patch.BCB, BCT=patch.BCT,
            vars=patch.vars, spectralIndexL=tile_cell0 + 1, tile_num=tile_num, ring_uniform_L=patch.ring_uniform_L,
            storage=patch.storage)

    def close(self):
        for g in self.__dict__.pop("_companions", {}).values():
            g.close()
        if getattr(self, "_h", None):
            self._lib.sx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- shapes
    @property
    def N(self):
        return int(self.dims.n_points)

    @property
    def V(self):
        return int(self.dims.n_vars)

    @property
    def D(self):
        return int(self.dims.n_derivs)

    @property
    def n_cols(self):
        return int(self.dims.n_cols)

    # -- state access (reference layouts, Fortran order == Julia column-major)
    def set_physical_values(self, values):
        v = np.asfortranarray(values, dtype=np.float64)
        assert v.shape == (self.N, self.V), (v.shape, (self.N, self.V))
        L.check(self._lib.sx_set_physical_values(self._h, v.ctypes.data_as(L.P_D)))

    @property
    def physical(self):
        out = np.zeros((self.N, self.V, self.D), order="F")
        L.check(self._lib.sx_get_physical(self._h, out.ctypes.data_as(L.P_D)))
        return out

    def get_state(self):
        """Restart blob of this tile (A coefficients + Adams-Bashforth history), see sx_get_state."""
        n = C.c_int64(0)
        L.check(self._lib.sx_state_size(self._h, C.byref(n)))
        out = np.zeros(n.value)
        L.check(self._lib.sx_get_state(self._h, out.ctypes.data_as(L.P_D)))
        return out

    def set_state(self, blob):
        b = np.ascontiguousarray(blob, dtype=np.float64)
        L.check(self._lib.sx_set_state(self._h, b.ctypes.data_as(L.P_D)))

    @property
    def var_np1(self):
        out = np.zeros((self.N, self.V), order="F")
        L.check(self._lib.sx_get_var_np1(self._h, out.ctypes.data_as(L.P_D)))
        return out

    @property
    def spectral(self):
        """tile.spectral (B coefficients) in the reference tile layout."""
        out = np.zeros((int(self.dims.s_tile), self.V), order="F")
        L.check(self._lib.sx_get_tile_spectral(self._h, out.ctypes.data_as(L.P_D)))
        return out

    def set_patch_spectral_b(self, shared):
        s = np.asfortranarray(shared, dtype=np.float64)
        assert s.shape == (int(self.dims.s_patch), self.V)
        L.check(self._lib.sx_set_patch_spectral_b(self._h, s.ctypes.data_as(L.P_D)))

    def set_patch_spectral_a(self, a):
        s = np.asfortranarray(a, dtype=np.float64)
        assert s.shape == (int(self.dims.s_patch), self.V)
        L.check(self._lib.sx_set_patch_spectral_a(self._h, s.ctypes.data_as(L.P_D)))

    @property
    def patchSpectral(self):
        out = np.zeros((int(self.dims.s_patch), self.V), order="F")
        L.check(self._lib.sx_get_patch_spectral_a(self._h, out.ctypes.data_as(L.P_D)))
        return out

    def evaluate(self, points, all_k=False, k_band=None):
        """The spectral state (the A coefficients the tile holds now) at arbitrary points of the tile: points [n, n_coord] with
        columns r[, lambda][, z] as getGridpoints returns them -> ndarray [n, V, D], slots as in `physical` (sx_evaluate).
        all_k=False cuts the azimuthal series at the kmax of the last ring at or below each radius, as tileTransform! does on the
        rings; all_k=True sums every wavenumber of the patch.  k_band=(kmin, kmax) sums the wavenumbers kmin <= k <= kmax only
        (sx_evaluate_band): (2, 2) is the wave-2 part of every field."""
        nc = int(self.dims.n_coord)
        p = np.asarray(points, dtype=np.float64)
        p = np.asfortranarray(p.reshape(-1, nc) if p.ndim != 2 else p)
        if p.shape[1] != nc:
            raise ValueError("points must have %d coordinate column(s)" % nc)
        out = np.zeros((p.shape[0], self.V, self.D), order="F")
        flags = L.EVAL_ALL_K if all_k else L.EVAL_RING_K
        if k_band is None:
            L.check(self._lib.sx_evaluate(self._h, p.ctypes.data_as(L.P_D), p.shape[0], flags, out.ctypes.data_as(L.P_D)))
        else:
            L.check(self._lib.sx_evaluate_band(self._h, p.ctypes.data_as(L.P_D), p.shape[0], flags, int(k_band[0]), int(k_band[1]),
                                               out.ctypes.data_as(L.P_D)))
        return out

    # -- Lagrangian parcels (sx_parcels_*)
    def _parcel_var(self, v):
        """1-based variable index of a velocity component given by name, by 1-based index, or None / 0 (no motion)"""
        if v is None or (isinstance(v, (int, np.integer)) and int(v) == 0):
            return 0
        if isinstance(v, str):
            names = self.patch_params.var_names()
            if v not in names:
                raise ValueError("velocity variable %r is not one of %s" % (v, names))
            return names.index(v) + 1
        return int(v)

    def set_parcels(self, points, velocity):
        """Create or replace the tile's parcel set: points [n, n_coord] with columns r[, lambda][, z] as getGridpoints returns them,
        velocity = one entry per coordinate, in that order (R: (u,), RZ: (u, w), RL: (u, v), RLZ: (u, v, w)), each a variable name, a
        1-based variable index, or None / 0 for no motion along that coordinate.  The components are speeds: the azimuthal one is
        the tangential wind.  An empty `points` removes the set.  Refusals leave an existing set as it is (sx_parcels_set)."""
        nc = int(self.dims.n_coord)
        p = np.asarray(points, dtype=np.float64)
        p = np.asfortranarray(p.reshape(-1, nc) if p.ndim != 2 else p)
        if p.shape[1] != nc:
            raise ValueError("points must have %d coordinate column(s)" % nc)
        vel = [velocity] if isinstance(velocity, (str, int, np.integer)) or velocity is None else list(velocity)
        if len(vel) != nc:
            raise ValueError("velocity must name %d component(s), one per coordinate of a %s grid" % (nc, self.patch_params.geometry))
        var = dict(zip(self.patch_params.geometry.lower(), (self._parcel_var(v) for v in vel)))
        L.check(self._lib.sx_parcels_set(self._h, p.shape[0], p.ctypes.data_as(L.P_D), var.get("r", 0), var.get("l", 0), var.get("z", 0)))

    def advance_parcels(self, dt):
        """One step of every active parcel with the A coefficients the tile holds now: one kernel on the tile's stream, no
        synchronisation (sx_parcels_advance).  Without a set it does nothing."""
        L.check(self._lib.sx_parcels_advance(self._h, float(dt)))

    @property
    def n_parcels(self):
        n = C.c_int64(0)
        L.check(self._lib.sx_parcels_count(self._h, C.byref(n)))
        return int(n.value)

    def parcels(self):
        """(positions [n, n_coord], velocity [n, n_coord] as last evaluated, status [n] int32: 0 active, 1 left radially, 2 left
        vertically); empty arrays without a set.  Synchronises."""
        n, nc = self.n_parcels, int(self.dims.n_coord)
        pos, vel, st = np.zeros((n, nc), order="F"), np.zeros((n, nc), order="F"), np.zeros(n, dtype=np.int32)
        L.check(self._lib.sx_parcels_get(self._h, pos.ctypes.data_as(L.P_D), vel.ctypes.data_as(L.P_D), st.ctypes.data_as(L.P_I32)))
        return pos, vel, st

    def get_parcel_state(self):
        """Restart blob of the parcel set (sx_parcels_get_state), or None without a set"""
        n = C.c_int64(0)
        L.check(self._lib.sx_parcels_state_size(self._h, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros(n.value)
        L.check(self._lib.sx_parcels_get_state(self._h, out.ctypes.data_as(L.P_D)))
        return out

    def set_parcel_state(self, blob):
        b = np.ascontiguousarray(blob, dtype=np.float64)
        L.check(self._lib.sx_parcels_set_state(self._h, b.ctypes.data_as(L.P_D), b.size))

    # -- elliptic inversion (sx_elliptic_solve)
    def invert(self, rhs, alpha=0.0, into=None, var=1):
        """Solve (lap_h - alpha) psi = f on the device from the A coefficients the tile holds now (sx_elliptic_solve) and write the
        A coefficients of psi into variable `var` (a name or a 1-based index) of the Grid `into`; returns that Grid, on which
        evaluate, harmonics, spectrum and tileTransform_ + physical then sample psi and its derivatives.
        rhs = ("field", f), ("vorticity", u, v) or ("divergence", u, v), the variables by name or 1-based index: f itself, or the
        vorticity v_r + v / r - u_l / r resp. the divergence u_r + u / r + v_l / r of the wind (u, v) (RL / RLZ grids).
        into=None makes a one-variable companion (companion_grid: psi = 0 at the outer edge, regular at the centre, the vertical
        conditions of the first source variable) on first use and keeps it; into=self writes a spare variable of this Grid.
        rhs may also be a field program - a list of (coef, r_power, [(var, slot), ...]) terms read from `physical` as it stands, the
        forcing of a balance or omega equation - which is projected first (project).
        The boundary conditions of psi are those of the destination variable.  One-tile patches only."""
        if isinstance(rhs, (tuple, list)) and rhs and not isinstance(rhs[0], str):
            # a field program as the forcing: projected into a one-variable companion (project), which is then the ("field", 1) source
            return self.project_companion(["f"]).project_from(self, [(0,) + tuple(t)[-3:] for t in rhs]).invert(("field", 1), alpha, into, var)
        if not isinstance(rhs, (tuple, list)) or not rhs or rhs[0] not in L.ELL_KIND or len(rhs) != (2 if rhs[0] == "field" else 3):
            raise ValueError("rhs must be ('field', f), ('vorticity', u, v) or ('divergence', u, v)")
        src = [self._parcel_var(v) for v in rhs[1:]]
        if into is None:
            names = self.patch_params.var_names()
            if not 1 <= src[0] <= len(names):
                raise ValueError("variable index %d out of range" % src[0])
            n0 = names[src[0] - 1]
            key = (bc_name((self.patch_params.BCB or {}).get(n0, "R0"), _CHEB_BCS), bc_name((self.patch_params.BCT or {}).get(n0, "R0"), _CHEB_BCS))
            cache = self.__dict__.setdefault("_companions", {})
            if key not in cache:
                cache[key] = companion_grid(self.patch_params, bcb=key[0], bct=key[1])
            into = cache[key]
        dst = into.patch_params.vars[var] if isinstance(var, str) else int(var)
        L.check(self._lib.sx_elliptic_solve(self._h, L.ELL_KIND[rhs[0]], src[0], src[1] if len(src) > 1 else 0, float(alpha), into._h, dst))
        return into

    # -- antiderivatives (sx_antiderivative)
    def antiderivative(self, var, axis="r", origin="low", weight_r=False, dst=None, var_dst=1):
        """The integral of variable `var` (a name or a 1-based index) up to a point, on the device from the A coefficients the tile
        holds now (sx_antiderivative), written as the A coefficients of variable `var_dst` of the Grid `dst`; returns that Grid, on
        which evaluate, harmonics, spectrum, crossings, extrema and tileTransform_ + physical then sample it like any field.
        axis="r": F(r) = int_{xmin}^{r} f ds (origin="low") or int_{r}^{xmax} f ds ("high"); weight_r=True integrates r f (the area
        element of a vortex: circulation, enclosed mass).  axis="z": F(z) = int_{zmin}^{z} f dz' or int_{z}^{zmax} f dz'.
        dst=None makes a one-variable companion on first use and keeps it, one per set of boundary conditions: the source's own
        vertical and radial conditions carried over, except that along the axis of integration the result is left free (R0) - an
        integral from xmin does not vanish at xmax.  dst=self writes a spare variable of this Grid.  `var` may also be a field
        program, a list of (coef, r_power, [(var, slot), ...]) terms read from `physical` as it stands (w from the divergence, the mass
        streamfunction from rho u), which is projected first (project).  One-tile patches only."""
        if axis not in L.INT_AXIS or origin not in L.INT_ORIGIN:
            raise ValueError("axis must be 'r' or 'z' and origin 'low' or 'high'")
        if isinstance(var, (tuple, list)):
            # a field program (terms as for invert's rhs): projected into a one-variable companion, which is then the source
            return self.project_companion(["f"]).project_from(self, [(0,) + tuple(t)[-3:] for t in var]).antiderivative(1, axis, origin, weight_r, dst, var_dst)
        src = self._parcel_var(var)
        if dst is None:
            gp = self.patch_params
            names = gp.var_names()
            if not 1 <= src <= len(names):
                raise ValueError("variable index %d out of range" % src)
            n0 = names[src - 1]
            of = lambda d, table: bc_name((d or {}).get(n0, "R0"), table)
            bcl, bcr = of(gp.BCL, _SPLINE_BCS), of(gp.BCR, _SPLINE_BCS)
            bcl0 = bc_name((gp.BCL_k0 or {}).get(n0, (gp.BCL or {}).get(n0, "R0")), _SPLINE_BCS)
            bcb, bct = of(gp.BCB, _CHEB_BCS), of(gp.BCT, _CHEB_BCS)
            key = ("R0", "R0", "R0", bcb, bct) if axis == "r" else (bcl, bcl0, bcr, "R0", "R0")
            cache = self.__dict__.setdefault("_antiderivative_companions", {})
            if key not in cache:
                cache[key] = companion_grid(gp, bcl=key[0], bcl_k0=key[1], bcr=key[2], bcb=key[3], bct=key[4], name="F")
            dst = cache[key]
        vd = dst.patch_params.vars[var_dst] if isinstance(var_dst, str) else int(var_dst)
        L.check(self._lib.sx_antiderivative(self._h, src, L.INT_AXIS[axis], L.INT_ORIGIN[origin], int(bool(weight_r)), dst._h, vd))
        return dst

    # -- field programs as variables (sx_project)
    def project(self, terms, into, source="physical", var_dst=None):
        """Evaluate a field program at this tile's gridpoints on the device and make its outputs the variables of the companion
        Grid `into` (sx_project): output o becomes variable var_dst[o] (names or 1-based indices of `into`; default 1, 2, ...), as
        var_np1 and, through into's own forward transform and banded solve, as B and A coefficients.  terms, source: as for reduce
        (the same programs, packed by pack_reduce_program against THIS grid).  `into` must have as many variables as the program has
        outputs, this grid's geometry, extent, cells, ring table and levels (companion_grid(..., names=[...])), and no equation set;
        its `physical` is stale until into.tileTransform_().  Nothing of this Grid changes.  Returns `into`.  One-tile patches only."""
        coef, packed, n_out = pack_reduce_program(self.patch_params, terms)
        if source not in L.REDUCE_SOURCE:
            raise ValueError("source must be 'physical' or 'state'")
        vd = _project_var_dst(into.patch_params, n_out, var_dst)
        L.check(self._lib.sx_project(self._h, L.REDUCE_SOURCE[source], len(coef), coef.ctypes.data_as(L.P_D), packed.ctypes.data_as(L.P_I32),
                                     n_out, into._h, vd.ctypes.data_as(L.P_I32) if len(vd) else None))
        return into

    def project_from(self, src, terms, source="physical", var_dst=None):
        """src.project(terms, self, ...): reads well where the companion is made in the same expression"""
        return src.project(terms, self, source, var_dst)

    def project_companion(self, names, **bcs):
        """The companion of this Grid with the variables `names` (companion_grid: every condition R0 unless `bcs` says otherwise -
        nothing is known of a derived field at the edges), made on first use and kept per (names, conditions)"""
        bcs = {**dict(bcl="R0", bcl_k0="R0", bcr="R0", bcb="R0", bct="R0"), **bcs}
        key = ("project", tuple(names), repr(sorted((k, sorted(v.items()) if isinstance(v, dict) else v) for k, v in bcs.items())))
        cache = self.__dict__.setdefault("_companions", {})
        if key not in cache:
            cache[key] = companion_grid(self.patch_params, names=list(names), **bcs)
        return cache[key]

    # -- function programs as variables (sx_derive)
    def derive(self, program, into, source="physical"):
        """Evaluate a function program at this tile's gridpoints on the device and make its outputs the variables of the companion
        Grid `into` (sx_derive): a field program's polynomial outputs followed by square roots, quotients, exp / log / pow / atan2 and
        the moist thermodynamics the model itself steps with.  program: outputs as pack_function_program reads them (a dict name ->
        expression or a list, one per variable of `into`, in its order), or what pack_function_program returned for THIS grid.  source
        and everything about `into` are Grid.project's.  Nothing of this Grid changes.  Returns `into`.  One-tile patches only."""
        fp = program if isinstance(program, FunctionProgram) else pack_function_program(self.patch_params, program)
        if source not in L.REDUCE_SOURCE:
            raise ValueError("source must be 'physical' or 'state'")
        if len(fp.reg_dst) != into.V:          # sx_derive reads one entry per variable of `into`
            raise ValueError("derive: %d outputs for the %d variables of the destination" % (len(fp.reg_dst), into.V))
        L.check(self._lib.sx_derive(self._h, L.REDUCE_SOURCE[source], *fp.args(), into._h, fp.reg_dst.ctypes.data_as(L.P_I32) if len(fp.reg_dst) else None))
        return into

    # -- onto another grid (sx_regrid)
    def regrid(self, dst_grid, centre=None, variables=None, outside="refuse", fill=None):
        """Lay this tile's state down on the Grid `dst_grid` (sx_regrid): every variable of dst_grid receives, at dst_grid's gridpoints,
        the continuous function evaluate(..., all_k=True) gives of a variable of this grid, as var_np1 and, through dst_grid's own
        forward transform and banded solve, as B and A.  variables [dst V]: the source variable of each (names or 1-based indices of
        THIS grid; default: dst_grid's own names looked up here).  centre=(x0, y0): dst_grid's axis in this grid's Cartesian frame
        (RL / RLZ only; None: the same axis).  Extent, cells, rings, levels and boundary conditions of the two may differ; dst_grid's
        [zmin, zmax] must lie within this grid's.  outside="refuse" fails when a column of dst_grid lies outside this grid's
        [xmin, xmax]; "fill" writes fill[v] (a scalar serves every variable) there.  Returns the number of such columns.
        dst_grid's `physical` and tendency history are stale: its next step must be t = 1.  Nothing of this Grid changes.  One-tile
        patches only."""
        if outside not in L.REGRID_OUTSIDE:
            raise ValueError("outside must be 'refuse' or 'fill'")
        vs = _regrid_var_src(self.patch_params, dst_grid.patch_params, variables)
        c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64).reshape(2)
        f = None if fill is None else np.ascontiguousarray(np.broadcast_to(np.asarray(fill, dtype=np.float64), (dst_grid.V,)))
        n = C.c_int64(0)
        L.check(self._lib.sx_regrid(self._h, dst_grid._h, None if c is None else c.ctypes.data_as(L.P_D), vs.ctypes.data_as(L.P_I32),
                                    L.REGRID_OUTSIDE[outside], None if f is None else f.ctypes.data_as(L.P_D), C.byref(n)))
        return int(n.value)

    def harmonics(self, radii, heights=None, all_k=False, slots=("u",)):
        """The azimuthal harmonics c_k(r, z) of the state (sx_harmonics) at every radius x every height: complex128 ndarray indexed
        [ir, iz, k, v, s], k = 0 .. kDim, s over `slots` in the order u, r, rr, z, zz (a view of the library's buffer).  The state is
        Re sum_k eps_k c_k e^{i k lambda}, eps_0 = 1, eps_k = 2; on a ring of the grid c_k is the discrete transform of the ring's
        values.  heights stays None on a grid without a vertical (iz has length 1).  all_k as for evaluate: entries above the
        wavenumber cap of a radius are zero."""
        names = [s for s in L.HARM_SLOTS if s in slots]
        if not names or len(names) != len(set(slots)) or set(slots) - set(L.HARM_SLOTS):
            raise ValueError("slots must be a non-empty subset of %s" % (L.HARM_SLOTS,))
        mask = sum(1 << L.HARM_SLOTS.index(s) for s in names)
        r = np.ascontiguousarray(np.asarray(radii, dtype=np.float64).reshape(-1))
        z = None if heights is None else np.ascontiguousarray(np.asarray(heights, dtype=np.float64).reshape(-1))
        nz = 1 if z is None else len(z)
        K = int(self.dims.kDim) + 1
        out = np.zeros((2 * K, nz, len(r), self.V, len(names)), order="F")
        L.check(self._lib.sx_harmonics(self._h, r.ctypes.data_as(L.P_D), len(r), None if z is None else z.ctypes.data_as(L.P_D),
                                       0 if z is None else len(z), L.EVAL_ALL_K if all_k else L.EVAL_RING_K, mask,
                                       out.ctypes.data_as(L.P_D)))
        c = out.T.view(np.complex128)                     # C-contiguous [s, v, ir, iz, 2K] -> [s, v, ir, iz, K]
        return c.transpose(2, 3, 4, 1, 0)

    def vortex_harmonics(self, centre, radii, heights=None, fields=("h",), n_az=None, kmax=4, motion=None):
        """The azimuthal harmonics of the state about `centre` = (x0, y0) in the Cartesian frame x = r cos lambda, y = r sin lambda,
        not about the grid's centre, on the device (sx_vortex_harmonics; reads the A coefficients the tile holds now).  radii are
        measured from the centre; heights stays None on a grid without a vertical.  fields: variable names (or 1-based indices) and
        ("wind", u, v) triples naming the grid's radial and tangential wind; a wind field gives TWO outputs, the radial and the
        tangential wind about the centre, with the storm motion `motion` = (cx, cy) subtracted when given.  n_az samples per circle
        (a multiple of 4; default: the smallest multiple of 4 above kDim + kmax, which does not alias when the centre is the grid's).
        Returns (c, status): c complex128 [n_out, n_rho, n_z, kmax + 1] with f = Re sum_k eps_k c_k e^{i k phi}, eps_0 = 1, eps_k = 2;
        status int32 [n_rho], 0 computed, 1 the circle leaves the tile (its outputs are NaN).  One-tile RL / RLZ patches."""
        packed, n_out = pack_vortex_fields(self.patch_params, fields)
        r = np.ascontiguousarray(np.asarray(radii, dtype=np.float64).reshape(-1))
        z = None if heights is None else np.ascontiguousarray(np.asarray(heights, dtype=np.float64).reshape(-1))
        nz = 1 if z is None else len(z)
        if n_az is None:
            n_az = default_vortex_n_az(int(self.dims.kDim), kmax)
        c0 = np.ascontiguousarray(np.asarray(centre, dtype=np.float64).reshape(-1))
        if len(c0) != 2:
            raise ValueError("centre must be (x0, y0)")
        m = None if motion is None else np.ascontiguousarray(np.asarray(motion, dtype=np.float64).reshape(-1))
        if m is not None and len(m) != 2:
            raise ValueError("motion must be (cx, cy)")
        K = max(int(kmax), 0) + 1
        out = np.zeros((2 * K, nz, len(r), n_out), order="F")
        status = np.zeros(len(r), dtype=np.int32)
        L.check(self._lib.sx_vortex_harmonics(self._h, c0.ctypes.data_as(L.P_D), None if m is None else m.ctypes.data_as(L.P_D),
                                              r.ctypes.data_as(L.P_D), len(r), None if z is None else z.ctypes.data_as(L.P_D),
                                              0 if z is None else len(z), int(n_az), int(kmax), len(packed), packed.ctypes.data_as(L.P_I32),
                                              out.ctypes.data_as(L.P_D), status.ctypes.data_as(L.P_I32)))
        c = out.T.view(np.complex128)                     # C-contiguous [n_out, n_rho, n_z, 2 K] -> [n_out, n_rho, n_z, K]
        return c, status

    def spectrum(self, pairs, kind="ring"):
        """Azimuthal power and cross spectra of the state on the device (sx_spectrum), from the A coefficients the tile holds now.
        pairs: a list of ((var_a, slot_a), (var_b, slot_b)), var a name or a 1-based index, slot one of u r rr z zz or 0 .. 4 (the
        slots of harmonics); a pair with a == b is a power spectrum; at most 16 pairs.  kind="ring": float64 ndarray
        [kDim + 1, tile rings, n_pairs], sum_level w_z eps_k Re(c_k^a conj(c_k^b)) at every ring - the radius-wavenumber diagram.
        kind="domain": [kDim + 1, n_pairs], the rings summed with 2 pi w_r: this tile's share of the domain integral per wavenumber.
        The sum over k is what reduce gives for the product field(a) field(b) (Parseval)."""
        packed = pack_spectrum_pairs(self.patch_params, pairs)
        if kind not in L.SPEC_KIND:
            raise ValueError("kind must be 'ring' or 'domain'")
        K = int(self.dims.kDim) + 1
        shape = (K, int(self.dims.tile_rDim), len(packed)) if kind == "ring" else (K, len(packed))
        out = np.zeros(shape, order="F")
        L.check(self._lib.sx_spectrum(self._h, L.SPEC_KIND[kind], len(packed), packed.ctypes.data_as(L.P_I32), out.ctypes.data_as(L.P_D)))
        return out

    def reduce(self, terms, kind="domain", source="physical"):
        """Integrals or azimuthal means of field products on the device (sx_reduce).  terms: a list of
        (out, coef, r_power, [(var, slot), ...]): coef * r^r_power * the product of the named fields is added to output `out`; var a
        name or a 1-based index, slot one of "" r rr l ll z zz or an index into `physical`'s slots; n_out = max(out) + 1.
        kind="domain": ndarray [n_out], this tile's share of the domain integral (Gauss-Legendre in r with the polar area element on
        RL / RLZ, 2 pi / L in lambda, Clenshaw-Curtis in z).  kind="azimuth": ndarray [tile rings, levels, n_out], the mean over
        lambda at every ring and level.  source="physical" reads `physical` as it stands (call tileTransform_ first);
        source="state" reads var_np1 (values only), complete after every step."""
        coef, packed, n_out = pack_reduce_program(self.patch_params, terms)
        if kind not in L.REDUCE_KIND or source not in L.REDUCE_SOURCE:
            raise ValueError("kind must be 'domain' or 'azimuth', source 'physical' or 'state'")
        nz = max(int(self.dims.zDim), 1)
        out = np.zeros(n_out) if kind == "domain" else np.zeros((int(self.dims.tile_rDim), nz, n_out), order="F")
        L.check(self._lib.sx_reduce(self._h, L.REDUCE_KIND[kind], L.REDUCE_SOURCE[source], len(coef), coef.ctypes.data_as(L.P_D),
                                    packed.ctypes.data_as(L.P_I32), n_out, out.ctypes.data_as(L.P_D)))
        return out

    def extrema(self, terms, kind="domain", source="physical"):
        """Minimum and maximum of field programs over the tile's gridpoints, with their locations, on the device (sx_extrema).
        terms, source: as for reduce (the same programs, packed by pack_reduce_program).  Returns (val, idx): kind="domain":
        float64 / int64 ndarrays [2, n_out], row 0 the minimum and row 1 the maximum; kind="azimuth": [2, tile rings, levels,
        n_out], minimum and maximum over lambda at every ring and level.  idx holds 0-based rows of getGridpoints(self).  Ties go to
        the lowest row (-0.0 == +0.0 is a tie); a NaN anywhere in a set makes both of its results NaN, with the lowest NaN row."""
        coef, packed, n_out = pack_reduce_program(self.patch_params, terms)
        if kind not in L.EXT_KIND or source not in L.REDUCE_SOURCE:
            raise ValueError("kind must be 'domain' or 'azimuth', source 'physical' or 'state'")
        nz = max(int(self.dims.zDim), 1)
        shape = (2, n_out) if kind == "domain" else (2, int(self.dims.tile_rDim), nz, n_out)
        val, idx = np.zeros(shape, order="F"), np.zeros(shape, dtype=np.int64, order="F")
        L.check(self._lib.sx_extrema(self._h, L.EXT_KIND[kind], L.REDUCE_SOURCE[source], len(coef), coef.ctypes.data_as(L.P_D),
                                     packed.ctypes.data_as(L.P_I32), n_out, val.ctypes.data_as(L.P_D), idx.ctypes.data_as(L.P_I64)))
        return val, idx

    def distribution(self, terms, edges, kind="domain", source="physical"):
        """Histogram of a field program over the tile's gridpoints, on the device (sx_distribution).  terms, source: as for reduce
        (packed by pack_reduce_program), 1 to 4 outputs: output 0 is the binned quantity q, outputs 1 .. 3 are integrands.  edges
        [n_bins + 1], finite and strictly increasing, n_bins <= 64.  Slots: 0 q < edges[0], 1 + b edges[b] <= q < edges[b + 1],
        n_bins + 1 q >= edges[-1], n_bins + 2 NaN.  kind="domain": one group, weights w_r w_l w_z (this tile's share: tiles add);
        kind="level": one group per level, weights w_r w_l (the horizontal area).  Returns Distribution(count int64 [n_bins + 3,
        groups], measure [n_bins + 3, groups] the sum of the weights, sums [n_bins + 3, n_out, groups] whose column 0 is the
        measure and column j the integral of integrand j over the points of the slot, edges).  Bitwise repeatable."""
        coef, packed, n_out = pack_reduce_program(self.patch_params, terms)
        if kind not in L.DIST_KIND or source not in L.REDUCE_SOURCE:
            raise ValueError("kind must be 'domain' or 'level', source 'physical' or 'state'")
        e = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64)
        nb = len(e) - 1
        groups = max(int(self.dims.zDim), 1) if kind == "level" else 1
        count = np.zeros((max(nb, 0) + 3, groups), dtype=np.int64, order="F")
        sums = np.zeros((max(nb, 0) + 3, max(n_out, 1), groups), order="F")
        L.check(self._lib.sx_distribution(self._h, L.DIST_KIND[kind], L.REDUCE_SOURCE[source], len(coef), coef.ctypes.data_as(L.P_D),
                                          packed.ctypes.data_as(L.P_I32), n_out, nb, e.ctypes.data_as(L.P_D),
                                          count.ctypes.data_as(L.P_I64), sums.ctypes.data_as(L.P_D)))
        return Distribution(count, sums[:, 0, :].copy(), sums, e)

    def refine_extremum(self, var, points, want="max", free=None, tol=None, max_iter=None):
        """The stationary point of variable `var` (a name or a 1-based index) nearest to each of `points` [n, n_coord], by Newton's
        iteration on the continuous spectral state, on the device (sx_extremum_refine; reads the A coefficients the tile holds now).
        want: "max", "min" or "any"; free: the coordinates that move, a string of r / l / z (default: all of the geometry) or a
        mask of SX_EXT_FREE_* bits - a frozen coordinate keeps its start value.  Returns Refined(pos [n, n_coord], value [n],
        grad [n, n_coord], status [n], iters [n]); status 0 converged, 1 / 2 left the tile radially / vertically, 3 inside the pole
        zone, 4 Hessian not definite as `want` asks, 5 max_iter reached.  One-tile patches only."""
        nc = int(self.dims.n_coord)
        p = np.asarray(points, dtype=np.float64)
        p = np.asfortranarray(p.reshape(-1, nc) if p.ndim != 2 else p)
        if p.shape[1] != nc:
            raise ValueError("points must have %d coordinate column(s)" % nc)
        if want not in L.EXT_WANT:
            raise ValueError("want must be 'max', 'min' or 'any'")
        n = p.shape[0]
        pos, grad = np.zeros((n, nc), order="F"), np.zeros((n, nc), order="F")
        value, status, iters = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        L.check(self._lib.sx_extremum_refine(self._h, self._parcel_var(var), L.EXT_WANT[want], free_mask(self.patch_params, free),
                                             0.0 if tol is None else float(tol), 0 if max_iter is None else int(max_iter), n,
                                             p.ctypes.data_as(L.P_D), pos.ctypes.data_as(L.P_D), value.ctypes.data_as(L.P_D),
                                             grad.ctypes.data_as(L.P_D), status.ctypes.data_as(L.P_I32), iters.ctypes.data_as(L.P_I32)))
        return Refined(pos, value, grad, status, iters)

    def crossings(self, terms, levels, rays, tol=None, max_iter=None, max_cross=4, return_profiles=False):
        """The radii at which a field program crosses `levels` along rays, on the device (sx_crossings; reads the A coefficients the
        tile holds now).  terms: a one-output program as for reduce (every out 0); rays [n_rays, n_coord - 1] with columns
        lambda[, z] (an R grid: the number of rays, or None for one); levels: up to 8.  Returns Crossings(radius [max_cross, n_levels,
        n_rays], dir of the same shape, count [n_levels, n_rays], status [n_rays], profiles): the first max_cross crossings of every
        level outward (unused entries NaN, dir 0), dir +1 where the program rises outward through the level and -1 where it falls,
        count the number found (it may exceed max_cross), status bit 0: a NaN on the ray, bit 1: a refinement ran out of
        iterations, bit 2: it met a NaN.  profiles: [num_cells + 3, n_profiles, n_rays] with return_profiles, else None.
        One-tile patches only."""
        coef, packed, n_out = pack_reduce_program(self.patch_params, terms)
        nrc = int(self.dims.n_coord) - 1
        if nrc == 0:
            n = 1 if rays is None else int(rays) if np.ndim(rays) == 0 else len(rays)
            q = np.zeros((n, 0))
        else:
            q = np.asarray(rays, dtype=np.float64)
            q = np.asfortranarray(q.reshape(-1, nrc) if q.ndim != 2 else q)
            if q.shape[1] != nrc:
                raise ValueError("rays must have %d coordinate column(s)" % nrc)
            n = q.shape[0]
        lev = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.float64)
        nl, mc = len(lev), int(max_cross)
        shape = (max(mc, 0), nl, n)
        radius, dirs = np.full(shape, np.nan, order="F"), np.zeros(shape, dtype=np.int32, order="F")
        count, status = np.zeros((nl, n), dtype=np.int32, order="F"), np.zeros(n, dtype=np.int32)
        prof = None
        if return_profiles:
            planes = reduce_planes(self.patch_params, terms) if len(coef) else np.zeros((0, 2), dtype=np.int32)
            slots = L.SLOTS[self.patch_params.geometry]
            keys = {(int(v), {"": 0, "r": 0, "rr": 0, "l": 1, "ll": 2, "z": 3, "zz": 4}[slots[int(s)]]) for v, s in planes}
            prof = np.zeros((int(self.dims.b_rDim), len(keys), n), order="F")
        L.check(self._lib.sx_crossings(self._h, len(coef), coef.ctypes.data_as(L.P_D), packed.ctypes.data_as(L.P_I32), n,
                                       q.ctypes.data_as(L.P_D) if nrc else None, nl, lev.ctypes.data_as(L.P_D),
                                       0.0 if tol is None else float(tol), 0 if max_iter is None else int(max_iter), mc,
                                       radius.ctypes.data_as(L.P_D), dirs.ctypes.data_as(L.P_I32), count.ctypes.data_as(L.P_I32),
                                       status.ctypes.data_as(L.P_I32), prof.ctypes.data_as(L.P_D) if prof is not None else None))
        return Crossings(radius, dirs, count, status, prof)

    def isosurface(self, terms, levels, columns, carry=0, tol=None, max_iter=None, max_cross=4, return_values=False, return_profiles=False):
        """The heights at which a field program crosses `levels` in columns, on the device (sx_isosurface; reads the A coefficients the
        tile holds now; RZ and RLZ grids).  terms: a program as for reduce with 1 + carry outputs - output 0 is the surface quantity,
        outputs 1 .. carry are evaluated on the surface; columns [n_cols, n_coord - 1] with columns r[, lambda]; levels: up to 8.
        Returns Isosurface(height [max_cross, n_levels, n_cols], dir of the same shape, count [n_levels, n_cols], status [n_cols],
        carry [carry, max_cross, n_levels, n_cols] or None, values [zDim, n_cols] or None, profiles [b_zDim, n_profiles, n_cols] or
        None): the first max_cross crossings of every level upward (unused entries NaN, dir 0), dir +1 where the program rises
        upward through the level and -1 where it falls, count the number found (it may exceed max_cross), status bit 0: a NaN in the
        column, bit 1: a refinement ran out of iterations, bit 2: it met a NaN.  values: the program at the zDim levels, bottom to
        top, as the kernel formed it.  One-tile patches only."""
        coef, packed, _ = pack_reduce_program(self.patch_params, terms)
        ncc = int(self.dims.n_coord) - 1
        q = np.asarray(columns, dtype=np.float64)
        q = np.asfortranarray(q.reshape(-1, max(ncc, 1)) if q.ndim != 2 else q)
        if q.shape[1] != ncc:
            raise ValueError("columns must have %d coordinate column(s)" % ncc)
        n, nc = q.shape[0], int(carry)
        lev = np.ascontiguousarray(np.atleast_1d(levels), dtype=np.float64)
        nl, mc = len(lev), int(max_cross)
        shape = (max(mc, 0), nl, n)
        height, dirs = np.full(shape, np.nan, order="F"), np.zeros(shape, dtype=np.int32, order="F")
        count, status = np.zeros((nl, n), dtype=np.int32, order="F"), np.zeros(n, dtype=np.int32)
        car = np.full((nc,) + shape, np.nan, order="F") if nc > 0 else None
        val = np.zeros((int(self.patch_params.zDim), n), order="F") if return_values else None
        prof = None
        if return_profiles:
            prof = np.zeros((int(self.patch_params.b_zDim), isosurface_check(self.patch_params, terms, nc), n), order="F")
        ptr = lambda a: a.ctypes.data_as(L.P_D) if a is not None else None
        L.check(self._lib.sx_isosurface(self._h, len(coef), coef.ctypes.data_as(L.P_D), packed.ctypes.data_as(L.P_I32), nc, n, ptr(q),
                                        nl, lev.ctypes.data_as(L.P_D), 0.0 if tol is None else float(tol),
                                        0 if max_iter is None else int(max_iter), mc, ptr(height), dirs.ctypes.data_as(L.P_I32),
                                        count.ctypes.data_as(L.P_I32), status.ctypes.data_as(L.P_I32), ptr(car), ptr(val), ptr(prof)))
        return Isosurface(height, dirs, count, status, car, val, prof)

    # -- statistics of field programs over time (sx_stats_*)
    def set_statistics(self, outputs, source="state", ops=None):
        """Attach (or replace) the tile's statistics set: per-gridpoint accumulators over time that live on the device
        (sx_stats_set).  outputs: a list of (op, terms[, threshold]), one entry per output - op one of "sum", "max", "min",
        "duration", terms the terms of that output as for reduce (their `out` is ignored), threshold for "duration" only - or a
        Program with ops = one op or (op, threshold) per output of the program.  source="state" reads var_np1 (no transform),
        "physical" reads `physical` as it stands (call tileTransform_ before every sample).  An empty `outputs` removes the set.
        Refusals leave an existing set as it is."""
        if source not in L.REDUCE_SOURCE:
            raise ValueError("source must be 'physical' or 'state'")
        coef, packed, n_out, op, thr = pack_statistics(self.patch_params, outputs, ops)
        L.check(self._lib.sx_stats_set(self._h, L.REDUCE_SOURCE[source], len(coef), coef.ctypes.data_as(L.P_D), packed.ctypes.data_as(L.P_I32),
                                       n_out, op.ctypes.data_as(L.P_I32), thr.ctypes.data_as(L.P_D)))

    def accumulate_statistics(self, time, weight):
        """One sample of the attached set from the planes as they stand: one kernel on the tile's stream, no synchronisation
        (sx_stats_accumulate).  weight = 0 is the "extrema only" sample.  Without a set it does nothing."""
        L.check(self._lib.sx_stats_accumulate(self._h, float(time), float(weight)))

    def reset_statistics(self):
        """Empty the accumulators and counters of the attached set; the program stays (sx_stats_reset)"""
        L.check(self._lib.sx_stats_reset(self._h))

    def describe_statistics(self):
        """(source, ops, thresholds) of the attached set - names as set_statistics takes them, a threshold None where the op has none -
        or None without a set (sx_stats_describe)"""
        src, n = C.c_int32(0), C.c_int32(0)
        op, thr = np.zeros(16, dtype=np.int32), np.zeros(16)
        L.check(self._lib.sx_stats_describe(self._h, C.byref(src), C.byref(n), op.ctypes.data_as(L.P_I32), thr.ctypes.data_as(L.P_D)))
        if n.value == 0:
            return None
        names = {v: k for k, v in L.STAT_OP.items()}
        ops = [names[int(o)] for o in op[:n.value]]
        return ({v: k for k, v in L.REDUCE_SOURCE.items()}[src.value], ops,
                [float(t) if o == "duration" else None for o, t in zip(ops, thr[:n.value])])

    def statistics(self):
        """The attached set's results as a Statistics object (sx_stats_get; synchronises)"""
        d = self.describe_statistics()
        if d is None:
            raise L.ScytheHipError("statistics: the tile has no statistics set")
        out, info = np.zeros((self.N, len(d[1]), 2), order="F"), np.zeros(5)
        L.check(self._lib.sx_stats_get(self._h, out.ctypes.data_as(L.P_D), info.ctypes.data_as(L.P_D)))
        return Statistics.from_raw(out, info, d[1])

    def get_statistics_state(self):
        """Restart blob of the statistics set (sx_stats_get_state), or None without a set"""
        n = C.c_int64(0)
        L.check(self._lib.sx_stats_state_size(self._h, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros(n.value)
        L.check(self._lib.sx_stats_get_state(self._h, out.ctypes.data_as(L.P_D)))
        return out

    def set_statistics_state(self, blob):
        b = np.ascontiguousarray(blob, dtype=np.float64)
        L.check(self._lib.sx_stats_set_state(self._h, b.ctypes.data_as(L.P_D), b.size))

    # -- operators
    def spectralTransform_(self):
        L.check(self._lib.sx_spectral_transform(self._h))

    def splineTransform_(self):
        L.check(self._lib.sx_spline_transform(self._h))

    def tileTransform_(self):
        L.check(self._lib.sx_tile_transform(self._h))

    def advance(self, t):
        L.check(self._lib.sx_advance(self._h, int(t)))

    def step(self, t):
        """One-tile patch: advanceTimestep + splineTransform! in one call (sx_step; replayed from a hipGraph with SX_GRAPH=1)."""
        L.check(self._lib.sx_step(self._h, int(t)))

    def physics(self, t):
        L.check(self._lib.sx_physics(self._h, int(t)))

    def max_abs(self):
        """max |var_np1[:, v]| per variable, reduced on the device (sx_max_abs)."""
        out = np.zeros(self.V)
        L.check(self._lib.sx_max_abs(self._h, out.ctypes.data_as(L.P_D)))
        return out

    def check_nan(self):
        f = C.c_int32(0)
        L.check(self._lib.sx_check_nan(self._h, C.byref(f)))
        return bool(f.value)

    def synchronize(self):
        L.check(self._lib.sx_synchronize(self._h))

    def set_stream(self, stream_ptr):
        L.check(self._lib.sx_set_stream(self._h, C.c_void_p(stream_ptr)))

    # -- device exchange helpers
    def tile_b_device(self):
        p, r, c = C.c_void_p(), C.c_int64(), C.c_int64()
        L.check(self._lib.sx_tile_b_device(self._h, C.byref(p), C.byref(r), C.byref(c)))
        return p.value, r.value, c.value

    def patch_a_device(self):
        p, r, c = C.c_void_p(), C.c_int64(), C.c_int64()
        L.check(self._lib.sx_patch_a_device(self._h, C.byref(p), C.byref(r), C.byref(c)))
        return p.value, r.value, c.value

    def bind_tile_b(self, dev_ptr):
        L.check(self._lib.sx_bind_tile_b(self._h, C.c_void_p(dev_ptr)))

    def bind_patch_b(self, dev_ptr, row_offsets):
        ro = np.ascontiguousarray(row_offsets, dtype=np.int64)
        assert len(ro) == int(self.dims.b_rDim)
        L.check(self._lib.sx_bind_patch_b(self._h, C.c_void_p(dev_ptr), ro.ctypes.data_as(L.P_I64)))

    def halo_add(self, dev_ptr):
        L.check(self._lib.sx_halo_add(self._h, C.c_void_p(dev_ptr)))

    # -- transposed (all-to-all) patch solve
    def a2a_configure(self, cell0, ncells, my_tile):
        n = len(cell0)
        c0 = (C.c_int32 * n)(*cell0)
        nc = (C.c_int32 * n)(*ncells)
        L.check(self._lib.sx_a2a_configure(self._h, n, my_tile, c0, nc))
        cs = np.zeros(n + 1, dtype=np.int64)
        L.check(self._lib.sx_a2a_col_starts(self._h, cs.ctypes.data_as(L.P_I64)))
        return cs

    def a2a_pack_b(self, dev_send):
        L.check(self._lib.sx_a2a_pack_b(self._h, C.c_void_p(dev_send)))

    def a2a_solve(self, dev_recv, dev_send):
        L.check(self._lib.sx_a2a_solve(self._h, C.c_void_p(dev_recv), C.c_void_p(dev_send)))

    def a2a_unpack_a(self, dev_recv):
        L.check(self._lib.sx_a2a_unpack_a(self._h, C.c_void_p(dev_recv)))

    # -- interface-only (partitioned) patch solve (sx_iface.hip): same call pattern as the transposed solve, 10 rows per tile
    def iface_configure(self, cell0, ncells, my_tile):
        n = len(cell0)
        L.check(self._lib.sx_iface_configure(self._h, n, my_tile, (C.c_int32 * n)(*cell0), (C.c_int32 * n)(*ncells)))
        cs = np.zeros(n + 1, dtype=np.int64)
        L.check(self._lib.sx_iface_col_starts(self._h, cs.ctypes.data_as(L.P_I64)))
        return cs

    def iface_local(self, dev_send):
        L.check(self._lib.sx_iface_local(self._h, C.c_void_p(dev_send)))

    def iface_reduce(self, dev_recv, dev_send):
        L.check(self._lib.sx_iface_reduce(self._h, C.c_void_p(dev_recv), C.c_void_p(dev_send)))

    def iface_apply(self, dev_recv):
        L.check(self._lib.sx_iface_apply(self._h, C.c_void_p(dev_recv)))

    def index_maps(self):
        """calcPatchMap / calcHaloMap (src/semiimplicit.jl:79-86): 1-based linear indices into one variable's column:
        (patch_owned, tile_owned, patch_halo, tile_halo)."""
        no, nh = C.c_int64(), C.c_int64()
        L.check(self._lib.sx_index_map_sizes(self._h, C.byref(no), C.byref(nh)))
        a = [np.zeros(n, dtype=np.int64) for n in (no.value, no.value, nh.value, nh.value)]
        L.check(self._lib.sx_index_maps(self._h, *[x.ctypes.data_as(L.P_I64) for x in a]))
        return tuple(a)

    # -- exchange over RCCL inside the library (sx_comm.cpp)
    def comm_prepare(self, cell0, ncells, my_tile, mode):
        """The non-collective part of comm_init (librccl bound, tile table checked, exchange buffers allocated): raises on
        THIS rank alone if it cannot be done, so that the ranks can agree before the collective comm_init."""
        n = len(cell0)
        L.check(self._lib.sx_comm_prepare(self._h, n, my_tile, (C.c_int32 * n)(*cell0), (C.c_int32 * n)(*ncells), EXCHANGE_MODES[mode]))

    def comm_init(self, cell0, ncells, my_tile, mode, unique_id):
        """Collective over all tiles: ncclCommInitRank on this tile's device + exchange buffers. mode "a2a" or "gather"."""
        n = len(cell0)
        c0 = (C.c_int32 * n)(*cell0)
        nc = (C.c_int32 * n)(*ncells)
        assert len(unique_id) == 128
        L.check(self._lib.sx_comm_init(self._h, n, my_tile, c0, nc, EXCHANGE_MODES[mode], bytes(unique_id)))

    def exchange(self):
        """Halo / shared sum / patch solve of one step on the handle's stream (src/semiimplicit.jl:320-329, 272-285)."""
        L.check(self._lib.sx_exchange(self._h))

    # -- timers
    def enable_timers(self, on=True):
        L.check(self._lib.sx_enable_timers(self._h, int(on)))

    def timer_only(self, name=None):
        """Time only the kernel with this timer name (None: all)."""
        L.check(self._lib.sx_timer_only(self._h, name.encode() if name else None))

    def reset_timers(self):
        L.check(self._lib.sx_reset_timers(self._h))

    def timers(self):
        n = C.c_int32(0)
        names = (C.c_char_p * 32)()
        ms = (C.c_double * 32)()
        calls = (C.c_int64 * 32)()
        L.check(self._lib.sx_get_timers(self._h, 32, names, ms, calls, C.byref(n)))
        return {names[i].decode(): (ms[i], calls[i]) for i in range(n.value)}

    def kernel_bytes(self, name):
        b = C.c_double(0.0)
        L.check(self._lib.sx_kernel_bytes(self._h, name.encode(), C.byref(b)))
        return b.value


EXCHANGE_MODES = {"a2a": 0, "gather": 1, "iface": 2}


def comm_unique_id():
    """ncclGetUniqueId through the library: 128 bytes that rank 0 hands to every other rank before Grid.comm_init."""
    buf = C.create_string_buffer(128)
    L.check(L.load().sx_comm_unique_id(buf))
    return buf.raw


def createGrid(gp: GridParameters, model: Optional[ModelParameters] = None):
    """createGrid(gp): the whole patch as one device-resident grid (src/semiimplicit.jl:130)."""
    if gp.geometry == "Z":
        raise ValueError("Z column model not implemented yet")     # src/spectralGrid.jl:86-88
    return Grid(gp, model)


def companion_grid(gp: GridParameters, bcl="R1T0", bcl_k0="R1T1", bcr="R1T0", bcb="R0", bct="R0", name="psi", names=None):
    """A one-variable Grid (no equation set) of the same geometry as the patch `gp`, to receive the solution of Grid.invert.
    The defaults pose the streamfunction / velocity potential of a vortex: zero at the outer edge (bcr), the wavenumbers k >= 1
    zero at the centre (bcl), the azimuthal mean with zero slope there (bcl_k0).  bcb / bct must be those of the source variables.
    names=[...] makes a companion with these variables instead (Grid.project writes all of them): every condition is then one name
    for all variables or a dict by variable (a variable it leaves out: R0)."""
    return Grid(companion_params(gp, bcl, bcl_k0, bcr, bcb, bct, name, names), None)


def companion_params(gp: GridParameters, bcl="R1T0", bcl_k0="R1T1", bcr="R1T0", bcb="R0", bct="R0", name="psi", names=None):
    """The GridParameters companion_grid creates its Grid from"""
    if names is not None:
        names = list(names)
        if not names or len(set(names)) != len(names):
            raise ValueError("names must be a non-empty list of distinct variable names")
        of = lambda c: {n: (c.get(n, "R0") if isinstance(c, dict) else c) for n in names}
        return GridParameters(geometry=gp.geometry, xmin=gp.xmin, xmax=gp.xmax, num_cells=gp.num_cells, l_q=gp.l_q, BCL=of(bcl), BCR=of(bcr),
                              BCL_k0=of(bcl_k0), zmin=gp.zmin, zmax=gp.zmax, zDim=gp.zDim, b_zDim=gp.b_zDim, BCB=of(bcb), BCT=of(bct),
                              vars={n: i + 1 for i, n in enumerate(names)}, ring_uniform_L=gp.ring_uniform_L)
    return GridParameters(geometry=gp.geometry, xmin=gp.xmin, xmax=gp.xmax, num_cells=gp.num_cells, l_q=gp.l_q, BCL={name: bcl},
                          BCR={name: bcr}, BCL_k0={name: bcl_k0}, zmin=gp.zmin, zmax=gp.zmax, zDim=gp.zDim, b_zDim=gp.b_zDim,
                          BCB={name: bcb}, BCT={name: bct}, vars={name: 1}, ring_uniform_L=gp.ring_uniform_L)


def elliptic_check(patch: GridParameters, var, k, alpha, g):
    """The host statement of Grid.invert for ONE right-hand side column g [num_cells + 3] and wavenumber k, with the boundary
    conditions of variable `var` (name or 1-based index) of the patch: a = Gamma_k^T K_k^-1 (-Gamma_k g) through the factors the
    device kernel applies (sx_elliptic_check: no handle, no device).  Raises what Grid.invert would refuse of the patch."""
    d, keep = grid_desc(patch)
    v = patch.vars[var] if isinstance(var, str) else int(var)
    rhs = np.ascontiguousarray(g, dtype=np.float64)
    if rhs.shape != (patch.num_cells + 3,):
        raise ValueError("g must have num_cells + 3 entries")
    a = np.zeros_like(rhs)
    L.check(L.load().sx_elliptic_check(C.byref(d), v, int(k), float(alpha), rhs.ctypes.data_as(L.P_D), a.ctypes.data_as(L.P_D)))
    return a


def antiderivative_check(patch: GridParameters, var, var_dst, axis="r", origin="low", weight_r=False, k=0, a_src=None):
    """The host statement of Grid.antiderivative for ONE column: a_src [num_cells + 3] (axis "r": wavenumber k selects the
    boundary-condition class of `var_dst`) or [b_zDim] (axis "z"), both variables (names or 1-based indices) of the one patch;
    the same host-built tables and the device kernel's arithmetic (sx_antiderivative_check: no handle, no device)."""
    if axis not in L.INT_AXIS or origin not in L.INT_ORIGIN:
        raise ValueError("axis must be 'r' or 'z' and origin 'low' or 'high'")
    d, keep = grid_desc(patch)
    vs, vd = (patch.vars[v] if isinstance(v, str) else int(v) for v in (var, var_dst))
    col = np.ascontiguousarray(a_src, dtype=np.float64)
    want = patch.num_cells + 3 if axis == "r" else int(d.b_zDim if d.b_zDim > 0 else 0)
    if col.ndim != 1 or (want and col.shape != (want,)):
        raise ValueError("a_src must have %d entries" % want)
    out = np.zeros_like(col)
    L.check(L.load().sx_antiderivative_check(C.byref(d), vs, vd, L.INT_AXIS[axis], L.INT_ORIGIN[origin], int(bool(weight_r)), int(k),
                                             col.ctypes.data_as(L.P_D), out.ctypes.data_as(L.P_D)))
    return out


def getGridpoints(grid: Grid):
    """R: vector; RL: [:,1]=r,[:,2]=lambda; RZ: r,z; RLZ: r,lambda,z (src/semiimplicit.jl:59)."""
    n, nc = grid.N, int(grid.dims.n_coord)
    out = np.zeros((n, nc), order="F")
    L.check(grid._lib.sx_get_gridpoints(grid._h, out.ctypes.data_as(L.P_D)))
    return out[:, 0].copy() if nc == 1 else out


def eval_basis(patch: GridParameters, var, point, all_k=False, tile_cell0=0, tile_num_cells=None):
    """The weights sx_evaluate applies at one point, for variable `var` (name or 1-based index), on the host (sx_eval_basis):
    (node0, w_r [3, 4], kcap, w_z [3, b_zDim] or None).  node0 is the 0-based patch row of the first of the 4 spline nodes."""
    d, keep = grid_desc(patch, tile_cell0, tile_num_cells)
    v = patch.vars[var] if isinstance(var, str) else int(var)
    pt = np.ascontiguousarray(np.atleast_1d(point), dtype=np.float64)
    if len(pt) != len(patch.geometry):
        raise ValueError("point must have %d coordinate(s)" % len(patch.geometry))
    node0, kcap = C.c_int32(-1), C.c_int32(-1)
    w_r = np.zeros((3, 4))
    w_z = np.zeros((3, patch.b_zDim)) if "Z" in patch.geometry else None
    L.check(L.load().sx_eval_basis(C.byref(d), v, pt.ctypes.data_as(L.P_D), L.EVAL_ALL_K if all_k else L.EVAL_RING_K, C.byref(node0),
                                   w_r.ctypes.data_as(L.P_D), C.byref(kcap), w_z.ctypes.data_as(L.P_D) if w_z is not None else None))
    return node0.value, w_r, kcap.value, w_z


# ----------------------------------------------------------------------------- integrals and azimuthal means (sx_reduce)
class Program(list):
    """An integrand program for Grid.reduce / ModelRun.integrate: a list of (out, coef, r_power, [(var, slot), ...]) terms with a
    name per output."""

    def __init__(self, terms=(), names=()):
        super().__init__(terms)
        self.names = list(names)


def pack_reduce_program(patch: GridParameters, terms):
    """terms -> (coef float64 [n], terms int32 [n, 11] = out, r_power, n_factors, var[4], slot[4] as sx_reduce reads them, n_out);
    variable and slot names are resolved against the patch, everything else is left to the library to refuse."""
    slots = L.SLOTS[patch.geometry] if patch is not None else ()      # patch=None: variables and slots by index only (project_point)
    coef = np.zeros(len(terms))
    packed = np.zeros((len(terms), 11), dtype=np.int32)
    for i, (out, c, p, factors) in enumerate(terms):
        if len(factors) > 4:
            raise ValueError("term %d has %d factors; at most 4" % (i, len(factors)))
        coef[i] = float(c)
        packed[i, :3] = int(out), int(p), len(factors)
        for f, (var, slot) in enumerate(factors):
            if isinstance(var, str) and (patch is None or var not in patch.vars):
                raise ValueError("term %d: unknown variable %r" % (i, var))
            if isinstance(slot, str) and slot not in slots:
                raise ValueError("term %d: an %s grid has no slot %r" % (i, patch.geometry if patch is not None else "unnamed", slot))
            packed[i, 3 + f] = patch.vars[var] if isinstance(var, str) else int(var)
            packed[i, 7 + f] = slots.index(slot) if isinstance(slot, str) else int(slot)
    n_out = int(packed[:, 0].max()) + 1 if len(terms) else 0
    return coef, packed, n_out


def reduce_weights(patch: GridParameters, tile_cell0=0, tile_num_cells=None):
    """The quadrature weights of Grid.reduce(kind="domain") for a tile, on the host (sx_reduce_weights): (w_r [3 cells],
    w_l [3 cells], w_z [zDim] or None).  w_r = DX (5, 8, 5) / 18 (times r on RL / RLZ), w_l = 2 pi / L, w_z = Clenshaw-Curtis."""
    d, keep = grid_desc(patch, tile_cell0, tile_num_cells)
    n = 3 * d.tile_num_cells
    w_r, w_l = np.zeros(n), np.zeros(n)
    w_z = np.zeros(patch.zDim) if "Z" in patch.geometry else None
    L.check(L.load().sx_reduce_weights(C.byref(d), w_r.ctypes.data_as(L.P_D), w_l.ctypes.data_as(L.P_D),
                                       w_z.ctypes.data_as(L.P_D) if w_z is not None else None))
    return w_r, w_l, w_z


def reduce_planes(patch: GridParameters, terms, source="physical", tile_cell0=0, tile_num_cells=None):
    """The distinct (var, slot) planes a program reads, in first-use order, as the validator of sx_reduce sees them
    (sx_reduce_planes): ndarray [n_planes, 2] of (1-based variable, slot index).  Raises what Grid.reduce would refuse."""
    d, keep = grid_desc(patch, tile_cell0, tile_num_cells)
    coef, packed, n_out = pack_reduce_program(patch, terms)
    planes = np.zeros((16, 2), dtype=np.int32)
    n = C.c_int32(0)
    L.check(L.load().sx_reduce_planes(C.byref(d), L.REDUCE_SOURCE[source], len(coef), packed.ctypes.data_as(L.P_I32), n_out,
                                      planes.ctypes.data_as(L.P_I32), C.byref(n)))
    return planes[:n.value].copy()


# ----------------------------------------------------------------------------- field programs as variables (sx_project)
def _project_var_dst(dst_patch: GridParameters, n_out, var_dst):
    """var_dst as sx_project reads it: int32 [n_out], 1-based; names resolved against the destination, default 1 .. n_out"""
    if var_dst is None:
        return np.arange(1, n_out + 1, dtype=np.int32)
    return np.array([dst_patch.vars[v] if isinstance(v, str) else int(v) for v in var_dst], dtype=np.int32)


def program_of_outputs(outputs):
    """A list of outputs, each a list of (coef, r_power, [(var, slot), ...]) terms, as the one term list Grid.project and Grid.reduce
    read: output o's terms get out = o (a term that already carries an `out` in front loses it)"""
    return [(o,) + tuple(t)[-3:] for o, terms in enumerate(outputs) for t in terms]


def project_check(patch: GridParameters, dst_patch: GridParameters, terms, source="physical", var_dst=None):
    """What Grid.project refuses of the two patches and the program, on the host (sx_project_check: no handle, no device); raises
    ScytheHipError with the library's message, returns None when the call would be accepted.  A descriptor carries no equation set
    and no handle: those two refusals are the call's own."""
    ds, k1 = grid_desc(patch)
    dd, k2 = grid_desc(dst_patch)
    coef, packed, n_out = pack_reduce_program(patch, terms)
    vd = _project_var_dst(dst_patch, n_out, var_dst)
    L.check(L.load().sx_project_check(C.byref(ds), C.byref(dd), L.REDUCE_SOURCE[source], len(coef), packed.ctypes.data_as(L.P_I32), n_out,
                                      vd.ctypes.data_as(L.P_I32) if len(vd) else None))


def project_point(terms, planes, values, r):
    """The outputs of a program at ONE point, on the host with k_project's arithmetic (sx_project_point): float64 [n_out].  terms: as
    for reduce with variables and slots by index, or a packed (coef, packed, n_out); planes [(var, slot), ...] lists every plane the
    program names, values [len(planes)] their values at the point, r its radius."""
    coef, packed, n_out = terms if isinstance(terms, tuple) and len(terms) == 3 and hasattr(terms[1], "shape") else pack_reduce_program(None, terms)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    packed = np.ascontiguousarray(packed, dtype=np.int32)
    pl = np.ascontiguousarray(np.asarray(planes, dtype=np.int32).reshape(-1, 2))
    val = np.ascontiguousarray(values, dtype=np.float64)
    if val.shape != (len(pl),):
        raise ValueError("values must have one entry per plane")
    out = np.zeros(int(n_out))
    L.check(L.load().sx_project_point(len(coef), coef.ctypes.data_as(L.P_D), packed.ctypes.data_as(L.P_I32), int(n_out), len(pl),
                                      pl.ctypes.data_as(L.P_I32), val.ctypes.data_as(L.P_D), float(r), out.ctypes.data_as(L.P_D)))
    return out


# ----------------------------------------------------------------------------- function programs (sx_derive)
class FunctionProgram:
    """A packed function program (pack_function_program): the mids as pack_reduce_program packs them (coef, terms, n_mid), ops int32
    [n_ops, 4] = fn, a, b, c, consts float64, reg_dst int32 [n_outputs] - the register of each output - and the outputs' names"""

    def __init__(self, coef, terms, n_mid, ops, consts, reg_dst, names):
        self.coef, self.terms, self.n_mid = np.ascontiguousarray(coef, dtype=np.float64), np.ascontiguousarray(terms, dtype=np.int32), int(n_mid)
        self.ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 4)
        self.consts = np.ascontiguousarray(consts, dtype=np.float64)
        self.reg_dst = np.ascontiguousarray(reg_dst, dtype=np.int32)
        self.names = list(names)

    def args(self, with_coef=True, with_consts=True):
        """the program as sx_derive / sx_derive_check / sx_derive_point take it, up to and including the constants"""
        P = lambda a, t: a.ctypes.data_as(t) if a.size else None
        return ((len(self.coef),) + ((P(self.coef, L.P_D),) if with_coef else ()) + (P(self.terms, L.P_I32), self.n_mid, len(self.ops), P(self.ops, L.P_I32),
                len(self.consts)) + ((P(self.consts, L.P_D),) if with_consts else ()))


def _is_terms(x):
    return isinstance(x, (list, tuple)) and (len(x) == 0 or isinstance(x[0], (list, tuple))) and not (len(x) and isinstance(x[0], str))


def pack_function_program(patch: GridParameters, outputs):
    """Outputs -> FunctionProgram.  outputs: a dict name -> output, or a list of outputs.  An output is a term list [(coef, r_power,
    [(var, slot), ...]), ...] as for Grid.project, or a nested expression
        ("sqrt", X)  ("div", X, Y)  ("atan2", X, Y)  ("select", A, X, Y)  ("temperature", S, RHO, QV)  ("ref", "sbar", "z")  "r"  "z"  a number
    (the operations: _lib.FN) whose leaves are term lists, names of other outputs of the dict, or numbers.  Term lists become the mids,
    numbers the constants, every other node one operation; identical sub-expressions become ONE register (structural sharing: a
    term list is compared term by term, a number bit by bit), and operands come before the operation that reads them.  Raises
    ValueError beyond the library's limits (16 mids, 32 operations, 16 constants), for an unknown operation or name, for a cycle of
    names, and for an output that is a bare number (it would need no kernel)."""
    named = dict(outputs) if isinstance(outputs, dict) else {}
    outs = list(outputs.values()) if isinstance(outputs, dict) else list(outputs)
    names = list(outputs) if isinstance(outputs, dict) else ["f%d" % (o + 1) for o in range(len(outs))]
    mids, mid_of, consts, const_of, ops, op_of, visiting = [], {}, [], {}, [], {}, []

    def operand(x):
        """register (>= 0) or constant (< 0) of a node"""
        if isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool):
            key = np.float64(x).tobytes()
            if key not in const_of:
                consts.append(float(x))
                const_of[key] = -len(consts)
            return const_of[key]
        if isinstance(x, str) and x not in ("r", "z"):
            if x not in named:
                raise ValueError("pack_function_program: %r is neither an output nor 'r' / 'z'" % (x,))
            if x in visiting:
                raise ValueError("pack_function_program: the outputs name one another in a cycle (%s)" % " -> ".join(visiting + [x]))
            visiting.append(x)
            reg = operand(named[x])
            visiting.pop()
            return reg
        if _is_terms(x):
            key = tuple((float(t[-3]), int(t[-2]), tuple((v, s) for v, s in t[-1])) for t in x)
            if key not in mid_of:
                mid_of[key] = len(mids)
                mids.append(key)
            return ("mid", mid_of[key])
        node = (x,) if isinstance(x, str) else tuple(x)
        fn = node[0]
        if fn not in L.FN:
            raise ValueError("pack_function_program: unknown operation %r" % (fn,))
        if fn == "ref":
            if len(node) != 3 or node[1] not in L.REF_PROFILE or node[2] not in L.REF_SLOT:
                raise ValueError("pack_function_program: ('ref', profile, slot) with profile in %s and slot in %s" % (sorted(L.REF_PROFILE), sorted(L.REF_SLOT)))
            key = (fn, L.REF_PROFILE[node[1]], L.REF_SLOT[node[2]])
        else:
            if len(node) - 1 != L.FN_ARITY.get(fn, 2):
                raise ValueError("pack_function_program: %r takes %d operand(s)" % (fn, L.FN_ARITY.get(fn, 2)))
            key = (fn,) + tuple(operand(a) for a in node[1:])
        if key not in op_of:
            op_of[key] = len(ops)
            ops.append(key)
        return ("op", op_of[key])

    tops = []
    for name, out in zip(names, outs):
        visiting[:] = [name] if isinstance(outputs, dict) else []
        reg = operand(out)
        if isinstance(reg, int):
            raise ValueError("pack_function_program: output %r is a bare number" % (name,))
        tops.append(reg)
    if len(mids) > 16 or len(ops) > 32 or len(consts) > 16:
        raise ValueError("pack_function_program: %d mids, %d operations, %d constants; the limits are 16, 32 and 16" % (len(mids), len(ops), len(consts)))
    n_mid = len(mids)
    reg = lambda x: x if isinstance(x, int) else x[1] + (n_mid if x[0] == "op" else 0)
    coef, terms, _ = pack_reduce_program(patch, [(o, c, p, list(f)) for o, key in enumerate(mids) for c, p, f in key])
    packed = np.zeros((len(ops), 4), dtype=np.int32)
    for i, key in enumerate(ops):
        packed[i, 0] = L.FN[key[0]]
        packed[i, 1:len(key)] = [reg(a) for a in key[1:]] if key[0] != "ref" else key[1:]
    return FunctionProgram(coef, terms, n_mid, packed, np.array(consts, dtype=np.float64), [reg(t) for t in tops], names)


def derive_check(patch: GridParameters, dst_patch: GridParameters, program, source="physical", has_ref_state=False):
    """What Grid.derive refuses of the two patches and the program, on the host (sx_derive_check: no handle, no device); raises
    ScytheHipError with the library's message.  has_ref_state: whether the source's model carries a reference state."""
    ds, k1 = grid_desc(patch)
    dd, k2 = grid_desc(dst_patch)
    fp = program if isinstance(program, FunctionProgram) else pack_function_program(patch, program)
    L.check(L.load().sx_derive_check(C.byref(ds), int(bool(has_ref_state)), C.byref(dd), L.REDUCE_SOURCE[source], *fp.args(False, False),
                                     len(fp.reg_dst), fp.reg_dst.ctypes.data_as(L.P_I32) if len(fp.reg_dst) else None))


def derive_point(program, planes, values, r, z=0.0, ref=None):
    """Every register of a function program at ONE point, on the host by the code k_derive runs (sx_derive_point): float64
    [n_mid + n_ops].  program: a FunctionProgram; planes [(var, slot), ...] (1-based variable, slot index) lists every plane the
    mids name, values their values at the point; r, z its coordinates; ref [3, 3] the reference state (profile, slot) at its level."""
    pl = np.ascontiguousarray(np.asarray(planes, dtype=np.int32).reshape(-1, 2))
    val = np.ascontiguousarray(values, dtype=np.float64)
    if val.shape != (len(pl),):
        raise ValueError("values must have one entry per plane")
    rf = None if ref is None else np.ascontiguousarray(ref, dtype=np.float64).reshape(3, 3)
    regs = np.zeros(program.n_mid + len(program.ops))
    L.check(L.load().sx_derive_point(*program.args(), len(pl), pl.ctypes.data_as(L.P_I32) if len(pl) else None, val.ctypes.data_as(L.P_D) if len(pl) else None,
                                     float(r), float(z), rf.ctypes.data_as(L.P_D) if rf is not None else None, regs.ctypes.data_as(L.P_D)))
    return regs


# ----------------------------------------------------------------------------- onto another grid (sx_regrid)
def _regrid_var_src(patch: GridParameters, dst_patch: GridParameters, variables):
    """var_src as sx_regrid reads it: int32 [dst V], 1-based variables of the source; default: the destination's names in the source"""
    if variables is None:
        missing = [n for n in dst_patch.var_names() if n not in patch.vars]
        if missing:
            raise ValueError("regrid: the source has no variable named %s (pass variables=[...])" % ", ".join(map(repr, missing)))
        variables = dst_patch.var_names()
    if len(variables) != len(dst_patch.vars):
        raise ValueError("regrid: %d source variables for the destination's %d" % (len(variables), len(dst_patch.vars)))
    return np.array([patch.vars[v] if isinstance(v, str) else int(v) for v in variables], dtype=np.int32)


def _regrid_centre(centre):
    return None if centre is None else np.ascontiguousarray(centre, dtype=np.float64).reshape(2)


def regrid_check(patch: GridParameters, dst_patch: GridParameters, centre=None, variables=None, outside="refuse"):
    """What Grid.regrid refuses of the two patches, the centre, the variables and `outside`, on the host (sx_regrid_check: no handle, no
    device); raises ScytheHipError with the library's message, returns None when the call would be accepted.  outside may be given as
    the library's integer."""
    ds, k1 = grid_desc(patch)
    dd, k2 = grid_desc(dst_patch)
    vs = _regrid_var_src(patch, dst_patch, variables)
    c = _regrid_centre(centre)
    L.check(L.load().sx_regrid_check(C.byref(ds), C.byref(dd), None if c is None else c.ctypes.data_as(L.P_D), vs.ctypes.data_as(L.P_I32),
                                     L.REGRID_OUTSIDE.get(outside, outside)))


def regrid_columns(gp_src: GridParameters, gp_dst: GridParameters, centre=None):
    """The coordinates in gp_src of every column of gp_dst about `centre`, in gp_dst's gridpoint order, from the function Grid.regrid
    sums at (sx_regrid_columns, on the host): (columns [n_cols, 1 or 2] - r_s[, lambda_s] -, inside [n_cols] bool)."""
    ds, k1 = grid_desc(gp_src)
    dd, k2 = grid_desc(gp_dst)
    c = _regrid_centre(centre)
    cp = None if c is None else c.ctypes.data_as(L.P_D)
    n = C.c_int64(0)
    L.check(L.load().sx_regrid_columns(C.byref(ds), C.byref(dd), cp, None, None, C.byref(n)))
    cols = np.zeros((n.value, 2 if "L" in gp_dst.geometry else 1), order="F")
    inside = np.zeros(n.value, dtype=np.int32)
    L.check(L.load().sx_regrid_columns(C.byref(ds), C.byref(dd), cp, cols.ctypes.data_as(L.P_D), inside.ctypes.data_as(L.P_I32), C.byref(n)))
    return cols, inside.astype(bool)


# ----------------------------------------------------------------------------- extrema and their refinement (sx_extrema, sx_extremum_refine)
Refined = collections.namedtuple("Refined", "pos value grad status iters")


def free_mask(patch: GridParameters, free=None):
    """SX_EXT_FREE_* mask from a string of r / l / z, a mask, or None = every coordinate of the geometry"""
    if free is None:
        free = patch.geometry.lower()
    if isinstance(free, str):
        if set(free) - set(L.EXT_FREE):
            raise ValueError("free must be made of the letters r, l, z")
        return sum(L.EXT_FREE[c] for c in set(free))
    return int(free)


def newton_step(patch: GridParameters, pos, d, want="max", free=None, tol=None, tile_cell0=0, tile_num_cells=None):
    """One step of refine_extremum's iteration on the host (sx_newton_step): pos [n_coord], d [10] = u, u_r, u_l, u_z, u_rr, u_rl,
    u_rz, u_ll, u_lz, u_zz -> (new_pos [n_coord], status), status -1 = took a step, go on."""
    desc, keep = grid_desc(patch, tile_cell0, tile_num_cells)
    p = np.ascontiguousarray(np.atleast_1d(pos), dtype=np.float64)
    dd = np.ascontiguousarray(d, dtype=np.float64)
    if len(p) != len(patch.geometry) or dd.shape != (10,):
        raise ValueError("pos must have %d coordinate(s) and d 10 entries" % len(patch.geometry))
    if want not in L.EXT_WANT:
        raise ValueError("want must be 'max', 'min' or 'any'")
    out, st = np.zeros(len(p)), C.c_int32(-2)
    L.check(L.load().sx_newton_step(C.byref(desc), L.EXT_WANT[want], free_mask(patch, free), 0.0 if tol is None else float(tol),
                                    p.ctypes.data_as(L.P_D), dd.ctypes.data_as(L.P_D), out.ctypes.data_as(L.P_D), C.byref(st)))
    return out, int(st.value)


# ----------------------------------------------------------------------------- level crossings along rays (sx_crossings)
Crossings = collections.namedtuple("Crossings", "radius dir count status profiles")


def bracket_step(state, flags, fx=0.0, width_tol=0.0, first=False):
    """One step of Grid.crossings' refinement on the host (sx_bracket_step): state [7] = a, d(a), b, d(b), ga, gb, x and flags [2] =
    (end replaced last, bisect next) -> (new state, new flags, status); first=True starts from the station interval in state[:4];
    status 0 finished, -1 evaluate d at state[6] and step again, 2 fx is NaN."""
    s = np.zeros(7)
    s[:len(state)] = np.asarray(state, dtype=np.float64)
    f = np.zeros(2, dtype=np.int32)
    f[:len(flags)] = np.asarray(flags, dtype=np.int32)
    st = C.c_int32(-2)
    L.check(L.load().sx_bracket_step(s.ctypes.data_as(L.P_D), f.ctypes.data_as(L.P_I32), 1 if first else 0, float(fx), float(width_tol),
                                     C.byref(st)))
    return s, f, int(st.value)


# ----------------------------------------------------------------------------- isosurfaces in columns (sx_isosurface)
Isosurface = collections.namedtuple("Isosurface", "height dir count status carry values profiles")


def isosurface_check(patch: GridParameters, terms, carry=0):
    """The number of column profiles Grid.isosurface forms for a program with 1 + carry outputs, on the host (sx_isosurface_check:
    no handle, no device).  Raises what Grid.isosurface would refuse of the grid and the program."""
    d, keep = grid_desc(patch)
    coef, packed, _ = pack_reduce_program(patch, terms)
    n = C.c_int32(-1)
    L.check(L.load().sx_isosurface_check(C.byref(d), len(coef), packed.ctypes.data_as(L.P_I32), int(carry), C.byref(n)))
    return int(n.value)


def column_series(zmin, zmax, a, z):
    """(value, d/dz, d2/dz2) at height z of the Chebyshev series with the zDim coefficients `a`, on the host (sx_column_series): the
    function Grid.isosurface's kernel evaluates at stations, trial points and for the carried outputs."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.zeros(3)
    L.check(L.load().sx_column_series(len(a), float(zmin), float(zmax), a.ctypes.data_as(L.P_D), float(z), out.ctypes.data_as(L.P_D)))
    return out


def columns_of(gp: GridParameters, points):
    """The columns [n_cols, n_coord - 1] = r[, lambda] of gridpoints r[, lambda], z as regular_gridpoints / cartesian_gridpoints
    list them (z fastest): the z coordinate dropped, every run of rows that share a column kept once."""
    if "Z" not in gp.geometry:
        raise ValueError("columns need an RZ or RLZ geometry")
    p = np.asarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] not in (len(gp.geometry), len(gp.geometry) - 1):
        raise ValueError("points must have %d coordinate column(s), or as many without z" % len(gp.geometry))
    c = p[:, :len(gp.geometry) - 1]
    keep = np.concatenate([[True], (c[1:] != c[:-1]).any(axis=1)]) if len(c) else np.zeros(0, dtype=bool)
    return np.ascontiguousarray(c[keep])


# ----------------------------------------------------------------------------- histograms of field programs (sx_distribution)
Distribution = collections.namedtuple("Distribution", "count measure sums edges")


def distribution_slot(edges, q):
    """The slot of q among len(edges) + 2 on the host (sx_distribution_slot): 0 below edges[0], 1 + b for edges[b] <= q < edges[b + 1],
    n_bins + 1 at or above edges[-1], n_bins + 2 for a NaN - the rule Grid.distribution's kernel applies, compiled from the same
    function."""
    e = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64)
    s = C.c_int32(-1)
    L.check(L.load().sx_distribution_slot(len(e) - 1, e.ctypes.data_as(L.P_D), float(q), C.byref(s)))
    return int(s.value)


def distribution_check(patch: GridParameters, terms, edges, kind="domain", source="physical", tile_cell0=0, tile_num_cells=None):
    """Raises what Grid.distribution would refuse of a call, on the host (sx_distribution_check)."""
    d, keep = grid_desc(patch, tile_cell0, tile_num_cells)
    coef, packed, n_out = pack_reduce_program(patch, terms)
    e = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64)
    L.check(L.load().sx_distribution_check(C.byref(d), L.DIST_KIND[kind] if isinstance(kind, str) else int(kind),
                                           L.REDUCE_SOURCE[source] if isinstance(source, str) else int(source), len(coef),
                                           packed.ctypes.data_as(L.P_I32), n_out, len(e) - 1, e.ctypes.data_as(L.P_D)))


# ----------------------------------------------------------------------------- statistics over time (sx_stats_*)
def pack_statistics(patch: GridParameters, outputs, ops=None):
    """outputs -> (coef, terms int32 [n, 11], n_out, op int32 [n_out], threshold float64 [n_out]) as sx_stats_set reads them.
    outputs: a list of (op, terms[, threshold]) - the terms of entry o become the terms of output o, whatever their own `out`
    says - or, with ops, a program as for Grid.reduce whose output o takes ops[o] = op or (op, threshold).  Raises ValueError for an
    unknown op, a "duration" without a threshold, a threshold on another op, or ops that do not match the program's outputs."""
    if ops is None:
        entries = list(outputs)
        terms, ops = [], []
        for o, e in enumerate(entries):
            if not isinstance(e, (tuple, list)) or len(e) not in (2, 3):
                raise ValueError("output %d is no (op, terms[, threshold])" % o)
            terms += [(o,) + tuple(t[-3:]) for t in e[1]]
            ops.append(e[0] if len(e) == 2 else (e[0], e[2]))
        n_given = len(entries)
    else:
        terms, ops = list(outputs), list(ops)
        n_given = len(ops)
    coef, packed, n_out = pack_reduce_program(patch, terms)
    if n_out > n_given:
        raise ValueError("the program has %d outputs, ops names %d" % (n_out, n_given))
    n_out = n_given                    # a trailing output without terms is the constant 0
    op, thr = np.zeros(max(n_out, 1), dtype=np.int32), np.zeros(max(n_out, 1))
    for o, e in enumerate(ops):
        name, t = (e, None) if isinstance(e, str) else (e[0], e[1] if len(e) > 1 else None)
        if name not in L.STAT_OP:
            raise ValueError("output %d: op %r is none of %s" % (o, name, sorted(L.STAT_OP)))
        if (name == "duration") != (t is not None):
            raise ValueError("output %d: a threshold goes with 'duration', and only with it" % o)
        op[o], thr[o] = L.STAT_OP[name], 0.0 if t is None else float(t)
    return coef, packed, n_out, op, thr


class Statistics:
    """Results of a statistics set: value [N, n_out] - the sum (hi + lo) for "sum" / "duration", the extremum for "max" / "min";
    time [N, n_out] - the time of the sample that set an extremum, NaN for the sum-like ops; residual [N, n_out] - the low word of a
    sum's stored pair (NaN for extrema); samples, elapsed (the sum of the weights; elapsed_lo its low word), t_first, t_last; ops.
    samples == 0 means "empty": extremum values are then NaN because nothing was seen, otherwise because q was NaN."""

    def __init__(self, value, time, residual, samples, elapsed, elapsed_lo, t_first, t_last, ops):
        self.value, self.time, self.residual, self.ops = value, time, residual, list(ops)
        self.samples, self.elapsed, self.elapsed_lo, self.t_first, self.t_last = samples, elapsed, elapsed_lo, t_first, t_last

    @classmethod
    def from_raw(cls, out, info, ops):
        """out [N, n_out, 2] and info [5] as sx_stats_get returns them"""
        sumlike = np.array([o in ("sum", "duration") for o in ops], dtype=bool)
        value = np.array(out[:, :, 0], order="F")
        time = np.where(sumlike[None, :], np.nan, out[:, :, 1])
        residual = np.where(sumlike[None, :], out[:, :, 1], np.nan)
        return cls(value, time, residual, int(info[0]), float(info[1] + info[2]), float(info[2]), float(info[3]), float(info[4]), ops)

    def mean(self, o):
        """value / elapsed of a "sum" output: its time mean over the window"""
        if self.ops[o] != "sum":
            raise ValueError("output %d is a %r, not a 'sum'" % (o, self.ops[o]))
        return self.value[:, o] / self.elapsed

    @classmethod
    def concatenate(cls, parts):
        """the tiles of a patch in tile order: the points concatenated; the counters are every tile's"""
        p0 = parts[0]
        return cls(np.concatenate([p.value for p in parts], axis=0), np.concatenate([p.time for p in parts], axis=0),
                   np.concatenate([p.residual for p in parts], axis=0), p0.samples, p0.elapsed, p0.elapsed_lo, p0.t_first, p0.t_last, p0.ops)


# ----------------------------------------------------------------------------- vortex-centred harmonics (sx_vortex_harmonics)
def pack_vortex_fields(patch: GridParameters, fields):
    """fields -> (int32 [n, 3] = kind, var_a, var_b as sx_vortex_harmonics reads them, n_out): a variable name or 1-based index is a
    scalar field, ("wind", u, v) a wind field with two outputs; names are resolved against the patch, the rest is left to the library"""
    fields = [fields] if isinstance(fields, (str, int, np.integer)) else list(fields)
    if len(fields) == 3 and fields[0] == "wind" and "wind" not in patch.vars:
        fields = [tuple(fields)]

    def var(v, i):
        if isinstance(v, str) and v not in patch.vars:
            raise ValueError("field %d: unknown variable %r" % (i, v))
        return patch.vars[v] if isinstance(v, str) else int(v)

    packed = np.zeros((len(fields), 3), dtype=np.int32)
    n_out = 0
    for i, f in enumerate(fields):
        if isinstance(f, (tuple, list)):
            if len(f) != 3 or f[0] != "wind":
                raise ValueError("field %d is neither a variable nor ('wind', u, v)" % i)
            packed[i] = L.VORTEX_WIND, var(f[1], i), var(f[2], i)
            n_out += 2
        else:
            packed[i] = L.VORTEX_SCALAR, var(f, i), 0
            n_out += 1
    return packed, n_out


def default_vortex_n_az(kDim, kmax):
    """the smallest multiple of 4 above kDim + kmax: the state holds wavenumbers up to kDim, so about the grid's own centre no
    harmonic k <= kmax is aliased"""
    return 4 * ((int(kDim) + max(int(kmax), 0)) // 4 + 1)


def vortex_check(patch: GridParameters, centre, radii, fields=("h",), n_az=16, kmax=4, tile_cell0=0, tile_num_cells=None):
    """What Grid.vortex_harmonics would do with a call, on the host (sx_vortex_check: no handle, no device): raises what it refuses
    of the grid, the centre, the radii, n_az, kmax and the fields; returns (n_out, status int32 [n_rho]) with the circle rule."""
    d, keep = grid_desc(patch, tile_cell0, tile_num_cells)
    packed, _ = pack_vortex_fields(patch, fields)
    r = np.ascontiguousarray(np.asarray(radii, dtype=np.float64).reshape(-1))
    c0 = np.ascontiguousarray(np.asarray(centre, dtype=np.float64).reshape(-1))
    if len(c0) != 2:
        raise ValueError("centre must be (x0, y0)")
    status = np.zeros(len(r), dtype=np.int32)
    n_out = C.c_int32(-1)
    L.check(L.load().sx_vortex_check(C.byref(d), c0.ctypes.data_as(L.P_D), r.ctypes.data_as(L.P_D), len(r), int(n_az), int(kmax),
                                     len(packed), packed.ctypes.data_as(L.P_I32), C.byref(n_out), status.ctypes.data_as(L.P_I32)))
    return int(n_out.value), status


# ----------------------------------------------------------------------------- azimuthal power and cross spectra (sx_spectrum)
def pack_spectrum_pairs(patch: GridParameters, pairs):
    """pairs -> int32 [n, 4] = var_a, slot_a, var_b, slot_b as sx_spectrum reads them; variable and slot names are resolved against
    the patch, everything else is left to the library to refuse."""
    packed = np.zeros((len(pairs), 4), dtype=np.int32)
    for i, pair in enumerate(pairs):
        if len(pair) != 2:
            raise ValueError("pair %d is no ((var, slot), (var, slot))" % i)
        for s, (var, slot) in enumerate(pair):
            if isinstance(var, str) and var not in patch.vars:
                raise ValueError("pair %d: unknown variable %r" % (i, var))
            if isinstance(slot, str) and slot not in L.HARM_SLOTS:
                raise ValueError("pair %d: %r is none of the slots %s" % (i, slot, L.HARM_SLOTS))
            packed[i, 2 * s] = patch.vars[var] if isinstance(var, str) else int(var)
            packed[i, 2 * s + 1] = L.HARM_SLOTS.index(slot) if isinstance(slot, str) else int(slot)
    return packed


def spectrum_check(patch: GridParameters, pairs, tile_cell0=0, tile_num_cells=None):
    """Raises what Grid.spectrum would refuse of a pair list, on the host (sx_spectrum_check: no handle, no device)."""
    d, keep = grid_desc(patch, tile_cell0, tile_num_cells)
    packed = pack_spectrum_pairs(patch, pairs)
    L.check(L.load().sx_spectrum_check(C.byref(d), len(packed), packed.ctypes.data_as(L.P_I32)))


def _speed2(wind, coef):
    """coef (u^2 [+ v^2]) as terms (coef, r_power, factors) of one output: the wind's square, stated once for invariants and
    field_programs"""
    return [(coef, 0, [(w, ""), (w, "")]) for w in wind]


def invariants(model: ModelParameters):
    """The conserved (or budget) integrals of an equation set as a Program for ModelRun.integrate:
    LinearShallowWater1D  mass = int h, energy = 1/2 int (g h^2 + H u^2);  LinearShallowWaterRL  the same with H (u^2 + v^2);
    LinearAdvection*      the first moment int q and the second moment int q^2 of the advected variable (variable 1)."""
    eq = model.equation_set
    pp = {(k if isinstance(k, str) else str(k)).lstrip(":"): v for k, v in model.physical_params.items()}
    if eq in ("LinearShallowWater1D", "LinearShallowWaterRL"):
        g, H = float(pp["g"]), float(pp["H"])
        wind = ("u", "v") if eq == "LinearShallowWaterRL" else ("u",)
        terms = [(0, 1.0, 0, [("h", "")]), (1, 0.5 * g, 0, [("h", ""), ("h", "")])] + [(1,) + t for t in _speed2(wind, 0.5 * H)]
        return Program(terms, ["mass", "energy"])
    if eq.startswith("LinearAdvection"):
        q = model.grid_params.var_names()[0]
        return Program([(0, 1.0, 0, [(q, "")]), (1, 1.0, 0, [(q, ""), (q, "")])], ["integral", "integral_of_square"])
    raise ValueError("equation set %r has no invariants defined" % eq)


def field_programs(model: ModelParameters, u="u", v="v"):
    """The derived fields of the wind (u, v) as outputs for ModelRun.project (and, through program_of_outputs, for reduce, extrema,
    distribution, statistics): a dict name -> [(coef, r_power, [(var, slot), ...]), ...] with
        vorticity       v_r + v / r - u_l / r     divergence      u_r + u / r + v_l / r      (RL / RLZ; on R / RZ: v_r and u_r)
        kinetic_energy  (u^2 + v^2) / 2           speed2          u^2 + v^2
    from the patch's geometry.  A grid without `v` (the 1-D sets) gets the u parts and no vorticity."""
    gp = model.grid_params
    if u not in gp.vars:
        raise ValueError("field_programs: the grid has no variable %r" % (u,))
    wind = (u, v) if v in gp.vars else (u,)
    polar = "L" in gp.geometry
    out = {"divergence": [(1.0, 0, [(u, "r")])] + ([(1.0, -1, [(u, "")])] if polar else [])}
    if len(wind) == 2:
        out["vorticity"] = [(1.0, 0, [(v, "r")])] + ([(1.0, -1, [(v, "")]), (-1.0, -1, [(u, "l")])] if polar else [])
        if polar:
            out["divergence"].append((1.0, -1, [(v, "l")]))
    out["kinetic_energy"] = _speed2(wind, 0.5)
    out["speed2"] = _speed2(wind, 1.0)
    return out


def function_programs(model: ModelParameters, u="u", v="v", h="h"):
    """The nonlinear derived fields of the wind (u, v) and the depth h as outputs for ModelRun.derive: a dict name -> expression with
        speed                sqrt(u^2 + v^2)
        inflow_angle         atan2(u, v): the angle of the wind off the tangential direction, positive outward
        potential_vorticity  (vorticity + f) / (D + h), for the sets with a depth parameter D: Hfree, the depth the continuity
                             equation of the slab and height-resolved shallow-water sets multiplies the divergence with
                             (-(Hfree + h) div), or H of the linear shallow-water sets (-H div); f = 0 where the set has none
        rossby_number        vorticity / f, where the set has a non-zero f
    and the grid's field_programs entries they are made of.  Outputs are left out where the grid lacks their variables."""
    gp = model.grid_params
    fp = field_programs(model, u, v)
    pp = {(k if isinstance(k, str) else str(k)).lstrip(":"): val for k, val in (model.physical_params or {}).items()}
    out = {"speed": ("sqrt", fp["speed2"])}
    if v in gp.vars:
        out["inflow_angle"] = ("atan2", [(1.0, 0, [(u, "")])], [(1.0, 0, [(v, "")])])
        f = float(pp.get("f", 0.0))
        depth = pp.get("Hfree", pp.get("H"))
        if depth is not None and h in gp.vars:
            out["potential_vorticity"] = ("div", fp["vorticity"] + [(f, 0, [])], [(float(depth), 0, []), (1.0, 0, [(h, "")])])
        if f != 0.0:
            out["rossby_number"] = ("div", fp["vorticity"], f)
    return out


def thermo_programs(model: ModelParameters, liquid=None):
    """The moist thermodynamic fields of Euler_test / rainfall_test as outputs for ModelRun.derive: a dict name -> expression with
        q_v  rho_d  T [K]  p [hPa]  rho  theta  theta_e  theta_rho  rh  q_sat
    on the totals s + sbar, xi + xibar, mu + mubar, each written expression by expression as the reference has it:
    thermodynamic_tuple, potential_temperature, reversible_theta_e and theta_rho (src/thermodynamics.jl:260-297), q_sat_liquid
    (:163-170), rh = e / e_s of reversible_theta_e's H_term, rho = rho_d (1 + q_v) for Euler_test (src/testModels.jl:166) and
    rho_d (1 + q_t) for rainfall_test (:476).  ahyp, dry_density, temperature, the pressure of thermodynamic_tuple, vapor_pressure,
    sat_pressure_liquid_buck and L_v are the library's own functions (the composites of sx_derive), so T and p are the model's.
    liquid: the liquid mixing ratio q_l as an expression; None is the reference's default argument mu_l = 0, q_l = ahyp(0) = 0, for
    Euler_test, and for rainfall_test q_l = ahyp(mu_c) + ahyp(mu_r) as the set forms it (src/testModels.jl:472-474).
    All ten need 42 operations and a program holds 32: derive nine in one call and theta_e (30) in another.  rainfall_test's theta_e
    with the set's own q_l needs 34 and does not pack; liquid=0.0 gives the reference's default there."""
    eq = model.equation_set
    if eq not in ("Euler_test", "rainfall_test"):
        raise ValueError("thermo_programs: equation set %r carries no (s, xi, mu)" % (eq,))
    from . import thermodynamics as TH
    var = lambda n: [(1.0, 0, [(n, "")])]
    S, XI, MU = (("add", var(n), ("ref", n + "bar", "")) for n in ("s", "xi", "mu"))
    q_v = ("ahyp", MU)
    rho_d = ("dry_density", XI)
    T = ("temperature", S, rho_d, q_v)
    p = ("pressure", T, rho_d, q_v)
    if liquid is None and eq == "rainfall_test":
        liquid = ("add", ("ahyp", var("mu_c")), ("ahyp", var("mu_r")))
    q_t = q_v if liquid is None else ("add", q_v, liquid)
    theta = ("mul", T, ("pow", ("div", TH.p_0, p), TH.Rd / TH.Cpd))
    e, es = ("vapor_pressure", p, q_v), ("esat_buck", T, p)
    cp = ("add", TH.Cpd, ("mul", TH.Cl, q_t))
    theta_term = ("mul", T, ("pow", ("div", TH.p_0, ("sub", p, e)), ("div", TH.Rd, cp)))
    rh = ("div", e, es)
    H_term = ("pow", rh, ("div", ("mul", -TH.Rv, q_v), cp))
    exp_term = ("exp", ("div", ("mul", ("l_v", T), q_v), ("mul", cp, T)))
    return {"q_v": q_v, "rho_d": rho_d, "T": T, "p": p, "rho": ("mul", rho_d, ("add", 1.0, q_v if eq == "Euler_test" else q_t)), "theta": theta,
            "theta_e": ("mul", ("mul", theta_term, H_term), exp_term),
            "theta_rho": ("div", ("mul", theta, ("add", 1.0, ("div", q_v, TH.Eps))), ("add", 1.0, q_t)), "rh": rh,
            "q_sat": ("div", ("mul", TH.Eps, es), ("sub", p, es))}


def regular_gridpoints(gp: GridParameters, nr, nl=None, nz=None):
    """An evenly spaced tensor grid in r[, lambda][, z], edges included (lambda: [0, 2 pi], both ends), as rows r[, lambda][, z] in
    getGridpoints' order: r slowest, z fastest."""
    axes = [np.linspace(gp.xmin, gp.xmax, int(nr))]
    if "L" in gp.geometry:
        if nl is None:
            raise ValueError("nl is needed on an %s grid" % gp.geometry)
        axes.append(np.linspace(0.0, 2.0 * np.pi, int(nl)))
    if "Z" in gp.geometry:
        if nz is None:
            raise ValueError("nz is needed on an %s grid" % gp.geometry)
        axes.append(np.linspace(gp.zmin, gp.zmax, int(nz)))
    mesh = np.meshgrid(*axes, indexing="ij")
    return np.stack([m.reshape(-1) for m in mesh], axis=1)


def cartesian_gridpoints(gp: GridParameters, nx, ny, nz=None):
    """x, y evenly spaced on [-xmax, xmax]^2 (x slowest; with nz, z levels on [zmin, zmax] fastest) mapped to (r, lambda); keeps the
    points with xmin <= r <= xmax.  Returns (points [n_kept, n_coord], index [n_kept] of every kept point in the full nx * ny
    [* nz] grid)."""
    if "L" not in gp.geometry:
        raise ValueError("a Cartesian grid needs an RL or RLZ geometry")
    x = np.linspace(-gp.xmax, gp.xmax, int(nx))
    y = np.linspace(-gp.xmax, gp.xmax, int(ny))
    axes = [x, y]
    if "Z" in gp.geometry:
        if nz is None:
            raise ValueError("nz is needed on an %s grid" % gp.geometry)
        axes.append(np.linspace(gp.zmin, gp.zmax, int(nz)))
    mesh = [m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij")]
    r = np.hypot(mesh[0], mesh[1])
    lam = np.mod(np.arctan2(mesh[1], mesh[0]), 2.0 * np.pi)
    keep = np.nonzero((r >= gp.xmin) & (r <= gp.xmax))[0]
    cols = [r[keep], lam[keep]] + ([mesh[2][keep]] if len(mesh) == 3 else [])
    return np.stack(cols, axis=1), keep


def num_columns(grid: Grid):
    return int(grid.dims.n_hpoints) if "Z" in grid.patch_params.geometry else 0


def checkCFL(grid: Grid):
    """checkCFL (src/semiimplicit.jl:737-751): error on NaN in physical[:, v, 1]."""
    if grid.check_nan():
        raise RuntimeError("NaN found in a model variable! CFL condition likely violated")
