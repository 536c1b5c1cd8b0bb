"""scythe.jl_amd - MI355X-native spectral-transform time stepping for Scythe.jl (hot path only).

The directory name contains a dot, so import it through the `scythe_jl_amd` shim at the repo root."""
from ._lib import load, ScytheHipError, LIB_PATH
from .model import (CubicBSpline, Chebyshev, GridParameters, ModelParameters, Grid, createGrid, getGridpoints,
                    calcTileSizes, num_columns, checkCFL, comm_unique_id, eval_basis, regular_gridpoints,
                    cartesian_gridpoints, Program, reduce_weights, reduce_planes, pack_reduce_program, invariants,
                    spectrum_check, pack_spectrum_pairs, companion_grid, elliptic_check, antiderivative_check, Refined, free_mask, newton_step,
                    Crossings, bracket_step, Isosurface, isosurface_check, column_series, columns_of, Distribution, distribution_slot, distribution_check,
                    pack_vortex_fields, default_vortex_n_az, vortex_check, Statistics, pack_statistics, companion_params, project_check,
                    project_point, program_of_outputs, field_programs, regrid_check, regrid_columns, FunctionProgram,
                    pack_function_program, derive_check, derive_point, function_programs, thermo_programs)
from .driver import (PatchLayout, LocalExchange, DistExchange, A2ALayout, LocalA2AExchange, DistA2AExchange, LibExchange, LocalLibExchange, ModelRun,
                     integrate_model, Located, WindRadii, Cfad, Exceedance, Quantile, VortexProfile, Swath)
from .io import read_physical_grid, write_output, write_gridded_output, write_parcels, write_statistics, statistics_header
from . import thermodynamics, reference_state
from .reference_state import ReferenceState, Chebyshev1D
