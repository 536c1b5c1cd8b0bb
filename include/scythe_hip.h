/*
 * scythe_hip.h — C ABI of libscythe_hip.so: the MI355X (gfx950) implementation of Scythe.jl's per-time-step
 * spectral-transform hot path.  Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * The reference (Julia) has no FFI for this path; the seam is the pair of remote calls the master issues per step
 * (SURVEY.md 8(b)).  Every entry point cites the reference call it replaces (paths relative to the reference tree).
 * The Julia-side `ccall` glue a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; sx_last_error() gives the message
 *     (the reference signals errors with Julia exceptions: src/Scythe.jl:40, src/semiimplicit.jl:745,
 *      src/spectralGrid.jl:88-91).
 *   - host arrays use the reference's own layouts (column-major as in Julia):
 *        physical[point, var, deriv]   point = (ring-major, lambda, z innermost)   src/semiimplicit.jl:48, 64
 *        spectral[index, var]          index = (z-mode, wavenumber block, radial node), node fastest
 *     host pointers are borrowed for the duration of the call only.
 *   - one handle per tile (= per worker process / GPU, src/semiimplicit.jl:179-184); calls on one handle are serial.
 *   - t is the 1-based step counter of model_loop (src/semiimplicit.jl:268); it selects Euler/AB2/AB3.
 */
#ifndef SCYTHE_HIP_H
#define SCYTHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SX_ABI_VERSION 2

/* geometry  (GridParameters.geometry, src/spectralGrid.jl:21, 63-94) */
enum { SX_GEOM_R = 0, SX_GEOM_RZ = 1, SX_GEOM_RL = 2, SX_GEOM_RLZ = 3 };

/* radial / vertical boundary-condition codes (CubicBSpline.* / Chebyshev.* Dicts, models/ *.jl) */
enum { SX_BC_R0 = 0, SX_BC_R1T0 = 1, SX_BC_R1T1 = 2, SX_BC_R1T2 = 3, SX_BC_R2T10 = 4, SX_BC_R2T20 = 5, SX_BC_R3 = 6,
       SX_BC_PERIODIC = 7 };

/* equation sets, selected by name in the reference (src/semiimplicit.jl:357-363) */
enum {
    SX_EQ_LINEAR_ADVECTION_1D = 0,   /* src/testModels.jl:1-20   */
    SX_EQ_LINEAR_ADVECTION_RZ = 1,   /* src/testModels.jl:22-45  */
    SX_EQ_LINEAR_ADVECTION_RL = 2,   /* src/testModels.jl:47-73  */
    SX_EQ_LINEAR_ADVECTION_RLZ = 3,  /* src/testModels.jl:75-98  */
    SX_EQ_ONEWAY_SW_SLAB = 4,        /* src/shallowWaterModels.jl:1-113   */
    SX_EQ_TWOWAY_SW_SLAB = 5,        /* src/shallowWaterModels.jl:115-233 */
    SX_EQ_ONEWAY_SW_HRBL = 6,        /* src/shallowWaterModels.jl:346-511 */
    SX_EQ_LINEAR_ACOUSTIC_RZ = 7,    /* synthetic vehicle for semiimplicit_adjustment (src/semiimplicit.jl:521-597);
                                        Euler_test's variable layout and implicit terms (src/testModels.jl:188-205)
                                        with a linearised pressure-gradient force */
    SX_EQ_EULER_TEST = 8,            /* src/testModels.jl:100-215: moist Euler RZ (s, xi, mu, u, w) about a reference state,
                                        semi-implicit in the vertical acoustic terms; needs sx_model_desc.ref_state */
    SX_EQ_LINEAR_SW_1D = 9,          /* src/shallowWaterModels.jl:235-259: LinearShallowWater1D (h, u) on an R grid */
    SX_EQ_LINEAR_SW_RL = 10,         /* src/shallowWaterModels.jl:261-298: LinearShallowWaterRL (h, u, v) on an RL grid */
    SX_EQ_RAINFALL_TEST = 11,        /* src/testModels.jl:387-585 + src/microphysics.jl:139-195: rainfall_test, Euler_test with
                                        Ooyama (2001) warm rain on an RZ grid (s, xi, mu, u, w, mu_c, mu_r, qss = variables
                                        1-8); needs sx_model_desc.ref_state, and xi_index 2 / w_index 5 when semi-implicit.
                                        After the explicit (and semi-implicit) step, condensation_adjustment runs per column.
                                        Kept for parity, a quirk of the reference: its two clamps min(q_v, q_cond) and
                                        max(-q_c, q_cond) take whole columns (Julia's lexicographic isless on vectors, not a
                                        broadcast), so each keeps ONE of its two arguments for the entire column, decided at
                                        the first level where the two differ (isequal: -0.0 != 0.0, NaN == NaN) */
    SX_EQ_NONE = 99                  /* transforms only: sx_advance copies physical[:, :, 1] into var_np1 */
};

/* physical_params, fixed positions (model.physical_params Dict, models/ *.jl).  SX_P_H (:H, the mean depth of the linear
 * shallow-water sets, src/shallowWaterModels.jl:244, 272) came after the first 12 without an ABI version change: see
 * sx_model_desc.params. */
enum { SX_P_G = 0, SX_P_K, SX_P_CD, SX_P_HFREE, SX_P_HB, SX_P_F, SX_P_S1, SX_P_C0, SX_P_KH, SX_P_UM, SX_P_VM,
       SX_P_PXI_BAR, SX_P_H, SX_NPARAMS };

/* GridParameters flattened (src/spectralGrid.jl:20-45; tile construction src/semiimplicit.jl:155-169).
 * The patch fields describe the whole domain; the tile fields select this handle's radial range. */
typedef struct sx_grid_desc {
    int32_t abi_version;      /* SX_ABI_VERSION */
    int32_t geometry;         /* SX_GEOM_* */
    double xmin, xmax;        /* patch extent */
    int32_t num_cells;        /* patch cells; rDim = 3*num_cells, b_rDim = num_cells + 3 */
    double l_q;               /* spline filter length (default 2.0) */
    int32_t nvars;
    const int32_t *bcl;       /* [nvars] patch left BC for wavenumbers k >= 1 (and for R / RZ grids) */
    const int32_t *bcl_k0;    /* [nvars] patch left BC for wavenumber 0, or NULL = same as bcl */
    const int32_t *bcr;       /* [nvars] patch right BC */
    double zmin, zmax;
    int32_t zDim, b_zDim;     /* b_zDim <= 0 selects min(zDim, floor((2 zDim - 1) / 3) + 1) */
    const int32_t *bcb;       /* [nvars] bottom BC or NULL = R0 */
    const int32_t *bct;       /* [nvars] top BC or NULL = R0 */
    int32_t ring_uniform_L;   /* 0: native rings (4 + 4 ri points, kmax = ri); L > 0: every ring has L points,
                                 kmax = min(ri, L/2 - 1), zero phase offset (SURVEY.md 8(d) "perf shape") */
    int32_t tile_cell0;       /* first patch cell of this tile  (= spectralIndexL - 1) */
    int32_t tile_num_cells;   /* cells in this tile */
    int32_t tile_num;         /* informational (GridParameters.tile_num) */
    int32_t storage_f32;      /* 0: everything fp64 (the reference's arithmetic, `const real = Float64`,
                                 src/spectralGrid.jl:12).  1: the DERIVATIVE slots of `physical` (and of the node-space
                                 transforms) are stored as fp32; the value slot, the arithmetic, every spectral array, the
                                 banded solve and the time-stepping state stay fp64, so no fp32 rounding ever enters the
                                 model state directly - only the tendencies see it.
                                 2: additionally the SPECTRAL transform intermediates - the vertically inverted coefficients
                                 (between the Chebyshev and the Fourier stage of tileTransform!) and the ring spectra (between
                                 the Fourier and the B-spline stage of spectralTransform!) - are stored as fp32, every sum still
                                 accumulated in fp64: "fp32 mixed-precision transforms".  Rounding is relative to each spectral
                                 coefficient (6e-8), so the derivative operators do not amplify it, but it enters the state
                                 once per step.  Uniform power-of-two ring tables with zDim 32 / 64 / 128 only. */
} sx_grid_desc;

/* ModelParameters subset the step needs (src/Scythe.jl:8-21) */
typedef struct sx_model_desc {
    double ts;
    int32_t equation_set;     /* SX_EQ_* */
    int32_t semiimplicit;     /* options[:semiimplicit] */
    const double *params;     /* [SX_NPARAMS]; only the first 12 (up to SX_P_PXI_BAR) are read unless equation_set is
                                 SX_EQ_LINEAR_SW_1D or SX_EQ_LINEAR_SW_RL, which also read params[SX_P_H]: a caller built
                                 against the 12-entry table (before SX_P_H) never has a 13th double read */
    int32_t w_index, xi_index;/* 1-based variable indices of "w" and "xi" (semi-implicit only), 0 = absent */
    int32_t col_var;          /* 1-based variable whose vertical BCs the column operators of HRBL use ("h",
                                 src/shallowWaterModels.jl:423), 0 = variable 1 */
    const double *ref_state;  /* ReferenceState (src/reference_state.jl:4-10) for Euler_test or rainfall_test, or NULL:
                                 [3][3][zDim] = (sbar, xibar, mubar) x (value, d/dz, d2/dz2) x level (0 = bottom);
                                 Pxi_bar travels in params[SX_P_PXI_BAR] */
} sx_model_desc;

typedef struct sx_dims {
    int64_t n_points;         /* tile gridpoints N (incl. z) */
    int64_t n_hpoints;        /* horizontal points (N / zDim) */
    int32_t n_vars, n_derivs, n_coord;  /* V, D, columns of getGridpoints */
    int32_t rDim, b_rDim;     /* patch */
    int32_t tile_rDim, tile_b_rDim;
    int32_t zDim, b_zDim;
    int32_t kDim, n_blocks;   /* patch kDim, 1 + 2 kDim */
    int32_t tile_kDim, tile_n_blocks;
    int64_t s_patch;          /* patch spectral entries per variable */
    int64_t s_tile;           /* tile spectral entries per variable (reference tile layout) */
    int64_t n_cols;           /* internal: V * b_zDim * n_blocks columns of the [node][col] spectral arrays */
} sx_dims;

typedef struct sx_handle sx_handle;

/* --- lifetime -------------------------------------------------------------------------------------------------- */
/* createGrid(GridParameters(...)) + createModelTile  (src/semiimplicit.jl:155-169, 44-124) */
int sx_create(const sx_grid_desc *grid, const sx_model_desc *model, sx_handle **out);
int sx_destroy(sx_handle *h);
const char *sx_last_error(void);
int sx_abi_version(void);
/* getfield(Scythe, Symbol(equation_set)) (src/semiimplicit.jl:359-361): name -> SX_EQ_*, -1 if not in scope */
int sx_equation_set_id(const char *name);

/* The planes of `physical` an equation set reads, which are the planes sx_advance's inverse transform produces (sx_tile_transform
 * produces all): masks[n_vars], bit d set where variable v's slot d (the geometry's slot order: u, r, rr, then l, ll and / or z, zz)
 * is read; variables beyond the set's own read the value only; a mask of 0 is a variable the step does not transform back at all.
 * Pure host helper, no handle needed. */
int sx_equation_slot_masks(int32_t equation_set, int32_t geometry, int32_t n_vars, int32_t *masks);
int sx_get_dims(const sx_handle *h, sx_dims *out);
/* launch on this hipStream_t (NULL = default stream) */
int sx_set_stream(sx_handle *h, void *hip_stream);
int sx_synchronize(sx_handle *h);

/* --- geometry ---------------------------------------------------------------------------------------------------- */
/* getGridpoints(tile) (src/semiimplicit.jl:59): out[n_points, n_coord] column-major; columns r[, lambda][, z] */
int sx_get_gridpoints(const sx_handle *h, double *out);
/* calcTileSizes(patch, n) (src/semiimplicit.jl:141): out[5, n] column-major rows = xmin, xmax, num_cells,
 * spectralIndexL, gridpoint count.  Pure host helper, no handle needed. */
int sx_calc_tile_sizes(const sx_grid_desc *patch, int32_t n_tiles, double *out);

/* Chebyshev column operators (Springsteel CBtransform! -> CAtransform! -> CItransform! / CIxtransform / CIxxtransform /
 * CIInttransform(C0 = 0); call sites src/reference_state.jl:95-117, 143-167, src/shallowWaterModels.jl:426-429) as dense
 * [zDim x zDim] row-major collocation matrices acting on the values of one column (index 0 = bottom), and the levels z.
 * Pure host helper for one-time set-up work such as the reference state; any output pointer may be NULL. */
int sx_cheb_column_ops(double zmin, double zmax, int32_t zDim, int32_t b_zDim, int32_t bcb, int32_t bct, double *z,
                       double *rec, double *dz, double *dzz, double *integ);

/* The two operators of semiimplicit_adjustment's column solve (src/semiimplicit.jl:586-595, 768-781) exactly as sx_create builds
 * them for a model with these levels, vertical boundary conditions of w, Pxi_bar and tau (0.5 ts at t = 1, 1.25 ts after): W maps the
 * right-hand side g to the values of w, X to dw/dz; dense [zDim x zDim] row-major.  The Helmholtz matrix is inverted in extended
 * precision and rounded once, so two assemblies agree to cond(H) x 2^-64 only, not to the last bit: a host-side check of the
 * semi-implicit kernels has to read the operators the device holds, which are these.  Pure host helper; either output may be NULL. */
int sx_semi_column_ops(double zmin, double zmax, int32_t zDim, int32_t b_zDim, int32_t bcb, int32_t bct, double pxi_bar, double tau,
                       double *W, double *X);

/* splineTransform!'s arithmetic for ONE right-hand side on the host, two ways: through the parallel-cyclic-reduction tables the
 * device kernel k_solve_pcr applies (csrc/sx_pcr.hip: elimination blocks of the constant matrix Gamma (P + eps_q Q) Gamma^T worked
 * out once in extended precision, applied level by level in double) and through the banded Cholesky factors the serial kernel
 * k_solve applies.  b, a_pcr, a_chol: [num_cells + 3] patch rows of one spectral column; levels: reduction levels of the tables.
 * Pure host helper (no handle, no device): it validates the table construction where there is no GPU; never on the step path. */
int sx_spline_solve_check(int32_t num_cells, double xmin, double xmax, double l_q, int32_t bcl, int32_t bcr, const double *b,
                          double *a_pcr, double *a_chol, int32_t *levels);

/* The same right-hand side through the tables of the partitioned one-tile solve (k_solve_part, csrc/sx_iface.hip: `parts` row blocks
 * balanced in unknowns, each with its own factor, coupled through 6 edge values per block), applied in double in the kernel's order,
 * and through the banded Cholesky factors.  b, a_part, a_chol: [num_cells + 3]; ranges [parts][2] (may be NULL): the first and last
 * partition whose edge values each partition's correction reads.  Refuses PERIODIC classes and partitions the interface form does not
 * admit.  Pure host helper: it validates the table construction where there is no GPU; never on the step path. */
int sx_solve_part_check(int32_t num_cells, double xmin, double xmax, double l_q, int32_t bcl, int32_t bcr, int32_t parts, const double *b,
                        double *a_part, double *a_chol, int32_t *ranges);

/* The launch shape the library takes for given dimensions, with the SX_* switches as the environment has them now (read by the
 * function sx_create uses): which kernel instantiation - its text, such as "k_sbw_mfma<64, 32, 256>", into kernel[kernel_cap];
 * empty where none runs or the handle would be refused - and its grid arithmetic.  in / out by kind:
 *   SX_PLAN_FORWARD  spectralTransform!'s radial inner products:  in = geometry, zDim, b_zDim, K2 (device blocks per row: 2 (kDim + 1),
 *                    or 1 without azimuth), variables in the window, tile cells, storage_f32 == 2;
 *                    out = threads, bw, groups, nseg, cps, segs (sliding-window kernels; 0 where a kernel has no such figure)
 *   SX_PLAN_ZINV     vertical inverse:  in = geometry, zDim, K2, storage_f32 == 2;  out = CT, grid_x
 *   SX_PLAN_PCR      parallel-cyclic-reduction solve:  in = largest block-row count of the spline classes, num_cells + 3, K2,
 *                    (variable, z-mode) groups of the launch;  out = R, log2 R, threads;  kernel: empty
 *   SX_PLAN_FORWARD_CELLS  whether spectralTransform! runs as k_fl_forward_cells + k_nodes_z (the forward FFT kernel sums its ring spectra
 *                    into the spline nodes itself; SX_SBW_MFMA=2: never; by default only on launches that fill a round of CUs with segments of at least 9 cells, SX_SBW_MFMA=3: wherever the kernels apply) and that pair's shapes:  in = geometry, zDim, b_zDim, K2,
 *                    variables of the handle, tile cells, storage_f32 == 2, ring_uniform_L (0: native rings);
 *                    out = taken (0 / 1), S (cells per radial segment), segments, threads, nodes per k_nodes_z workgroup, node runs;
 *                    kernel: "k_fl_forward_cells<log2 L>", empty where the pair is not taken (SX_PLAN_FORWARD then names the launch)
 *   SX_PLAN_SOLVE    the contiguous one-tile B -> A solve:  in = num_cells + 3, any PERIODIC class (0 / 1) + 1, contiguous B (0 / 1) + 1,
 *                    right-hand sides of the launch;  out = partitions (0: not the partitioned kernel), threads per workgroup;
 *                    kernel: "k_solve_part" where the launch takes it, else "k_solve" (or k_solve_pcr, where SX_PLAN_PCR's tables exist
 *                    and the column count is at most SX_PCR_MAXCOLS)
 *   SX_PLAN_RZ_INVERSE  tileTransform! on a fused RZ grid (b_zDim <= zDim <= 256):  in = zDim, b_zDim, tile cells, variables,
 *                    storage_f32 (0 / 1);  out = grid x, grid y, grid z, dynamic LDS bytes, K chunks, 1 where the launch first raises
 *                    the kernel's dynamic-LDS limit above 64 KB;  kernel: "k_rz_inverse_nodes<double | float>" - grid x = ceil(cells / 13),
 *                    LDS = 8 (16 Zp + 3 * 16 * 65 + 3 * 39 * 4) bytes with Zp = b_zDim rounded up to its chunks of 32 rows - or, with
 *                    SX_RZ_INV=0 or where that LDS exceeds 64 KB, "k_rz_inverse<double | float>": grid x = ceil(3 cells / 16),
 *                    LDS = 8 * 3 * 16 Zp bytes with chunks of 64 rows.  Both: grid y = variables, grid z = ceil(ceil(zDim / 16) / 4)
 *   SX_PLAN_RZ_FORWARD  spectralTransform! on a fused RZ grid:  in = zDim, b_zDim, tile cells, variables in the window;
 *                    out = grid x = ceil((cells + 3) / 16), grid y = variables, grid z = ceil(nmt / mt_per_wg), mt_per_wg = min(nmt, 4)
 *                    with nmt = ceil(b_zDim / 16), K chunks = ceil(zDim / 64), LDS = 8 (16 * 64 chunks + 19 * 3 * 4) bytes;  kernel: "k_rz_forward"
 *   SX_PLAN_SEMI     the semi-implicit adjustment:  in = zDim, columns;  out = workgroups, threads, level tiles per wave trip, K chunks,
 *                    dynamic LDS bytes, 1 where the launch first raises the kernel's dynamic-LDS limit above 64 KB;  kernel: "k_semi_mfma" -
 *                    workgroups = ceil(columns / 16), threads = 64 min(8, ceil(zDim / 16)), that many level tiles per trip, K chunks =
 *                    ceil(zDim / 64), LDS = 8 * 4 * 16 * 64 chunks bytes - or, with SX_SEMI_MFMA=0, "k_semiimplicit": cpb = max(1, 256 / zDim)
 *                    columns per workgroup, workgroups = ceil(columns / cpb), threads = cpb zDim, LDS = 8 * 3 threads bytes, 0 tiles and chunks
 * Pure host helper (no handle, no device): the tests name the launch shapes they cover from it; never on the step path. */
enum { SX_PLAN_FORWARD = 0, SX_PLAN_ZINV = 1, SX_PLAN_PCR = 2, SX_PLAN_FORWARD_CELLS = 3, SX_PLAN_SOLVE = 4, SX_PLAN_RZ_INVERSE = 5,
       SX_PLAN_RZ_FORWARD = 6, SX_PLAN_SEMI = 7 };
int sx_launch_plan(int32_t kind, const int32_t *in, int32_t *out, char *kernel, int32_t kernel_cap);

/* The work lists of the native-ring DFT launches (csrc/sx_dft.hip) of a tile of cells cell0 .. cell0 + num_cells - 1 with Springsteel's
 * ragged rings: pairs (tile ring, x) in launch order, most expensive first; items[2 cap] receives them where cap holds them all
 * (items may be null: counts only; too small a cap is an error); counts[0] = pairs, counts[1] = of which - listed first - pairs of rings with kmax > 319.
 *   SX_DFT_LIST_RLZ         RLZ grids: x = variable; planes[n_vars] = derivative planes asked of each variable (0: no pair; the forward
 *                           list is the one with 1 everywhere)
 *   SX_DFT_LIST_RL_INVERSE  RL grids, inverse: x = part of 8 row tiles of the quarter ring (n_vars, planes: not read)
 *   SX_DFT_LIST_RL_FORWARD  RL grids, forward: x = part of 128 wavenumbers
 * Pure host helper (no handle, no device): the tests compare the lists with the rule stated here; never on the step path. */
enum { SX_DFT_LIST_RLZ = 0, SX_DFT_LIST_RL_INVERSE = 1, SX_DFT_LIST_RL_FORWARD = 2 };
int sx_dft_work_list(int32_t kind, int32_t cell0, int32_t num_cells, int32_t n_vars, const int32_t *planes, int32_t *items, int64_t cap,
                     int32_t *counts);

/* --- state in / out (host pointers, reference layouts) ------------------------------------------------------------- */
/* read_physical_grid -> physical[:, v, 1]  (src/semiimplicit.jl:134): values[n_points, n_vars] */
int sx_set_physical_values(sx_handle *h, const double *values);
/* tile.physical (src/semiimplicit.jl:305, 290): out[n_points, n_vars, n_derivs] */
int sx_get_physical(sx_handle *h, double *out);
/* mtile.var_np1 (src/semiimplicit.jl:21, 731): out[n_points, n_vars] */
int sx_get_var_np1(sx_handle *h, double *out);
/* tile.spectral after calcTendency (src/semiimplicit.jl:323): out[s_tile, n_vars] B coefficients */
int sx_get_tile_spectral(sx_handle *h, double *out);
/* sharedSpectral -> device (src/semiimplicit.jl:285 input): shared[s_patch, n_vars] B coefficients */
int sx_set_patch_spectral_b(sx_handle *h, const double *shared);
/* mtile.patchSpectral (src/semiimplicit.jl:289): out[s_patch, n_vars] A coefficients */
int sx_get_patch_spectral_a(sx_handle *h, double *out);
int sx_set_patch_spectral_a(sx_handle *h, const double *a);

/* calcPatchMap / calcHaloMap (src/semiimplicit.jl:79-86) as 1-based linear indices into ONE variable's column of the
 * reference layouts (add (v - 1) * s_patch resp. (v - 1) * s_tile for variable v):
 *   patch_owned[i] <-> tile_owned[i]   sharedSpectral[patchIndexMap] .= tileView            (:323)   n_owned entries
 *   patch_halo[i]  <-> tile_halo[i]    put!(haloSend, haloSendView) on this tile (:320);  on the NEXT tile
 *                                      sharedSpectral[haloReceiveIndexMap] .+= buffer (:326-329) with haloReceiveIndexMap =
 *                                      this tile's patch_halo                                         n_halo entries
 * The last tile owns all its rows (n_halo = 0).  Any output pointer may be NULL. */
int sx_index_map_sizes(const sx_handle *h, int64_t *n_owned, int64_t *n_halo);
int sx_index_maps(const sx_handle *h, int64_t *patch_owned, int64_t *tile_owned, int64_t *patch_halo, int64_t *tile_halo);

/* --- restart state (the reference can only restart from a physical_out CSV, which loses the
 * Adams-Bashforth history; this blob lets a run continue bit-identically) ------------------------------------------- */
/* The tile's A coefficients (its own radial nodes) and the tendency history expdot_nm1 / expdot_nm2 (and impdot_nm1 / nm2
 * when semi-implicit) as of the last completed step, in the library's device layout: an opaque blob for a handle created
 * from the same descriptors.  n_doubles from sx_state_size; sx_set_state must be followed by sx_advance(h, t + 1) with the
 * t of the step the state was taken after (t >= 2; earlier steps have no full history and restart from the values). */
int sx_state_size(const sx_handle *h, int64_t *n_doubles);
int sx_get_state(sx_handle *h, double *out);
int sx_set_state(sx_handle *h, const double *in);

/* --- the hot path -------------------------------------------------------------------------------------------------- */
/* spectralTransform!(tile) on var_np1 (calcTendency, src/semiimplicit.jl:728-735) -> tile B coefficients */
int sx_spectral_transform(sx_handle *h);
/* splineTransform!(patchSplines, patchSpectral, gp, sharedSpectral, tile) (src/semiimplicit.jl:237, 285) */
int sx_spline_transform(sx_handle *h);
/* tileTransform!(patchSplines, patchSpectral, gp, tile, splineBuffer) (src/semiimplicit.jl:241, 305) */
int sx_tile_transform(sx_handle *h);
/* advanceTimestep up to and including calcTendency (src/semiimplicit.jl:305-317):
 * tileTransform! -> equation set -> explicit_timestep [-> semiimplicit_adjustment] -> spectralTransform!
 * Only the derivative planes the equation set reads are produced, and on uniform rings part of them never leaves the
 * node-space form: after sx_advance the contents of `physical` are unspecified - call sx_tile_transform (the output path,
 * src/semiimplicit.jl:289-290) before sx_get_physical. */
int sx_advance(sx_handle *h, int32_t t);
/* model_loop's body for a ONE-tile patch (src/semiimplicit.jl:268-285 with a single worker): advanceTimestep followed by
 * splineTransform!, i.e. sx_advance(h, t) + sx_spline_transform(h) in one call.  With SX_GRAPH=1 in the environment at sx_create the
 * step's kernel launches are captured into a hipGraph - once per rotation of the tendency-history buffers, from the third step
 * this handle executes (Adams-Bashforth-3: the launch arguments then repeat with period 3) - and replayed: ONE graph launch per
 * step instead of 5-9 kernel launches, for grids whose step is shorter than the host takes to enqueue it (R, RZ and small RL
 * grids).  Bit-identical to the plain launches; timers on, or a failed capture, fall back to them.  The captured graphs hold the
 * stream and the B buffers' pointers: sx_set_stream (to another stream), sx_bind_tile_b (to another buffer) and sx_bind_patch_b drop
 * them, and the next sx_step captures again. */
int sx_step(sx_handle *h, int32_t t);
/* physical_model only (src/semiimplicit.jl:357-363) on the current tile.physical.
 * What the call covers: the equation set's tendency and the explicit step (Euler at t = 1, AB2 at t = 2, AB3 from t = 3) into
 * var_np1, then the semi-implicit adjustment where the model has it and condensation_adjustment for rainfall_test, in that order.
 * The shallow-water sets also write their diagnostic w into physical[:, 6, 1] (1-based); no other plane of `physical` changes.
 * t = 1 restarts the tendency history. */
int sx_physics(sx_handle *h, int32_t t);
/* checkCFL (src/semiimplicit.jl:737-751): flag = 1 if any NaN in the model state (scans var_np1, which every
 * sx_advance / sx_set_physical_values leaves complete; a NaN in physical[:, v, 1] always reaches it) */
int sx_check_nan(sx_handle *h, int32_t *flag);
/* on-device diagnostic: out[n_vars] = max |var_np1[:, v]| after the last step; with the grid spacing
 * the caller forms the advective CFL number without pulling a field to the host.  A NaN anywhere in a variable makes its
 * maximum NaN (like maximum(abs, x) in Julia).  No allocation per call: the scratch lives with the handle. */
int sx_max_abs(sx_handle *h, double *out);

/* --- evaluation at arbitrary points --------------------------------------------------------------------------------
 * The state is the continuous function u(r, lambda, z) = sum A[zm, blk, node] phi_node(r) F_blk(lambda) C_zm(z); tileTransform!
 * (src/semiimplicit.jl:241, 305) samples it at the tile's own gridpoints only.  sx_evaluate samples the A coefficients the handle
 * holds now (the patch rows sx_tile_transform reads) anywhere in the tile:
 *   points[n_points, n_coord] column-major, columns r[, lambda][, z] as sx_get_gridpoints returns them;
 *   out[n_points, n_vars, n_derivs] column-major, slots as in `physical` (u, r, rr[, l, ll][, z, zz]).
 * r within the tile's extent and z within [zmin, zmax], both ends included; lambda any finite real.  A NaN / Inf coordinate, an r or z
 * out of range or a null pointer with n_points > 0 fail the call before anything is written to out.
 * Azimuthal truncation: the inverse transform at ring ri sums the wavenumbers k <= kmax[ri] only.  SX_EVAL_RING_K: at radius r the
 * kmax of the last patch ring whose radius is <= r (ring 1 below the first ring; piecewise constant in r, and the tile's own
 * gridpoints give what sx_tile_transform + sx_get_physical give).  SX_EVAL_ALL_K: every wavenumber of the patch (smooth in r).
 * Vertical: with a = CA b, CA the boundary-condition projection of the variable's (bcb, bct), the DCT-I series
 * a0 + 2 sum a_k T_k(x) + a_{N-1} T_{N-1}(x) at x = (z - mid) / (-Lz / 2); z, zz from the coefficient-space derivative.
 * Runs on the handle's stream and returns after the copy-out; reads A only: `physical`, var_np1, the tendency history, the B arrays
 * and captured graphs stay as they are (a deferred diagnostic variable is brought up to date first, as for every reader of A). */
enum { SX_EVAL_RING_K = 0, SX_EVAL_ALL_K = 1 };
int sx_evaluate(sx_handle *h, const double *points, int64_t n_points, int32_t flags, double *out);
/* sx_evaluate restricted to a wavenumber band: only the wavenumbers kmin <= k <= min(kmax, kcap) of the azimuthal series are summed
 * (k = 0 is the azimuthal mean), everything else as sx_evaluate.  0 <= kmin <= kmax; a kmax above sx_dims.kDim is clamped; kmin > kmax or
 * a negative bound is refused.  sx_evaluate is the band (0, kDim), bit for bit.  On a grid without an azimuth only k = 0 exists. */
int sx_evaluate_band(sx_handle *h, const double *points, int64_t n_points, int32_t flags, int32_t kmin, int32_t kmax, double *out);
/* The weights sx_evaluate applies at ONE point of the tile the descriptor selects, for variable var: node0 = 0-based patch row of the
 * first of the 4 spline nodes, w_r = phi, phi', phi'' at them, kcap as above, w_z[s][zm] = row s (value, d/dz, d2/dz2) of the
 * vertical operator at the point's z (RZ / RLZ grids; untouched otherwise).  Refuses what sx_evaluate refuses; any output pointer
 * may be NULL.  Pure host helper (no handle, no device): the basis arithmetic is testable where there is no GPU. */
int sx_eval_basis(const sx_grid_desc *grid, int32_t var /*1-based*/, const double *point /*[n_coord]*/, int32_t flags,
                  int32_t *node0, double *w_r /*[3][4]*/, int32_t *kcap, double *w_z /*[3][b_zDim]*/);

/* --- azimuthal harmonics of the state ---------------------------------------------------------------------------------
 * With F_blk as above (block 0 -> 1, block 2k -> 2 cos k lambda, block 2k + 1 -> -2 sin k lambda) the state at (r, z) is
 *     u(r, lambda, z) = Re sum_{k = 0}^{kcap(r)} eps_k c_k(r, z) e^{i k lambda},   eps_0 = 1, eps_k = 2 for k >= 1,
 * and the coefficient blocks are the harmonics themselves:
 *     c_k(r, z) = sum_node sum_zm (A[zm, 2k, node] + i A[zm, 2k + 1, node]) phi_node(r) Wz[zm](z)
 * (Im c_0 = 0: block 1 is padding and is never read).  On a ring of the grid, for k <= kmax[ring] < L / 2, c_k is the discrete
 * transform (1 / L) sum_j u_j e^{-i k lambda_j} of the ring's values.  No Fourier transform is taken and nothing but A is read.
 * slot_mask picks any subset of five slots, bits 0..4 = u, r, rr, z, zz: radial weights phi, phi', phi'', phi, phi and vertical
 * operator row 0, 0, 0, 1, 2 (value, d/dz, d2/dz2).  lambda derivatives are i k c_k and are left to the caller.
 * The radial weights, the wavenumber cap kcap(r) (flags SX_EVAL_RING_K / SX_EVAL_ALL_K) and the vertical rows are those of sx_evaluate
 * (sx_eval_basis returns them); entries with k > kcap(r) are exact zeros.
 *   radii[n_r]: any order, duplicates allowed, within the tile's extent, both ends included;
 *   heights[n_z]: within [zmin, zmax]; a grid without a vertical takes heights = NULL, n_z = 0 (one "height") and no z / zz bit;
 *   out[2 (kDim + 1), n_z, n_r, n_vars, n_slots] column-major, n_slots = popcount(slot_mask) in the order u, r, rr, z, zz: the tensor
 *   product of the radii and the heights.  The first axis is the device block axis (re, im interleaved): viewed as complex the array
 *   is [kDim + 1, n_z, n_r, n_vars, n_slots].  kDim = sx_dims.kDim; a grid without an azimuth has kDim = 0 and c_0 = the value.
 * Refused, with a message and before anything is written to out: a NaN / Inf or out-of-range radius or height; n_r < 0 or n_z < 0;
 * slot_mask 0 or with a bit the geometry has no slot for; flags other than the two above; a null pointer with a non-zero count;
 * a grid whose b_zDim exceeds 128 (the vertical modes of a column are held in registers).
 * n_r == 0 succeeds and writes nothing.  A result does not depend on which other radii are in the call (bitwise).
 * Runs on the handle's stream and returns after the copy-out; reads A only: `physical`, var_np1, the tendency history, the B arrays
 * and captured graphs stay as they are (a deferred diagnostic variable is brought up to date first, as for every reader of A). */
enum { SX_HARM_U = 1, SX_HARM_R = 2, SX_HARM_RR = 4, SX_HARM_Z = 8, SX_HARM_ZZ = 16 };
int sx_harmonics(sx_handle *h, const double *radii, int32_t n_r, const double *heights, int32_t n_z,
                 int32_t flags, int32_t slot_mask, double *out);

/* --- azimuthal power and cross spectra of the state --------------------------------------------------------------------
 * How much variance, energy or flux sits in each azimuthal wavenumber, per ring and for the domain, from A alone.
 * A pair is two planes (var_a, slot_a), (var_b, slot_b): var 1-based, slot 0..4 = u, r, rr, z, zz, the five slots of sx_harmonics with
 * their radial weights and vertical rows.  n_pairs <= 16 per call; a pair with a == b is a power spectrum.
 * At tile ring i (the radius sx_get_gridpoints prints, truncation SX_EVAL_RING_K: kcap = kmax[ring], as sx_tile_transform) and level
 * j (the Chebyshev-Gauss-Lobatto height sx_get_gridpoints prints)
 *     P_k(i, j) = eps_k Re(c_k^a conj(c_k^b)) = eps_k (a[2k] b[2k] + a[2k + 1] b[2k + 1]),   eps_0 = 1, eps_k = 2 for k >= 1,
 * a[blk], b[blk] the per-block harmonic values sx_harmonics returns at (r_i, z_j); block 1 is padding, is never read and counts as 0.
 * Entries with k > kmax[ring] are exact zeros; on a grid without an azimuth kDim = 0 and P_0 is the pointwise product.
 * Kind.  SX_SPEC_RING: out[kDim + 1, tile ring, n_pairs] column-major = sum_level w_z[level] P_k(ring, level) (without a vertical: P_k
 * itself), the radius-wavenumber diagram.  SX_SPEC_DOMAIN: out[kDim + 1, n_pairs] = sum_ring 2 pi w_r[ring] (the ring value above),
 * this tile's share of the domain integral per wavenumber.  w_r, w_z are the arrays sx_reduce_weights returns and 2 pi stands for
 * w_l[ring] L[ring] (1 on a grid without an azimuth, as in sx_reduce).  Tiles own disjoint cells: a patch spectrum is the sum of the
 * tile results (domain kind) or their concatenation (ring kind).  Level-resolved spectra are what sx_harmonics gives.
 * Identity (Parseval; every ring table has 2 kmax[ring] < L[ring]): sum_k out_domain[k, p] equals sx_reduce(SX_REDUCE_DOMAIN,
 * SX_REDUCE_PHYSICAL) of the one-term program field(a) field(b) after sx_tile_transform, and sum_k out_ring[k, ring, p] equals the
 * w_z-weighted level sum of its SX_REDUCE_AZIMUTH result.
 * Refused, with a message and before anything is written to out: a null pointer with a non-zero count; n_pairs < 0 or > 16; an unknown
 * kind; a var or slot out of range; a z / zz slot on a grid without a vertical; a grid whose b_zDim exceeds 128 (as sx_harmonics).
 * n_pairs == 0 succeeds and writes nothing.
 * Sums are double-double, each by a fixed lane in a fixed order that depends on the grid and the pair list alone (no floating-point
 * atomics): two calls on the same data agree bitwise, and a pair's result does not depend on the other pairs of the call.
 * Runs on the handle's stream and returns after the copy-out; reads A only: `physical`, var_np1, the tendency history, the B arrays
 * and captured graphs stay as they are (a deferred diagnostic variable is brought up to date first, as for every reader of A). */
enum { SX_SPEC_RING = 0, SX_SPEC_DOMAIN = 1 };
int sx_spectrum(sx_handle *h, int32_t kind, int32_t n_pairs, const int32_t *pairs /*[n_pairs][4] = var_a, slot_a, var_b, slot_b*/,
                double *out);
/* the validator sx_spectrum itself calls: refuses what sx_spectrum refuses of a pair list.  Pure host helper, no handle and no device */
int sx_spectrum_check(const sx_grid_desc *grid, int32_t n_pairs, const int32_t *pairs);

/* --- Lagrangian parcels ----------------------------------------------------------------------------------------------------
 * Tracer points that move with the model on the device: positions, history and status live in device memory and one kernel launch
 * (k_parcels) per step forms every weight from the positions, sums the velocity from A and moves the parcels.
 * A parcel is a point (r[, lambda][, z]) in the coordinates of sx_get_gridpoints.  Three 1-based variable indices (var_r, var_l, var_z)
 * name the velocity components; 0 = no motion along that coordinate; a non-zero index for a coordinate the geometry lacks is refused.
 * All three are speeds (length per time): var_l is the tangential wind, not an angular rate.
 * Velocity: the value slot of those variables at the parcel, summed from the A coefficients the handle holds now with the SX_EVAL_ALL_K
 * truncation (smooth in r: a path sees no ring-to-ring jumps) and sx_evaluate's vertical series and boundary-condition projection:
 * what sx_evaluate(..., SX_EVAL_ALL_K) returns in slot 0, up to rounding.
 * Motion.  R / RZ: dx/dt = u, dz/dt = w.  RL / RLZ, in Cartesian form so that the centre is an ordinary point: X = r cos lambda,
 * Y = r sin lambda, dX/dt = u cos lambda - v sin lambda, dY/dt = u sin lambda + v cos lambda, afterwards r = hypot(X, Y) and
 * lambda = atan2(Y, X) kept in (-pi, pi]; at r == 0 lambda = 0.  The history holds the Cartesian velocity, not (u, v).
 * Time stepping: every parcel counts its own steps - Euler, then AB2, from the third step AB3, with explicit_timestep's coefficients
 * (src/semiimplicit.jl:672-698) - and every step makes one velocity evaluation.
 * Leaving: a parcel whose update has r outside the tile's radial extent or z outside [zmin, zmax] stays at its last inside position and
 * keeps a status, 0 active, 1 left radially, 2 left vertically (radially wins); it is never evaluated again.  Exception: on an R / RZ
 * grid whose var_r variable has PERIODIC conditions on both sides x wraps into [xmin, xmax).
 * One-tile patches are the intended use: a tile's parcels that cross its edge are frozen, not handed to the neighbour.
 *
 * sx_parcels_set creates or replaces the set (step counters 0); positions[n, n_coord] column-major.  n == 0 removes the set and frees
 * its memory.  Refused before anything is touched - an existing set stays as it is: a NaN / Inf coordinate, an r or z out of range, a
 * variable index out of range or for a missing coordinate, a null pointer with n > 0.  lambda may be any finite real; it is reduced
 * into (-pi, pi] in extended precision on the host.
 * sx_parcels_advance enqueues ONE kernel on the handle's stream and returns: no allocation, no copy, no synchronisation.  It reads A and
 * the parcel arrays and writes the parcel arrays only: `physical`, var_np1, the tendency history, the B arrays and captured graphs stay
 * as they are (a deferred diagnostic variable that is a velocity component is brought up to date first, as for every reader of A).
 * A non-finite dt is refused; without a set the call succeeds and does nothing.  A parcel's path does not depend on how many other
 * parcels the set holds or on their order (bitwise): which lane sums which column, and the order of the reduction, follow from the grid.
 * sx_parcels_get synchronises and copies out positions[n, n_coord], the velocity last evaluated [n, n_coord] (u[, v][, w], zero for an
 * index 0) and status[n]; any pointer may be NULL.  sx_parcels_count gives n (0 without a set).
 * sx_parcels_get_state / sx_parcels_set_state: positions, velocity, both history levels, counters, status and the three variable
 * indices as an opaque blob of sx_parcels_state_size doubles (0 without a set) for a handle created from the same descriptors; a run
 * resumed from it (together with sx_set_state) continues bitwise.  sx_kernel_bytes("k_parcels") gives the A bytes of the last advance. */
int sx_parcels_set(sx_handle *h, int64_t n, const double *positions, int32_t var_r, int32_t var_l, int32_t var_z);
int sx_parcels_count(const sx_handle *h, int64_t *n);
int sx_parcels_advance(sx_handle *h, double dt);
int sx_parcels_get(sx_handle *h, double *positions, double *velocity, int32_t *status);
int sx_parcels_state_size(const sx_handle *h, int64_t *n_doubles);
int sx_parcels_get_state(sx_handle *h, double *out);
int sx_parcels_set_state(sx_handle *h, const double *in, int64_t n_doubles);

/* --- elliptic inversion: streamfunction, velocity potential ------------------------------------------------------------
 * Solves, for the solution variable and every wavenumber k of the patch (k = 0 only on R / RZ grids),
 *     (lap_h - alpha) psi = f,    lap_h = (1 / J) d_r (J d_r) - k^2 / r^2  (RL / RLZ, J = r);   d_x^2  (R / RZ, J = 1)
 * in the weak form, in the patch's own spline basis phi_m (m = 0 .. num_cells + 2), with the 7-diagonal matrices
 *     S[i][j] = int J phi_i' phi_j' dr     T[i][j] = int phi_i phi_j / r dr (RL / RLZ only)     M[i][j] = int J phi_i phi_j dr
 *     N[i][j] = int r phi_i phi_j' dr      M0[i][j] = int phi_i phi_j dr
 * formed on the host in extended precision by Gauss-Legendre quadrature with 8 points per cell (exact for S, M, N, M0; for T the rule
 * is the definition) and rounded once.  With Gamma_k the boundary-condition projection of the solution variable as splineTransform!
 * applies it (its bcl_k0 for k = 0, its bcl for k >= 1, its bcr):
 *     K_k = Gamma_k (S + k^2 T + alpha M) Gamma_k^T  (SPD),     K_k x = -Gamma_k g,     a = Gamma_k^T x
 * per z-mode and per re / im block; block 1 (Im c_0) is never read and is written as zero.  With c_k = A[2k] + i A[2k + 1] as in
 * sx_harmonics the right-hand side g is one of
 *     SX_ELL_FIELD       var_a = the field f:        g = M a_f                                           any geometry; var_b ignored
 *     SX_ELL_VORTICITY   var_a = u, var_b = v:       r zeta = r v_r + v - u_lambda                       RL / RLZ only
 *                          g_re = (N + M0) v_re + k M0 u_im      g_im = (N + M0) v_im - k M0 u_re
 *     SX_ELL_DIVERGENCE  var_a = u, var_b = v:       r delta = r u_r + u + v_lambda                      RL / RLZ only
 *                          g_re = (N + M0) u_re - k M0 v_im      g_im = (N + M0) u_im + k M0 v_re
 * No derivative plane and no transform is taken: A is the only input.  The banded Cholesky factor of every K_k is worked out on the
 * host in extended precision, rounded once and kept with the source handle for the last (alpha, boundary conditions) used.
 *
 * sx_elliptic_solve writes the patch A rows of variable var_dst (1-based) of dst - the rows sx_tile_transform / sx_evaluate /
 * sx_harmonics / sx_spectrum of dst read, so everything the library has then samples psi and its derivatives.  dst may be src itself
 * (a spare variable of the model) or a one-variable companion handle with SX_EQ_NONE.  Runs on src's stream and returns after the
 * kernel has completed; reads A of src only (a deferred diagnostic variable is brought up to date first, as for every reader of A)
 * and writes only var_dst's A columns of dst: `physical`, var_np1, the tendency history, the B arrays, parcels and captured graphs of
 * both handles and every other variable's A stay bitwise as they are.  No floating-point atomics, a fixed order: two calls agree
 * bitwise and a column's result does not depend on the launch shape.
 * Refused, with a message and before anything is written: a null handle; an unknown rhs_kind; a variable index out of range; var_dst
 * equal to a source variable when dst == src; vorticity / divergence on R / RZ; a src or dst that is not a one-tile patch; a dst that
 * differs from src in geometry, xmin, xmax, num_cells, ring table, kDim, zDim, b_zDim, zmin or zmax; a source variable whose vertical
 * (bcb, bct) differs from var_dst's (the z-mode columns are carried over one to one); PERIODIC radial conditions on var_dst; a
 * non-finite or negative alpha; alpha == 0 with a k = 0 class that fixes the value on neither side (singular); on RL / RLZ with
 * xmin == 0 a k >= 1 class whose constrained basis does not vanish at r = 0 (decided from Gamma and phi(xmin): int phi phi / r has no
 * meaning for such a class); a K_k with a non-positive pivot.
 * sx_kernel_bytes("k_elliptic") gives the source columns in + the destination columns out + the factors of the last solve.
 *
 * sx_elliptic_check applies the same host-built factors to ONE right-hand side g for one wavenumber k, with the arithmetic of the
 * kernel from g on (fold with Gamma_k, the two sweeps, Gamma_k^T): a = Gamma_k^T K_k^-1 (-Gamma_k g).  It refuses what the solve
 * refuses of a descriptor, and a k outside 0 .. kDim.  Pure host helper (no handle, no device): the matrix construction and the
 * sweep are testable where there is no GPU. */
enum { SX_ELL_FIELD = 0, SX_ELL_VORTICITY = 1, SX_ELL_DIVERGENCE = 2 };
int sx_elliptic_solve(sx_handle *src, int32_t rhs_kind, int32_t var_a, int32_t var_b, double alpha, sx_handle *dst, int32_t var_dst);
int sx_elliptic_check(const sx_grid_desc *grid, int32_t var_dst, int32_t k, double alpha, const double *g /*[num_cells + 3]*/,
                      double *a /*[num_cells + 3]*/);

/* --- antiderivatives: radial and vertical --------------------------------------------------------------------------------
 * The integral of a variable UP TO A POINT, returned as a field that everything else can sample:
 *     SX_INT_R:  F(r) = int_{xmin}^{r} w f ds (SX_INT_FROM_LOW)   or   int_{r}^{xmax} w f ds (SX_INT_FROM_HIGH),   w = 1 (SX_INT_W_ONE) or
 *                r (SX_INT_W_R: the integrand r f, on any geometry)
 *     SX_INT_Z:  F(z) = int_{zmin}^{z} f dz' (FROM_LOW)   or   int_{z}^{zmax} f dz' = F(zmax) - F(z) (FROM_HIGH);   weight must be 0
 * A of src is the only input and the patch A rows of variable var_dst (1-based) of dst the only output, per (z-mode, re / im block)
 * column; block 1 (Im c_0) is never read and is written as zero.  dst is src itself (a spare variable) or a one-variable companion
 * handle with SX_EQ_NONE, as for sx_elliptic_solve.
 *
 * Radial.  With f = sum_j a_j phi_j in the patch's spline basis, F is projected onto var_dst's spline space exactly as the model
 * projects any field - a_dst = Gamma^T (Gamma (P + eps_q Q) Gamma^T)^-1 Gamma b, the B -> A of splineTransform! with var_dst's own class
 * (its bcl_k0 for k = 0, its bcl for k >= 1, its bcr) AND ITS l_q FILTER, through the Cholesky factor the handle's own solve uses - but
 * with the EXACT right-hand side b_i = int phi_i F dr, not the 3-point quadrature of the mish.  With Phi_j(r) = int_{xmin}^{r} w phi_j,
 * c_j = int w phi_j and m_i = int phi_i:
 *     b_i = sum_{|j - i| <= 3} Pband[i][j] a_j + m_i sum_{j <= i - 4} c_j a_j      (FROM_LOW;  FROM_HIGH: sum_{j >= i + 4}, its own band)
 * because phi_j ends before phi_i begins for j <= i - 4.  Pband [nb][7], c [nb], m [nb] are formed on the host in extended precision by
 * 8-point Gauss-Legendre quadrature per cell (exact: phi_i Phi_j is piecewise of degree <= 8), rounded once, and kept with the source
 * handle for the last (origin, weight, radial conditions of var_dst) used; a second call with the same key uploads nothing.  The running
 * sum is serial and in a fixed order per column.
 *
 * Vertical.  The A columns hold the truncated Chebyshev coefficients b; with the factors of the vertical transform
 *     Z = CB T Ic CA_src  [b_zDim][b_zDim]   (FROM_LOW: zero at zmin;   FROM_HIGH: CB (1 e_top^T - I) T Ic CA_src)
 * (CA_src with var_src's (bcb, bct); products in extended precision, rounded once) and A_dst[m][zm][blk] = sum_zm' Z[zm][zm'] A_src[m][zm'][blk]
 * for every node row and block.  On grids with at least 16 blocks per z-mode and b_zDim <= 64 the product runs on the f64 matrix
 * cores; otherwise (RZ grids: 1 block) one lane forms one output in a fixed order.
 *
 * Runs on src's stream and returns after completion; a deferred diagnostic variable is brought up to date first.  `physical`,
 * var_np1, the tendency history, B, parcels, statistics, captured graphs of both handles and every other variable's A stay bitwise
 * as they are.  No atomics, nothing across lanes: two calls agree bitwise, and a column's radial result does not depend on the launch
 * shape.
 * Refused, with a message and before anything is written: a null handle; an unknown axis, origin or weight; a variable index out of
 * range; var_dst == var_src when dst == src; a src or dst that is not a one-tile patch; a dst that differs from src in geometry, xmin,
 * xmax, num_cells, ring table, kDim, zDim, b_zDim, zmin or zmax; SX_INT_Z on a grid without a vertical; a non-zero weight with SX_INT_Z;
 * PERIODIC radial conditions on var_dst (SX_INT_R); for SX_INT_R a var_src whose (bcb, bct) differs from var_dst's (the z-mode columns
 * are carried one to one); for SX_INT_Z a var_src whose radial conditions (bcl, bcl_k0, bcr) differ from var_dst's (the rows are
 * carried one to one).
 * sx_kernel_bytes("k_antiderivative_r") gives the source columns in + the destination columns out + the tables + the intermediate
 * (the right-hand side and the forward sweep's vector each make one round trip through the destination columns: 4 x the live
 * destination columns); sx_kernel_bytes("k_antiderivative_z") gives 2 x 8 x nb x b_zDim x K2 + Z.
 *
 * sx_antiderivative_check states the same for ONE column on the host with the same tables and the kernel's arithmetic operation for
 * operation (radial: band, running sum, the two sweeps; vertical: the row sums in index order): a_src / a_dst are [num_cells + 3]
 * (radial, wavenumber k selects var_dst's class) or [b_zDim] (vertical, k only range-checked).  It refuses what the call refuses of a
 * descriptor, and a k outside 0 .. kDim.  Pure host helper (no handle, no device). */
enum { SX_INT_R = 0, SX_INT_Z = 1 };
enum { SX_INT_FROM_LOW = 0, SX_INT_FROM_HIGH = 1 };
enum { SX_INT_W_ONE = 0, SX_INT_W_R = 1 };          /* radial only: integrand f or r f, on any geometry */
int sx_antiderivative(sx_handle *src, int32_t var_src, int32_t axis, int32_t origin, int32_t weight, sx_handle *dst, int32_t var_dst);
int sx_antiderivative_check(const sx_grid_desc *grid, int32_t var_src, int32_t var_dst, int32_t axis, int32_t origin, int32_t weight,
                            int32_t k, const double *a_src, double *a_dst);

/* --- integrals and azimuthal means of field products ------------------------------------------------------------------
 * On-device diagnostics: budgets and azimuthal means / eddy covariances without pulling `physical` to the host.
 * Integrand program: n_terms <= 64 monomial terms feed n_out <= 16 outputs.  Term t is
 *     coef[t] * r^p * prod_{f < nf} field(var_f, slot_f)        added to output out_t,
 * nf = 0 .. 4 (nf = 0: the measure itself, area or volume), p an integer in [-2, 2], r the point's first coordinate (the double
 * sx_get_gridpoints returns), var 1-based, slot an index into `physical`'s derivative slots of the geometry (u, r, rr[, l, ll][, z, zz]).
 * Factor entries at f >= nf are ignored.  A program names at most 16 distinct (var, slot) planes; a sum that is no monomial (vorticity
 * squared) is written out as several terms.
 * Source.  SX_REDUCE_PHYSICAL: `physical` as it stands - defined only after sx_tile_transform, exactly as for sx_get_physical; with
 * storage_f32 the derivative slots are read in the type they are stored in.  SX_REDUCE_STATE: var_np1, slot 0 only; it is complete
 * after every sx_advance / sx_set_physical_values (what sx_check_nan relies on), so this source costs no transform.
 * Kind.  SX_REDUCE_AZIMUTH: out[tile ring, level, n_out] column-major, the ring fastest = (1 / L_ring) sum_lambda integrand, the
 * azimuthal mean at every ring and level (R / RZ grids: L = 1, the pointwise value).  SX_REDUCE_DOMAIN: out[n_out] =
 * sum_points w_r[ring] w_l[ring] w_z[level] integrand, this tile's share of the domain integral (tiles own disjoint cells: a patch
 * integral is the sum of the tile results), with
 *     w_r = DX (5, 8, 5) / 18 * J(r)   3-point Gauss-Legendre on each cell, whose nodes the radial gridpoints are (exact to degree 5
 *                                      per cell; NOT the 8:5:8 projection weights of the transforms), J = r on RL / RLZ, 1 on R / RZ
 *     w_l = 2 pi / L_ring              1 without an azimuth
 *     w_z = Clenshaw-Curtis weights of the zDim Chebyshev-Gauss-Lobatto levels times (zmax - zmin) / 2 (exact to degree zDim - 1),
 *                                      1 without a vertical
 * formed on the host in extended precision and rounded once.
 * Refused, with a message and before anything is written to out: a null pointer with a non-zero count; n_terms > 64, n_out > 16, more
 * than 16 planes; var, slot, out, p or n_factors out of range; a slot other than 0 with SX_REDUCE_STATE; p < 0 on a tile with a
 * gridpoint at r == 0.
 * Sums are accumulated in double-double, each by a fixed lane in a fixed order that depends on the grid and the program alone (no
 * floating-point atomics): two calls on the same data agree bitwise, and the rounding error does not grow with the point count.
 * sx_reduce runs on the handle's stream and returns after the copy-out; it reads only: `physical`, var_np1, the tendency history, A, B
 * and captured graphs stay as they are, and it does not run the tile transform itself. */
enum { SX_REDUCE_DOMAIN = 0, SX_REDUCE_AZIMUTH = 1 };
enum { SX_REDUCE_PHYSICAL = 0, SX_REDUCE_STATE = 1 };
/* terms[n_terms][11] = out, r_power, n_factors, var[4], slot[4] */
int sx_reduce(sx_handle *h, int32_t kind, int32_t source, int32_t n_terms, const double *coef,
              const int32_t *terms, int32_t n_out, double *out);
/* pure host helpers, no handle and no device (the pattern of sx_eval_basis) */
/* the weights above for the tile the descriptor selects; any output pointer may be NULL, w_z is untouched without a vertical */
int sx_reduce_weights(const sx_grid_desc *grid, double *w_r /*[3 tile_num_cells]*/,
                      double *w_l /*[3 tile_num_cells]*/, double *w_z /*[zDim]*/);
/* the validator sx_reduce itself calls: refuses what sx_reduce refuses of a program, and returns the distinct (var, slot) planes it
 * names in first-use order (n_factors = 0 names none); planes / n_planes may be NULL and are written on success only */
int sx_reduce_planes(const sx_grid_desc *grid, int32_t source, int32_t n_terms, const int32_t *terms,
                     int32_t n_out, int32_t *planes /*[16][2]*/, int32_t *n_planes);

/* --- extrema of field programs, refined to sub-grid accuracy -----------------------------------------------------------
 * How strong is the vortex and where is it: the extrema of a field program over the gridpoints with their locations (sx_extrema), and
 * the refinement of a gridpoint extremum to the stationary point of the continuous spectral function (sx_extremum_refine).
 *
 * sx_extrema.  Program and source are exactly those of sx_reduce (the same terms[n_terms][11], the same limits, SX_REDUCE_PHYSICAL /
 * SX_REDUCE_STATE, validated by sx_reduce_planes itself: whatever sx_reduce refuses is refused here, before anything is written).
 * Output o at a gridpoint is q_o = sum of its terms coef r^p prod field, in plain fp64 in term order starting from +0.0 (nothing is
 * summed across points); with storage_f32 the derivative slots are read in the type they are stored in.
 * SX_EXT_DOMAIN: val[2, n_out], idx[2, n_out] column-major, row 0 the minimum and row 1 the maximum over this tile's gridpoints.
 * SX_EXT_AZIMUTH: val[2, tile ring, level, n_out] and idx of the same shape, the ring faster than the level as in sx_reduce: minimum and
 * maximum over lambda at every ring and level (R / RZ grids: the pointwise value and its own index).
 * idx is the 0-based row of sx_get_gridpoints: pt = (first[ring] + l) * zDim + z.
 * Order.  Candidates are compared as (value, index): ties go to the lowest point index, -0.0 == +0.0 is a tie (val is the value AT idx, up to the sign of a zero: an output starts from +0.0, so -0.0 comes back as +0.0),
 * and a NaN comes before every number: if the integrand is NaN at any point of a set, both results of that set are NaN with idx the
 * lowest NaN point (Julia's findmax).  This order is total, so folding with it is associative and commutative: the result is unique,
 * not merely repeatable - it cannot depend on the launch shape, the ring pieces or the workgroup count.  No atomics.
 * Runs on the handle's stream and returns after the copy-out; reads only: `physical`, var_np1, the tendency history, A, B, parcels and
 * captured graphs stay as they are, and it does not run the tile transform.  sx_kernel_bytes("k_extrema") gives the planes named x
 * n_points x their element size of the last call.
 *
 * sx_extremum_refine finds, for the value slot of variable var (1-based), the stationary point of u(r, lambda, z) nearest to each of
 * the n start points start[n, n_coord] (column-major, the coordinates of sx_get_gridpoints) by a safeguarded Newton iteration that
 * runs inside ONE kernel launch (k_refine), one workgroup per point.  u and its 9 derivatives of order <= 2 (the mixed ones included)
 * are summed from the A coefficients the handle holds now with the SX_EVAL_ALL_K truncation (smooth in r, as for the parcels) and
 * sx_evaluate's vertical series and boundary-condition projection.  Lane count and reduction order are those of k_parcels, chosen from
 * the grid alone: a point's result is bitwise independent of the other points of the call.  lambda of a start within [-2 pi, 2 pi] (every
 * gridpoint's) is used as given, so a frozen lambda comes back bitwise; outside, it is reduced into (-pi, pi] in extended precision on the
 * host; a lambda that moves is kept in (-pi, pi].  Every iteration evaluates the derivatives at the position and takes the step of sx_newton_step;
 * after the last step one more evaluation is made, so that value[n] and grad[n, n_coord] (u_r[, u_lambda][, u_z], native coordinates,
 * as the r, l, z slots of sx_evaluate) are those AT pos[n, n_coord].  iters[n] counts the steps taken.
 * free_mask names the coordinates that move; a frozen coordinate keeps its start value (freeze z when the gridpoint extremum sits on
 * the top or bottom level, freeze lambda for the radius of maximum wind along a ray).  free_mask == 0 evaluates value and gradient at
 * the starts: status 0, iters 0.  tol <= 0 selects 1e-9, max_iter <= 0 selects 20.
 * status:  0 converged, pos = the stationary point;  1 the step left the tile radially, 2 vertically: pos = the last inside position;
 *   3 inside the pole zone (r < 1e-6 DX on an RL / RLZ tile whose first cell starts at xmin == 0, with r and lambda free): pos as it
 *   is - the Cartesian transform divides by r and has no accuracy left there, and stopping bounds the error at 1e-6 DX, which is where
 *   an axisymmetric vortex centred on the pole ends; a start at r == 0 returns 3 at once;  4 the reduced Hessian is not definite in
 *   the sense `want` asks for (SX_EXT_MAX: every pivot of its L D L^T < 0; SX_EXT_MIN: > 0; SX_EXT_ANY: finite and non-zero), or the
 *   step is not finite: no step is taken, pos = the current position;  5 max_iter steps taken: pos = the last position.
 * Refused, with a message and before anything is written: a null pointer with n > 0; var out of range; want not in {-1, 0, 1}; a
 * free_mask bit for a coordinate the geometry lacks (or an unknown bit); a NaN / Inf or out-of-range start (as sx_evaluate); a
 * non-finite tol; a handle that is not a one-tile patch; a grid whose weights do not fit the 64 KB of LDS of one workgroup:
 * 2 (kDim + 1) + zDim + 3 b_zDim + 48 > 8192 doubles.
 * Reads A only (a deferred diagnostic variable is brought up to date first, as for every reader of A): `physical`, var_np1, the
 * tendency history, the B arrays, parcels and captured graphs stay bitwise as they are.  sx_kernel_bytes("k_refine") gives the A bytes of
 * the last call: 4 node rows x the variable's columns (the padding block left out) x evaluations (steps + 1), summed over the points.
 *
 * sx_newton_step is lane 0's arithmetic on the host (pure helper, no handle and no device; the same function compiled for both): from
 * pos[n_coord] and d[10] = u, u_r, u_l, u_z, u_rr, u_rl, u_rz, u_ll, u_lz, u_zz (entries of a coordinate the geometry lacks: 0) it
 * forms the step and the decision; *status = -1 means "took a step, go on".
 *   Coordinates: the free native ones, except that on RL / RLZ with r and lambda both free the (r, lambda) block is transformed to
 *   Cartesian (X, Y) by the chain rule - u_X = u_r c - u_l s / r, u_XX = c^2 u_rr - 2 s c a + s^2 b, u_YY = s^2 u_rr + 2 s c a + c^2 b,
 *   u_XY = s c (u_rr - b) + (c^2 - s^2) a with a = u_rl / r - u_l / r^2, b = u_r / r + u_ll / r^2, u_Xz = u_rz c - u_lz s / r and the Y
 *   counterparts - and the step is taken in (X, Y[, z]), so the centre is an ordinary point; afterwards r = hypot, lambda = atan2
 *   kept in (-pi, pi], 0 at r == 0.  Rows and columns of frozen coordinates are deleted, the <= 3 x 3 system H step = -grad is solved
 *   by L D L^T without pivoting, and the pivots decide the definiteness.
 *   Safeguards: the whole step is scaled by ONE factor so that its horizontal length (hypot(dX, dY), |dr|, or r |dlambda| when only
 *   lambda is free) is <= DX and |dz| <= (zmax - zmin) / 8.  Converged (status 0, new_pos = the position after the step): horizontal
 *   length <= tol DX and |dz| <= tol (zmax - zmin).  Leaving (1, 2; radially wins) and the other stops return new_pos = pos.
 * Refused: a null pointer; what every host helper refuses of a descriptor; want, free_mask, tol as above; a NaN / Inf or out-of-range
 * pos. */
enum { SX_EXT_DOMAIN = 0, SX_EXT_AZIMUTH = 1 };
enum { SX_EXT_MIN = -1, SX_EXT_ANY = 0, SX_EXT_MAX = 1 };
enum { SX_EXT_FREE_R = 1, SX_EXT_FREE_L = 2, SX_EXT_FREE_Z = 4 };
int sx_extrema(sx_handle *h, int32_t kind, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms,
               int32_t n_out, double *val, int64_t *idx);
int sx_extremum_refine(sx_handle *h, int32_t var, int32_t want, int32_t free_mask, double tol, int32_t max_iter,
                       int64_t n, const double *start /*[n, n_coord]*/, double *pos /*[n, n_coord]*/, double *value /*[n]*/,
                       double *grad /*[n, n_coord]*/, int32_t *status /*[n]*/, int32_t *iters /*[n]*/);
int sx_newton_step(const sx_grid_desc *grid, int32_t want, int32_t free_mask, double tol, const double *pos /*[n_coord]*/,
                   const double *d /*[10]*/, double *new_pos /*[n_coord]*/, int32_t *status);

/* --- level crossings of field programs along rays: wind radii -----------------------------------------------------------
 * How large is the vortex: the radii at which a field program crosses given levels along rays (the radius of gale-force wind per
 * azimuth, the radius of a height or vorticity contour).
 * Program: exactly sx_reduce's (the same terms[n_terms][11], coef and limits, validated by sx_reduce_planes itself with the slot rules of
 * SX_REDUCE_PHYSICAL) with ONE output: every term's out is 0.  A ray q is (lambda_q, z_q): rays[n_rays, n_coord - 1] column-major; a grid
 * without an azimuth has no lambda, one without a vertical no z; an R grid has no ray coordinate at all (rays is not read, every ray is
 * the one ray).  On ray q
 *     g_q(r) = sum_t coef[t] r^p_t prod_f field(var_f, slot_f)(r, lambda_q, z_q)
 * in plain fp64, in term order, starting from +0.0 (as sx_extrema forms it), every field the CONTINUOUS spectral function of sx_evaluate
 * with the SX_EVAL_ALL_K truncation (smooth in r, as for the parcels and sx_extremum_refine) and sx_evaluate's vertical series and
 * boundary-condition projection, summed from the A coefficients the handle holds now.  For each of the n_levels <= 8 levels c_j the
 * call returns the radii where d = g_q(r) - c_j changes sign, ordered outward.
 * Stage 1, k_ray_profiles.  Along a ray the sums over lambda and z do not depend on r, so a field on a ray is a cubic spline in r with
 * the coefficients P[m] = sum_blk sum_zm A[zm, blk, m] F_blk^(sl)(lambda_q) Wz^(sz)[zm](z_q), m over the tile's num_cells + 3 patch
 * rows: the ray's profile.  Slots u, r, rr share the profile (sl, sz) = (0, 0) and differ in phi, phi', phi''; l, ll take F', F''; z, zz
 * the vertical rows 1, 2: at most 16 profiles, numbered in the order the program first names them.  Per variable the profiles of all
 * rays are ONE matrix product [rows x columns] [columns x rays] on the f64 matrix cores; the ray weights are formed on the device with
 * k_parcels' arithmetic (a lambda within [-2 pi, 2 pi] is used as given; outside, it is reduced into (-pi, pi] in extended precision on
 * the host).  The order of the sum over the columns depends on the grid alone, and ray tiles are padded with zero weights: a ray's
 * profile is bitwise independent of the other rays of the call and of their number.
 * Stage 2, k_crossings, one wave per ray.  Stations: the tile's inner end, its 3 tile_num_cells radial gridpoints (the doubles
 * sx_get_gridpoints returns) and its outer end, n_st = 3 tile_num_cells + 2, taken by the lanes in chunks of 64.  g at a radius is, per
 * plane, the 4-node spline sum of the profile with the weights phi, phi' / DX, phi'' / DX^2 of sx_eval_basis formed in plain fp64
 * from delta = (r - x_node) / DX, then the program.  With neg(d) = (d < 0), the interval [s_i, s_i+1] holds a crossing when
 * neg(d_i) != neg(d_i+1) and neither value is NaN: an exact zero counts as non-negative, so a root exactly on a station is counted
 * once.  dir is +1 where d rises outward and -1 where it falls.  An interval with a NaN end holds no crossing and sets bit 0 of the
 * ray's status.  LIMIT: two sign changes inside one station interval are not seen.
 * Refinement, one lane per crossing: a bracketed iteration on d from the profiles that always keeps the sign change between its inner
 * end a and outer end b - false position through (a, ga), (b, gb), where an end that stays twice in a row has its g halved (Illinois); the
 * trial point is the midpoint a + (b - a) / 2 instead when the false position is not strictly inside, or when the step before did not
 * halve the bracket.  It stops when b - a <= tol DX, when d == 0 exactly at an end or at a trial point, or after max_iter steps (bit 1
 * of status; a NaN at a trial point: bit 2), and returns the end with the smaller |d|, the inner one on a tie.  tol <= 0 selects 1e-9,
 * max_iter <= 0 selects 60.
 * Results, column-major: radius[max_cross, n_levels, n_rays] and dir of the same shape hold the first max_cross crossings outward, unused
 * entries NaN and 0; count[n_levels, n_rays] is the number of crossings FOUND and may exceed max_cross; status[n_rays]; profiles (may be
 * NULL) [num_cells + 3, n_profiles, n_rays].  No atomics and nothing is summed across rays: the result for a ray and a level is bitwise
 * independent of the other rays and levels of the call and of the launch shape.
 * Refused, with a message and before anything is written: a null pointer with a non-zero count; whatever sx_reduce_planes refuses;
 * a term whose out is not 0; n_levels outside [1, 8]; max_cross outside [1, 16]; a NaN / Inf ray coordinate or level, or a z out of
 * range; a non-finite tol; more than 2^20 rays; a negative r_power on an RL / RLZ tile whose first station is r == 0; a handle that is
 * not a one-tile patch; a grid whose ray weights do not fit the 64 KB of LDS of one workgroup:
 * 32 (kDim + 1) + 48 b_zDim + 16 zDim + 576 > 8192 doubles (no azimuth: without the first term; no vertical: b_zDim = 1, zDim = 0).
 * n_rays == 0 succeeds and writes nothing.
 * Runs on the handle's stream and returns after the copy-out; reads A only (a deferred diagnostic variable is brought up to date first,
 * as for every reader of A): `physical`, var_np1, the tendency history, the B arrays, parcels and captured graphs stay bitwise as they
 * are.  sx_kernel_bytes("k_ray_profiles") gives the A columns of the variables named and the ray coordinates in + the profiles out of
 * the last call, sx_kernel_bytes("k_crossings") the profiles in + the results out.
 *
 * sx_bracket_step is one step of that refinement on the host (pure helper, no handle and no device; the same function compiled for
 * both).  state[7] = a, d(a), b, d(b), ga, gb, x and flags[2] = the end the last step replaced (-1 inner, +1 outer, 0 none), whether
 * the next trial is a bisection; both are read and written.  first != 0: state[0..3] holds a station interval; the helper sets
 * the rest and, unless the bracket is finished already, the first trial point x (fx is ignored).  first == 0: fx = d(x) enters.
 * *status: 0 finished, -1 evaluate d at x and call again, 2 fx is NaN (the bracket stays).  width_tol is tol DX.  The result is a when
 * |d(a)| <= |d(b)|, else b.  Refused: a null pointer; a non-finite width_tol; a bracket that is not finite with a <= b or over which d
 * does not change sign; a trial point outside the bracket. */
int sx_crossings(sx_handle *h, int32_t n_terms, const double *coef, const int32_t *terms, int64_t n_rays,
                 const double *rays /*[n_rays, n_coord - 1]*/, int32_t n_levels, const double *levels, double tol, int32_t max_iter,
                 int32_t max_cross, double *radius /*[max_cross, n_levels, n_rays]*/, int32_t *dir /*same shape*/,
                 int32_t *count /*[n_levels, n_rays]*/, int32_t *status /*[n_rays]*/, double *profiles /*may be NULL*/);
int sx_bracket_step(double *state /*[7]*/, int32_t *flags /*[2]*/, int32_t first, double fx, double width_tol, int32_t *status);

/* --- isosurfaces of field programs in columns: heights, fields on them ---------------------------------------------------
 * At what height, and what is there: the heights at which a field program reaches given values in columns (the freezing level, the
 * top of the inflow layer, a cloud top, an isentropic surface) and other outputs of the program evaluated on that surface.  RZ and
 * RLZ grids; the transpose of sx_crossings.
 * Program: exactly sx_reduce's (the same terms[n_terms][11], coef and limits, validated by sx_reduce_planes itself with the slot rules
 * of SX_REDUCE_PHYSICAL) with 1 + n_carry outputs, 0 <= n_carry <= 8: output 0 is the surface quantity g, outputs 1 .. n_carry are
 * carried.  Every output is formed in plain fp64, in term order, starting from +0.0.  Column c is (r_c) on RZ and (r_c, lambda_c) on
 * RLZ: columns[n_cols, n_coord - 1] column-major.  Every field is the CONTINUOUS spectral function of sx_evaluate with the
 * SX_EVAL_ALL_K truncation, summed from the A coefficients the handle holds now.  For each of the n_levels <= 8 levels c_j the call
 * returns the heights where d = g(z) - c_j changes sign, ordered upward.
 * Stage 1, k_column_profiles.  In a column the sums over the radial nodes and over lambda do not depend on z, so a field in a column
 * is a Chebyshev series in z.  For the profile kind (var, sr, sl), sr the radial and sl the azimuthal derivative order,
 *     C[zm] = sum_blk sum_{node = cell .. cell + 3} A[zm, blk, node] phi_node^(sr)(r_c) / DX^sr F_blk^(sl)(lambda_c),   zm < b_zDim,
 * cell the radial cell of r_c.  Slots u, z, zz share (0, 0); r and rr take sr = 1, 2; l and ll take sl = 1, 2: at most 16 kinds per
 * program, numbered in the order the program first names them (sx_isosurface_check returns the count).  The weights are formed on the
 * device from the column coordinates with k_parcels' arithmetic: phi in plain fp64 from delta = (r - x_node) / DX, cos / sin of k lambda
 * (a lambda within [-2 pi, 2 pi] is used as given; outside, it is reduced into (-pi, pi] in extended precision on the host).  The host
 * sorts the columns by radial cell and cuts each cell's columns into batches of at most 16.  RLZ: per variable and batch the profiles
 * are ONE product on the f64 matrix cores, z-modes x columns over K = (block, node); the K order is block 0, 2, 3, ... (the padding
 * block 1 is never read), node 0 .. 3 within a block, whatever the columns are, and a short batch is padded with zero weights.  RZ: K
 * is the 4 nodes, one lane per output, the same sum.  A column's profile is bitwise independent of the other columns of the call, of
 * their number and of their order.
 * Series.  The full series of a profile is a = CA C (zDim coefficients), CA the projection of the variable's (bcb, bct) class that
 * sx_evaluate and k_parcels use, rounded to fp64 once; a' = Dc a and a'' = Dc a' are its derivatives, Dc the coefficient-space d/dz
 * rounded to fp64 once.  Every entry of the three is summed in index order from +0.0, product then sum, no fused multiply-add.  A field
 * at height z is s(z) = sum_n a_n t_n(x), x = (z - mid) / (-Lz / 2) clamped to [-1, 1], t_0 = 1, t_n = 2 T_n, t_{zDim-1} = T_{zDim-1}; the
 * z and zz slots use a' and a''.  T_n is formed by the RECURRENCE T_0 = 1, T_1 = x, T_{n+1} = 2 x T_n - T_{n-1}, and s is summed for
 * n ascending from a_0, product then sum, no fused multiply-add: this is the definition (it is not k_parcels' c_n cos(n acos x), whose
 * rounding differs).  It is ONE function compiled for host and device: the kernel uses it at stations, at trial points and for the
 * carried outputs, and sx_column_series runs it on the host: out[3] = s, and the same function on a' and a'' formed as above.
 * Stage 2, k_isosurface, one wave per column.  Stations: the zDim levels, bottom to top (the doubles sx_get_gridpoints returns; the
 * ends are stations), taken by the lanes in chunks of 64.  values (may be NULL) [zDim, n_cols] receives g at the stations exactly as
 * the kernel formed it.  Sign rule, NaN rule (bit 0 of the column's status), numbering, refinement and the returned end are
 * sx_crossings': with neg(d) = (d < 0) the interval [s_i, s_i+1] holds a crossing when neg(d_i) != neg(d_i+1) and neither is NaN, so a
 * root exactly on a station is counted once; dir is +1 where d rises upward; each crossing is refined by its own lane with the bracket
 * iteration of sx_bracket_step until b - a <= width_tol = tol (zmax - zmin), d == 0 exactly, or max_iter steps (bit 1; a NaN at a trial
 * point: bit 2).  tol <= 0 selects 1e-9, max_iter <= 0 selects 60.  The carried outputs are evaluated at the returned height.
 * LIMIT: two sign changes inside one station interval are not seen.
 * Results, column-major: height[max_cross, n_levels, n_cols] and dir of the same shape hold the first max_cross crossings upward,
 * carry[n_carry, max_cross, n_levels, n_cols] the carried outputs there; unused entries are NaN (height, carry) and 0 (dir).
 * count[n_levels, n_cols] is the number of crossings FOUND and may exceed max_cross; status[n_cols]; profiles (may be NULL)
 * [b_zDim, n_profiles, n_cols].  carry is NULL if and only if n_carry == 0.
 * Guarantees.  No atomics, and nothing is summed across columns.  The result for a column and a level is bitwise independent of the
 * other columns of the call, of their number and order, of the other levels, of n_carry, of whether values / profiles are asked for,
 * and of the launch shape.  Reads A only (a deferred diagnostic variable is brought up to date first, as for every reader of A):
 * `physical`, var_np1, the tendency history, the B arrays, parcels, statistics and captured graphs stay bitwise as they are.
 * Refused, with a message and before anything is written: a null pointer with a non-zero count; whatever sx_reduce_planes refuses; a
 * term whose out is above n_carry; n_carry outside [0, 8]; n_levels outside [1, 8]; max_cross outside [1, 16]; a grid without a
 * vertical (R, RL); a NaN / Inf coordinate or level; an r outside the tile's ends; a non-finite tol; more than 2^20 columns; a
 * negative r_power with a column at r == 0; a handle that is not a one-tile patch; a grid whose per-workgroup tables pass the 64 KB
 * of LDS: k_column_profiles needs 32 (kDim + 1) + 2304 <= 8192 doubles (RLZ: cos / sin of 16 columns and the staged tile of A),
 * k_isosurface (planes named + 2) zDim <= 8192 doubles.  n_cols == 0 succeeds and writes nothing.
 * Runs on the handle's stream and returns after the copy-out.  sx_kernel_bytes("k_column_profiles") gives the live A elements of the
 * 4 node rows once per batch and variable (RZ: per column and profile) and the column coordinates in + the profiles out of the last
 * call, sx_kernel_bytes("k_isosurface") the profiles in + heights, directions, carried outputs, counts, status and station values out.
 *
 * sx_isosurface_check validates the grid and the program on the host (pure helper, no handle and no device: every refusal above that
 * needs neither the columns nor the handle) and returns the number of profiles. */
int sx_isosurface(sx_handle *h, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_carry, int64_t n_cols,
                  const double *columns /*[n_cols, n_coord - 1]: r (RZ); r, lambda (RLZ)*/, int32_t n_levels, const double *levels,
                  double tol, int32_t max_iter, int32_t max_cross, double *height /*[max_cross, n_levels, n_cols]*/,
                  int32_t *dir /*same shape*/, int32_t *count /*[n_levels, n_cols]*/, int32_t *status /*[n_cols]*/,
                  double *carry /*[n_carry, max_cross, n_levels, n_cols]; NULL iff n_carry == 0*/, double *values /*[zDim, n_cols], may be NULL*/,
                  double *profiles /*[b_zDim, n_profiles, n_cols], may be NULL*/);
int sx_column_series(int32_t zDim, double zmin, double zmax, const double *a /*[zDim]*/, double z, double *out /*[3]*/);
int sx_isosurface_check(const sx_grid_desc *grid, int32_t n_terms, const int32_t *terms, int32_t n_carry, int32_t *n_profiles);

/* --- histograms of field programs: CFADs, areas, quantiles -------------------------------------------------------------
 * How much of the domain holds which values: the area inside an isotach, integrated kinetic energy above thresholds, contoured
 * frequency-by-altitude diagrams, percentiles - without pulling `physical` to the host.
 * Program and source are exactly those of sx_reduce (the same terms[n_terms][11] and coef, SX_REDUCE_PHYSICAL / SX_REDUCE_STATE with
 * their slot rules, validated by sx_reduce_planes itself; with storage_f32 the derivative slots are read in the type they are stored
 * in), with 1 <= n_out <= 4:
 *   output 0 is the binned quantity q, formed per gridpoint as sx_extrema forms an output: plain fp64, term order, from +0.0 - a host
 *     twin in float64 reproduces every point's slot exactly;
 *   outputs 1 .. n_out - 1 are integrands g_j: per point every term is multiplied by the point's weight without a rounding of the
 *     product (fma) and added in double-double, as in sx_reduce: the roundings of a sum are sx_reduce's;
 *   sums[:, 0, :] is the measure: the sum of the weights themselves.
 * Slots.  n_bins + 3 per group, 1 <= n_bins <= 64, edges[n_bins + 1] finite and strictly increasing: slot 0 underflow (q < edges[0],
 * -inf included), slot 1 + b holds edges[b] <= q < edges[b + 1], slot n_bins + 1 overflow (q >= edges[n_bins], +inf included), slot
 * n_bins + 2 holds NaN.  The slot is the number of edges <= q, found by bisection with exact fp64 comparisons - never by arithmetic on
 * (q - e0) / width; -0.0 compares equal to 0.0.  sx_distribution_slot is that rule on the host (pure helper, no handle and no
 * device; the same function compiled for both).
 * Kind.  SX_DIST_DOMAIN: one group, weight w_r w_l w_z of sx_reduce_weights: this tile's share of the patch distribution (tiles
 * add).  SX_DIST_LEVEL: one group per level, weight w_r w_l, the horizontal area on each level: the CFAD; on a grid without a
 * vertical it has one group and equals SX_DIST_DOMAIN.
 * count[n_bins + 3, groups] (column-major, the slot fastest) is the number of gridpoints per slot; sums[n_bins + 3, n_out, groups] the
 * measure and the integrals over the points of each slot.  An empty slot returns exactly 0 and +0.0.
 * Determinism.  count is exact.  sums use no floating-point atomics: each is accumulated in double-double in an order that depends on
 * the grid, n_bins and the slots the data falls into alone (a fixed lane tree per wave and slot, the waves of a workgroup in wave
 * order, a fixed number of workgroups in block order): two calls on the same data agree bitwise.
 * Refused, with a message and before anything is written: a null pointer with a non-zero count; whatever sx_reduce_planes refuses;
 * n_out outside [1, 4]; n_bins outside [1, 64]; an edge that is NaN / Inf or not strictly above its predecessor; an unknown kind;
 * SX_DIST_LEVEL where the bins of every level do not fit the LDS of one workgroup:
 *     zDim (n_bins + 3) (16 n_out + 4) + 8 (n_bins + 1) > 163840 bytes (the 160 KB of one compute unit)
 * (64 levels x 64 bins with one integrand fit, 64 levels x 40 bins with three do not).  sx_distribution_check refuses the
 * same on the host (pure helper, no handle and no device).
 * sx_distribution runs on the handle's stream and returns after the copy-out; it reads only: `physical`, var_np1, the tendency
 * history, A, B, parcels and captured graphs stay as they are, and it does not run the tile transform.  Multi-tile handles are allowed.
 * sx_kernel_bytes("k_distribution") gives the planes named x n_points x their element size of the last call. */
enum { SX_DIST_DOMAIN = 0, SX_DIST_LEVEL = 1 };
int sx_distribution(sx_handle *h, int32_t kind, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_out,
                    int32_t n_bins, const double *edges /*[n_bins + 1]*/, int64_t *count /*[n_bins + 3, groups]*/,
                    double *sums /*[n_bins + 3, n_out, groups]*/);
int sx_distribution_slot(int32_t n_bins, const double *edges /*[n_bins + 1]*/, double q, int32_t *slot);
int sx_distribution_check(const sx_grid_desc *grid, int32_t kind, int32_t source, int32_t n_terms, const int32_t *terms, int32_t n_out,
                          int32_t n_bins, const double *edges /*[n_bins + 1]*/);

/* --- vortex-centred azimuthal harmonics and wind profiles ---------------------------------------------------------------
 * Every other azimuthal diagnostic is taken about the grid's centre; a vortex that has drifted from it mixes its symmetric part with a
 * spurious wave 1 there.  sx_vortex_harmonics takes the harmonics about a given centre (sx_extremum_refine finds one).  RL and RLZ
 * grids, one-tile patches.
 * centre = (x0, y0) in the Cartesian frame x = r cos lambda, y = r sin lambda; radii[n_rho] >= 0 measured from the centre; heights[n_z]
 * (a grid without a vertical: NULL and 0, as for sx_harmonics); n_az samples per circle at phi_j = 2 pi j / n_az:
 *     x_j = x0 + rho cos phi_j,  y_j = y0 + rho sin phi_j,  r_j = hypot(x_j, y_j),  lambda_j = atan2(y_j, x_j) in (-pi, pi], 0 at r == 0
 * (the rules of the parcels).  The state is summed from the A coefficients the handle holds now with the SX_EVAL_ALL_K truncation
 * (smooth in r) and sx_evaluate's vertical series, boundary-condition classes and clamped radial cell, value slot only, and
 *     c_k(rho_i, z_l) = (1 / n_az) sum_j f(x_j, y_j, z_l) e^{-i k phi_j},   k = 0 .. kmax,
 * in the convention of sx_harmonics: f = Re sum_k eps_k c_k e^{i k phi}, eps_0 = 1, eps_k = 2.
 * fields[n_fields][3] = kind, var_a, var_b (1-based), n_fields <= 8:
 *   SX_VORTEX_SCALAR  one output, the value of var_a (var_b is ignored);
 *   SX_VORTEX_WIND    (var_a, var_b) are the grid's radial and tangential wind (u, v); TWO outputs, the radial and the tangential wind
 *                     about the centre: rad_j + i tan_j = (u_j + i v_j) e^{i (lambda_j - phi_j)}.  With motion = (cx, cy) the storm
 *                     motion is subtracted, in closed form and from wave 1 alone: c_1 -= (cx - i cy) / 2 (radial), (cy + i cx) / 2
 *                     (tangential).
 * n_out = scalar fields + 2 wind fields, in field order, radial before tangential.  out[2 (kmax + 1), n_z, n_rho, n_out] column-major,
 * re / im interleaved.  status[n_rho]: 0 computed; 1 the circle leaves the tile's radial extent [lo, hi], decided on the host in
 * closed form: with d = hypot(x0, y0) and tol = 8 eps (d + rho + hi),  d + rho > hi + tol,  or  lo > 0 and |d - rho| < lo - tol  (a
 * circle tangent to the edge is inside; a sample an ulp beyond the edge is evaluated in the clamped last cell).  Such a circle gets no
 * workgroup and its outputs are NaN.
 * The Fourier sum commutes with the vertical product: k_vortex_rings accumulates sum_j e^{-i k phi_j} q_j g_v[j][zm] over the vertical
 * MODES (g_v: the sums over nodes and wavenumber blocks at sample j, one pass over 4 node rows of A for all distinct source variables
 * of the call; e^{-i k phi_j} from an n_az-entry table formed on the host in extended precision, indexed by (k j) mod n_az), and
 * k_vortex_finish applies the value rows of the vertical operator at the n_z heights once, to (kmax + 1) b_zDim numbers instead of
 * n_az n_z samples.  No atomics, fixed orders that depend on the grid and on (n_az, kmax, fields) alone: a circle's result is bitwise
 * the same alone, among other circles and in a second call, and an output's does not depend on the other fields of the call.
 * Refused, with a message and before anything is written: a NaN or Inf in centre, motion, radii or heights; a negative radius; a height
 * outside [zmin, zmax]; n_az < 4, not a multiple of 4, or > 4096; kmax < 0, 2 kmax >= n_az or kmax > 32; n_fields outside 1 .. 8; an
 * unknown kind; a variable index out of range; a null pointer with a non-zero count; an R or RZ grid; a handle that is not a one-tile
 * patch; accumulators that do not fit the 64 KB of LDS of one workgroup (n_acc = 1 per scalar, 4 per wind field; n_src = the distinct
 * variables named):  2 (kDim + 1) + 2 n_acc (kmax + 1) b_zDim + n_src b_zDim > 8192  or  4 (kmax + 1) b_zDim > 8192 doubles.
 * n_rho == 0 succeeds and writes nothing.
 * Runs on the handle's stream and returns after the copy-out; reads A only (a deferred diagnostic variable is brought up to date first,
 * as for every reader of A): `physical`, var_np1, the tendency history, the B arrays, parcels and captured graphs stay bitwise as they
 * are.  sx_kernel_bytes("k_vortex_rings") gives the A bytes of the last call, counted per sample point as k_parcels counts them: live
 * circles x n_az x distinct source variables x 4 rows x b_zDim x (2 kDim + 1) x 8.  Timers k_vortex_rings, k_vortex_finish.
 *
 * sx_vortex_check is the host statement of the same validation (everything above that a descriptor decides: not motion, not heights)
 * and of the circle rule: n_out and status[n_rho] as the call would return them.  Pure host helper (no handle, no device). */
enum { SX_VORTEX_SCALAR = 0, SX_VORTEX_WIND = 1 };
int sx_vortex_harmonics(sx_handle *h, const double centre[2], const double *motion /*[2] or NULL*/,
                        const double *radii, int32_t n_rho, const double *heights, int32_t n_z,
                        int32_t n_az, int32_t kmax, int32_t n_fields, const int32_t *fields /*[n_fields][3]*/,
                        double *out /*[2 (kmax + 1), n_z, n_rho, n_out] column-major, re / im interleaved*/,
                        int32_t *status /*[n_rho]*/);
int sx_vortex_check(const sx_grid_desc *grid, const double centre[2], const double *radii, int32_t n_rho,
                    int32_t n_az, int32_t kmax, int32_t n_fields, const int32_t *fields, int32_t *n_out, int32_t *status);

/* --- statistics of field programs over time: swaths, means, totals ------------------------------------------------------
 * Per-gridpoint accumulators that live with the handle and are updated on the device, one kernel (k_stats) per sample: the
 * maximum-wind swath (the largest wind speed each gridpoint has seen, and when), accumulated fields, time means and eddy covariances
 * over a window, the duration for which a point stayed above a threshold - without pulling `physical` or var_np1 to the host.
 * A statistics set is a program plus one operation per output.  The program is exactly sx_reduce's (the same terms[n_terms][11], coef
 * and limits, SX_REDUCE_PHYSICAL / SX_REDUCE_STATE with their slot rules, validated by sx_reduce_planes itself: whatever sx_reduce
 * refuses is refused here); op[o] belongs to output o < n_out <= 16.  The value of output o at a gridpoint is q_o as sx_extrema forms
 * it: plain fp64, the terms added in term order starting from +0.0, r^p formed as r, r r, 1 / r or 1 / (r r), the factors multiplied
 * in order; with storage_f32 the derivative slots are read in the type they are stored in.
 * A sample is one call sx_stats_accumulate(h, time, weight).  At every gridpoint of the tile and for every output it updates two
 * doubles, acc[o][2][N] on the device with the point fastest:
 *   SX_STAT_SUM       (hi, lo)       the double-double sum of weight q: the rounding error of the product is recovered with an fma
 *                                    (ph = w q, pl = fma(w, q, -ph)) and the pair is added with the two-sum of sx_reduce.  Skipped when
 *                                    weight == 0.
 *   SX_STAT_MAX / MIN (value, time)  the running extremum of q and the `time` of the sample that set it.  A later sample replaces the
 *                                    pair only when its q is strictly greater (MAX) / smaller (MIN): a tie, -0.0 == +0.0 included,
 *                                    keeps the earlier sample.  A NaN comes before every number (sx_extrema's order): once q is NaN
 *                                    at a point the pair stays (NaN, time of the first NaN sample).
 *   SX_STAT_DURATION  (hi, lo)       the double-double sum of weight over the samples with q >= threshold[o], an exact fp64
 *                                    comparison (a NaN q is not counted).  Skipped when weight == 0.
 * weight == 0 is the "extrema only" sample: it takes the initial state into a swath without giving it a time weight.  time and
 * weight must be finite; a negative weight is allowed.
 * The handle also counts the samples and keeps the double-double sum of the weights (elapsed) and the first and last time.
 * Empty.  Before the first sample SUM and DURATION pairs are (+0.0, +0.0) and MAX / MIN pairs are (NaN, NaN).  Every point gets every
 * sample, so one counter per set tells the two NaNs apart: samples == 0 means "empty"; with samples > 0 a NaN value means "q was NaN",
 * and its time is then a finite sample time.
 * Nothing is summed across points, there are no atomics: a point's result depends on that point's own sequence of (q, time, weight)
 * alone, bitwise, not on the launch shape, the other points, the other outputs of the set or the tiling of the patch.
 *
 * sx_stats_set validates, packs the program and allocates n_out x 2 x N doubles; all accumulators and counters start empty.  A new set
 * replaces an old one; n_out == 0 removes the set and frees its memory (the other arguments are then not read).  threshold[n_out] is
 * read for DURATION outputs only and may be NULL when there is none.
 * sx_stats_reset keeps the program and empties accumulators and counters (windowed means, hourly totals); without a set it does nothing.
 * sx_stats_accumulate enqueues ONE kernel on the handle's stream and returns: no allocation, no copy, no synchronisation, no transform.
 * It reads the planes the program names and reads and writes the accumulators only: `physical`, var_np1, the tendency history, A, the B
 * arrays, parcels and captured graphs stay bitwise as they are.  With SX_REDUCE_PHYSICAL the caller has run sx_tile_transform, exactly
 * as for sx_reduce.  It is no part of sx_step's captured graph.  Without a set the call succeeds and launches nothing.
 * sx_stats_get synchronises and copies out[N, n_out, 2] column-major (the point fastest, then the output, then the slot) and
 * info[5] = samples, elapsed hi, elapsed lo, first time, last time (the times NaN without a sample); info may be NULL.  In the copy
 * only, slot 0 of a SUM / DURATION output is hi + lo rounded once and slot 1 the stored lo; the stored pair stays a pair.
 * sx_stats_describe returns the attached set's source, n_out (0 without a set: nothing else is written), op[16] and threshold[16] (the
 * first n_out entries; a threshold is 0 where the op has none), so that a restart can be checked; any output pointer may be NULL.
 * sx_stats_get_state / sx_stats_set_state: program, ops, thresholds, counters and the raw accumulator pairs as an opaque blob of
 * sx_stats_state_size doubles (0 without a set); a run resumed from it continues bitwise.  A blob taken on a handle with another
 * number of gridpoints is refused.
 * Refused, with a message and before anything is written - an existing set, its accumulators and the out buffers stay as they are: a
 * null pointer with a non-zero count; whatever sx_reduce_planes refuses; an unknown op; a NaN / Inf threshold of a DURATION output; a
 * NaN / Inf time or weight; sx_stats_get or sx_stats_get_state without a set; an allocation that fails (the message names the bytes
 * asked for).  Multi-tile handles are allowed: tiles own disjoint points and each accumulates its own.
 * sx_kernel_bytes("k_stats") gives the bytes of the last sample: the planes named x N x their element size + n_out x N x 32 (every
 * pair read and written; the outputs a weight == 0 sample skips are counted all the same: an upper bound). */
enum { SX_STAT_SUM = 0, SX_STAT_MAX = 1, SX_STAT_MIN = 2, SX_STAT_DURATION = 3 };
int sx_stats_set(sx_handle *h, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_out,
                 const int32_t *op /*[n_out]*/, const double *threshold /*[n_out] or NULL*/);
int sx_stats_reset(sx_handle *h);
int sx_stats_accumulate(sx_handle *h, double time, double weight);
int sx_stats_get(sx_handle *h, double *out /*[N, n_out, 2] column-major*/, double *info /*[5] or NULL*/);
int sx_stats_describe(const sx_handle *h, int32_t *source, int32_t *n_out, int32_t *op /*[16]*/, double *threshold /*[16]*/);
int sx_stats_state_size(const sx_handle *h, int64_t *n_doubles);
int sx_stats_get_state(sx_handle *h, double *out);
int sx_stats_set_state(sx_handle *h, const double *in, int64_t n_doubles);

/* --- field programs projected onto the spectral basis: derived fields as variables --------------------------------------
 * What turns a program into a variable: sx_project evaluates a field program at the gridpoints of src on the device, writes output o
 * as the var_np1 plane of variable var_dst[o] (1-based) of the companion handle dst, and runs dst's own forward transform and banded
 * solve.  dst's variables are then spectral fields like any other - sx_evaluate, sx_harmonics, sx_spectrum, sx_vortex_harmonics,
 * sx_elliptic_solve (SX_ELL_FIELD), sx_antiderivative, sx_extremum_refine and sx_tile_transform apply to the vorticity, a flux, the
 * kinetic energy, the forcing of a balance equation.  The projection is the one the model applies to its own nonlinear tendencies:
 * the same quadrature, the boundary-condition classes of dst's variables, dst's l_q filter and dst's truncation; no new numerics.
 * Program and source are exactly those of sx_reduce (the same terms[n_terms][11], coef and limits, SX_REDUCE_PHYSICAL / SX_REDUCE_STATE
 * with their slot rules, validated by sx_reduce_planes itself).  The value of output o at a gridpoint is q_o as sx_extrema and
 * sx_stats_accumulate form it: plain fp64, the terms added in term order starting from +0.0, r^p formed as r, r r, 1 / r or 1 / (r r),
 * the factors multiplied in order; with storage_f32 the derivative slots are read in the type they are stored in.  A NaN or Inf is
 * written as it comes out.  A product of two fields holds wavenumbers and z-modes up to the sum of the factors': what lies beyond
 * dst's truncation aliases on the mish exactly as it does in the model's own tendencies.
 * One kernel (k_project: streaming, a lane per two consecutive points where N is even, one otherwise; no atomics, nothing across
 * lanes) on src's stream; dst's stream waits on an event recorded behind it and then runs launch_fl_forward, launch_sb, launch_solve
 * for every variable of dst - the launches behind sx_spectral_transform + sx_spline_transform.  No device-wide synchronisation; the
 * call returns after completion.  With SX_REDUCE_PHYSICAL the caller has run sx_tile_transform, as for sx_reduce; a deferred diagnostic
 * variable of src is brought up to date first.
 * Everything of src stays bitwise as it is: `physical`, var_np1, the tendency history, A, B, parcels, statistics, captured graphs.  In
 * dst var_np1, B and A of every variable are overwritten; dst's `physical` is not touched and is stale until sx_tile_transform.  Two
 * calls agree bitwise, and one output's coefficients do not depend on what the other outputs of the call are.
 * Refused, with a message and before anything is written: a null handle; a null coef, terms or var_dst with a non-zero count;
 * dst == src (the forward chain reads var_np1, which is the model's state); a src or dst that is not a one-tile patch; a dst that
 * differs from src in geometry, xmin, xmax, num_cells, ring table, zDim, zmin or zmax (b_zDim may differ: the projection truncates as
 * dst says; kDim follows from the ring table); n_out other than dst's number of variables; a var_dst that is not a permutation of
 * 1 .. n_out; a dst whose equation set is not SX_EQ_NONE; whatever sx_reduce_planes refuses; an output with no term (its plane would be
 * zero by accident, not by request).
 * sx_kernel_bytes("k_project") gives the planes named x N x their element size (8, 4 for an fp32-stored plane) + n_out x N x 8.
 *
 * sx_project_check is that validation for two descriptors, on the host (all but the null handles, dst == src and the equation set, which
 * a descriptor does not carry); sx_project calls it.  sx_project_point states the n_out outputs at ONE point on the host with the
 * kernel's arithmetic, packed and formed by the code the kernel uses: val[j] is the value of plane (planes[j][0], planes[j][1]) there
 * and r the point's radius; every plane a term names must be listed.  Pure host helpers (no handle, no device). */
int sx_project(sx_handle *src, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_out, sx_handle *dst,
               const int32_t *var_dst /*[n_out], 1-based, a permutation of 1 .. n_out*/);
int sx_project_check(const sx_grid_desc *src, const sx_grid_desc *dst, int32_t source, int32_t n_terms, const int32_t *terms, int32_t n_out,
                     const int32_t *var_dst);
int sx_project_point(int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_out, int32_t n_planes,
                     const int32_t *planes /*[n_planes][2]*/, const double *val /*[n_planes]*/, double r, double *out /*[n_out]*/);

/* --- function programs: nonlinear derived fields as variables (speed, potential vorticity, T, p, theta_e) ---------------
 * A field program is polynomial.  A FUNCTION program is a field program, whose n_mid <= 16 outputs are now called the mids, followed by
 * a list of n_ops <= 32 operations on a register file per gridpoint:
 *     registers 0 .. n_mid - 1   the mids at the point (q_o exactly as sx_project forms it)
 *     register  n_mid + i        the result of operation i, ops[i][4] = fn, a, b, c
 * An operand >= 0 is a register and must be lower than the operation's own register - the list is in evaluation order -; an operand
 * k < 0 is the constant consts[-1 - k], n_consts <= 16.  Operands an operation does not take are ignored.
 * Exactly rounded operations, one IEEE operation each (the library is built without contraction, so the host reproduces them bit
 * for bit):
 *     ADD a + b   SUB a - b   MUL a * b   DIV a / b   NEG -a   ABS |a|   SQRT sqrt(a)
 *     MIN, MAX    the smaller / larger of a and b; if a is NaN the result is a, else if b is NaN it is b (a NaN operand is
 *                 returned, never dropped); of two equal operands (-0.0 and +0.0 among them) the result is a
 *     SELECT      a >= 0 ? b : c; a NaN a takes c
 * Math-library operations (within the library's error of the rounded argument; host and device libraries differ in the last bits):
 *     EXP exp(a)   LOG log(a)   POW pow(a, b)   ATAN2 atan2(a, b)
 * Point data (no register operands):
 *     R           the point's first coordinate (the double sx_get_gridpoints returns)
 *     Z           the point's height; refused on R / RL grids
 *     REF         a = profile (0 sbar, 1 xibar, 2 mubar), b = slot (0 value, 1 d/dz, 2 d2/dz2), both literal: the entry of the
 *                 source handle's sx_model_desc.ref_state [3][3][zDim] at the point's level; refused when the source has none
 * Composites, which call the functions the equation-set kernels call (csrc/sx_thermo.hpp): a diagnosed temperature is bit for bit
 * the one Euler_test / rainfall_test step with
 *     AHYP ahyp(a)   DRY_DENSITY dry_density(a)   TEMPERATURE temperature(s = a, rho_d = b, q_v = c)   PRESSURE pressure(Tk = a, rho_d = b,
 *     q_v = c) [hPa]   VAPOR_PRESSURE vapor_pressure(p = a, q_v = b)   ESAT_BUCK sat_pressure_liquid_buck(Tk = a, p = b)   L_V L_v(Tk = a)
 * An argument outside a function's domain (the root of a negative, the logarithm of zero, a division by zero) gives the IEEE NaN / Inf
 * at that point and nowhere else; it is not refused.
 *
 * sx_derive evaluates the program at every gridpoint of src (k_derive: streaming, one lane per point, the planes the mids name loaded
 * once, the register file a column of LDS per lane, the operation list uniform across the wave; no atomics, nothing across lanes),
 * writes register reg_dst[v] as the var_np1 plane of variable v (0-based position) of the companion handle dst - a mid may be written
 * directly, a register may serve several variables, and dst has at most 48 variables, the size of the register file - and runs dst's
 * forward transform and banded solve.  Source, streams, the event between them, what is overwritten in dst and
 * what stays bitwise in src are exactly sx_project's, and so are the refusals of the handles and of the two grids.  Two calls agree
 * bitwise, and a register's value does not depend on what else the program computes.
 * Refused, with a message and before anything is written: a null handle; a null pointer with a non-zero count; dst == src; a dst with
 * an equation set; a src or dst that is not a one-tile patch, or grids that differ (sx_project); whatever sx_reduce_planes refuses of
 * the mids (n_mid in place of n_out); a mid with no term; n_ops > 32; n_consts > 16; an unknown fn; an operand that names the
 * operation's own or a later register, or a constant beyond n_consts; Z on a grid without a vertical; REF on a source without a
 * reference state, or with a profile or slot outside 0 .. 2; n_reg_dst other than dst's number of variables, or more than 48; a reg_dst outside
 * 0 .. n_mid + n_ops - 1.
 * sx_kernel_bytes("k_derive") gives the planes named x N x their element size (8, 4 for an fp32-stored plane) + dst n_vars x N x 8.
 *
 * sx_derive_check is that validation for two descriptors on the host (all but the null handles, dst == src and the equation set);
 * has_ref_state says whether the source carries a reference state, which a descriptor does not.  sx_derive_point states every
 * register at ONE point on the host, packed and formed by the code the kernel runs: val[j] is the value of plane (planes[j][0],
 * planes[j][1]) there, r and z the point's coordinates, ref[profile][slot] the reference state at its level (NULL: REF is refused;
 * Z is always allowed).  Pure host helpers (no handle, no device). */
enum { SX_FN_ADD = 0, SX_FN_SUB, SX_FN_MUL, SX_FN_DIV, SX_FN_NEG, SX_FN_ABS, SX_FN_MIN, SX_FN_MAX, SX_FN_SQRT, SX_FN_SELECT,
       SX_FN_EXP, SX_FN_LOG, SX_FN_POW, SX_FN_ATAN2, SX_FN_R, SX_FN_Z, SX_FN_REF, SX_FN_AHYP, SX_FN_TEMPERATURE, SX_FN_ESAT_BUCK,
       SX_FN_DRY_DENSITY, SX_FN_PRESSURE, SX_FN_VAPOR_PRESSURE, SX_FN_L_V, SX_FN_COUNT };
int sx_derive(sx_handle *src, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_mid,
              int32_t n_ops, const int32_t *ops /*[n_ops][4] = fn, a, b, c*/, int32_t n_consts, const double *consts,
              sx_handle *dst, const int32_t *reg_dst /*[dst n_vars]: the register each destination variable receives*/);
int sx_derive_check(const sx_grid_desc *src, int32_t has_ref_state, const sx_grid_desc *dst, int32_t source, int32_t n_terms,
                    const int32_t *terms, int32_t n_mid, int32_t n_ops, const int32_t *ops, int32_t n_consts, int32_t n_reg_dst,
                    const int32_t *reg_dst);
int sx_derive_point(int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_mid, int32_t n_ops, const int32_t *ops,
                    int32_t n_consts, const double *consts, int32_t n_planes, const int32_t *planes /*[n_planes][2]*/,
                    const double *val /*[n_planes]*/, double r, double z, const double *ref /*[3][3] or NULL*/,
                    double *regs /*[n_mid + n_ops]*/);

/* --- onto another grid: resize, re-level, re-centre -------------------------------------------------------------------
 * The restart-at-new-resolution and vortex-following primitive: sx_regrid lays the state of src down on the grid of dst.  It adds no
 * numerics of its own: the values are the continuous function sx_evaluate defines, the coefficients the projection
 * sx_spectral_transform + sx_spline_transform apply.
 *
 * Value.  Variable v (0-based) of dst receives, at every gridpoint of dst, the value slot of src's variable var_src[v] (1-based; the
 * same source variable may be named more than once): the function sx_evaluate returns with SX_EVAL_ALL_K - every wavenumber of the
 * patch at every radius -, summed on the device from the A coefficients src holds now (a deferred diagnostic variable is brought up to
 * date first).  It is written as dst's var_np1 plane, and dst's own forward chain - what sx_spectral_transform + sx_spline_transform
 * launch - then runs for every variable of dst, on dst's stream behind an event (as in sx_project).  The call returns after completion.
 *
 * What changes.  In dst: var_np1, B and A are overwritten; `physical` and the tendency history are stale - run sx_tile_transform
 * before reading `physical`, and the next sx_advance / sx_step of dst must be t = 1 (an Euler step: the Adams-Bashforth history belongs
 * to another grid).  dst may carry any equation set.  src stays bitwise as it is: state, history, `physical`, parcels, statistics.
 *
 * Geometry.  R -> R, RZ -> RZ, RL -> RL and RLZ -> RLZ only.  xmin, xmax, num_cells, the ring table, the boundary conditions and l_q of
 * the two grids are independent.  centre = (x0, y0) is the position of dst's axis in src's Cartesian frame (x = r cos lambda,
 * y = r sin lambda); it is allowed on RL / RLZ only, and NULL means (0, 0).  A column (r, lambda) of dst lies in src at
 *     x = x0 + r cos lambda,  y = y0 + r sin lambda,  r_s = hypot(x, y),  lambda_s = atan2(y, x)
 * in plain fp64, every operation rounded on its own; with centre NULL or exactly (0, 0) the map is the identity on (r, lambda), bit for
 * bit.  The map is one function compiled for host and device; sx_regrid_columns runs it on the host and returns the source coordinates
 * of every column of dst in dst's gridpoint order (a column is the zDim consecutive gridpoints of one (r, lambda)):
 * columns[n_cols, n_h] column-major, n_h = 1 (r_s; R / RZ) or 2 (r_s, lambda_s; RL / RLZ) - n_coord - 1 on a grid with a vertical -,
 * inside[n_cols], *n_cols the count; any of the three may be NULL (NULL columns and inside: the count alone).  sx_regrid sums at these
 * same doubles (a lambda_s beyond 2 pi in magnitude - the identity map of a native ring's last points - is reduced into (-pi, pi] in
 * extended precision before the kernel reads it, as sx_isosurface reduces it).
 *
 * Vertical.  dst's [zmin, zmax] must lie within src's; zDim, b_zDim, the level set and the vertical boundary-condition classes may all
 * differ.  The vertical row is sx_evaluate's: the DCT-I series of CA e_zm of the SOURCE variable's (bcb, bct) class at dst's levels,
 * formed in extended precision and rounded to fp64 once (the matrix E [zDim_dst][b_zDim_src], cached per level set of dst).
 *
 * Outside the source.  A column of dst is outside when its r_s lies outside src's [xmin, xmax] (the ends count as inside); inside[c] = 0
 * marks it.  outside = SX_REGRID_REFUSE fails the call before anything is written when there is such a column; SX_REGRID_FILL writes
 * fill[v] at every level of such a column and counts the columns in *n_outside (may be NULL; 0 with SX_REGRID_REFUSE).  fill [dst n_vars]
 * must then be non-null and finite; with SX_REGRID_REFUSE it is not read.
 *
 * Two stages.  Stage 1: the per-column series C[zm] of every source variable named - sx_isosurface's profiles of kind
 * (0, 0), by its kernels k_column_profiles / k_column_profiles_rz, the inside columns sorted by source cell and batched as there.  Stage
 * 2, k_regrid_levels: var_np1[z, column, v] = sum_zm E_v[z][zm] C_v[zm][column] on the f64 matrix cores (RLZ; 16 columns x 16 levels per
 * product, K = zm ascending in one fixed chain, zero-padded to 16 / 4) or one lane per output (R, RL, RZ: the fma chain over zm from
 * +0.0; without a vertical b_zDim = 1, E = (1) and the stage is a copy).  Which of the two runs follows from the geometry alone.  No
 * atomics, nothing summed across columns.  Guarantees: two calls agree bitwise; a column's values do not depend on the other columns of
 * dst; one variable's result does not depend on what the other entries of var_src are.
 *
 * Refused, with a message and before any write: null handles; dst == src; either handle not a one-tile patch; geometries that differ; a
 * centre on R / RZ; a non-finite centre; a null var_src or an entry outside 1 .. src n_vars; an unknown `outside`; more than 2^20 columns
 * of dst; an invalid vertical grid (4 <= zDim <= 256, b_zDim <= zDim, zmax > zmin, of both) or a dst extent beyond src's; the LDS limit
 * of k_column_profiles (32 (kDim + 1) + 2304 <= 8192 doubles, src's kDim); with SX_REGRID_REFUSE a column outside; with SX_REGRID_FILL a
 * null or non-finite fill.  sx_regrid_check is that validation for two descriptors on the host (all but the null handles, dst == src
 * and fill); sx_regrid calls the same code.  sx_regrid_check and sx_regrid_columns are pure host helpers (no handle, no device).
 * sx_kernel_bytes(src, "k_regrid_levels") gives the last call's profiles in (b_zDim x inside columns x 8 per variable of dst) + E + the
 * column table + dst's var_np1 planes out; "k_column_profiles" is not updated by sx_regrid. */
enum { SX_REGRID_REFUSE = 0, SX_REGRID_FILL = 1 };
int sx_regrid(sx_handle *src, sx_handle *dst, const double *centre /*[2] or NULL*/, const int32_t *var_src /*[dst n_vars], 1-based*/,
              int32_t outside, const double *fill /*[dst n_vars] or NULL*/, int64_t *n_outside /*may be NULL*/);
int sx_regrid_check(const sx_grid_desc *src, const sx_grid_desc *dst, const double *centre, const int32_t *var_src, int32_t outside);
int sx_regrid_columns(const sx_grid_desc *src, const sx_grid_desc *dst, const double *centre, double *columns /*[n_cols, n_h]*/,
                      int32_t *inside /*[n_cols]*/, int64_t *n_cols);

/* --- tile <-> patch exchange on the device (src/semiimplicit.jl:320-329, 272-285) ---------------------------------- */
/* The tile's B coefficients live in a [tile_b_rDim][n_cols] row-major device array (row = radial node).
 * Rows [0, tile_num_cells) are owned (patchIndexMap), rows [tile_num_cells, +3) are the halo sent to the next
 * tile (haloSendIndexMap); the last tile owns all its rows. */
int sx_tile_b_device(sx_handle *h, void **dev_ptr, int64_t *n_rows, int64_t *n_cols);
/* Make sx_spectral_transform / sx_advance write the tile's B rows at dev_ptr (e.g. inside an all-gather buffer). */
int sx_bind_tile_b(sx_handle *h, void *dev_ptr);
/* sharedSpectral[haloReceiveIndexMap] .+= haloReceiveBuffer (src/semiimplicit.jl:329): B rows 0..2 += recv[3][n_cols] */
int sx_halo_add(sx_handle *h, const void *dev_recv);
/* Source of the patch-level B for sx_spline_transform: row m of the patch is at dev_base + row_offset[m] doubles.
 * dev_base = NULL restores the internal buffer (filled by sx_set_patch_spectral_b or, for a one-tile patch,
 * by sx_spectral_transform). */
int sx_bind_patch_b(sx_handle *h, const void *dev_base, const int64_t *row_offset /* [b_rDim] host */);
/* device pointer of the patch A array [b_rDim][n_cols] */
int sx_patch_a_device(sx_handle *h, void **dev_ptr, int64_t *n_rows, int64_t *n_cols);

/* --- transposed (all-to-all) patch solve -----------------------------------------------------------------------------
 * Scalable alternative to halo + all-gather + redundant solve (src/semiimplicit.jl:320-329, 285) for n tiles = n GPUs.
 * The columns of the [node][col] arrays are split into n contiguous ranges of whole (variable, z-mode) groups
 * (sx_a2a_col_starts). Per step, after sx_advance:
 *   1. sx_a2a_pack_b      tile B rows -> send buffer [dest d][row j < tile_b_rDim][cols of d]
 *   2. all-to-all         every tile's rows for my columns arrive as [tile t][row j][my cols]
 *   3. sx_a2a_solve       sums the rows two tiles share (the reference's halo add), solves my columns for the whole
 *                         patch, writes the solution rows back in the same [tile t][row j][my cols] layout
 *   4. all-to-all         reverse direction
 *   5. sx_a2a_unpack_a    [owner d][row j][cols of d] -> the patch A rows this tile evaluates
 * tile_cell0 / tile_num_cells describe all n tiles (calcTileSizes rows 4 and 3, 0-based cell0). */
int sx_a2a_configure(sx_handle *h, int32_t n_tiles, int32_t my_tile, const int32_t *tile_cell0, const int32_t *tile_num_cells);
int sx_a2a_col_starts(sx_handle *h, int64_t *out /* [n_tiles + 1] */);
int sx_a2a_pack_b(sx_handle *h, void *dev_send);
int sx_a2a_solve(sx_handle *h, const void *dev_recv, void *dev_send);
int sx_a2a_unpack_a(sx_handle *h, const void *dev_recv);

/* --- interface-only (partitioned) patch solve ---------------------------------------------------------------------------
 * instead of the redundant whole-patch solve of src/semiimplicit.jl:285 every tile solves its OWN rows
 * (a chain of n / N rows) and only what couples tiles travels: per tile and column its 6 edge values and the <= 4 rows whose
 * coefficient another tile owns (the 3 halo rows of src/semiimplicit.jl:320-329, PERIODIC wrap rows) go to the owner of
 * the column's reduced system, 6 right-hand-side corrections and the <= 4 foreign coefficients come back.  Per step, after
 * sx_advance:
 *   1. sx_iface_local     tile-local banded solve of the tile's B rows; its 10 rows -> send buffer [dest d][10][cols of d]
 *   2. all-to-all         arrive as [tile t][10][my cols]
 *   3. sx_iface_reduce    one dense [10 N x 10 N] operator per boundary-condition class (built at configure) per column
 *   4. all-to-all         reverse direction
 *   5. sx_iface_apply     a = y' + Z c  ->  the patch A rows this tile evaluates
 * Column split and table arguments as for sx_a2a_*; needs >= 2 tiles with >= 6 free coefficients each. */
int sx_iface_configure(sx_handle *h, int32_t n_tiles, int32_t my_tile, const int32_t *tile_cell0, const int32_t *tile_num_cells);
int sx_iface_col_starts(sx_handle *h, int64_t *out /* [n_tiles + 1] */);
int sx_iface_local(sx_handle *h, void *dev_send);
int sx_iface_reduce(sx_handle *h, const void *dev_recv, void *dev_send);
int sx_iface_apply(sx_handle *h, const void *dev_recv);

/* --- exchange over RCCL, inside the library --------------------------------------------------------------------------
 * One process per GPU, one tile per process (src/semiimplicit.jl:179-184).  The reference's per-step exchange - the halo
 * chain tile -> tile + 1 (src/semiimplicit.jl:203-219, 320-329), the shared sum on the master (:272-282) and the patch solve
 * on every worker (:285) - runs here as ncclSend / ncclRecv / ncclAllGather on the handle's stream, ordered with the
 * kernels by that stream alone.  librccl is bound with dlopen on first use (SX_RCCL_LIB overrides the search; a copy the
 * process has already mapped is reused).  A Julia host needs only ccall:
 *   rank 0: sx_comm_unique_id(id) -> hand the 128 bytes to every worker (the master's RemoteChannels will do)
 *   all   : sx_comm_init(h, n_tiles, my_tile, cell0, ncells, mode, id)      (collective; after hipSetDevice / sx_create)
 *   step  : sx_advance(h, t); sx_exchange(h);                               (replaces :320-329, :272-285)
 * mode 0 = transposed solve (two all-to-alls of B / A rows, each rank solves its share of the columns for the whole
 * patch: scales), mode 1 = the reference's protocol (halo rows to the next tile, all-gather of the owned rows, redundant
 * patch solve), mode 2 = interface-only solve (tile-local solves, two all-to-alls of 10 rows per tile: least traffic and the
 * shortest recurrence; with one tile it is the plain solve).  tile_cell0 / tile_num_cells describe all n tiles (calcTileSizes rows 4 and 3, 0-based cell0).
 * sx_comm_attach does the same with a communicator the host already owns (ncclComm_t, e.g. from NCCL.jl); it is not
 * destroyed with the handle.  After sx_exchange the patch A coefficients this tile evaluates are in place for the next
 * sx_advance / sx_tile_transform.
 * sx_comm_prepare is the part of sx_comm_init / sx_comm_attach that can fail on one rank alone (binding librccl, checking
 * the tile table, allocating the exchange buffers) and is NOT collective: a host that wants to fall back cleanly calls it on
 * every rank, agrees on the outcome through its own channel, and enters the collective sx_comm_init on all ranks or on none
 * (sx_comm_init prepares by itself when this was not called).  A failed set-up leaves the handle without exchange state. */
int sx_comm_unique_id(char *out128);
int sx_comm_prepare(sx_handle *h, int32_t n_tiles, int32_t my_tile, const int32_t *tile_cell0, const int32_t *tile_num_cells,
                    int32_t mode);
int sx_comm_init(sx_handle *h, int32_t n_tiles, int32_t my_tile, const int32_t *tile_cell0, const int32_t *tile_num_cells,
                 int32_t mode, const char *id128);
int sx_comm_attach(sx_handle *h, int32_t n_tiles, int32_t my_tile, const int32_t *tile_cell0, const int32_t *tile_num_cells,
                   int32_t mode, void *nccl_comm);
int sx_exchange(sx_handle *h);
/* The same exchange with all n tiles in ONE process on one GPU (handles hs[0..n-1] = tiles 0..n-1): identical buffer geometry
 * and offset tables, every send / receive pair replaced by a device-to-device copy.  For single-GPU multi-tile runs and for
 * testing the exchange without RCCL (which refuses two ranks on one device). */
int sx_comm_init_local(sx_handle **hs, int32_t n_tiles, const int32_t *tile_cell0, const int32_t *tile_num_cells, int32_t mode);
int sx_exchange_local(sx_handle **hs, int32_t n_tiles);

/* --- measurement ---------------------------------------------------------------------------------------------------- */
/* hipEvent timers around every kernel on the handle's stream (off by default). */
int sx_enable_timers(sx_handle *h, int32_t on);
int sx_reset_timers(sx_handle *h);
/* restrict the event pairs to the kernel with this timer name (NULL = every kernel): two event records per launch cost
 * ~4 us each on the stream, so a timed region that only needs its dominant kernel's duration should not pay for all */
int sx_timer_only(sx_handle *h, const char *name);
/* names[i] borrowed static strings; ms[i] accumulated milliseconds; calls[i] launches. Returns count via n. */
int sx_get_timers(sx_handle *h, int32_t max, const char **names, double *ms, int64_t *calls, int32_t *n);
/* algorithmic bytes of the last launch under that timer name (SURVEY.md 8(d) accounting; a diagnostics entry point that launches
 * several times per call: of the last call); 0 before the first, and for a name without a byte model or unknown.  The count is kept
 * whether timers are on or not and whatever sx_timer_only names.  Three names report the handle's
 * device allocations instead: "alloc.d_Fl" (ring spectra; 0 where k_fl_forward_cells + k_nodes_z are taken and they are never
 * allocated), "alloc.d_Fn" (node spectra and edge partials of that pair; 0 otherwise), "alloc.total" (everything sx_create allocated) */
int sx_kernel_bytes(sx_handle *h, const char *name, double *bytes);

#ifdef __cplusplus
}
#endif
#endif /* SCYTHE_HIP_H */
