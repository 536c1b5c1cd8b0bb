// Internal declarations of libscythe_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "scythe_hip.h"

// a failed HIP call becomes the library's error text, naming the call and the place of the use
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) ::sx::set_error(std::string(#x) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

namespace sx {

void set_error(const std::string &msg);

constexpr int DFT_KMAX_SINGLE = 319;   // largest kmax whose coefficient sets fit the LDS beside the twiddle table (sx_dft.hip)
constexpr int MUBAR = 3;   // CubicBSpline.mubar: mish points per cell (src/spectralGrid.jl:24)

// ---- host-side operator construction (sx_setup.cpp) ---------------------------------------------------------------
struct SplineClass {
    int bcl = 0, bcr = 0;
    int nfree = 0, periodic = 0, rl = 0, rr = 0;
    double gl[3][2] = {}, gr[3][2] = {};   // dependent boundary coefficients in terms of the first/last two free ones
    std::vector<double> Lband;             // [b_rDim][4]  L[i][i-3..i]
    std::vector<double> Larrow;            // [3][b_rDim]  last three rows of L (periodic only)
    // kept for the interface-only (partitioned) patch solve, which factors the diagonal blocks of the tiles (sx_iface.hip)
    std::vector<double> Mdense;                             // [nfree][nfree]  Gamma (P + eps_q Q) Gamma^T before factoring
    std::vector<std::vector<std::pair<int, double>>> Gam;   // Gamma as sparse rows: free unknown -> (patch row, weight)
};

struct ChebOps {
    int bcb = 0, bct = 0;
    double zmin = 0, zmax = 0;
    std::vector<double> z;       // [nz] gridpoints, index 0 = bottom
    std::vector<double> T;       // [nz][nz]  coefficients -> values              (Chebyshev.dct_matrix)
    std::vector<double> Dc;      // [nz][nz]  coefficient-space d/dz
    std::vector<double> CB;      // [Zb][nz]  values -> truncated b
    std::vector<double> CA;      // [nz][Zb]  b -> a (padding + BC projection)
    std::vector<double> M[3];    // [nz][Zb]  b -> value, d/dz, d2/dz2
    std::vector<double> Mint;    // [nz][nz]  values -> (CB, CA, CIInt) integral from the bottom
    std::vector<double> Mdz;     // [nz][nz]  values -> (CB, CA, CIx) truncated derivative
    std::vector<double> Mrec;    // [nz][nz]  values -> (CB, CA, CI) truncated reconstruction
    std::vector<double> Mdzz;    // [nz][nz]  values -> (CB, CA, CIxx) truncated second derivative
};

// Parallel-cyclic-reduction form of a spline class's solve a = Gamma^T (Gamma (P + eps_q Q) Gamma^T)^-1 Gamma b (sx_pcr.hip): the free
// unknowns in blocks of 3 (the half-bandwidth), block-tridiagonal; level l combines block row i with rows i -+ 2^l,
//   r_i <- r_i - alpha[l][i] r_{i - 2^l} - gamma[l][i] r_{i + 2^l},
// with the elimination blocks alpha = L D^-1, gamma = U D^-1 of the CONSTANT matrix worked out once, here, in extended precision;
// after `levels` steps the system is block diagonal (x_i = dinv[i] r_i).  PERIODIC classes: the band part M_b by the same
// elimination, the corner blocks by a rank-6 correction x = y - G (E^T y) over the first and last three unknowns.
struct PcrTables {
    int n = 0, nblk = 0, levels = 0, periodic = 0;
    std::vector<double> coef;     // [levels][nblk][18]  alpha (3 x 3 row-major), gamma (3 x 3)
    std::vector<double> dinv;     // [nblk][9]
    std::vector<int> gin_row;     // [3 nblk][4]  patch rows m whose b enters free unknown j (Gamma b), -1 = none
    std::vector<double> gin_w;    // [3 nblk][4]
    std::vector<int> gout_j;      // [nb][2]      free unknowns that make patch row m (Gamma^T x), -1 = none
    std::vector<double> gout_w;   // [nb][2]
    std::vector<double> G;        // periodic: [3 nblk][6]
};
bool build_pcr_tables(const SplineClass &sc, int nb, PcrTables &out, std::string &err);
// the same arithmetic the kernel applies (double, level by level), on the host: b / a are patch rows [nb]
void pcr_apply_host(const PcrTables &t, int nb, const double *b, double *a);
// the serial statement of the same solve (banded Cholesky factors of build_spline_class), on the host
void cholesky_apply_host(const SplineClass &sc, int nb, const double *b, double *a);
void basis_tables(double DX, double phi[4][MUBAR][4]);
// offset of Gauss point mu from its cell's centre, in cells: ring mu of cell c lies at r = xmin + DX (c + 0.5 + gauss_offset(mu))
inline double gauss_offset(int mu) {
    const double o = std::sqrt(3.0 / 5.0) / 2.0;
    return mu == 0 ? -o : mu == 1 ? 0.0 : o;
}
// the radius of tile ring i and the height of level n as sx_get_gridpoints prints them
inline double ring_radius(double xmin, double DX, int cell0, int i) { return xmin + DX * (cell0 + i / MUBAR + 0.5 + gauss_offset(i % MUBAR)); }
inline double level_height(double zmin, double zmax, int nz, int n) {
    return std::cos(n * M_PI / (nz - 1)) * (-0.5 * (zmax - zmin)) + 0.5 * (zmin + zmax);
}
void quad_weights(double DX, double w[MUBAR]);
int bc_rank(int bc);
bool build_spline_class(int nc, double DX, double l_q, int bcl, int bcr, SplineClass &out, std::string &err);
bool build_cheb_ops(double zmin, double zmax, int nz, int Zb, int bcb, int bct, ChebOps &out, std::string &err);
// Helmholtz operator of calc_Helmholtz_semiimplicit_matrix (src/semiimplicit.jl:768-781) folded with the
// collocation matrices:  Wmat = T H^-1,  Xmat = T Dc H^-1   (both [nz][nz], acting on the shifted right-hand side)
bool build_helmholtz(const ChebOps &w, double pxi_bar, double tau, std::vector<double> &Wmat, std::vector<double> &Xmat,
                     std::string &err);
void ring_table(int has_l, int uniform_L, int ri /*1-based patch ring*/, int &L, int &kmax, double &off);

// ---- evaluation at arbitrary points (sx_setup.cpp: the geometry, the weights; sx_eval.hip: sx_eval_basis, sx_evaluate and its kernel) ------
struct EvalGeom {       // what the weights of one point depend on: from a descriptor (desc_geom) or a handle (eval_geom_of)
    int has_l = 0, has_z = 0, nc = 0, cell0 = 0, ncells = 0, uniform_L = 0, kDim = 0, nz = 1, Zb = 1;
    double xmin = 0, xmax = 0, DX = 0, zmin = 0, zmax = 0;
    double tile_lo() const { return cell0 == 0 ? xmin : xmin + cell0 * DX; }
    double tile_hi() const { return cell0 + ncells == nc ? xmax : xmin + (cell0 + ncells) * DX; }
};
struct EvalVert {       // one vertical boundary-condition class
    int bcb = 0, bct = 0;
    std::vector<long double> W[3];   // [nz][Zb]  CA, Dc CA, Dc Dc CA
};
struct RadialPt {       // one radius as k_harmonics and k_spectrum read it
    double wr[12];      // [3][4] phi, phi', phi'' at nodes cell .. cell + 3
    int cell, kcap, orig, pad;   // patch row of the first node; wavenumber cap; index in the chunk (k_harmonics)
};
static_assert(sizeof(RadialPt) == 112 && offsetof(RadialPt, cell) == 96 && offsetof(RadialPt, kcap) == 100 && offsetof(RadialPt, orig) == 104,
              "k_harmonics and k_spectrum read this layout");
bool desc_ok(const sx_grid_desc *gd, const char *who);   // what every pure host helper refuses of a descriptor
EvalGeom desc_geom(const sx_grid_desc *gd);              // of a descriptor that desc_ok has passed (vertical fields: the caller checks them)
// phi, phi', phi'' at the 4 nodes of r's cell ([3][4]), that cell, and the wavenumber cap, as the kernels' point records hold them
void eval_radial_pt(const EvalGeom &g, double r, int flags, double (&wr)[12], int &cell, int &kcap);
std::vector<double> cheb_dc(double zmin, double zmax, int nz);   // [nz][nz] coefficient-space d/dz (ChebOps::Dc): extended precision, rounded once
bool build_eval_vert(double zmin, double zmax, int nz, int Zb, int bcb, int bct, EvalVert &out, std::string &err);
void eval_vert_weights(const EvalVert &ev, double zmin, double zmax, int nz, int Zb, double z, double *w /*[3][Zb]*/);
// eval_vert_weights of n heights as k_harmonics and k_spectrum stage them: [cls][height tile][row 3][Zp][16 heights], Zp = Zb rounded
// up to 4, zero-padded in heights and modes.  No classes (a grid without a vertical): one class, one height, the row {1, 0, 0}.
std::vector<double> height_tiles(const std::vector<EvalVert> &vert, const double *heights, int n, double zmin, double zmax, int nz, int Zb);
// quadrature weights of sx_reduce's domain integral (sx_setup.cpp); reads the geometry fields of g only (not kDim, Zb)
void reduce_weights(const EvalGeom &g, double *w_r /*[3 ncells]*/, double *w_l /*[3 ncells]*/, double *w_z /*[nz]*/);

// ---- elliptic inversion (sx_setup.cpp: the matrices and the factors; sx_elliptic.hip: sx_elliptic_solve, sx_elliptic_check, the kernel) ----
struct EllBands {       // the five 7-diagonal matrices of the patch's spline basis in extended precision: entry (i, j) at [i][j - i + 3]
    int nb = 0;
    std::vector<long double> S, T, M, N, M0;     // int J phi' phi', int phi phi / r (RL / RLZ), int J phi phi, int r phi phi', int phi phi
};
struct EllClass {       // one boundary-condition class of the solution variable with the factors of its wavenumbers k_lo .. k_hi
    int bcl = 0, bcr = 0, n = 0, rl = 0, rr = 0, k_lo = 0, k_hi = 0;
    double gl[3][2] = {}, gr[3][2] = {};         // as SplineClass
    std::vector<std::vector<std::pair<int, double>>> Gam;
    // [k - k_lo][nb][4]: row i of the banded Cholesky factor of K_k as L[i][i - 3], L[i][i - 2], L[i][i - 1], 1 / L[i][i] - the layout
    // of SplineClass::Lband with the reciprocal in the diagonal's place
    std::vector<double> L;
};
void build_elliptic_bands(int has_l, double xmin, double xmax, int nc, EllBands &out);
// refuses PERIODIC, alpha = 0 with a k = 0 class that fixes the value on neither side, a k >= 1 class that does not vanish at r = 0 on
// an RL / RLZ grid with xmin = 0 (both decided from Gamma and phi at the ends), and a non-positive pivot
bool build_elliptic_class(const EllBands &eb, int has_l, double xmin, int bcl, int bcr, int k_lo, int k_hi, double alpha, EllClass &out,
                          std::string &err);
void elliptic_apply_host(const EllClass &c, int k, int nb, const double *g /*[nb]*/, double *a /*[nb]*/);

// ---- antiderivatives (sx_setup.cpp: the tables; sx_antiderivative.hip: sx_antiderivative, sx_antiderivative_check, the kernels) ----
// Radial: b_i = int phi_i F dr of F(r) = int_{xmin}^{r} w f (FROM_LOW) or int_{r}^{xmax} w f (FROM_HIGH), f = sum_j a_j phi_j, split into
// a 7-diagonal band and a running sum (include/scythe_hip.h, "antiderivatives").  The tables are kept in WALK order: step s is patch
// row s (FROM_LOW, upward) or nb - 1 - s (FROM_HIGH, downward), window slot d of step s is the row of step s - 3 + d, so that the
// kernel and its host statement are one loop for both origins.
struct AntiTables {
    int nb = 0, origin = 0, weight = 0;
    std::vector<double> P;      // [nb][7]  P[s][d]: int phi_row(s) Phi_row(s - 3 + d) (Psi for FROM_HIGH); 0 outside the patch
    std::vector<double> c;      // [nb]     c[s] = int w phi_row(s)
    std::vector<double> m;      // [nb]     m[s] = int phi_row(s)
};
void build_antiderivative_tables(double xmin, double xmax, int nc, int origin, int weight, AntiTables &out);
// The projection that goes with the exact right-hand side: Gamma (P + eps_q Q) Gamma^T of one boundary-condition class with the EXACT
// Gram matrix P = int phi phi (the model's own P is its 3-point quadrature of it and pairs only with right-hand sides formed by that
// rule), Q = int phi''' phi''', eps_q from l_q.  sc: ranks, boundary rows and Gamma of the class (no Lband); F: its banded Cholesky factor
// rows as k_antiderivative_r reads them, [nb][4] = L[i][i - 3], L[i][i - 2], L[i][i - 1], 1 / L[i][i].  Refuses PERIODIC and too few cells.
bool build_antiderivative_class(double xmin, double xmax, int nc, double l_q, int bcl, int bcr, SplineClass &sc, std::vector<double> &F,
                                std::string &err);
// the arithmetic of k_antiderivative_r, operation for operation, on the host: one column a_src [nb] -> a_dst [nb]
void antiderivative_r_host(const AntiTables &t, const SplineClass &sc, const double *F /*[nb][4]*/, const double *a_src, double *a_dst);
// Z^T [Kp][Mp] (Kp = b_zDim rounded up to 4, Mp to 16, zero-padded): Z = CB T Ic CA (FROM_LOW, zero at zmin) or CB (1 e_top^T - I) T Ic CA
// (FROM_HIGH: F(zmax) - F(z)) with CA of the source's (bcb, bct), products in extended precision, rounded once
bool build_antiderivative_z(double zmin, double zmax, int nz, int Zb, int bcb, int bct, int origin, std::vector<double> &ZT, int &Kp, int &Mp,
                            std::string &err);

// ---- device memory and per-handle state of the diagnostics entry points (sx_evaluate, sx_harmonics, sx_reduce, sx_spectrum, sx_parcels_*, sx_elliptic_solve, sx_extrema, sx_crossings, sx_distribution, sx_vortex_harmonics, sx_stats_*, sx_antiderivative, sx_isosurface, sx_project, sx_regrid, sx_derive) ----
template <class T>
struct DevBuf {         // owns one device array; reads as the pointer
    T *p = nullptr;
    size_t cap = 0;     // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    bool alloc(size_t n) {      // replaces what is there
        release();
        if (hipMalloc((void **)&p, n * sizeof(T)) != hipSuccess) { p = nullptr; return false; }
        cap = n;
        return true;
    }
    // scratch that follows the size of the call: kept while it is large enough, replaced with a quarter to spare
    bool grow(size_t need, const char *who) {
        if (need <= cap || alloc(need + need / 4)) return true;
        set_error(std::string(who) + ": hipMalloc of the scratch failed");
        return false;
    }
    // a table sized once (synchronous copy); err: the whole error text
    bool upload(const T *v, size_t n, const char *err) {
        if (alloc(std::max<size_t>(n, 1)) && (!n || hipMemcpy(p, v, sizeof(T) * n, hipMemcpyHostToDevice) == hipSuccess)) return true;
        release();
        set_error(err);
        return false;
    }
    bool upload(const std::vector<T> &v, const char *err) { return upload(v.data(), v.size(), err); }
};
struct DiagState {      // what one of these entry points keeps with the handle: made on first use, deleted by sx_destroy
    virtual ~DiagState() = default;
};
enum { DIAG_EVAL, DIAG_HARM, DIAG_REDUCE, DIAG_SPEC, DIAG_PARCELS, DIAG_ELLIPTIC, DIAG_EXTREMA, DIAG_CROSSINGS, DIAG_DISTRIBUTION, DIAG_VORTEX, DIAG_STATS, DIAG_ANTIDERIVATIVE, DIAG_ISOSURFACE, DIAG_PROJECT, DIAG_REGRID, DIAG_DERIVE, DIAG_SCAN, DIAG_COUNT };   // sx_handle::diag, in the order sx_destroy deletes them (DIAG_SCAN, the table the field-program scans share, after all of them: sx_redprog.hpp)
struct EvalClasses {    // the vertical boundary-condition classes of a handle's variables (eval_classes)
    std::vector<EvalVert> vert;       // empty without a vertical
    std::vector<int> vcls;            // [V] class of each variable
    DevBuf<int> d_vcls;
    DevBuf<double> d_w3;              // [ncls][3][nz][Zb] CA, Dc CA, Dc Dc CA of every class (EvalVert::W rounded once): the point kernels' rows
};

// ---- device-side tables handed to the kernels -----------------------------------------------------------------------
// `physical` [slot][v][N] and the node-space transforms G [slot][v][NG] as the kernels see them: the VALUE slot (slot 0)
// is always fp64 - it is time-stepping state - while the derivative slots 1..D-1 are ST = double, or float in the
// fp32-storage mode (sx_grid_desc.storage_f32).  For ST = double `der` = `val` + V * N: the plain [D][V][N] array.
template <class ST>
struct Planes {
    double *val;          // [V][n]
    ST *der;              // [D-1][V][n]
};
template <class ST>
__host__ __device__ inline Planes<ST> planes_of(double *base, int V, int64_t n) {
    return Planes<ST>{base, reinterpret_cast<ST *>(base + (int64_t)V * n)};
}

// Cell-independent constants of the cell-wise equation-set kernel (sx_physics.hip), filled by sx_create; kernel arguments, so
// scalar registers and no loads: basis weights phi / phi' / phi'' of a cell's 3 Gauss points at its 4 nodes, and what it takes to
// recompute r exactly as sx_create tabulates it
struct CellConsts {
    double phiw[3][MUBAR][4];
    double xmin, DX, goff[MUBAR];
    int gcell0;           // patch index of the tile's first cell
};

// explicit_timestep (src/semiimplicit.jl:672-698): var_np1 from the value u, its tendency e and the tendencies e1, e2 of the two
// steps before (Euler at t = 1, AB2 at t = 2, AB3 from then on).  Stated once: the equation-set kernels (sx_physics.hip) and the
// parcel kernel (sx_parcels.hip) step with it.
__device__ __forceinline__ double ab_value(int t, double ts, double u, double e, double e1, double e2) {
    if (t == 1) return u + (ts * e);
    if (t == 2) return u + (0.5 * ts) * ((3.0 * e) - e1);
    return u + ((ts / 12.0) * ((23.0 * e) - (16.0 * e1) + (5.0 * e2)));
}

struct ColJob {
    int64_t in_off, out_off, mat_off;
};

// semiimplicit_adjustment (src/semiimplicit.jl:521-597): what its kernels need
struct SemiArgs {
    double *np1;
    const double *In, *I1, *I2;
    const double *MrecT, *MdzT, *WT, *XT;
    int64_t N;
    int nz, t, wi, xi;
    double ts, tau, pxi;
};

// ---- kernel-selection switches (environment, read once per handle by read_switches: sx_api.cpp) ---------------------
// The member initialiser is the value of an unset variable.  DESIGN.md has the table with what each one was measured for.
struct Switches {
    // second stream for the inner-ring chain of sx_advance (launch_inverse_and_physics); off unless SX_OVERLAP=1: measured
    // +2.6 % (669 vs 653 steps/s) - the two chains compete for the same HBM bandwidth - and it blurs the per-kernel timers
    int overlap = 0;
    int use_graph = 0;      // SX_GRAPH=1: hipGraph replay of a one-tile step (sx_step), one instantiated graph per history rotation
    int node_mode = 1;      // SX_NODE_MODE=0: ring-wise inverse everywhere (sx_create decides where the node-space form applies at all)
    int defer_diag = 0;     // SX_DEFER_DIAG=1: asks for sx_handle::defer_diag (sx_create decides whether the handle qualifies)
    int fft_reg = 1;        // 256-point transforms of the inverse kernels and of k_fl_forward_cells: register-resident passes with lane swaps (SX_FFT_REG=0: every pass through LDS)
    int dft_mfma = 1;       // native rings: the matrix-core DFT kernels (SX_DFT_MFMA=0: scalar kernels instead, debugging)
    int dft_half_wg = 1;    // eighth-wave kernel as two 256-thread workgroups per CU where one set + half a twiddle table fit 80 KB (SX_DFT_HALFWG=0: one 512-thread workgroup)
    int dft_eighth = 2;     // merged kernel: eighth-wave units of two planes (round 4; SX_DFT_EIGHTH=0: quarter-wave units of up to four)
    int dft_merge = 1;      // RLZ native rings: merged-pass inverse DFT kernel (SX_DFT_MERGE=0: one set per pass, whole tiles per wave)
    int rl_quarter = 1;     // RL grids: quarter-wave DFT kernels over one work list (SX_DFT_RLQ=0: the half-ring kernels in two ring classes)
    int dft_half = 0;       // SX_DFT_HALF=1: the half-ring forward DFT kernel on native rings (A/B)
    int dft_classes = 0;    // SX_DFT_CLASSES=n: launch classes of the older DFT kernels (experiments; <= 0: the launcher's own count)
    // vertical inverse inside the node FFT kernel where fft_fused_zinv holds (sx_fft.hip has the measurements); SX_FUSE_ZINV=0: k_zinv
    // writes Az for every node and the node FFT kernel reads it back; 2: fused, workgroups in plain grid order (fabric-traffic comparison)
    int fuse_zinv = 1;
    int zinv_ct = 0;        // SX_ZINV_CT=n: column tiles per wave of k_zinv (A/B; values without a kernel take the default: plan_zinv)
    // k_sbw_mfma (matrix-core vertical contraction, operator in registers) for zDim 64 / 32 (SX_SBW_MFMA=0: k_sbw).  1 also takes the
    // forward pair that sums the ring spectra into the spline nodes inside the FFT kernel where it applies (k_fl_forward_cells +
    // k_nodes_z: plan_fwd_cells, by default on launches of the measured kind only); SX_SBW_MFMA=2: k_sbw_mfma over ring spectra through d_Fl
    // everywhere, the A/B and cross-check form; SX_SBW_MFMA=3: the forward pair wherever its kernels apply, small tiles included
    int sbw_mfma = 1;
    int sbw_prefetch = 0;   // k_sbw requests the next cell's ring spectra before contracting the current node (SX_SBW_PF=0: off)
    // zDim 64: 256-thread workgroups of 32 blocks, two per CU - one loads while the other contracts (0.127 -> 0.118 ms;
    // SX_SBW_T256=0 restores the 512-thread form)
    int sbw_t256 = 1;
    int sbw_seg = 0;        // SX_SBW_SEG=n: segments per (block group, variable) of the sliding-window kernels (experiments; <= 0: by size)
    int wide = 1;           // 16-byte-per-lane loads / stores in the equation-set kernels (SX_WIDE=0: the 8-byte forms, A/B timing)
    // SX_SOLVE_PCR: 0 k_solve everywhere, 1 k_solve_pcr wherever its tables exist, 2 k_solve_part wherever its tables exist and k_solve
    // elsewhere, -1 by the plans (plan_solve_part, pcr_wanted)
    int solve_pcr = -1;
    int64_t pcr_maxcols = 16384;   // SX_PCR_MAXCOLS
    int pcr_r = 0;          // SX_PCR_R=n: columns per workgroup of k_solve_pcr (<= 0: by column count)
    int rz_fused = 1;       // RZ grids: the fused radius-on-the-matrix-cores kernels of sx_rz.hip (SX_RZ_FUSED=0: the general kernels)
    int rz_inv = 1;         // fused RZ inverse by node tiles (SX_RZ_INV=0: the ring-tile form, A/B)
    int semi_mfma = 1;      // semi-implicit column operators on the matrix cores (SX_SEMI_MFMA=0: k_semiimplicit)
};
Switches read_switches();   // from the environment (sx_api.cpp)

// ---- launch plans (sx_plan.cpp): which kernel and which grid, from plain integers - no handle, no device ---------------
// The launchers dispatch on them; sx_launch_plan hands them to the tests, which therefore name the shapes the library launches.
enum class SbKernel {
    refused,   // fp32 ring spectra (storage_f32 = 2) where the matrix-core kernel does not apply: sx_create refuses the handle
    sb, sbz, rz_forward, sbw_32, sbw_32_pf, sbw_64, sbw_64_pf, sbw_128, mfma_32, mfma_64, mfma_64_t256, mfma_128,
    mfma_32_f32, mfma_64_f32, mfma_64_t256_f32, mfma_128_f32
};
struct SbPlan {      // the sliding-window kernels' grid is (ceil(K2 / bw), v_cnt, segs); the other fields are 0 for k_sb / k_sbz / k_rz_forward
    SbKernel kernel = SbKernel::refused;
    int threads = 0, bw = 0;              // threads and wavenumber blocks per workgroup
    int groups = 0, nseg = 0, cps = 0, segs = 0;   // ceil(K2 / bw) v_cnt; segments aimed at; cells per segment; segments
};
enum class ZinvKernel { none /* R / RL grids, fused RZ */, colmat, mfma_2_1, mfma_4_1, mfma_4_2, mfma_8_1, mfma_8_2, mfma_8_4 };   // mfma_<MT>_<CT>
struct ZinvPlan {
    ZinvKernel kernel = ZinvKernel::none;
    bool f32 = false;                     // OT of k_colmat_mfma: float (fp32 spectra) or double
    int CT = 1, grid_x = 0;               // column tiles per wave, ceil(K2 / (64 CT))
};
// k_fl_forward_cells + k_nodes_z in place of the forward FFT kernel + the matrix-core sliding-window kernel (on: the pair is taken)
struct CellsPlan {
    bool on = false;
    int logL = 0, threads = 0;            // forward kernel: log2 of the ring length, threads per workgroup
    int S = 0, segs = 0;                  // cells per radial segment (>= 3: a node lies in at most two segments), segments
    SbKernel zk = SbKernel::refused;      // k_nodes_z's shape is the sliding-window kernel's: mfma_32 / mfma_64 / mfma_64_t256 / mfma_128
    int zthreads = 0, bw = 0, nps = 0, zsegs = 0;   // k_nodes_z: threads, wavenumber blocks per workgroup, nodes per workgroup, node runs
};
struct PcrPlan { int R = 1, logR = 0, threads = 64; };
constexpr int PCR_IPT = 4;     // row items (patch row, column) per thread while k_solve_pcr loads B and stores A: nb * R <= 4 * blockDim (plan_pcr)
SbPlan plan_sb(int geometry, int nz, int Zb, int K2, int v_cnt, int ncells, int sp32, const Switches &sw);
ZinvPlan plan_zinv(int geometry, int nz, int K2, int sp32, const Switches &sw);
// nvars: ALL the handle's variables (the segment length must not depend on the variable window: one side array serves every launch);
// v_cnt: the window k_nodes_z covers; uniform_L: the ring table's uniform length, 0 for native rings
CellsPlan plan_fwd_cells(int geometry, int nz, int Zb, int K2, int nvars, int v_cnt, int ncells, int sp32, int uniform_L, const Switches &sw);
PcrPlan plan_pcr(int nblk_max, int b_rDim, int K2, int ngroups, const Switches &sw);
// k_solve_part (sx_iface.hip): PART_P waves of a workgroup each own a block of at most PART_NR unknowns of the same 64 columns
constexpr int PART_P = 4, PART_NR = 44;
// partitions of the one-tile solve over ncols right-hand sides, 0 where the launch keeps k_solve / k_solve_pcr
int plan_solve_part(int b_rDim, int periodic, int contiguous, int64_t ncols, const Switches &sw);
// The fused RZ kernels and the semi-implicit column solve (sx_rz.hip): one MFMA row tile of RZ_T rings / nodes / columns per workgroup,
// operator fragments of RZ_KC K steps (4 rows each) in registers at once, RZ_CT = RZ_T - 3 cells per workgroup of the nodes form
constexpr int RZ_T = 16, RZ_KC = 16, RZ_CT = RZ_T - 3;
constexpr int RZ_NODES_KC = 8, RZ_NODES_ZS = 65;       // k_rz_inverse_nodes: K steps per chunk, row stride of its Az tile (64 levels + 1)
constexpr int LDS_DEFAULT_MAX = 65536;                 // dynamic LDS a kernel may ask for without hipFuncAttributeMaxDynamicSharedMemorySize
struct RzInvPlan {       // tileTransform! on a fused RZ grid
    bool nodes = true, f32 = false;       // k_rz_inverse_nodes<ST> (13 cells per workgroup) or k_rz_inverse<ST> (16 rings); ST = float / double
    int gx = 0, gy = 0, gz = 0;           // ceil(cells / 13) or ceil(rings / 16); variables; groups of 4 level tiles (one per wave)
    int lds = 0, chunks = 0;              // dynamic LDS bytes; K chunks of 32 (nodes form) or 64 (ring-tile form) coefficient rows
    bool attr = false;                    // the launch raises the kernel's dynamic-LDS limit first (lds > LDS_DEFAULT_MAX)
};
struct RzFwdPlan { int gx = 0, gy = 0, gz = 0, mt_per_wg = 0, chunks = 0, lds = 0; };   // k_rz_forward: ceil(nodes / 16), variables, mode-tile groups
struct SemiPlan {        // semiimplicit_adjustment
    bool mfma = true;                     // k_semi_mfma (16 columns per workgroup) or k_semiimplicit (256 / zDim columns, at least 1)
    int wgs = 0, threads = 0;
    int tiles_per_trip = 0;               // k_semi_mfma: waves = level tiles taken per trip of its `kt += nw` loops; 0 for k_semiimplicit
    int chunks = 0, lds = 0;              // k_semi_mfma: K chunks of 64 levels; dynamic LDS bytes
    bool attr = false;
    int cpb = 0;                          // k_semiimplicit: columns per workgroup
};
RzInvPlan plan_rz_inverse(int nz, int Zb, int ncells, int V, int f32, const Switches &sw);
RzFwdPlan plan_rz_forward(int nz, int Zb, int ncells, int v_cnt);
SemiPlan plan_semi(int nz, int64_t ncol, const Switches &sw);
std::string kernel_name(SbKernel k);      // "k_sbw_mfma<64, 32, 256>", ...; empty for `refused`
std::string kernel_name(const RzInvPlan &p);  // "k_rz_inverse_nodes<double>", "k_rz_inverse<float>", ...
std::string kernel_name(const ZinvPlan &p);   // "k_colmat_mfma<8, double, 4>", ...; empty for `none`

struct Timer {
    const char *name;
    double ms = 0.0;
    int64_t calls = 0;
    double bytes = 0;       // algorithmic bytes of the last launch (or entry-point call) under this name: sx_kernel_bytes
};

struct PendingEvent {
    int timer;
    hipEvent_t a, b;
};

}  // namespace sx

struct sx_handle {
    sx::Switches sw;   // every SX_* kernel-selection switch, as the environment had it at sx_create
    // geometry
    int geom = 0, has_l = 0, has_z = 0;
    double xmin = 0, xmax = 0, DX = 0, l_q = 2.0, zmin = 0, zmax = 0;
    int nc = 0, V = 0, D = 0, ncoord = 1, rDim = 0, b_rDim = 0, nz = 1, Zb = 1, nsz = 1;
    int cell0 = 0, ncells = 0, nrings = 0, nbt = 0, tile_num = 0, uniform_L = 0;
    int kDim = 0, K2 = 1, kDim_t = 0, K2t = 1, kmax_max = 0, L_max = 1;   // K2: device row width (padded, see sx_kernels.hip)
    int K2ref = 1;                                                         // reference block count 1 + 2 kDim
    int64_t N = 0, Nh = 0, C = 0, S_patch = 0, S_tile = 0;
    int slot[7] = {-1, -1, -1, -1, -1, -1, -1};
    std::vector<int> hL, hkmax;
    std::vector<double> hoff;
    std::vector<int64_t> hpstart;
    std::vector<int> bcl, bcl0, bcr, bcb, bct;
    // model
    double ts = 0;
    int eq = SX_EQ_NONE, semi = 0, w_index = 0, xi_index = 0, col_var = 0;
    double par[SX_NPARAMS] = {};
    int rot = 0;   // rotation of the expdot / impdot history buffers
    // device
    hipStream_t stream = nullptr;
    double *d_A = nullptr, *d_Bfull = nullptr, *d_Btile = nullptr, *d_Btile_own = nullptr;
    const double *d_Bsrc = nullptr;
    int64_t *d_rowoff = nullptr, *d_aoff = nullptr, *d_neg1 = nullptr;
    // transposed (all-to-all) solve
    int a2a_n = 0, a2a_me = 0, a2a_g0 = 0, a2a_g1 = 0;
    std::vector<int64_t> a2a_colstart;          // [n + 1] column (not group) starts
    std::vector<int> a2a_cell0, a2a_ncells;
    int *d_a2a_owner = nullptr;
    int64_t *d_a2a_soff = nullptr, *d_a2a_cw = nullptr, *d_a2a_cs = nullptr, *d_a2a_offA = nullptr, *d_a2a_offB = nullptr;
    hipStream_t stream2 = nullptr;      // second stream for the inner-ring chain of sx_advance (Switches::overlap)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // native-ring DFT launches (sx_dft.hip): (ring, variable) work items, most expensive first; [0] inverse with the
    // equation-set slot mask, [1] inverse with every slot, [2] forward
    int *d_dft_items[3] = {nullptr, nullptr, nullptr};
    int n_dft_items[3] = {0, 0, 0};
    int n_dft_big[3] = {0, 0, 0};            // of which (listed first) rings with kmax > DFT_KMAX_SINGLE: chunked kernels
    int dft_lcap_small = 0, dft_kcap_small = 0;   // largest ring length / kmax among the other rings
    // hipGraph replay of a one-tile step (sx_step; Switches::use_graph): one instantiated graph per history rotation
    int plain_steps = 0;
    hipGraphExec_t graph_exec[3] = {nullptr, nullptr, nullptr};
    hipStream_t graph_stream = nullptr;      // capture / replay stream when the handle runs on the (uncapturable) null stream
    int *d_rlq_items[2] = {nullptr, nullptr};    // (ring, part) items of the RL inverse / forward launch, most expensive first
    int n_rlq_items[2] = {0, 0};
    // SX_DEFER_DIAG=1 (one-tile HRBL runs on the FFT path): the diagnostic variable w is written by the equation set before it is
    // read (src/shallowWaterModels.jl:69, 430), so its spline coefficients are consumed by OUTPUT only; sx_advance then sends
    // the five prognostic variables through the forward transform and the solve, and w's follow on demand (flush_diag) when
    // something reads A or B.  v_lo / v_cnt: the variable window the forward-path launchers cover.
    int defer_diag = 0, v_lo = 0, v_cnt = 0;
    bool diag_dirty = false;
    std::vector<int> hmask_full, hmask_eq;       // host copies of d_mask_full / d_mask_eq
    bool in_advance = false;    // set while sx_advance launches the equation set (the diagnostic w plane is then not stored)
    bool L_all_mult4 = false;   // every ring length is a multiple of 4 (native rings are): the MFMA DFT kernels apply
    sx::CellConsts cell_consts = {};
    double *d_ref = nullptr;    // ReferenceState [3][3][nz] (Euler_test)
    int f32 = 0;   // fp32 storage of the derivative slots of d_phys / d_G (typed by the launchers)
    int sp32 = 0;  // storage_f32 = 2: the spectral transform intermediates d_Az and d_Fl are fp32 as well (fp64 accumulation)
    double *d_Az = nullptr, *d_phys = nullptr, *d_np1 = nullptr, *d_E[3] = {}, *d_I[3] = {};
    double *d_Fl = nullptr;     // ring spectra; not allocated where cells.on
    sx::CellsPlan cells;        // forward pair of the handle (plan_fwd_cells with v_cnt = V; the launchers re-plan for their window)
    double *d_Fn = nullptr;     // cells.on: node spectra [nbt][V][nz][K2], then the open edge partials of every segment but the last [segs - 1][3][V][nz][K2]
    size_t fl_bytes = 0, fn_bytes = 0;   // device bytes of d_Fl / d_Fn
    double *d_phi = nullptr, *d_wq = nullptr;
    int *d_L = nullptr, *d_kmax = nullptr;
    int64_t *d_pstart = nullptr, *d_twoff = nullptr, *d_phoff = nullptr;
    double2 *d_tw = nullptr, *d_ph = nullptr;
    double *d_MzT = nullptr;    // operators of d_Mz transposed: [v][sz][Zb][nz]
    double *d_Mz = nullptr, *d_CB = nullptr, *d_MintT = nullptr, *d_MdzT = nullptr, *d_MrecT = nullptr;
    double *d_WT[2] = {}, *d_XT[2] = {};
    double tau[2] = {0, 0};
    int *d_cls = nullptr, *d_cmeta = nullptr;   // cmeta [ncls][4] = nfree, periodic, rl, rr
    double *d_gl = nullptr, *d_gr = nullptr, *d_Lband = nullptr, *d_Larrow = nullptr, *d_Ldinv = nullptr;
    double *d_r = nullptr, *d_cosl = nullptr, *d_sinl = nullptr, *d_z = nullptr;
    int *d_flag = nullptr;
    unsigned long long *d_maxabs = nullptr;   // [V] scratch of sx_max_abs
    void *comm_state = nullptr;               // RCCL exchange state (sx_comm.cpp)
    void *iface_state = nullptr;              // interface-only patch solve (sx_iface.hip)
    void *pcr_state = nullptr;                // parallel-cyclic-reduction tables and launch lists (sx_pcr.hip)
    // partitioned one-tile solve (k_solve_part, sx_iface.hip): tables of every class, built by sx_create where the plan can take them
    int part_P = 0;                           // 0: no tables
    int *d_part_meta = nullptr;
    double *d_part_tab = nullptr;
    std::unique_ptr<sx::DiagState> diag[sx::DIAG_COUNT];   // states of the diagnostics entry points, made on first use (sx_eval.hip ... sx_parcels.hip)
    double *d_CBT = nullptr;                  // CB transposed [nz][Zb] (sx_rz.hip)
    std::vector<sx::SplineClass> classes;     // host copies of the spline classes (d_cls indexes them)
    std::vector<int> hcls;                    // host copy of d_cls: [v][2] -> class of (k = 0, k >= 1)
    int *d_mask_full = nullptr, *d_mask_eq = nullptr;   // per-variable bit masks of derivative slots to produce
    int mask_eq_bits = 0, mask_full_bits = 0;            // total number of (variable, slot) planes in each mask
    int mask_eq_val = 0, mask_full_val = 0, mask_node_val = 0;   // of which value-slot planes (always fp64)
    // node-space ("radial last") inverse for uniform rings: rings [0, R_in) keep the ring-wise path (their wavenumber
    // truncation depends on the ring), rings [R_in, nrings) are evaluated from node-space transforms inside the equation set
    int node_mode = 0, node_active = 0, R_in = 0, mask_node_bits = 0;
    int64_t NG = 0;
    double *d_G = nullptr, *d_nphi = nullptr;
    int *d_nkmax = nullptr, *d_mask_node = nullptr;
    int64_t *d_npstart = nullptr, *d_nphoff = nullptr;
    sx::ColJob *d_jobs_zinv_full = nullptr, *d_jobs_zinv_eq = nullptr, *d_jobs_zf = nullptr;
    int njobs_zinv_full = 0, njobs_zinv_eq = 0;
    int ncls = 0;
    size_t dev_bytes = 0;
    std::vector<void *> allocs;
    // timers
    int timers_on = 0;
    std::string timer_only;           // when set, only this kernel gets its event pair
    std::vector<sx::Timer> timers;
    std::vector<sx::PendingEvent> pending;
    std::vector<hipEvent_t> event_pool;
};

namespace sx {
// kernel launchers (transforms, solve, pack: sx_kernels.hip; equation sets: sx_physics.hip); a failed launch goes to set_error
inline dim3 grid1(int64_t n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }
void launch_zinv(sx_handle *h, bool full);
void launch_rl_inverse(sx_handle *h, bool full);
bool fft_path_ok(const sx_handle *h);
// zDim with matrix-core column kernels (the HRBL equation set, the sliding-window forward transform)
inline bool mfma_levels(int nz) { return nz == 32 || nz == 64 || nz == 128; }
// the matrix-core shape: uniform power-of-two rings with such a zDim; zb_bound: b_zDim also fits k_sbw_mfma's row tiles
inline bool mfma_shape(const sx_handle *h, bool zb_bound = false) {
    return fft_path_ok(h) && h->has_z && mfma_levels(h->nz) && (!zb_bound || (h->nz <= 64 ? h->Zb <= 64 : h->Zb <= 96));
}
bool fft_fused_zinv(const sx_handle *h);
bool dft_mfma_ok(const sx_handle *h);
// work lists of the native-ring DFT launches (sx_dft.hip): (ring, x) items, most expensive first; x is a variable (RLZ) or a part (RL)
using DftItems = std::vector<std::array<int, 2>>;
// the items (ring, x), x < nparts(ring), whose cost(ring, x) is positive, in order of decreasing cost - workgroups are dispatched in
// blockIdx order, so the cheap items fill the tail of the launch; equal costs keep the order (ring, x)
template <class NParts, class Cost>
DftItems dft_work_items(int nrings, NParts nparts, Cost cost) {
    std::vector<std::array<int64_t, 3>> it;       // (cost, ring, x)
    for (int r = 0; r < nrings; r++)
        for (int x = 0, n = nparts(r); x < n; x++) {
            const int64_t c = cost(r, x);
            if (c > 0) it.push_back({c, r, x});
        }
    std::stable_sort(it.begin(), it.end(), [](const auto &a, const auto &b) { return a[0] > b[0]; });
    DftItems out;
    for (const auto &e : it) out.push_back({(int)e[1], (int)e[2]});
    return out;
}
bool dft_upload_items(sx_handle *h, const DftItems &it, int **d_items, int *n_items, bool counted);
DftItems rlq_items(const std::vector<int> &hL, const std::vector<int> &hkmax, int which);      // RL grids: [0] inverse, [1] forward
void launch_rl_inverse_dft(sx_handle *h, const int *d_mask);
void launch_fl_forward_dft(sx_handle *h);
void launch_rl_inverse_fft(sx_handle *h, const int *d_mask, int n_rings = -1);
void launch_node_fft(sx_handle *h);
void launch_fl_forward_fft(sx_handle *h);
void launch_fl_forward_cells(sx_handle *h, const CellsPlan &p);
void launch_physics(sx_handle *h, int t);
void launch_inverse_and_physics(sx_handle *h, int t);
void launch_copy_slot0(sx_handle *h);
void launch_fl_forward(sx_handle *h);
void launch_sb(sx_handle *h);
void launch_solve(sx_handle *h);
void launch_solve_a2a(sx_handle *h, const double *recv, double *send);
void launch_a2a_pack(sx_handle *h, double *buf, int unpack);
void launch_halo_add(sx_handle *h, const double *recv);
void launch_nan_check(sx_handle *h);
void launch_max_abs(sx_handle *h, unsigned long long *d_out);
// The bracket of one timed kernel launch (or of the launches one timer name covers): a launcher opens
// `TimedLaunch scope(h, "k_name", bytes);` where its timed region starts and lets the scope end where the region ends, early returns
// included.  bytes: the algorithmic bytes of this launch, every array it touches counted once (DESIGN.md "Kernels and rooflines"),
// stated by the launcher from the quantities it launches with; 0.0 where the kernel has no byte model.  Construction looks the name up
// (first use appends it: sx_get_timers lists names in that order), stores the bytes under it - timers on or off, the name excluded by
// sx_timer_only or not: sx_kernel_bytes answers from there - and, with timers on and the name not excluded, records the begin event
// on h->stream as it is then.  Destruction checks the launch - a failed one goes to set_error as
// "k_name: <hip error text>" - and records the scope's own end event on the stream the begin event went to.
// Scopes do not nest: a launcher called inside its caller's scope (launch_solve_part, launch_solve_pcr, launch_semi_mfma) opens none.
class TimedLaunch {
public:
    TimedLaunch(sx_handle *h, const char *name, double bytes);
    ~TimedLaunch();
    TimedLaunch(const TimedLaunch &) = delete;
    TimedLaunch &operator=(const TimedLaunch &) = delete;

private:
    const char *name;
    hipStream_t stream = nullptr;
    hipEvent_t end = nullptr;      // null: this launch is not timed
};
// for an entry point whose call launches nothing (no variables, an empty set): the name, if it has a timer, reads `bytes` from now on
void set_kernel_bytes(sx_handle *h, const char *name, double bytes);
void timers_flush(sx_handle *h);
// ---- the byte models' shared terms (w = 8: fp64) ----
// bytes per point of a set of `bits` (variable, slot) planes of `physical` / G, `val` of them value planes: those are always fp64,
// the derivative slots 4 bytes wide in the fp32-storage mode
inline double plane_bytes(const sx_handle *h, int bits, int val) { return 8.0 * val + (h->f32 ? 4.0 : 8.0) * (bits - val); }
// ... of the planes an inverse transform writes: every slot (tileTransform!) or the equation set's
inline double out_plane_bytes(const sx_handle *h, bool full) {
    return full ? plane_bytes(h, h->mask_full_bits, h->mask_full_val) : plane_bytes(h, h->mask_eq_bits, h->mask_eq_val);
}
int zinv_rows(const sx_handle *h, bool full);       // rows of Az that launch_zinv(h, full) fills (sx_kernels.hip)
double az_count(const sx_handle *h, bool full);     // entries the azimuthal inverse that follows it reads: those rows of Az, or the tile's A rows
// entries of what the forward azimuthal transform writes: the ring spectra, or with the forward pair that sums them into the nodes
// the node spectra + the segments' edge partials
inline double fl_count(const sx_handle *h) {
    return h->cells.on ? (double)(h->nbt + 3 * (h->cells.segs - 1)) * h->V * h->nz * h->K2 : (double)h->nrings * h->V * h->nz * h->K2;
}
// node-space units actually transformed and read: cell c of the outer rings combines nodes c .. c + 3 and the first such cell is
// R_in / 3, so nodes [R_in / 3, nbt) - 132 of 174 at the bench grid; the nodes below feed the ring-wise inner rings only
inline double node_units(const sx_handle *h) { return (double)(h->nbt - h->R_in / MUBAR); }
inline double node_points(const sx_handle *h) { return node_units(h) * (double)h->uniform_L * h->nz; }       // points of their transforms (NGu)
void clear_error();
int error_status();   // 1 if set_error has been called since the last clear_error
void comm_release(sx_handle *h);
void flush_diag(sx_handle *h);
void graphs_release(sx_handle *h);
void iface_release(sx_handle *h);
void pcr_release(sx_handle *h);
template <class S>
inline S *diag_state(const sx_handle *h, int which) { return static_cast<S *>(h->diag[which].get()); }
EvalGeom eval_geom_of(const sx_handle *h);
sx_grid_desc desc_of(const sx_handle *h);      // the handle's grid as the pure host validators read it (no boundary conditions)
// what sx_evaluate refuses of a point: its radius, its height; the two and a finite lambda, of every point of a list
bool eval_radius_ok(const EvalGeom &g, double r, std::string &why);
bool eval_height_ok(const EvalGeom &g, double z, std::string &why);
bool eval_points_ok(const sx_handle *h, const double *pts /*[n_coord][n]*/, int64_t n, const char *who, const char *noun);
const EvalClasses *eval_classes(sx_handle *h);   // made on first use (sx_eval.hip); null when that failed
// lambda into (-pi, pi], reduced in extended precision (sx_eval.hip).  sx_parcels_set wraps every lambda; sx_extremum_refine,
// sx_crossings and sx_isosurface only one outside [-2 pi, 2 pi]: a gridpoint's lambda is used as given (frozen, it comes back bitwise)
double wrap_lambda(double lam);
// what sx_crossings and sx_isosurface refuse alike of the program's coefficients, the levels, the bounds and the count n of `noun`
// (count: its argument's name), in the order the header lists (sx_crossings.hip)
bool scan_args_ok(const sx_handle *h, const char *who, const char *count, const char *noun, int n_terms, const double *coef, int n_levels,
                  int max_cross, const double *levels, int64_t n, double tol);
int default_bzdim(int zDim);                   // b_zDim of a descriptor that leaves it 0 (sx_api.cpp)
bool rz_fused(const sx_handle *h);
void launch_rz_inverse(sx_handle *h, const int *d_mask);
void launch_rz_forward(sx_handle *h);
void launch_semi_mfma(sx_handle *h, const SemiArgs &a);
bool pcr_wanted(sx_handle *h, int64_t ncols);
void launch_solve_pcr(sx_handle *h, bool linear, const double *Bsrc, const int64_t *boffA, const int64_t *boffB, double *A,
                      const int64_t *aoffA, const int64_t *aoffB, int vz0, int ng, int64_t stride);
bool part_prepare(sx_handle *h);             // sx_create: the tables of k_solve_part where its plan can apply; false: an upload failed
void launch_solve_part(sx_handle *h, const double *B, double *A, int vz0, int ng);
bool tile_table_ok(const sx_handle *h, int n, int me, const int32_t *cell0, const int32_t *ncells);
#ifdef SX_PHASES
void phases_dump();
void fft_phases_dump();
void sbw_phases_dump();
void dft_phases_dump();
#endif
}  // namespace sx
