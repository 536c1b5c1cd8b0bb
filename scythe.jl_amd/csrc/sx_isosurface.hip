// sx_isosurface / sx_column_series / sx_isosurface_check: the heights at which a field program crosses given levels in columns, and
// other outputs of the program carried onto those surfaces (include/scythe_hip.h).  The transpose of sx_crossings.
//
// In a column (r[, lambda]) the radial and azimuthal sums of the spectral state do not depend on z: a field in the column is a
// Chebyshev series in z whose b_zDim truncated coefficients, the column's PROFILE, are one contraction of A,
//   C[zm] = sum_blk sum_{node = cell .. cell + 3} A[zm, blk, node] phi_node^(sr)(r) / DX^sr F_blk^(sl)(lambda).
// k_column_profiles (grids with an azimuth) runs it on the f64 matrix cores per batch of at most 16 columns of one radial cell: a wave
// owns 16 z-modes x the batch's columns of one variable, stages the live A elements of the cell's 4 node rows through LDS (coalesced
// block runs in, the A-operand layout out: one K step is the 4 nodes of one block), forms the B operand phi F on the fly from the
// lane's own spline weights and the wave's table of cos / sin k lambda (both sx_point.hpp's), and keeps one accumulator per (radial,
// azimuthal) order the program names.  The K order is block 0, 2, 3, ... (block 1 is the padding block and is never read), node
// 0 .. 3 within a block, whatever the columns are; columns of the product do not mix and a short batch is padded with zero
// weights: a column's profile is bitwise independent of the other columns of the call, of their number and of their order.
// Without an azimuth (RZ) K is 4 and k_column_profiles_rz takes one lane per output instead.
//
// k_isosurface: one wave per column.  The wave expands the profiles into the full series a = CA C, a' = Dc a, a'' = Dc a' in LDS
// once, then runs scan_crossings (sx_point.hpp: the loop k_crossings runs) over the stations (the zDim levels, bottom to top), the
// program evaluated from the series with column_series - the function sx_column_series runs on the host: the crossings of a level
// are numbered upward and every crossing is refined by its own lane with bracket_step.  No atomics, nothing summed across columns.
#include "sx_colprof.hpp"
#include "sx_point.hpp"
#include "sx_redprog.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

namespace sx {

constexpr int ISO_CARRY = 8;

typedef double iso_d4 __attribute__((ext_vector_type(4)));

// ---- what host and device share ----------------------------------------------------------------------------------------------------
// The series at a height: sum_n a_n t_n(x), x = (z - mid) / (-Lz / 2) clamped to [-1, 1], t_0 = 1, t_n = 2 T_n (0 < n < nz - 1),
// t_{nz-1} = T_{nz-1}, with T_n by the recurrence T_0 = 1, T_1 = x, T_{n+1} = 2 x T_n - T_{n-1}; plain fp64, n ascending, no fused
// multiply-add.  This is the definition: stations, trial points and carried outputs all go through it.
__host__ __device__ inline double column_series(int nz, double zmin, double zmax, const double *a, double z) {
    const double mid = (zmin + zmax) / 2.0, half = (zmax - zmin) / 2.0;
    const double x = fmin(fmax((z - mid) / (-half), -1.0), 1.0);
    const double x2 = 2.0 * x;
    double tm = 1.0, t = x, s = a[0];
    for (int n = 1; n < nz; n++) {
        s = s + a[n] * (n == nz - 1 ? t : 2.0 * t);
        const double tn = x2 * t - tm;
        tm = t; t = tn;
    }
    return s;
}

// ---- stage 1: the column profiles (the argument record, the batches and the LDS size: sx_colprof.hpp) ---------------------------------
// grid (ceil(b_zDim / 16), batches, variables named)
__global__ __launch_bounds__(64) void k_column_profiles(ColProfArgs a) {
    extern __shared__ double lds[];
    double2 *cs = reinterpret_cast<double2 *>(lds);
    double *sA = lds + 32 * (size_t)(a.kDim + 1);
    const int lane = threadIdx.x, j = lane & 15, kk = lane >> 4;
    const int m0 = blockIdx.x * 16;
    const IsoBatch b = a.batch[blockIdx.y];
    const IsoVar pv = a.v[blockIdx.z];

    // ---- the weights of the batch's columns: this lane's node kk of column j; a column beyond the batch's takes no weight
    const bool col_on = j < b.n;
    double phi[3] = {0.0, 0.0, 0.0};
    if (col_on) {
        const double r = a.cols[a.order[b.first + j]];
#pragma unroll
        for (int d = 0; d < 3; d++) phi[d] = point_phi(a.xmin, a.DX, b.cell, kk, r, d);
    }
    az_table16(cs, a.kDim, lane, [&](int q) { return q < b.n ? a.cols[(int64_t)a.n_cols + a.order[b.first + q]] : 0.0; });

    // ---- the product: K = (block, node), one block per step
    iso_d4 acc[ISO_KINDS];
#pragma unroll
    for (int p = 0; p < ISO_KINDS; p++) acc[p] = iso_d4{0.0, 0.0, 0.0, 0.0};
    const double *__restrict__ Av = a.A + (int64_t)b.cell * a.C + (int64_t)pv.var * a.Zb * a.K2;
    const int cl = lane & 31, rh = lane >> 5;
    for (int c0 = 0; c0 < a.K2; c0 += ISO_KC) {
        __syncthreads();                                           // the tile (and, the first time, the table) of the pass before
        const int blk_in = c0 + cl;
        const bool blk_on = blk_in < a.K2 && !az_padding(blk_in);  // never read
#pragma unroll 4
        for (int rr = 0; rr < 32; rr++) {
            const int row = 2 * rr + rh, node = row >> 4, zm = m0 + (row & 15);
            sA[row * ISO_AS + cl] = blk_on && zm < a.Zb ? Av[(int64_t)node * a.C + (int64_t)zm * a.K2 + blk_in] : 0.0;
        }
        __syncthreads();
        for (int s = 0; s < ISO_KC; s++) {
            const int blk = c0 + s;
            if (blk >= a.K2) break;                                // uniform
            if (az_padding(blk)) continue;
            const double av = sA[(kk * 16 + j) * ISO_AS + s];      // A operand: row (z-mode) lane & 15, column (node) lane >> 4
            double F0, F1, F2;
            az_factors(blk, cs + j, 16, F0, F1, F2);
            if (pv.prof[0] >= 0) acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, phi[0] * F0, acc[0], 0, 0, 0);
            if (pv.prof[1] >= 0) acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, phi[1] * F0, acc[1], 0, 0, 0);
            if (pv.prof[2] >= 0) acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, phi[2] * F0, acc[2], 0, 0, 0);
            if (pv.prof[3] >= 0) acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, phi[0] * F1, acc[3], 0, 0, 0);
            if (pv.prof[4] >= 0) acc[4] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, phi[0] * F2, acc[4], 0, 0, 0);
        }
    }
    // C / D layout of v_mfma_f64_16x16x4: column lane & 15, row (lane >> 4) + 4 reg
    if (!col_on) return;
    const int64_t c = a.order[b.first + j];
#pragma unroll
    for (int p = 0; p < ISO_KINDS; p++) {
        if (pv.prof[p] < 0) continue;
        double *__restrict__ dst = a.P + (c * a.nprof + pv.prof[p]) * a.Zb;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = m0 + kk + 4 * r;
            if (m < a.Zb) dst[m] = acc[p][r];
        }
    }
}

// grids without an azimuth: K is the 4 nodes and the matrix unit has nothing to do.  One lane per output (z-mode, profile, column), the
// same sum: node 0 .. 3 by multiply-adds from +0.0
__global__ __launch_bounds__(256) void k_column_profiles_rz(ColProfArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)a.n_cols * a.nprof * a.Zb) return;
    const int zm = (int)(e % a.Zb), p = (int)(e / a.Zb % a.nprof);
    const int64_t c = e / ((int64_t)a.Zb * a.nprof);
    const double r = a.cols[c];
    const int cell = point_cell(a.xmin, a.DX, a.cell_lo, a.cell_hi, r);
    const double *__restrict__ Av = a.A + (int64_t)cell * a.C + ((int64_t)a.pvar[p] * a.Zb + zm) * a.K2;
    double acc = 0.0;
#pragma unroll
    for (int node = 0; node < 4; node++) acc = fma(Av[(int64_t)node * a.C], point_phi(a.xmin, a.DX, cell, node, r, a.psr[p]), acc);
    a.P[e] = acc;
}

// ---- stage 2: scan and refine ------------------------------------------------------------------------------------------------------
struct IsoArgs {
    const double *P;                      // [n_cols][nprof][Zb]
    const double *cols;                   // r of the columns (the program's r powers)
    const double *tab;                    // CA^T [ncls][Zb][nz] | Dc^T [nz][nz] | the stations [nz]
    double *height, *carry, *values;      // [n_cols][n_levels][max_cross]; ... [n_carry]; [n_cols][nz]
    int *dir, *count, *status;            // as height; [n_cols][n_levels]; [n_cols]
    RedProg g;
    uint8_t pser[RED_PLANES];             // plane -> its series in LDS
    uint8_t fcls[RED_PLANES], fneed[RED_PLANES], fser[RED_PLANES][3];   // profile -> vertical class, z orders named (bits), series of each (n_ser, n_ser + 1: scratch)
    double level[SCAN_LEVELS];
    double wtol, zmin, zmax;              // wtol = tol (zmax - zmin)
    int n_cols, nprof, Zb, nz, ncls, n_ser, n_levels, max_iter, max_cross, n_carry;
};

static size_t iso_lds(int n_ser, int nz) { return sizeof(double) * (size_t)(n_ser + 2) * nz; }

// the planes of the program at height z of the wave's column
__device__ inline void iso_planes(const IsoArgs &a, const double *ser, double z, double (&val)[RED_PLANES]) {
#pragma unroll
    for (int j = 0; j < RED_PLANES; j++) val[j] = j < a.g.n_planes ? column_series(a.nz, a.zmin, a.zmax, ser + (int)a.pser[j] * a.nz, z) : 0.0;
}

// grid (n_cols), one wave
__global__ __launch_bounds__(64) void k_isosurface(IsoArgs a) {
    extern __shared__ double ser[];       // [n_ser + 2][nz]
    const int lane = threadIdx.x, nz = a.nz;
    const int64_t q = blockIdx.x;
    const double *__restrict__ Pq = a.P + q * a.nprof * a.Zb;
    const double *__restrict__ DcT = a.tab + (size_t)a.ncls * a.Zb * nz;
    const double *__restrict__ zst = DcT + (size_t)nz * nz;

    // ---- the series of the profiles: a = CA C, a' = Dc a, a'' = Dc a', each entry summed in index order from +0.0, plain fp64
    for (int p = 0; p < a.nprof; p++) {
        const double *__restrict__ CAT = a.tab + (size_t)a.fcls[p] * a.Zb * nz;
        const double *__restrict__ Cp = Pq + (int64_t)p * a.Zb;
        const int need = a.fneed[p];
        double *s0 = ser + (int)a.fser[p][0] * nz, *s1 = ser + (int)a.fser[p][1] * nz, *s2 = ser + (int)a.fser[p][2] * nz;
        for (int n = lane; n < nz; n += 64) {
            double acc = 0.0;
            for (int zm = 0; zm < a.Zb; zm++) acc = acc + CAT[(size_t)zm * nz + n] * Cp[zm];
            s0[n] = acc;
        }
        __syncthreads();
        if (need & 6) {
            for (int n = lane; n < nz; n += 64) {
                double acc = 0.0;
                for (int m = 0; m < nz; m++) acc = acc + DcT[(size_t)m * nz + n] * s0[m];
                s1[n] = acc;
            }
            __syncthreads();
        }
        if (need & 4) {
            for (int n = lane; n < nz; n += 64) {
                double acc = 0.0;
                for (int m = 0; m < nz; m++) acc = acc + DcT[(size_t)m * nz + n] * s1[m];
                s2[n] = acc;
            }
            __syncthreads();
        }
    }

    const RedPow pw = red_pow(a.cols[q]);
    const int64_t e0 = q * a.n_levels * a.max_cross;
    const ScanOut o = {a.height + e0, a.dir + e0, a.count + q * a.n_levels, a.status + q, a.values + q * nz, a.carry + e0 * a.n_carry, a.n_carry};
    scan_crossings(
        nz, a.level, a.n_levels, a.wtol, a.max_iter, a.max_cross, o, [&](int s) { return zst[s]; },
        [&](double z) {
            double val[RED_PLANES];
            iso_planes(a, ser, z, val);
            return red_output(a.g, 0, val, pw);
        },
        [&](double z, double *car) {
            double val[RED_PLANES];
            iso_planes(a, ser, z, val);
            for (int c = 0; c < a.n_carry; c++) car[c] = red_output(a.g, 1 + c, val, pw);
        });
}

// ---- what sx_regrid shares (sx_colprof.hpp) ------------------------------------------------------------------------------------------
void colprof_batches(const sx_handle *h, const double *r, int64_t n, std::vector<int> &idx, std::vector<IsoBatch> &batches) {
    const int cell_lo = h->cell0, cell_hi = h->cell0 + h->ncells - 1;
    std::vector<int> cell(n);
    idx.resize(n);
    batches.clear();
    for (int64_t i = 0; i < n; i++) cell[i] = point_cell(h->xmin, h->DX, cell_lo, cell_hi, r[i]);
    std::iota(idx.begin(), idx.end(), 0);
    if (!h->has_l) return;
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return cell[x] < cell[y]; });
    for (int i = 0; i < (int)n;) {
        int j = i;
        while (j < (int)n && j - i < ISO_BATCH && cell[idx[j]] == cell[idx[i]]) j++;
        batches.push_back(IsoBatch{i, j - i, cell[idx[i]], 0});
        i = j;
    }
}

void colprof_grid_args(const sx_handle *h, ColProfArgs &pa) {
    pa.A = h->d_A; pa.C = h->C; pa.Zb = h->Zb; pa.K2 = h->K2; pa.kDim = h->kDim;
    pa.cell_lo = h->cell0; pa.cell_hi = h->cell0 + h->ncells - 1; pa.xmin = h->xmin; pa.DX = h->DX;
}

void launch_column_profiles(sx_handle *h, const ColProfArgs &pa, int n_batches, int nv, double bytes) {
    TimedLaunch scope(h, "k_column_profiles", bytes);
    if (h->has_l)
        hipLaunchKernelGGL(k_column_profiles, dim3((unsigned)((pa.Zb + 15) / 16), (unsigned)n_batches, (unsigned)nv), dim3(64), colprof_lds(h->kDim),
                           h->stream, pa);
    else
        hipLaunchKernelGGL(k_column_profiles_rz, grid1((int64_t)pa.n_cols * pa.nprof * pa.Zb, 256), dim3(256), 0, h->stream, pa);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct IsoState : DiagState {
    DevBuf<double> d_tab;               // CA^T of the classes | Dc^T | the stations, uploaded once per handle
    bool tab_ready = false;
    DevBuf<double> d_cols, d_P, d_out;  // d_out: height | carry | values
    DevBuf<int> d_idx, d_ri;            // order | batches;  dir | count | status
};

// What the program asks of the two kernels, from the grid and the program alone
struct IsoPlan {
    int32_t planes[RED_PLANES][2];
    int n_planes = 0, nprof = 0, nv = 0, n_ser = 0;
    IsoVar v[RED_PLANES];
    uint8_t pvar[RED_PLANES], psr[RED_PLANES];     // profile -> variable, radial order
    uint8_t pprof[RED_PLANES], pz[RED_PLANES];     // plane -> profile, z order
    uint8_t pser[RED_PLANES], fneed[RED_PLANES], fser[RED_PLANES][3];
};

// validates (who: the entry point named in the messages) and plans; 0 on success
static int iso_plan(const sx_grid_desc *gd, const EvalGeom &g, const char *who, int n_terms, const int32_t *terms, int n_carry, IsoPlan &pl) {
    const std::string w = std::string(who) + ": ";
    if (gd->geometry != SX_GEOM_RZ && gd->geometry != SX_GEOM_RLZ) { set_error(w + "the grid has no vertical (RZ and RLZ grids only)"); return 1; }
    if (n_carry < 0 || n_carry > ISO_CARRY) { set_error(w + "n_carry must be 0 .. 8"); return 1; }
    if (sx_reduce_planes(gd, SX_REDUCE_PHYSICAL, n_terms, terms, 1 + n_carry, &pl.planes[0][0], &pl.n_planes)) return 1;   // a term whose out is above n_carry included
    if (g.nz < 4 || g.nz > 256 || g.Zb < 1 || g.Zb > g.nz || !(g.zmax > g.zmin)) { set_error(w + "invalid vertical grid (need 4 <= zDim <= 256, b_zDim <= zDim, zmax > zmin)"); return 1; }
    std::memset(pl.v, 0, sizeof(pl.v));
    std::memset(pl.fneed, 0, sizeof(pl.fneed));
    for (int j = 0; j < pl.n_planes; j++) {
        const int s = pl.planes[j][1], m = (gd->geometry == SX_GEOM_RZ && s >= 3) ? s + 2 : s;      // u r rr l ll z zz
        const int kind = m < 3 ? m : m < 5 ? m : 0, zo = m >= 5 ? m - 4 : 0, var = pl.planes[j][0] - 1;
        int v = 0;
        while (v < pl.nv && pl.v[v].var != var) v++;
        if (v == pl.nv) {
            pl.v[v].var = var;
            for (int k = 0; k < ISO_KINDS; k++) pl.v[v].prof[k] = -1;
            pl.nv++;
        }
        if (pl.v[v].prof[kind] < 0) {
            pl.pvar[pl.nprof] = (uint8_t)var; pl.psr[pl.nprof] = (uint8_t)(kind < 3 ? kind : 0);
            pl.v[v].prof[kind] = pl.nprof++;
        }
        pl.pprof[j] = (uint8_t)pl.v[v].prof[kind]; pl.pz[j] = (uint8_t)zo;
        pl.fneed[pl.pprof[j]] |= (uint8_t)(1 << zo);
    }
    // the series kept in LDS: one per (profile, z order) a plane names, in profile order; what is only a step on the way goes to scratch
    for (int p = 0; p < pl.nprof; p++)
        for (int zo = 0; zo < 3; zo++) pl.fser[p][zo] = (pl.fneed[p] >> zo & 1) ? (uint8_t)pl.n_ser++ : 0xff;
    for (int p = 0; p < pl.nprof; p++)
        for (int zo = 0; zo < 2; zo++)
            if (pl.fser[p][zo] == 0xff) pl.fser[p][zo] = (uint8_t)(pl.n_ser + zo);
    for (int j = 0; j < pl.n_planes; j++) pl.pser[j] = pl.fser[pl.pprof[j]][pl.pz[j]];
    if (g.has_l && colprof_lds(g.kDim) > ISO_LDS_MAX) {
        set_error(w + "the tables of one column batch do not fit the LDS (need 32 (kDim + 1) + 2304 <= 8192 doubles)");
        return 1;
    }
    if (iso_lds(pl.n_ser, g.nz) > ISO_LDS_MAX) {
        set_error(w + "the series of one column do not fit the LDS (need (planes named + 2) zDim <= 8192 doubles)");
        return 1;
    }
    return 0;
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_isosurface_check(const sx_grid_desc *grid, int32_t n_terms, const int32_t *terms, int32_t n_carry, int32_t *n_profiles) {
    clear_error();
    IsoPlan pl;
    if (!desc_ok(grid, "sx_isosurface_check")) return 1;
    if (iso_plan(grid, desc_geom(grid), "sx_isosurface_check", n_terms, terms, n_carry, pl)) return 1;
    if (n_profiles) *n_profiles = pl.nprof;
    return 0;
}

int sx_column_series(int32_t zDim, double zmin, double zmax, const double *a, double z, double *out) {
    clear_error();
    if (!a || !out) { set_error("sx_column_series: null argument"); return 1; }
    if (zDim < 4 || zDim > 256 || !std::isfinite(zmin) || !std::isfinite(zmax) || !(zmax > zmin)) { set_error("sx_column_series: invalid vertical grid (need 4 <= zDim <= 256, zmax > zmin)"); return 1; }
    if (!(z >= zmin && z <= zmax)) { set_error("sx_column_series: z is NaN or outside [zmin, zmax]"); return 1; }
    // a' = Dc a, a'' = Dc a' as k_isosurface forms them: each entry summed in index order from +0.0, plain fp64
    const std::vector<double> Dc = cheb_dc(zmin, zmax, zDim);
    std::vector<double> a1(zDim), a2(zDim);
    const double *src = a;
    for (std::vector<double> *dst : {&a1, &a2}) {
        for (int n = 0; n < zDim; n++) {
            double acc = 0.0;
            for (int m = 0; m < zDim; m++) acc = acc + Dc[(size_t)n * zDim + m] * src[m];
            (*dst)[n] = acc;
        }
        src = dst->data();
    }
    out[0] = column_series(zDim, zmin, zmax, a, z);
    out[1] = column_series(zDim, zmin, zmax, a1.data(), z);
    out[2] = column_series(zDim, zmin, zmax, a2.data(), z);
    return 0;
}

int sx_isosurface(sx_handle *h, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_carry, int64_t n_cols,
                  const double *columns, int32_t n_levels, const double *levels, double tol, int32_t max_iter, int32_t max_cross,
                  double *height, int32_t *dir, int32_t *count, int32_t *status, double *carry, double *values, double *profiles) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    const char *who = "sx_isosurface";
    const sx_grid_desc gd = desc_of(h);
    const EvalGeom g = eval_geom_of(h);
    IsoPlan pl;
    if (iso_plan(&gd, g, who, n_terms, terms, n_carry, pl)) return 1;
    if (!scan_args_ok(h, who, "n_cols", "columns", n_terms, coef, n_levels, max_cross, levels, n_cols, tol)) return 1;
    if (n_cols > 0 && (!columns || !height || !dir || !count || !status || (n_carry > 0 && !carry))) { set_error("sx_isosurface: null argument with n_cols > 0"); return 1; }
    if (n_carry == 0 && carry) { set_error("sx_isosurface: carry must be NULL when n_carry == 0"); return 1; }
    bool neg_p = false;
    for (int t = 0; t < n_terms; t++) neg_p = neg_p || terms[(size_t)t * RED_TERM_W + 1] < 0;
    std::string why;
    for (int64_t i = 0; i < n_cols; i++) {
        const std::string at = "sx_isosurface: column " + std::to_string(i) + ": ";
        if (h->has_l && !std::isfinite(columns[n_cols + i])) { set_error(at + "a coordinate is NaN or Inf"); return 1; }
        if (!eval_radius_ok(g, columns[i], why)) { set_error(at + why); return 1; }
        if (neg_p && columns[i] == 0.0) { set_error(at + "a negative r_power in a column at r == 0"); return 1; }
    }
    if (n_cols == 0) return 0;

    const EvalClasses *k = eval_classes(h);
    if (!k) return 1;
    if (!h->diag[DIAG_ISOSURFACE]) h->diag[DIAG_ISOSURFACE].reset(new IsoState());
    IsoState *st = diag_state<IsoState>(h, DIAG_ISOSURFACE);
    const int Zb = h->Zb, nz = h->nz, ncls = (int)k->vert.size(), nprof = pl.nprof, ncc = h->ncoord - 1;
    if (!st->tab_ready) {
        std::vector<double> tab((size_t)ncls * Zb * nz + (size_t)nz * nz + nz);
        for (int c = 0; c < ncls; c++)
            for (int n = 0; n < nz; n++)
                for (int zm = 0; zm < Zb; zm++) tab[((size_t)c * Zb + zm) * nz + n] = (double)k->vert[c].W[0][(size_t)n * Zb + zm];
        const std::vector<double> Dc = cheb_dc(h->zmin, h->zmax, nz);
        double *DcT = tab.data() + (size_t)ncls * Zb * nz;
        for (int n = 0; n < nz; n++)
            for (int m = 0; m < nz; m++) DcT[(size_t)m * nz + n] = Dc[(size_t)n * nz + m];
        for (int n = 0; n < nz; n++) DcT[(size_t)nz * nz + n] = level_height(h->zmin, h->zmax, nz, n);
        if (!st->d_tab.upload(tab, "sx_isosurface: hipMalloc of the vertical operators failed")) return 1;
        st->tab_ready = true;
    }

    // the columns by radial cell (within a cell the caller's order), each cell's in batches of at most 16
    std::vector<double> c0((size_t)ncc * n_cols);
    std::memcpy(c0.data(), columns, sizeof(double) * c0.size());
    if (h->has_l)                                  // a lambda outside [-2 pi, 2 pi] into (-pi, pi]
        for (int64_t i = 0; i < n_cols; i++)
            if (std::fabs(columns[n_cols + i]) > 6.283185307179586) c0[n_cols + i] = wrap_lambda(columns[n_cols + i]);
    std::vector<int> idx;
    std::vector<IsoBatch> batches;
    colprof_batches(h, columns, n_cols, idx, batches);
    const size_t n_P = (size_t)std::max(nprof, 1) * Zb * n_cols, n_hgt = (size_t)max_cross * n_levels * n_cols;
    const size_t n_car = n_hgt * n_carry, n_val = (size_t)nz * n_cols, n_int = n_hgt + (size_t)n_levels * n_cols + n_cols;
    const size_t n_idx = (size_t)n_cols + 4 * batches.size();
    if (!st->d_cols.grow(c0.size(), who) || !st->d_P.grow(n_P, who) || !st->d_out.grow(n_hgt + n_car + n_val, who) || !st->d_idx.grow(n_idx, who) ||
        !st->d_ri.grow(n_int, who))
        return 1;
    flush_diag(h);                                 // as for every reader of A
    HIPCHK(hipMemcpyAsync(st->d_cols, c0.data(), sizeof(double) * c0.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(st->d_idx, idx.data(), sizeof(int) * n_cols, hipMemcpyHostToDevice, h->stream));
    if (!batches.empty()) HIPCHK(hipMemcpyAsync(st->d_idx + n_cols, batches.data(), sizeof(IsoBatch) * batches.size(), hipMemcpyHostToDevice, h->stream));
    if (error_status()) return 1;

    ColProfArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    colprof_grid_args(h, pa);
    pa.cols = st->d_cols; pa.order = st->d_idx; pa.batch = reinterpret_cast<const IsoBatch *>(st->d_idx + n_cols); pa.P = st->d_P;
    pa.n_cols = (int)n_cols; pa.nprof = nprof;
    std::memcpy(pa.v, pl.v, sizeof(pa.v));
    std::memcpy(pa.pvar, pl.pvar, sizeof(pa.pvar));
    std::memcpy(pa.psr, pl.psr, sizeof(pa.psr));
    // the live A elements of the 4 node rows once per batch and variable (RZ: once per column and profile), the coordinates in, the profiles out
    const double live = h->has_l ? 2.0 * h->kDim + 1.0 : 1.0;
    if (nprof > 0)
        launch_column_profiles(h, pa, (int)batches.size(), pl.nv,
                               8.0 * (4.0 * Zb * live * (h->has_l ? (double)batches.size() * pl.nv : (double)n_cols * nprof) + (double)ncc * n_cols +
                                      (double)Zb * nprof * n_cols));
    else
        set_kernel_bytes(h, "k_column_profiles", 0.0);

    IsoArgs ia;
    std::memset(&ia, 0, sizeof(ia));
    ia.P = st->d_P; ia.cols = st->d_cols; ia.tab = st->d_tab;
    ia.height = st->d_out; ia.carry = st->d_out + n_hgt; ia.values = st->d_out + n_hgt + n_car;
    ia.dir = st->d_ri; ia.count = st->d_ri + n_hgt; ia.status = st->d_ri + n_hgt + (size_t)n_levels * n_cols;
    red_pack(ia.g, pl.planes, pl.n_planes, n_terms, coef, terms, 1 + n_carry);
    std::memcpy(ia.pser, pl.pser, sizeof(ia.pser));
    std::memcpy(ia.fneed, pl.fneed, sizeof(ia.fneed));
    std::memcpy(ia.fser, pl.fser, sizeof(ia.fser));
    for (int p = 0; p < nprof; p++) ia.fcls[p] = (uint8_t)k->vcls[pl.pvar[p]];
    for (int j = 0; j < n_levels; j++) ia.level[j] = levels[j];
    ia.wtol = (tol <= 0.0 ? 1e-9 : tol) * (h->zmax - h->zmin); ia.zmin = h->zmin; ia.zmax = h->zmax;
    ia.n_cols = (int)n_cols; ia.nprof = nprof; ia.Zb = Zb; ia.nz = nz; ia.ncls = ncls; ia.n_ser = pl.n_ser; ia.n_levels = n_levels;
    ia.max_iter = max_iter <= 0 ? 60 : max_iter; ia.max_cross = max_cross; ia.n_carry = n_carry;
    // the profiles in; heights, directions, carried outputs, counts, status and the station values out
    {
        TimedLaunch scope(h, "k_isosurface", 8.0 * (double)Zb * nprof * n_cols + (12.0 + 8.0 * n_carry) * (double)n_hgt + 4.0 * ((double)n_levels + 1.0) * n_cols + 8.0 * (double)n_val);
        hipLaunchKernelGGL(k_isosurface, dim3((unsigned)n_cols), dim3(64), iso_lds(pl.n_ser, nz), h->stream, ia);
    }

    std::vector<double> ro(n_hgt + n_car + (values ? n_val : 0)), rp(profiles ? (size_t)nprof * Zb * n_cols : 0);   // held back until the call has succeeded: a failed call writes nothing
    std::vector<int> ri(n_int);
    HIPCHK(hipMemcpyAsync(ro.data(), st->d_out, sizeof(double) * ro.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ri.data(), st->d_ri, sizeof(int) * n_int, hipMemcpyDeviceToHost, h->stream));
    if (!rp.empty()) HIPCHK(hipMemcpyAsync(rp.data(), st->d_P, sizeof(double) * rp.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (error_status()) return 1;
    std::memcpy(height, ro.data(), sizeof(double) * n_hgt);
    if (n_car) std::memcpy(carry, ro.data() + n_hgt, sizeof(double) * n_car);
    if (values) std::memcpy(values, ro.data() + n_hgt + n_car, sizeof(double) * n_val);
    std::memcpy(dir, ri.data(), sizeof(int) * n_hgt);
    std::memcpy(count, ri.data() + n_hgt, sizeof(int) * n_levels * n_cols);
    std::memcpy(status, ri.data() + n_hgt + (size_t)n_levels * n_cols, sizeof(int) * n_cols);
    if (!rp.empty()) std::memcpy(profiles, rp.data(), sizeof(double) * rp.size());
    return 0;
}

}  // extern "C"
