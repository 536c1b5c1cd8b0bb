// What the kernels that sum the spectral state A at a point given at run time share: k_parcels (sx_parcels.hip), k_refine
// (sx_extrema.hip), k_ray_profiles and k_crossings (sx_crossings.hip), k_column_profiles, k_column_profiles_rz and k_isosurface
// (sx_isosurface.hip) and k_vortex_rings (sx_vortex.hip).  A point's weights - the 4 spline values of its radial cell, the azimuthal
// factor of a block, the Chebyshev row at its height - are formed on the device in plain fp64, and every one of these kernels stands
// under a bitwise promise: a parcel, ray, column or circle does not depend on the others of the call, k_refine agrees with
// sx_newton_step and the two scans with sx_bracket_step step for step, and sx_crossings refines on the spline k_ray_profiles made.
// Stated once, operation for operation, so that the kernels agree because they run the same functions (the library is built with
// -ffp-contract=off and every fused multiply-add is an explicit fma: inlining does not change a bit).  The scan that k_crossings and
// k_isosurface run over their stations is here as well; the bracket iteration it refines with is sx_bracket.hpp.
#pragma once
#include "sx_bracket.hpp"
#include "sx_internal.hpp"
#include <cmath>

namespace sx {

// ---- the radial spline ------------------------------------------------------------------------------------------------------------
// d-th derivative of the cardinal cubic B-spline (bspl of sx_setup.cpp)
__host__ __device__ inline double point_bspl(double delta, int d) {
    const double z = fabs(delta);
    if (z >= 2.0) return 0.0;
    const double s = delta > 0 ? 1.0 : -1.0;
    const double p = 2.0 - z, q = z < 1.0 ? 1.0 - z : 0.0;
    if (d == 0) return p * p * p / 6.0 - 4.0 * q * q * q / 6.0;
    if (d == 1) return -s * (p * p / 2.0 - 2.0 * q * q);
    return p - 4.0 * q;
}

// the radial cell of r, clamped to the tile's cells: the patch row of the first of its 4 nodes
__host__ __device__ inline int point_cell(double xmin, double DX, int cell_lo, int cell_hi, double r) {
    const int cell = (int)floor((r - xmin) / DX);
    return cell < cell_lo ? cell_lo : cell > cell_hi ? cell_hi : cell;
}

// phi^(d) / DX^d of node `node` of cell `cell` at r (sx_eval_basis' statement in plain fp64): delta = (r - x_node) / DX
__host__ __device__ inline double point_phi(double xmin, double DX, int cell, int node, double r, int d) {
    const double delta = (r - (xmin + (double)(cell - 1 + node) * DX)) / DX;
    const double b = point_bspl(delta, d);
    return d == 0 ? b : d == 1 ? b / DX : b / (DX * DX);
}

// the orders 0 .. ND - 1 at the cell's 4 nodes
template <int ND>
__host__ __device__ inline void point_basis(double xmin, double DX, int cell, double r, double (&phi)[ND][4]) {
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int d = 0; d < ND; d++) phi[d][j] = point_phi(xmin, DX, cell, j, r, d);
}

// ---- the azimuth ------------------------------------------------------------------------------------------------------------------
// Column blk of a z-mode is block 0 (k = 0), block 1 (the padding, Im of k = 0: never read), Re k at 2 k, Im k at 2 k + 1.  From
// t = (cos k lambda, sin k lambda) the factor F_blk and its lambda derivatives are: block 0: 1, 0, 0; Re k: 2 cos, -2 k sin,
// -2 k^2 cos; Im k: -2 sin, -2 k cos, 2 k^2 sin.  cs: the point's table, entry k at cs[k * stride] (az_table: stride 1; az_table16: the
// point's column cs + q, stride 16).  k is formed once, here, for the table index and the factor k: a caller that forms the index
// itself leaves the compiler two shifts to fold differently, which cost k_ray_profiles two instructions per K step.
__device__ inline bool az_padding(int blk) { return blk == 1; }
__device__ inline double az_value(int blk, double2 t) { return blk == 0 ? 1.0 : 2.0 * ((blk & 1) ? -t.y : t.x); }
__device__ inline double az_factor(int blk, const double2 *cs, int stride) { return az_value(blk, cs[(blk >> 1) * stride]); }
__device__ inline void az_factors(int blk, const double2 *cs, int stride, double &F0, double &F1, double &F2) {
    const int k = blk >> 1;
    const double2 t = cs[k * stride];
    const double kd = (double)k;
    const double y = (blk & 1) ? -t.x : -t.y;
    F0 = az_value(blk, t); F1 = 2.0 * kd * y; F2 = -(kd * kd) * F0;
}

// cs[k] = (cos, sin) k lambda of one point, k = 0 .. kDim, by the T lanes of its workgroup.  |lambda| <= 2 pi: the product is off by
// at most 2 k pi eps
__device__ inline void az_table(double2 *cs, int kDim, double lam, int tid, int T) {
    for (int k = tid; k <= kDim; k += T) {
        double s, c;
        sincos((double)k * lam, &s, &c);
        cs[k] = make_double2(c, s);
    }
}
// the same for the 16 points of a wave's tile, cs[k][16]; lam_of(q): lambda of point q of the tile
template <class Lam>
__device__ inline void az_table16(double2 *cs, int kDim, int lane, Lam lam_of) {
    for (int e = lane; e < 16 * (kDim + 1); e += 64) {
        double s, c;
        sincos((double)(e >> 4) * lam_of(e & 15), &s, &c);
        cs[e] = make_double2(c, s);
    }
}

// ---- the vertical -----------------------------------------------------------------------------------------------------------------
// The Chebyshev row at height z: x = (z - mid) / (-Lz / 2) clamped to [-1, 1], theta = acos x, t_n = (n == 0 || n == nz - 1 ? 1 : 2)
// cos n theta; and its product with column zm of a class row W [nz][Zb] (EvalClasses::d_w3), an fma chain over n from +0.0
__device__ inline double cheb_theta(double zmin, double zmax, double z) {
    const double mid = (zmin + zmax) / 2.0, half = (zmax - zmin) / 2.0;
    const double x = fmin(fmax((z - mid) / (-half), -1.0), 1.0);
    return acos(x);
}
__device__ inline double cheb_entry(int n, int nz, double th) {
    return ((n == 0 || n == nz - 1) ? 1.0 : 2.0) * cos((double)n * th);
}
__device__ inline double cheb_weight(const double *t, int t_stride, const double *W_zm, int nz, int Zb) {
    double acc = 0.0;
    for (int n = 0; n < nz; n++) acc = fma(t[n * t_stride], W_zm[(size_t)n * Zb], acc);
    return acc;
}

// ---- the sum over a point's workgroup -----------------------------------------------------------------------------------------------
// lanes of the workgroup that sums one point's columns of A (k_parcels, k_refine): from the grid alone, so that a point's result does
// not depend on the other points of the launch
constexpr int PARCEL_T = 256;             // lanes per point on grids with many columns (the bench grid: ~11,000 per variable)
constexpr int PARCEL_T_SMALL = 64;        // one wave: rl_cha_bell2024's 601 columns are 10 per lane
constexpr int PARCEL_WAVE_COLS = 1024;
inline int parcel_threads(const sx_handle *h) { return (int64_t)h->Zb * h->K2 <= PARCEL_WAVE_COLS ? PARCEL_T_SMALL : PARCEL_T; }

// acc[m] summed over the T lanes: butterfly within a wave, then the waves in order.  Every lane calls it (it holds a barrier); the
// sums are thread 0's acc on return.  red [T / 64][M]
template <int M>
__device__ inline void point_sum(double (&acc)[M], double *red, int tid, int T) {
    const int lane = tid & 63, wave = tid >> 6, nw = T >> 6;
#pragma unroll
    for (int m = 0; m < M; m++) {
        double x = acc[m];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) red[wave * M + m] = x;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int m = 0; m < M; m++) {
        double x = red[m];
        for (int w = 1; w < nw; w++) x += red[w * M + m];
        acc[m] = x;
    }
}

// ---- scan and refine: the crossings of levels along one ray or column ----------------------------------------------------------------
constexpr int SCAN_LEVELS = 8, SCAN_MAX = 16;
constexpr int64_t SCAN_COUNT_MAX = (int64_t)1 << 20;      // rays / columns of one call

struct ScanOut {                          // one ray's / column's part of the outputs
    double *root;                         // [n_levels][max_cross]
    int *dir, *count, *status;            // as root; [n_levels]; one
    double *values;                       // [n_st] the program at the stations, or null
    double *carry;                        // [n_levels][max_cross][n_carry]
    int n_carry;
};

// One wave.  Lanes take the stations 0 .. n_st - 1 in chunks of 64, compare neighbours (the last lane's value is carried into the next
// chunk), number the crossings of a level in station order with a ballot, and every crossing is refined by its own lane with
// bracket_step.  station(s): the coordinate of station s; value(x): the program there; carried(x, c): writes the outputs carried onto
// the root x to c [n_carry].  Entries no crossing took are NaN / 0.
template <class Station, class Value, class Carried>
__device__ inline void scan_crossings(int n_st, const double (&level)[SCAN_LEVELS], int n_levels, double wtol, int max_iter, int max_cross,
                                      const ScanOut &o, Station station, Value value, Carried carried) {
    __shared__ int s_cnt[SCAN_LEVELS];
    const int lane = threadIdx.x;
    int cnt[SCAN_LEVELS];
#pragma unroll
    for (int j = 0; j < SCAN_LEVELS; j++) cnt[j] = 0;
    int status = 0;
    double carry_g = 0.0, carry_x = 0.0;
    for (int base = 0; base < n_st; base += 64) {
        const int s = base + lane;
        const bool has = s < n_st;
        const double x = station(has ? s : n_st - 1);
        const double g = value(x);
        if (o.values && has) o.values[s] = g;
        double gp = __shfl_up(g, 1, 64), xp = __shfl_up(x, 1, 64);
        if (lane == 0) { gp = carry_g; xp = carry_x; }            // the chunk before ended on station base - 1
        carry_g = __shfl(g, 63, 64); carry_x = __shfl(x, 63, 64);
        const bool iv = has && s > 0;                              // this lane owns the interval [s - 1, s]
#pragma unroll
        for (int j = 0; j < SCAN_LEVELS; j++) {
            if (j >= n_levels) break;
            const double c = level[j];
            const double d0 = gp - c, d1 = g - c;
            const bool nan = iv && (d0 != d0 || d1 != d1);
            const bool cross = iv && !nan && ((d0 < 0.0) != (d1 < 0.0));
            if (__ballot(nan)) status |= 1;
            const unsigned long long mask = __ballot(cross);
            const int pos = cnt[j] + __popcll(mask & ((1ull << lane) - 1ull));
            cnt[j] += __popcll(mask);
            if (cross && pos < max_cross) {
                Bracket B;
                B.a = xp; B.fa = d0; B.b = x; B.fb = d1;
                int st = bracket_start(B, wtol);
                for (int it = 0; st < 0 && it < max_iter; it++) st = bracket_step(B, value(B.x) - c, wtol);
                if (st != 0) status |= st < 0 ? 2 : 4;
                const double xr = bracket_root(B);
                o.root[j * max_cross + pos] = xr;
                o.dir[j * max_cross + pos] = d0 < 0.0 ? 1 : -1;
                if (o.n_carry > 0) carried(xr, o.carry + (j * max_cross + pos) * o.n_carry);
            }
        }
    }
    // bits 1 and 2 are a lane's own: fold them over the wave
    status = (status & 1) | (__ballot(status & 2) ? 2 : 0) | (__ballot(status & 4) ? 4 : 0);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < SCAN_LEVELS; j++)
            if (j < n_levels) { s_cnt[j] = cnt[j]; o.count[j] = cnt[j]; }
        *o.status = status;
    }
    __syncthreads();
    for (int e = lane; e < n_levels * max_cross; e += 64) {        // the entries no crossing took
        const int j = e / max_cross, pos = e - j * max_cross;
        if (pos >= s_cnt[j]) {
            o.root[e] = __builtin_nan(""); o.dir[e] = 0;
            for (int c = 0; c < o.n_carry; c++) o.carry[e * o.n_carry + c] = __builtin_nan("");
        }
    }
}

}  // namespace sx
