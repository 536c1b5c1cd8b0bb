// sx_crossings / sx_bracket_step: the radii at which a field program crosses given levels along rays (include/scythe_hip.h,
// DESIGN.md 15).
//
// Along a ray (lambda, z) the azimuthal and vertical sums of the spectral state do not depend on r: the state on the ray is a cubic
// spline in r whose coefficients, the ray's PROFILE, are one contraction of A,
//   P[prof][q][m] = sum_col A[m][var, col] W[col][q],   W[col][q] = F_blk^(sl)(lambda_q) Wz^(sz)[zm](z_q),   col = (zm, blk),
// a [rows x ncol] [ncol x n_rays] product per variable.  k_ray_profiles runs it on the f64 matrix cores: a wave owns 16 patch rows x
// 16 rays of one variable, stages 16 x CROSS_KC tiles of A through LDS (coalesced row pieces in, the A-operand layout lane =
// (col & 3) * 16 + row out), forms the B operand - the ray weights - on the fly from the wave's tables of cos / sin k lambda and of
// the vertical rows (the functions of sx_point.hpp, which k_parcels runs too), and keeps one accumulator per (lambda order, z order)
// the program names.  The K order is col = 0, 1, 2, ... whatever the rays are, columns of the matrix product do not mix, and a ray
// tile is padded with zero weights: a ray's profile is bitwise independent of the other rays of the call and of their number.
//
// k_crossings: one wave per ray runs scan_crossings (sx_point.hpp) over the stations (inner end, radial gridpoints, outer end), the
// program evaluated from the profiles (4 multiply-adds per plane): the crossings of a level are numbered outward and every crossing
// is refined by its own lane with bracket_step - the function sx_bracket_step runs on the host.  No atomics, nothing summed across rays.
#include "sx_point.hpp"
#include "sx_redprog.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

constexpr int CROSS_KINDS = 5;            // profile kinds of a variable: value, d/dlambda, d2/dlambda2, d/dz, d2/dz2
constexpr int CROSS_KC = 32;              // columns of A per staged tile: 8 K steps
constexpr int CROSS_AS = 36;              // row stride of the staged tile in doubles
constexpr size_t CROSS_LDS_MAX = 64 * 1024;

typedef double cross_d4 __attribute__((ext_vector_type(4)));

// ---- stage 1: the ray profiles -----------------------------------------------------------------------------------------------------
struct ProfVar {
    int var, cls;                         // 0-based variable, its vertical class
    int prof[CROSS_KINDS];                // profile number of each kind, -1 = not named
};
struct ProfArgs {
    const double *A;                      // [b_rDim][C]
    const double *w3;                     // [ncls][3][nz][Zb] CA, Dc CA, Dc Dc CA: EvalClasses::d_w3 (null without a vertical)
    const double *rays;                   // [n_coord - 1][n_rays]: lambda[, z]; |lambda| <= 2 pi
    double *P;                            // [n_rays][nprof][rows]
    int64_t C;
    int n_rays, rows, row0, nprof, Zb, nz, K2, kDim, has_l, has_z;
    double zmin, zmax;
    ProfVar v[RED_PLANES];
};

// doubles of LDS: cs [kDim + 1][16] double2 (grids with an azimuth) | wz [3][Zb][16] | tz [nz][16] | sA [16][CROSS_AS]
static size_t prof_lds(const sx_handle *h) {
    const size_t Zb = h->has_z ? h->Zb : 1, nz = h->has_z ? h->nz : 0;
    return sizeof(double) * ((h->has_l ? 32 * (size_t)(h->kDim + 1) : 0) + 48 * Zb + 16 * nz + 16 * CROSS_AS);
}

// grid (ceil(rows / 16), ceil(n_rays / 16), variables named)
__global__ __launch_bounds__(64) void k_ray_profiles(ProfArgs a) {
    extern __shared__ double lds[];
    double2 *cs = reinterpret_cast<double2 *>(lds);
    double *wz = lds + (a.has_l ? 32 * (size_t)(a.kDim + 1) : 0);
    double *tz = wz + 48 * (size_t)a.Zb;
    double *sA = tz + 16 * (size_t)(a.has_z ? a.nz : 0);
    const int lane = threadIdx.x, j = lane & 15, kk = lane >> 4;
    const int m0 = blockIdx.x * 16, q0 = blockIdx.y * 16;
    const ProfVar pv = a.v[blockIdx.z];

    // ---- the weights of the 16 rays (sx_point.hpp; a ray beyond the call's takes lambda = 0, the lowest level, and no weight)
    if (a.has_l) az_table16(cs, a.kDim, lane, [&](int jj) { return q0 + jj < a.n_rays ? a.rays[q0 + jj] : 0.0; });
    if (a.has_z) {
        const double *zr = a.rays + (a.has_l ? (int64_t)a.n_rays : 0);
        for (int e = lane; e < 16 * a.nz; e += 64) {
            const int q = q0 + (e & 15);
            const double z = q < a.n_rays ? zr[q] : a.zmin;        // a named local: written as the call's argument it costs 30 VGPRs
            tz[e] = cheb_entry(e >> 4, a.nz, cheb_theta(a.zmin, a.zmax, z));
        }
        __syncthreads();
        const double *w3 = a.w3 + (size_t)pv.cls * 3 * a.nz * a.Zb;
        for (int e = lane; e < 48 * a.Zb; e += 64) {
            const int m = e / (16 * a.Zb), zm = (e - m * 16 * a.Zb) >> 4, jj = e & 15;
            const bool need = m == 0 ? (pv.prof[0] >= 0 || pv.prof[1] >= 0 || pv.prof[2] >= 0) : pv.prof[2 + m] >= 0;
            wz[e] = need ? cheb_weight(tz + jj, 16, w3 + (size_t)m * a.nz * a.Zb + zm, a.nz, a.Zb) : 0.0;
        }
    } else {
        if (lane < 48) wz[lane] = lane < 16 ? 1.0 : 0.0;           // Zb = 1 without a vertical
    }

    // ---- the product: K = the columns of the variable in their own order, 4 per step
    cross_d4 acc[CROSS_KINDS];
#pragma unroll
    for (int p = 0; p < CROSS_KINDS; p++) acc[p] = cross_d4{0.0, 0.0, 0.0, 0.0};
    const int ncol = a.Zb * a.K2;
    const double *__restrict__ Av = a.A + (int64_t)a.row0 * a.C + (int64_t)pv.var * ncol;
    const bool ray_on = q0 + j < a.n_rays;
    const int cl = lane & 31, rh = lane >> 5;
    for (int c0 = 0; c0 < ncol; c0 += CROSS_KC) {
        __syncthreads();                                           // the tile (and, the first time, the weights) of the pass before
        const int col = c0 + cl;
        const bool col_on = col < ncol && !(a.has_l && col % a.K2 == 1);      // block 1 is the padding block: never read
#pragma unroll
        for (int rr = 0; rr < 8; rr++) {
            const int row = 2 * rr + rh;
            sA[row * CROSS_AS + cl] = col_on && m0 + row < a.rows ? Av[(int64_t)(m0 + row) * a.C + col] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < CROSS_KC / 4; s++) {
            if (c0 + 4 * s >= ncol) break;                         // uniform
            const int kc = c0 + 4 * s + kk;
            const bool on = kc < ncol;
            const int kcl = on ? kc : ncol - 1;
            const int zm = kcl / a.K2, blk = kcl - zm * a.K2;
            const double av = sA[j * CROSS_AS + 4 * s + kk];       // A operand: row lane & 15, column lane >> 4
            double F0 = 1.0, F1 = 0.0, F2 = 0.0;
            if (a.has_l) az_factors(blk, cs + j, 16, F0, F1, F2);
            const bool pad = a.has_l && az_padding(blk);           // ahead of `live`: inside it the call keeps a branch per K step
            const bool live = on && ray_on && !pad;
            const double z0 = live ? wz[zm * 16 + j] : 0.0;
            if (pv.prof[0] >= 0) acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, F0 * z0, acc[0], 0, 0, 0);
            if (pv.prof[1] >= 0) acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, F1 * z0, acc[1], 0, 0, 0);
            if (pv.prof[2] >= 0) acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, F2 * z0, acc[2], 0, 0, 0);
            if (pv.prof[3] >= 0) acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, live ? F0 * wz[(a.Zb + zm) * 16 + j] : 0.0, acc[3], 0, 0, 0);
            if (pv.prof[4] >= 0) acc[4] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, live ? F0 * wz[(2 * a.Zb + zm) * 16 + j] : 0.0, acc[4], 0, 0, 0);
        }
    }
    // C / D layout of v_mfma_f64_16x16x4: column lane & 15, row (lane >> 4) + 4 reg
    if (!ray_on) return;
#pragma unroll
    for (int p = 0; p < CROSS_KINDS; p++) {
        if (pv.prof[p] < 0) continue;
        double *__restrict__ dst = a.P + ((int64_t)(q0 + j) * a.nprof + pv.prof[p]) * a.rows;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = m0 + kk + 4 * r;
            if (m < a.rows) dst[m] = acc[p][r];
        }
    }
}

// ---- what host and device share: the stations, the basis (point_basis: sx_point.hpp; the bracket step: sx_bracket.hpp) -------------
struct CrossGeom {
    double xmin, DX, lo, hi;              // the tile's radial extent as eval_radius_ok reads it
    int cell0, ncells, n_st;              // stations: lo, the 3 ncells radial gridpoints, hi
};

// the radius of station s: the doubles sx_get_gridpoints prints (ring_radius) between the tile's ends
__host__ __device__ inline double cross_station(const CrossGeom &G, int s) {
    if (s <= 0) return G.lo;
    if (s >= G.n_st - 1) return G.hi;
    const int i = s - 1, mu = i % MUBAR;
    const double o = sqrt(3.0 / 5.0) / 2.0;
    return G.xmin + G.DX * (G.cell0 + i / MUBAR + 0.5 + (mu == 0 ? -o : mu == 1 ? 0.0 : o));
}

// phi, phi', phi'' of the 4 nodes of r's cell (sx_eval_basis' statement in plain fp64); returns the cell = patch row of the first node
__host__ __device__ inline int cross_basis(const CrossGeom &G, double r, double (&phi)[3][4]) {
    const int cell = point_cell(G.xmin, G.DX, G.cell0, G.cell0 + G.ncells - 1, r);
    point_basis<3>(G.xmin, G.DX, cell, r, phi);
    return cell;
}

// ---- stage 2: scan and refine ------------------------------------------------------------------------------------------------------
struct CrossArgs {
    const double *P;                      // [n_rays][nprof][rows]
    double *radius;                       // [n_rays][n_levels][max_cross] as the caller's column-major [max_cross, n_levels, n_rays]
    int *dir, *count, *status;            // as radius; [n_rays][n_levels]; [n_rays]
    RedProg g;
    uint8_t pprof[RED_PLANES], pd[RED_PLANES];     // plane -> profile number, radial order 0 .. 2
    double level[SCAN_LEVELS];
    double wtol;                          // tol DX
    int n_rays, rows, nprof, n_levels, max_iter, max_cross;
    CrossGeom G;
};

// g_q(r): the planes from the ray's profiles, then the program in term order from +0.0
__device__ inline double cross_value(const CrossArgs &a, const double *__restrict__ Pq, double r) {
    double phi[3][4];
    const int cell = cross_basis(a.G, r, phi);
    double val[RED_PLANES];
#pragma unroll
    for (int j = 0; j < RED_PLANES; j++) {
        val[j] = 0.0;
        if (j < a.g.n_planes) {
            const double *__restrict__ p = Pq + (int64_t)a.pprof[j] * a.rows + (cell - a.G.cell0);
            const int d = a.pd[j];
            double w[4];
#pragma unroll
            for (int n = 0; n < 4; n++) w[n] = d == 0 ? phi[0][n] : d == 1 ? phi[1][n] : phi[2][n];
            val[j] = fma(w[3], p[3], fma(w[2], p[2], fma(w[1], p[1], w[0] * p[0])));
        }
    }
    return red_output(a.g, 0, val, red_pow(r));
}

// grid (n_rays), one wave
__global__ __launch_bounds__(64) void k_crossings(CrossArgs a) {
    const int64_t q = blockIdx.x;
    const double *__restrict__ Pq = a.P + q * a.nprof * a.rows;
    const int64_t e0 = q * a.n_levels * a.max_cross;
    const ScanOut o = {a.radius + e0, a.dir + e0, a.count + q * a.n_levels, a.status + q, nullptr, nullptr, 0};
    scan_crossings(a.G.n_st, a.level, a.n_levels, a.wtol, a.max_iter, a.max_cross, o,
                   [&](int s) { return cross_station(a.G, s); }, [&](double r) { return cross_value(a, Pq, r); }, [](double, double *) {});
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct CrossState : DiagState {
    DevBuf<double> d_rays, d_P, d_rad;
    DevBuf<int> d_i;                    // dir | count | status
};

bool scan_args_ok(const sx_handle *h, const char *who, const char *count, const char *noun, int n_terms, const double *coef, int n_levels,
                  int max_cross, const double *levels, int64_t n, double tol) {
    const std::string w = std::string(who) + ": ";
    if (n_terms > 0 && !coef) { set_error(w + "null coef with n_terms > 0"); return false; }
    if (n_levels < 1 || n_levels > SCAN_LEVELS) { set_error(w + "n_levels must be 1 .. 8"); return false; }
    if (max_cross < 1 || max_cross > SCAN_MAX) { set_error(w + "max_cross must be 1 .. 16"); return false; }
    if (!levels) { set_error(w + "null levels"); return false; }
    if (n < 0) { set_error(w + count + " is negative"); return false; }
    if (n > SCAN_COUNT_MAX) { set_error(w + "more than 2^20 " + noun + " in one call"); return false; }
    if (!std::isfinite(tol)) { set_error(w + "tol is NaN or Inf"); return false; }
    for (int j = 0; j < n_levels; j++)
        if (!std::isfinite(levels[j])) { set_error(w + "level " + std::to_string(j) + " is NaN or Inf"); return false; }
    if (h->ncells != h->nc) { set_error(w + "one-tile patches only"); return false; }
    return true;
}

static CrossGeom cross_geom(const EvalGeom &g) {
    CrossGeom G;
    G.xmin = g.xmin; G.DX = g.DX; G.lo = g.tile_lo(); G.hi = g.tile_hi();
    G.cell0 = g.cell0; G.ncells = g.ncells; G.n_st = MUBAR * g.ncells + 2;
    return G;
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_crossings(sx_handle *h, int32_t n_terms, const double *coef, const int32_t *terms, int64_t n_rays, const double *rays,
                 int32_t n_levels, const double *levels, double tol, int32_t max_iter, int32_t max_cross, double *radius, int32_t *dir,
                 int32_t *count, int32_t *status, double *profiles) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    const char *who = "sx_crossings";
    const sx_grid_desc gd = desc_of(h);
    int32_t planes[RED_PLANES][2], n_planes = 0;
    if (sx_reduce_planes(&gd, SX_REDUCE_PHYSICAL, n_terms, terms, 1, &planes[0][0], &n_planes)) return 1;      // one output: out = 0 in every term
    if (!scan_args_ok(h, who, "n_rays", "rays", n_terms, coef, n_levels, max_cross, levels, n_rays, tol)) return 1;
    const EvalGeom g = eval_geom_of(h);
    if (h->has_l && g.tile_lo() == 0.0)
        for (int t = 0; t < n_terms; t++)
            if (terms[(size_t)t * RED_TERM_W + 1] < 0) { set_error("sx_crossings: a negative r_power on a tile whose first station is r == 0"); return 1; }
    if (prof_lds(h) > CROSS_LDS_MAX) {
        set_error("sx_crossings: the weights of one ray tile do not fit the LDS (need 32 (kDim + 1) + 48 b_zDim + 16 zDim + 576 <= 8192 doubles)");
        return 1;
    }
    const int nrc = h->ncoord - 1;                 // coordinates of a ray
    if (n_rays > 0 && ((nrc > 0 && !rays) || !radius || !dir || !count || !status)) { set_error("sx_crossings: null argument with n_rays > 0"); return 1; }
    std::string why;
    for (int64_t i = 0; i < n_rays; i++) {
        if (h->has_l && !std::isfinite(rays[i])) { set_error("sx_crossings: ray " + std::to_string(i) + ": a coordinate is NaN or Inf"); return 1; }
        if (h->has_z && !eval_height_ok(g, rays[(int64_t)(nrc - 1) * n_rays + i], why)) { set_error("sx_crossings: ray " + std::to_string(i) + ": " + why); return 1; }
    }
    if (n_rays == 0) return 0;

    // the profiles the planes need: (variable, kind), numbered in first-use order and grouped by variable
    ProfArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    CrossArgs ca;
    std::memset(&ca, 0, sizeof(ca));
    int nv = 0, nprof = 0;
    for (int j = 0; j < n_planes; j++) {
        int m = 0;
        while (h->slot[m] != planes[j][1]) m++;    // u r rr l ll z zz
        const int kind = m < 3 ? 0 : m - 2, var = planes[j][0] - 1;
        int v = 0;
        while (v < nv && pa.v[v].var != var) v++;
        if (v == nv) {
            pa.v[v].var = var;
            for (int k = 0; k < CROSS_KINDS; k++) pa.v[v].prof[k] = -1;
            nv++;
        }
        if (pa.v[v].prof[kind] < 0) pa.v[v].prof[kind] = nprof++;
        ca.pprof[j] = (uint8_t)pa.v[v].prof[kind];
        ca.pd[j] = (uint8_t)(m < 3 ? m : 0);
    }
    const EvalClasses *k = h->has_z ? eval_classes(h) : nullptr;
    if (h->has_z && !k) return 1;
    if (!h->diag[DIAG_CROSSINGS]) h->diag[DIAG_CROSSINGS].reset(new CrossState());
    CrossState *st = diag_state<CrossState>(h, DIAG_CROSSINGS);
    const int Zb = h->has_z ? h->Zb : 1, nz = h->has_z ? h->nz : 1, rows = h->nbt;
    for (int v = 0; v < nv; v++) pa.v[v].cls = k ? k->vcls[pa.v[v].var] : 0;

    const size_t n_ray = (size_t)std::max(nrc, 1) * n_rays, n_P = (size_t)std::max(nprof, 1) * rows * n_rays;
    const size_t n_rad = (size_t)max_cross * n_levels * n_rays, n_int = n_rad + (size_t)n_levels * n_rays + n_rays;
    if (!st->d_rays.grow(n_ray, who) || !st->d_P.grow(n_P, who) || !st->d_rad.grow(n_rad, who) || !st->d_i.grow(n_int, who)) return 1;
    std::vector<double> r0(n_ray, 0.0);
    if (nrc > 0) std::memcpy(r0.data(), rays, sizeof(double) * nrc * n_rays);
    if (h->has_l)                                  // a lambda outside [-2 pi, 2 pi] into (-pi, pi]
        for (int64_t i = 0; i < n_rays; i++)
            if (std::fabs(rays[i]) > 6.283185307179586) r0[i] = wrap_lambda(rays[i]);
    flush_diag(h);                                 // as for every reader of A
    HIPCHK(hipMemcpyAsync(st->d_rays, r0.data(), sizeof(double) * n_ray, hipMemcpyHostToDevice, h->stream));
    if (error_status()) return 1;

    pa.A = h->d_A; pa.w3 = k ? (const double *)k->d_w3 : nullptr; pa.rays = st->d_rays; pa.P = st->d_P;
    pa.C = h->C; pa.n_rays = (int)n_rays; pa.rows = rows; pa.row0 = h->cell0; pa.nprof = nprof;
    pa.Zb = Zb; pa.nz = nz; pa.K2 = h->K2; pa.kDim = h->kDim; pa.has_l = h->has_l; pa.has_z = h->has_z;
    pa.zmin = h->zmin; pa.zmax = h->zmax;
    // A columns of the variables named (the padding block left out) and the ray coordinates in, the profiles out
    if (nv > 0) {
        TimedLaunch scope(h, "k_ray_profiles", 8.0 * ((double)rows * Zb * (h->has_l ? 2 * h->kDim + 1 : 1) * nv + (double)nrc * n_rays + (double)rows * nprof * n_rays));
        hipLaunchKernelGGL(k_ray_profiles, dim3((unsigned)((rows + 15) / 16), (unsigned)((n_rays + 15) / 16), (unsigned)nv), dim3(64), prof_lds(h),
                           h->stream, pa);
    } else {
        set_kernel_bytes(h, "k_ray_profiles", 0.0);
    }

    ca.P = st->d_P; ca.radius = st->d_rad; ca.dir = st->d_i; ca.count = st->d_i + n_rad; ca.status = st->d_i + n_rad + (size_t)n_levels * n_rays;
    red_pack(ca.g, planes, n_planes, n_terms, coef, terms, 1);
    for (int j = 0; j < n_levels; j++) ca.level[j] = levels[j];
    ca.G = cross_geom(g);
    ca.wtol = (tol <= 0.0 ? 1e-9 : tol) * h->DX;
    ca.n_rays = (int)n_rays; ca.rows = rows; ca.nprof = nprof; ca.n_levels = n_levels;
    ca.max_iter = max_iter <= 0 ? 60 : max_iter; ca.max_cross = max_cross;
    // the profiles in; radii, directions, counts and status out
    {
        TimedLaunch scope(h, "k_crossings", 8.0 * (double)rows * nprof * n_rays + 12.0 * (double)n_rad + 4.0 * ((double)n_levels + 1.0) * n_rays);
        hipLaunchKernelGGL(k_crossings, dim3((unsigned)n_rays), dim3(64), 0, h->stream, ca);
    }

    std::vector<double> rr(n_rad), rp(profiles ? (size_t)nprof * rows * n_rays : 0);      // held back until the call has succeeded: a failed call writes nothing
    std::vector<int> ri(n_int);
    HIPCHK(hipMemcpyAsync(rr.data(), st->d_rad, sizeof(double) * n_rad, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ri.data(), st->d_i, sizeof(int) * n_int, hipMemcpyDeviceToHost, h->stream));
    if (!rp.empty()) HIPCHK(hipMemcpyAsync(rp.data(), st->d_P, sizeof(double) * rp.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (error_status()) return 1;
    std::memcpy(radius, rr.data(), sizeof(double) * n_rad);
    std::memcpy(dir, ri.data(), sizeof(int) * n_rad);
    std::memcpy(count, ri.data() + n_rad, sizeof(int) * n_levels * n_rays);
    std::memcpy(status, ri.data() + n_rad + (size_t)n_levels * n_rays, sizeof(int) * n_rays);
    if (!rp.empty()) std::memcpy(profiles, rp.data(), sizeof(double) * rp.size());
    return 0;
}

int sx_bracket_step(double *state, int32_t *flags, int32_t first, double fx, double width_tol, int32_t *status) {
    clear_error();
    if (!state || !flags || !status) { set_error("sx_bracket_step: null argument"); return 1; }
    if (!std::isfinite(width_tol)) { set_error("sx_bracket_step: width_tol is NaN or Inf"); return 1; }
    Bracket B;
    B.a = state[0]; B.fa = state[1]; B.b = state[2]; B.fb = state[3]; B.ga = state[4]; B.gb = state[5]; B.x = state[6];
    B.side = flags[0]; B.bis = flags[1];
    if (!std::isfinite(B.a) || !std::isfinite(B.b) || !(B.a <= B.b)) { set_error("sx_bracket_step: the bracket needs finite a <= b"); return 1; }
    if (B.fa != B.fa || B.fb != B.fb || ((B.fa < 0.0) == (B.fb < 0.0) && B.a < B.b)) { set_error("sx_bracket_step: d does not change sign over the bracket"); return 1; }
    if (!first && !(B.x >= B.a && B.x <= B.b)) { set_error("sx_bracket_step: the trial point lies outside the bracket"); return 1; }
    *status = first ? bracket_start(B, width_tol) : bracket_step(B, fx, width_tol);
    state[0] = B.a; state[1] = B.fa; state[2] = B.b; state[3] = B.fb; state[4] = B.ga; state[5] = B.gb; state[6] = B.x;
    flags[0] = B.side; flags[1] = B.bis;
    return 0;
}

}  // extern "C"
