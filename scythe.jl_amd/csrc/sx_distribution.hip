// sx_distribution / sx_distribution_slot / sx_distribution_check: histograms of field programs - how much of the domain holds which
// values (include/scythe_hip.h).
//
// k_distribution streams the planes a program names exactly as k_reduce does (sx_redprog.hpp: a thread keeps ONE level and strides over
// the lambdas of a ring piece; grids without an azimuth: thread = point), forms output 0 - the binned quantity q - in plain fp64 as
// k_extrema forms an output, finds its slot by comparisons against the edges (dist_slot, the function sx_distribution_slot runs on the
// host), and forms the point's contributions: the weight itself (the measure) and, per integrand, sum_terms weight * term with the
// product unrounded (fma) in double-double.  A FIXED number of workgroups each walk a contiguous run of the work list and keep their
// bins in LDS, so the scratch in HBM is workgroups x bins and does not grow with the grid:
//   SX_DIST_DOMAIN  bins per wave [slot][output].  Per batch of 64 points a wave loops over the distinct slots present (ballot); the
//                   lanes of one slot are added in a fixed lane tree (the other lanes enter as zero), lane 0 adds the result to the
//                   wave's bins.  At the end the waves are added in wave order.
//   SX_DIST_LEVEL   bins per workgroup [level][slot][output].  Lanes of a wave that share a level are lane / zDim apart and take turns
//                   in that order; the waves take turns in wave order (a barrier each).  No two lanes ever touch one bin at once.
// k_distribution_final adds the workgroups' bins in block order (8 runs of blocks side by side, then the runs in order).  Counts are
// integers; no sum is formed atomically: which lane adds what, and in which order, follows from the grid, n_bins and the slots the data
// falls into, so two calls on the same data agree bitwise.
#include "sx_redprog.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

constexpr int DIST_OUT = 4, DIST_BINS = 64;
constexpr int DIST_WG = 512;              // workgroups of k_distribution at most: two per CU of the 256
constexpr int DIST_PARTS = 8;             // runs of workgroups k_distribution_final adds side by side
constexpr int DIST_FE = 32;               // bins per workgroup of k_distribution_final
constexpr size_t DIST_LDS_MAX = 160 * 1024;   // the LDS of one CU: above 64 KB one workgroup per CU

// The slot of q among n_bins + 3: 0 underflow, 1 + b for edges[b] <= q < edges[b + 1], n_bins + 1 overflow, n_bins + 2 NaN.  The
// number of edges <= q, by bisection with exact comparisons (-0.0 == 0.0; -inf below every edge, +inf above).
__host__ __device__ inline int dist_slot(int n_bins, const double *edges, double q) {
    if (q != q) return n_bins + 2;
    int lo = 0, hi = n_bins + 1;          // edges[lo - 1] <= q < edges[hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct DistArgs {
    const RedItem *items;                 // ring pieces (grids with an azimuth)
    const int64_t *pstart;
    const double *rh, *wrl, *wz, *edges;  // radius per horizontal point, w_r w_l per ring, w_z per level, [n_bins + 1]
    double2 *part;                        // [workgroup][group][slot][output] (hi, lo)
    unsigned *pcnt;                       // [workgroup][group][slot]
    int64_t N, n_work;                    // points; ring pieces, or runs of RED_T points
    int V, nz, n_bins, level;             // level: bins per level (SX_DIST_LEVEL on a grid with a vertical)
};

// One point: its slot and its contributions (hi, lo)[output]: [0] the weight, [j] the integrand j times the weight
template <class ST>
__device__ inline int dist_point(const Planes<ST> &P, int V, int64_t N, int64_t pt, double r, double w, const RedProg &g, int n_bins,
                                 const double *edges, double (&hi)[DIST_OUT], double (&lo)[DIST_OUT]) {
    double val[RED_PLANES];
    red_load_planes<ST>(P, V, N, pt, g, val);
    const RedPow pw = red_pow(r);
    const double q = red_output(g, 0, val, pw);
    hi[0] = w; lo[0] = 0.0;
#pragma unroll
    for (int o = 1; o < DIST_OUT; o++) {
        hi[o] = lo[o] = 0.0;
        for (int t = g.start[o]; t < g.start[o + 1]; t++) {       // empty at o >= n_out
            const double x = red_term(g, t, val, pw);
            const double ph = w * x, pl = fma(w, x, -ph);
            dd_add(hi[o], lo[o], ph, pl);
        }
    }
    return dist_slot(n_bins, edges, q);
}

// SX_DIST_DOMAIN: the wave's 64 points into the wave's bins tab [slot][output], cnt [slot]
__device__ inline void dist_add_wave(bool valid, int slot, const double (&hi)[DIST_OUT], const double (&lo)[DIST_OUT], int n_out, int lane,
                                     double2 *tab, unsigned *cnt) {
    unsigned long long todo = __ballot(valid);
    while (todo) {                                                // uniform: every lane holds the same mask
        const int s = __shfl(slot, __ffsll((long long)todo) - 1);
        const bool mine = valid && slot == s;
        const unsigned long long m = __ballot(mine);
#pragma unroll
        for (int o = 0; o < DIST_OUT; o++) {
            if (o >= n_out) continue;
            double a = mine ? hi[o] : 0.0, b = mine ? lo[o] : 0.0;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {             // lane 0 ends with the tree ((0 + 32) + (16 + 48)) + ...
                const double xa = __shfl_down(a, off), xb = __shfl_down(b, off);
                dd_add(a, b, xa, xb);
            }
            if (lane == 0) {
                double2 t = tab[s * n_out + o];
                dd_add(t.x, t.y, a, b);
                tab[s * n_out + o] = t;
            }
        }
        if (lane == 0) cnt[s] += (unsigned)__popcll(m);
        todo &= ~m;
    }
}

// SX_DIST_LEVEL: the workgroup's points into its bins tab [level][slot][output], cnt [level][slot].  Lanes of a wave with one level are
// zDim lanes apart: they take turns by lane / zDim, the waves by their number.
__device__ inline void dist_add_level(bool valid, int z, int slot, const double (&hi)[DIST_OUT], const double (&lo)[DIST_OUT], int n_out, int S,
                                      int nz, int lane, int wave, int nwaves, double2 *tab, unsigned *cnt) {
    const int turn = lane / nz, turns = (63 + nz) / nz;
    for (int w = 0; w < nwaves; w++) {
        if (wave == w) {
            for (int k = 0; k < turns; k++) {
                if (valid && turn == k) {
                    const int e = z * S + slot;
                    cnt[e] += 1u;
#pragma unroll
                    for (int o = 0; o < DIST_OUT; o++) {
                        if (o >= n_out) continue;
                        double2 t = tab[e * n_out + o];
                        dd_add(t.x, t.y, hi[o], lo[o]);
                        tab[e * n_out + o] = t;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // turn k's bins are written before turn k + 1 reads them
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
    }
}

// grid = workgroups (<= DIST_WG); workgroup b takes the work items [n_work b / grid, n_work (b + 1) / grid).
// RINGS: an item is a ring piece; a thread's level is tid % nz, its first lambda lam0 + tid / nz, its stride RED_T / nz lambdas.
// !RINGS (every ring has one lambda): an item is a run of RED_T points; thread = point.
// LDS: tab [tables][groups S n_out] double2 | edges [n_bins + 1] | cnt [tables][groups S]; tables = waves (domain) or 1 (level)
template <class ST, bool RINGS>
__global__ __launch_bounds__(RED_T) void k_distribution(Planes<ST> P, DistArgs a, RedProg g) {
    extern __shared__ double2 dist_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = RED_T / 64;
    const int nz = a.nz, S = a.n_bins + 3, n_out = g.n_out, groups = a.level ? nz : 1, tables = a.level ? 1 : nwaves;
    const int EC = groups * S, E = EC * n_out;
    double2 *tab = dist_lds;
    double *edges = reinterpret_cast<double *>(tab + (size_t)tables * E);
    unsigned *cnt = reinterpret_cast<unsigned *>(edges + a.n_bins + 1);
    for (int e = tid; e < tables * E; e += RED_T) tab[e] = make_double2(0.0, 0.0);
    for (int e = tid; e < tables * EC; e += RED_T) cnt[e] = 0u;
    for (int e = tid; e <= a.n_bins; e += RED_T) edges[e] = a.edges[e];
    __syncthreads();
    double2 *wtab = tab + (a.level ? 0 : wave * E);
    unsigned *wcnt = cnt + (a.level ? 0 : wave * EC);

    const int64_t w0 = a.n_work * blockIdx.x / gridDim.x, w1 = a.n_work * (blockIdx.x + 1) / gridDim.x;
    double hi[DIST_OUT], lo[DIST_OUT];
    if (RINGS) {
        const int G = RED_T / nz, z = tid % nz, gl = tid / nz;
        const double wzz = a.level ? 1.0 : a.wz[z];
        for (int64_t i = w0; i < w1; i++) {
            const RedItem it = a.items[i];
            const int64_t h0 = a.pstart[it.ring];
            const double r = a.rh[h0], wr = a.wrl[it.ring];
            const double w = a.level ? wr : wr * wzz;
            for (int l0 = it.lam0; l0 < it.lam0 + it.nlam; l0 += G) {      // uniform trip count: the bins are shared
                const bool valid = gl < G && l0 + gl < it.lam0 + it.nlam;
                int slot = 0;
                if (valid) slot = dist_point<ST>(P, a.V, a.N, (h0 + l0 + gl) * nz + z, r, w, g, a.n_bins, edges, hi, lo);
                if (a.level) dist_add_level(valid, z, slot, hi, lo, n_out, S, nz, lane, wave, nwaves, wtab, wcnt);
                else dist_add_wave(valid, slot, hi, lo, n_out, lane, wtab, wcnt);
            }
        }
    } else {
        for (int64_t i = w0; i < w1; i++) {
            const int64_t pt = i * RED_T + tid;
            const bool valid = pt < a.N;
            int slot = 0, z = 0;
            if (valid) {
                const int64_t ring = pt / nz;
                z = (int)(pt - ring * nz);
                const double wr = a.wrl[ring];
                slot = dist_point<ST>(P, a.V, a.N, pt, a.rh[ring], a.level ? wr : wr * a.wz[z], g, a.n_bins, edges, hi, lo);
            }
            if (a.level) dist_add_level(valid, z, slot, hi, lo, n_out, S, nz, lane, wave, nwaves, wtab, wcnt);
            else dist_add_wave(valid, slot, hi, lo, n_out, lane, wtab, wcnt);
        }
    }
    __syncthreads();
    // the workgroup's bins: the waves' in wave order (domain), or the table as it is (level)
    for (int e = tid; e < E; e += RED_T) {
        double2 t = tab[e];
        for (int w = 1; w < tables; w++) dd_add(t.x, t.y, tab[w * E + e].x, tab[w * E + e].y);
        a.part[(int64_t)blockIdx.x * E + e] = t;
    }
    for (int e = tid; e < EC; e += RED_T) {
        unsigned c = cnt[e];
        for (int w = 1; w < tables; w++) c += cnt[w * EC + e];
        a.pcnt[(int64_t)blockIdx.x * EC + e] = c;
    }
}

// grid = ceil(E / DIST_FE); thread = (bin e = (group S + slot) n_out + output, run p of DIST_PARTS): run p adds the workgroups
// [nwg p / 8, nwg (p + 1) / 8) in block order, then the runs are added in order.  sums [slot, output, group], count [slot, group]
// column-major.
__global__ __launch_bounds__(DIST_FE * DIST_PARTS) void k_distribution_final(const double2 *__restrict__ part, const unsigned *__restrict__ pcnt,
                                                                             int nwg, int groups, int S, int n_out, double *__restrict__ sums,
                                                                             unsigned long long *__restrict__ count) {
    __shared__ double s_hi[DIST_FE * DIST_PARTS], s_lo[DIST_FE * DIST_PARTS];
    __shared__ unsigned long long s_c[DIST_FE * DIST_PARTS];
    const int tid = threadIdx.x, el = tid % DIST_FE, p = tid / DIST_FE;
    const int EC = groups * S, E = EC * n_out, e = blockIdx.x * DIST_FE + el;
    const int k0 = (int)((int64_t)nwg * p / DIST_PARTS), k1 = (int)((int64_t)nwg * (p + 1) / DIST_PARTS);
    double a = 0.0, b = 0.0;
    unsigned long long c = 0;
    for (int k = k0; k < k1; k++) {
        if (e < E) { const double2 x = part[(int64_t)k * E + e]; dd_add(a, b, x.x, x.y); }
        if (e < EC) c += pcnt[(int64_t)k * EC + e];
    }
    s_hi[tid] = a; s_lo[tid] = b; s_c[tid] = c;
    __syncthreads();
    if (p != 0) return;
    for (int q = 1; q < DIST_PARTS; q++) {
        dd_add(a, b, s_hi[q * DIST_FE + el], s_lo[q * DIST_FE + el]);
        c += s_c[q * DIST_FE + el];
    }
    if (e < E) {
        const int o = e % n_out, s = e / n_out % S, gr = e / n_out / S;
        sums[s + (int64_t)S * (o + (int64_t)n_out * gr)] = a + b;
    }
    if (e < EC) count[e % S + (int64_t)S * (e / S)] = c;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct DistState : DiagState {      // the work list and the weights: the handle's scan table (sx_redprog.hpp)
    DevBuf<double> d_edges;         // [DIST_BINS + 1]
    DevBuf<double2> d_part;
    DevBuf<unsigned> d_pcnt;
    DevBuf<double> d_sums;
    DevBuf<unsigned long long> d_count;
};

static DistState *dist_state(sx_handle *h) {
    if (h->diag[DIAG_DISTRIBUTION]) return diag_state<DistState>(h, DIAG_DISTRIBUTION);
    std::unique_ptr<DistState> st(new DistState());
    if (!st->d_edges.upload(std::vector<double>(DIST_BINS + 1, 0.0), "sx_distribution: hipMalloc / hipMemcpy of the work list failed")) return nullptr;
    h->diag[DIAG_DISTRIBUTION] = std::move(st);
    return diag_state<DistState>(h, DIAG_DISTRIBUTION);
}

// LDS of one workgroup of k_distribution
static size_t dist_lds_bytes(int groups, int tables, int n_bins, int n_out) {
    return (size_t)tables * groups * (n_bins + 3) * (16 * (size_t)n_out + 4) + 8 * (size_t)(n_bins + 1);
}

// what sx_distribution and sx_distribution_check refuse of a call, in the header's order; the planes of the program on success
static bool dist_args_ok(const sx_grid_desc *gd, int kind, int source, int n_terms, const int32_t *terms, int n_out, int n_bins,
                         const double *edges, int32_t (*planes)[2], int32_t *n_planes) {
    if (sx_reduce_planes(gd, source, n_terms, terms, n_out, &planes[0][0], n_planes)) return false;
    if (n_out < 1 || n_out > DIST_OUT) { set_error("sx_distribution: n_out must be 1 .. 4 (output 0 is binned, 1 .. 3 are integrands)"); return false; }
    if (n_bins < 1 || n_bins > DIST_BINS) { set_error("sx_distribution: n_bins must be 1 .. 64"); return false; }
    if (!edges) { set_error("sx_distribution: null edges"); return false; }
    for (int b = 0; b <= n_bins; b++) {
        if (!std::isfinite(edges[b])) { set_error("sx_distribution: edge " + std::to_string(b) + " is NaN or Inf"); return false; }
        if (b > 0 && !(edges[b] > edges[b - 1])) { set_error("sx_distribution: edge " + std::to_string(b) + " is not above edge " + std::to_string(b - 1)); return false; }
    }
    if (kind != SX_DIST_DOMAIN && kind != SX_DIST_LEVEL) { set_error("sx_distribution: kind must be SX_DIST_DOMAIN or SX_DIST_LEVEL"); return false; }
    const bool has_z = gd->geometry == SX_GEOM_RZ || gd->geometry == SX_GEOM_RLZ;
    if (kind == SX_DIST_LEVEL && has_z && dist_lds_bytes(gd->zDim, 1, n_bins, n_out) > DIST_LDS_MAX) {
        set_error("sx_distribution: SX_DIST_LEVEL keeps zDim (n_bins + 3) (16 n_out + 4) + 8 (n_bins + 1) = " +
                  std::to_string(dist_lds_bytes(gd->zDim, 1, n_bins, n_out)) + " bytes of bins in the LDS of one workgroup; the limit is 163840");
        return false;
    }
    return true;
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_distribution_slot(int32_t n_bins, const double *edges, double q, int32_t *slot) {
    clear_error();
    if (!edges || !slot) { set_error("sx_distribution_slot: null argument"); return 1; }
    if (n_bins < 1 || n_bins > DIST_BINS) { set_error("sx_distribution_slot: n_bins must be 1 .. 64"); return 1; }
    for (int b = 0; b <= n_bins; b++)
        if (!std::isfinite(edges[b]) || (b > 0 && !(edges[b] > edges[b - 1]))) {
            set_error("sx_distribution_slot: edge " + std::to_string(b) + " is NaN / Inf or not above its predecessor");
            return 1;
        }
    *slot = dist_slot(n_bins, edges, q);
    return 0;
}

int sx_distribution_check(const sx_grid_desc *gd, int32_t kind, int32_t source, int32_t n_terms, const int32_t *terms, int32_t n_out,
                          int32_t n_bins, const double *edges) {
    clear_error();
    if (!desc_ok(gd, "sx_distribution_check")) return 1;
    int32_t planes[RED_PLANES][2], n_planes = 0;
    return dist_args_ok(gd, kind, source, n_terms, terms, n_out, n_bins, edges, planes, &n_planes) ? 0 : 1;
}

int sx_distribution(sx_handle *h, int32_t kind, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_out,
                    int32_t n_bins, const double *edges, int64_t *count, double *sums) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    const sx_grid_desc gd = desc_of(h);
    int32_t planes[RED_PLANES][2], n_planes = 0;
    if (!dist_args_ok(&gd, kind, source, n_terms, terms, n_out, n_bins, edges, planes, &n_planes)) return 1;
    if (!red_coef_ok("sx_distribution", n_terms, coef)) return 1;
    if (!count || !sums) { set_error("sx_distribution: null count or sums"); return 1; }
    ScanGrid *sg = scan_grid(h, "sx_distribution", true);
    DistState *st = sg ? dist_state(h) : nullptr;
    if (!st) return 1;

    RedProg prog;
    red_pack(prog, planes, n_planes, n_terms, coef, terms, n_out);

    const int level = kind == SX_DIST_LEVEL && h->has_z, groups = level ? h->nz : 1, S = n_bins + 3;
    const int64_t n_work = h->has_l ? sg->n_items : scan_flat_blocks(h);
    const int nwg = (int)std::min<int64_t>(DIST_WG, std::max<int64_t>(1, n_work));
    const size_t EC = (size_t)groups * S, E = EC * n_out;
    if (!st->d_part.grow((size_t)nwg * E, "sx_distribution") || !st->d_pcnt.grow((size_t)nwg * EC, "sx_distribution") ||
        !st->d_sums.grow(E, "sx_distribution") || !st->d_count.grow(EC, "sx_distribution"))
        return 1;
    HIPCHK(hipMemcpyAsync(st->d_edges, edges, sizeof(double) * (n_bins + 1), hipMemcpyHostToDevice, h->stream));
    if (error_status()) return 1;

    DistArgs a;
    a.items = sg->d_items; a.pstart = h->d_pstart; a.rh = h->d_r; a.wrl = sg->d_wrl; a.wz = sg->d_wz; a.edges = st->d_edges;
    a.part = st->d_part; a.pcnt = st->d_pcnt;
    a.N = h->N; a.n_work = n_work; a.V = h->V; a.nz = h->nz; a.n_bins = n_bins; a.level = level;
    const size_t lds = dist_lds_bytes(groups, level ? 1 : RED_T / 64, n_bins, n_out);
    {
        TimedLaunch scope(h, "k_distribution", red_bytes(h, source, planes, n_planes));
        scan_dispatch(h, source, [&](auto st_t, auto rings, auto P) {
            const auto kern = k_distribution<decltype(st_t), decltype(rings)::value>;
            if (lds > 65536) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(RED_T), lds, h->stream, P, a, prog);
        });
    }
    {
        TimedLaunch scope(h, "k_distribution_final", 0.0);
        hipLaunchKernelGGL(k_distribution_final, grid1((int64_t)E, DIST_FE), dim3(DIST_FE * DIST_PARTS), 0, h->stream, st->d_part, st->d_pcnt, nwg,
                           groups, S, n_out, st->d_sums, st->d_count);
    }
    std::vector<double> rs(E);           // held back until the call has succeeded: a failed call writes nothing
    std::vector<unsigned long long> rc(EC);
    HIPCHK(hipMemcpyAsync(rs.data(), st->d_sums, sizeof(double) * E, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(rc.data(), st->d_count, sizeof(unsigned long long) * EC, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (error_status()) return 1;
    std::memcpy(sums, rs.data(), sizeof(double) * E);
    for (size_t q = 0; q < EC; q++) count[q] = (int64_t)rc[q];
    return 0;
}

}  // extern "C"
