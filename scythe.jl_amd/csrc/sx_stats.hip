// sx_stats_*: per-gridpoint statistics of field programs over time - swaths, means, totals, durations (include/scythe_hip.h,
// DESIGN.md 19).
//
// k_stats is a streaming kernel: per sample it reads the planes the program names once, and reads and writes two doubles per output
// and point.  It walks the ring pieces of the handle's scan table (sx_redprog.hpp) so that r is one value per ring, as in k_reduce / k_extrema /
// k_distribution; a piece is a contiguous run of points (the level fastest), which the threads of a workgroup take in order, W
// consecutive points (levels) per lane: W = 2 where zDim is even - every access of a plane or an accumulator is then 16 bytes per
// lane (8 for an fp32-stored plane) - else 1.  gridDim.y workgroups share a piece so that a launch has enough waves to keep loads in
// flight whatever the ring length.  Grids without an azimuth: lane = W consecutive points of the flat array.
// Per stride a lane loads every plane first, then, output by output with the output a compile-time index, the accumulator pair,
// forms q with red_output as ext_point does, updates the pair and stores it.  Nothing is summed across points: no atomics, no LDS, no
// cross-lane work, and a point's result cannot depend on which lane or workgroup took it.
#include "sx_redprog.hpp"
#include <cmath>
#include <cstring>
#include <limits>

namespace sx {

constexpr int STAT_WG_TARGET = 4096;      // workgroups of a launch aimed at: 16 per CU of the 256, 4 waves each
constexpr int STAT_HDR = 10;              // doubles of the blob before the program
constexpr double STAT_MAGIC = 5.7464e4;

struct StatProg {
    RedProg g;
    double thr[RED_OUT];
    int8_t op[RED_OUT];
};

// one sample of one output at one point: (a, b) is (hi, lo) or (value, time); what the header says of the four operations
__device__ inline void stat_update(int op, double q, double thr, double time, double w, bool first, double &a, double &b) {
    if (op == SX_STAT_SUM) {
        const double ph = w * q, pl = fma(w, q, -ph);
        dd_add(a, b, ph, pl);
    } else if (op == SX_STAT_DURATION) {
        if (q >= thr) dd_add(a, b, w);
    } else {
        const bool better = op == SX_STAT_MAX ? q > a : q < a;
        if (first || (a == a && (q != q || better))) { a = q; b = time; }
    }
}

// W consecutive points from pt, every output: acc [output][2][N]
template <class ST, int W>
__device__ inline void stat_points(const Planes<ST> &P, int V, int64_t N, int64_t pt, double r, const StatProg &sp, double *__restrict__ acc,
                                   double time, double w, bool first) {
    using VD = typename StatVec<W>::d;
    double val0[RED_PLANES], val1[RED_PLANES];      // one array per point: each stays in registers (val1 is not used when W = 1)
    stat_load_planes<ST, W>(P, V, N, pt, sp.g, val0, val1);
    const RedPow pw = red_pow(r);
#pragma unroll
    for (int o = 0; o < RED_OUT; o++) {
        if (o >= sp.g.n_out) continue;
        const int op = sp.op[o];
        if (w == 0.0 && (op == SX_STAT_SUM || op == SX_STAT_DURATION)) continue;      // the "extrema only" sample
        VD *pa = reinterpret_cast<VD *>(acc + (int64_t)(2 * o) * N + pt), *pb = reinterpret_cast<VD *>(acc + (int64_t)(2 * o + 1) * N + pt);
        const VD xa = *pa, xb = *pb;
        double q[W], a[W], b[W];
        red_output<W>(sp.g, o, val0, val1, pw, pw, q);
        a[0] = stat_lane(xa, 0); b[0] = stat_lane(xb, 0);
        stat_update(op, q[0], sp.thr[o], time, w, first, a[0], b[0]);
        if constexpr (W == 2) {
            a[1] = stat_lane(xa, 1); b[1] = stat_lane(xb, 1);
            stat_update(op, q[1], sp.thr[o], time, w, first, a[1], b[1]);
        }
        VD ya, yb;
        stat_pack(ya, a); stat_pack(yb, b);
        *pa = ya; *pb = yb;
    }
}

// RINGS: grid = (pieces, parts); the piece's nlam * nz points from (pstart[ring] + lam0) * nz are dealt to the parts x RED_T lanes, W each.
// !RINGS (every ring has one lambda): grid = ceil(N / (RED_T W)); lane = W consecutive points, which share a ring (W divides nz).
template <class ST, bool RINGS, int W>
__global__ __launch_bounds__(RED_T) void k_stats(Planes<ST> P, int V, int64_t N, int nz, const RedItem *__restrict__ items,
                                                 const int64_t *__restrict__ pstart, const double *__restrict__ rh, StatProg sp,
                                                 double *__restrict__ acc, double time, double w, int first) {
    if (RINGS) {
        const RedItem it = items[blockIdx.x];
        const int64_t h0 = pstart[it.ring], base = (h0 + it.lam0) * nz;
        const double r = rh[h0];
        const int n = it.nlam * nz;                       // a multiple of W
        for (int i = ((int)blockIdx.y * RED_T + (int)threadIdx.x) * W; i < n; i += (int)gridDim.y * RED_T * W)
            stat_points<ST, W>(P, V, N, base + i, r, sp, acc, time, w, first != 0);
    } else {
        const int64_t pt = ((int64_t)blockIdx.x * RED_T + threadIdx.x) * W;
        if (pt >= N) return;
        stat_points<ST, W>(P, V, N, pt, rh[pt / nz], sp, acc, time, w, first != 0);
    }
}

// the empty accumulators: (+0.0, +0.0) for SUM / DURATION, (NaN, NaN) for MAX / MIN
__global__ void k_stats_fill(double *__restrict__ acc, int64_t N, int n_out, StatProg sp) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * N * n_out) return;
    const int op = sp.op[e / (2 * N)];
    acc[e] = op == SX_STAT_MAX || op == SX_STAT_MIN ? __builtin_nan("") : 0.0;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct StatsState : DiagState {     // The work list: the handle's scan table (sx_redprog.hpp)
    int parts = 1;                  // workgroups per piece (stat_install)
    // the set
    DevBuf<double> d_acc;           // [n_out][2][N]
    int source = 0, n_terms = 0, n_out = 0, n_planes = 0;
    int32_t planes[RED_PLANES][2] = {};
    std::vector<double> coef;       // the program as it was given: what the blob carries
    std::vector<int32_t> terms;
    int32_t op[RED_OUT] = {};
    double thr[RED_OUT] = {};
    StatProg prog;
    // counters
    int64_t samples = 0;
    double el_hi = 0, el_lo = 0, t_first = 0, t_last = 0;
    void clear_counters() {
        samples = 0; el_hi = el_lo = 0.0;
        t_first = t_last = std::numeric_limits<double>::quiet_NaN();
    }
};

static StatsState *sstate(const sx_handle *h) { return diag_state<StatsState>(h, DIAG_STATS); }
static bool sum_like(int op) { return op == SX_STAT_SUM || op == SX_STAT_DURATION; }
static int stat_width(const sx_handle *h) { return h->has_z && h->nz % 2 == 0 ? 2 : 1; }

static void stat_fill(sx_handle *h, StatsState *st, double *acc) {
    const int64_t n = 2 * h->N * st->n_out;
    hipLaunchKernelGGL(k_stats_fill, grid1(n, 256), dim3(256), 0, h->stream, acc, h->N, st->n_out, st->prog);
    HIPCHK(hipGetLastError());
}

// what sx_stats_set and sx_stats_set_state refuse of a set (n_out >= 1), in the header's order; the planes of the program on success
static bool stat_args_ok(sx_handle *h, const char *who, int source, int n_terms, const double *coef, const int32_t *terms, int n_out,
                         const int32_t *op, const double *thr, int32_t (*planes)[2], int32_t *n_planes) {
    const sx_grid_desc gd = desc_of(h);
    if (!red_accept(who, &gd, source, n_terms, coef, terms, n_out, planes, n_planes)) return false;
    if (!op) { set_error(std::string(who) + ": null op with n_out > 0"); return false; }
    for (int o = 0; o < n_out; o++) {
        if (op[o] < SX_STAT_SUM || op[o] > SX_STAT_DURATION) {
            set_error(std::string(who) + ": op[" + std::to_string(o) + "] = " + std::to_string(op[o]) + " is none of SX_STAT_SUM, SX_STAT_MAX, SX_STAT_MIN, SX_STAT_DURATION");
            return false;
        }
        if (op[o] != SX_STAT_DURATION) continue;
        if (!thr) { set_error(std::string(who) + ": null threshold with a SX_STAT_DURATION output"); return false; }
        if (!std::isfinite(thr[o])) { set_error(std::string(who) + ": threshold[" + std::to_string(o) + "] of a SX_STAT_DURATION output is NaN or Inf"); return false; }
    }
    return true;
}

// make the state and the scan table; install the validated set with the accumulators `raw` (host, [n_out][2][N]) or empty.  All or
// nothing: a set that is there stays until the new one is complete
static bool stat_install(sx_handle *h, const char *who, int source, int n_terms, const double *coef, const int32_t *terms, int n_out,
                         const int32_t *op, const double *thr, const int32_t (*planes)[2], int n_planes, const double *raw) {
    if (!h->diag[DIAG_STATS]) h->diag[DIAG_STATS].reset(new StatsState());
    StatsState *st = sstate(h);
    const ScanGrid *sg = scan_grid(h, "sx_stats", false);
    if (!sg) return false;
    // workgroups per piece (a function of the grid alone): enough for STAT_WG_TARGET workgroups, never more than a piece has strides
    int longest = 1;
    for (const RedItem &it : sg->items) longest = std::max(longest, it.nlam * h->nz);
    const int strides = (longest + RED_T * stat_width(h) - 1) / (RED_T * stat_width(h));
    st->parts = std::max(1, std::min(strides, (STAT_WG_TARGET + sg->n_items - 1) / std::max(sg->n_items, 1)));
    const size_t n_acc = (size_t)2 * n_out * h->N;
    DevBuf<double> d_acc;
    if (!d_acc.alloc(n_acc)) {
        (void)hipGetLastError();
        set_error(std::string(who) + ": hipMalloc of " + std::to_string(n_acc * sizeof(double)) + " bytes for the accumulators failed");
        return false;
    }
    HIPCHK(hipStreamSynchronize(h->stream));      // a sample of the set that goes may still be in flight
    if (error_status()) return false;
    st->d_acc.swap(d_acc);                        // the set that goes is freed on return
    st->source = source; st->n_terms = n_terms; st->n_out = n_out; st->n_planes = n_planes;
    std::memcpy(st->planes, planes, sizeof(st->planes));
    st->coef.assign(coef, coef + n_terms);
    st->terms.assign(terms, terms + (size_t)n_terms * RED_TERM_W);
    std::memset(&st->prog, 0, sizeof(st->prog));
    red_pack(st->prog.g, planes, n_planes, n_terms, coef, terms, n_out);
    for (int o = 0; o < RED_OUT; o++) {
        st->op[o] = o < n_out ? op[o] : 0;
        st->thr[o] = o < n_out && op[o] == SX_STAT_DURATION ? thr[o] : 0.0;
        st->prog.op[o] = (int8_t)st->op[o]; st->prog.thr[o] = st->thr[o];
    }
    st->clear_counters();
    set_kernel_bytes(h, "k_stats", 0.0);      // the new set has taken no sample
    if (raw) {
        HIPCHK(hipMemcpyAsync(st->d_acc, raw, sizeof(double) * n_acc, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));      // raw is borrowed for the call only
    } else {
        stat_fill(h, st, st->d_acc);
    }
    return !error_status();
}

static void stat_drop(sx_handle *h) {
    StatsState *st = sstate(h);
    if (!st || st->n_out == 0) return;
    HIPCHK(hipStreamSynchronize(h->stream));
    st->d_acc.release();
    st->n_out = st->n_terms = st->n_planes = 0;
    st->coef.clear(); st->terms.clear();
    st->clear_counters();
    set_kernel_bytes(h, "k_stats", 0.0);
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_stats_set(sx_handle *h, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_out, const int32_t *op,
                 const double *threshold) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    if (n_out == 0) {
        stat_drop(h);
        return error_status();
    }
    int32_t planes[RED_PLANES][2] = {}, n_planes = 0;
    if (!stat_args_ok(h, "sx_stats_set", source, n_terms, coef, terms, n_out, op, threshold, planes, &n_planes)) return 1;
    return stat_install(h, "sx_stats_set", source, n_terms, coef, terms, n_out, op, threshold, planes, n_planes, nullptr) ? 0 : 1;
}

int sx_stats_reset(sx_handle *h) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    StatsState *st = sstate(h);
    if (!st || st->n_out == 0) return 0;
    stat_fill(h, st, st->d_acc);
    st->clear_counters();
    return error_status();
}

int sx_stats_accumulate(sx_handle *h, double time, double weight) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    if (!std::isfinite(time)) { set_error("sx_stats_accumulate: time is NaN or Inf"); return 1; }
    if (!std::isfinite(weight)) { set_error("sx_stats_accumulate: weight is NaN or Inf"); return 1; }
    StatsState *st = sstate(h);
    if (!st || st->n_out == 0) return 0;
    const ScanGrid *sg = scan_grid(h, "sx_stats", false);      // there since the set was installed
    if (!sg) return 1;
    {
        TimedLaunch scope(h, "k_stats", red_bytes(h, st->source, st->planes, st->n_planes) + 32.0 * st->n_out * (double)h->N);
        scan_dispatch(h, st->source, [&](auto st_t, auto rings, auto P) {
            constexpr bool RINGS = decltype(rings)::value;
            auto launch = [&](auto width) {
                constexpr int W = decltype(width)::value;
                const dim3 grid = RINGS ? dim3((unsigned)sg->n_items, (unsigned)st->parts) : dim3(scan_flat_blocks(h, W));
                hipLaunchKernelGGL((k_stats<decltype(st_t), RINGS, W>), grid, dim3(RED_T), 0, h->stream, P, h->V, h->N, h->nz, sg->d_items, h->d_pstart,
                                   h->d_r, st->prog, st->d_acc, time, weight, st->samples == 0 ? 1 : 0);
            };
            if (stat_width(h) == 2) launch(std::integral_constant<int, 2>());
            else launch(std::integral_constant<int, 1>());
        });
    }
    if (error_status()) return 1;
    if (st->samples == 0) st->t_first = time;
    st->t_last = time;
    st->samples++;
    const double s = st->el_hi + weight, b = s - st->el_hi;        // the two-sum of dd_add, on the host
    st->el_lo += (st->el_hi - (s - b)) + (weight - b);
    st->el_hi = s;
    return 0;
}

int sx_stats_get(sx_handle *h, double *out, double *info) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    StatsState *st = sstate(h);
    if (!st || st->n_out == 0) { set_error("sx_stats_get: the handle has no statistics set"); return 1; }
    if (!out) { set_error("sx_stats_get: null out"); return 1; }
    const size_t N = (size_t)h->N;
    for (int o = 0; o < st->n_out; o++)
        for (int s = 0; s < 2; s++)
            HIPCHK(hipMemcpyAsync(out + ((size_t)s * st->n_out + o) * N, st->d_acc + ((size_t)2 * o + s) * N, sizeof(double) * N,
                                  hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (error_status()) return 1;
    for (int o = 0; o < st->n_out; o++) {          // the copy's slot 0 of a sum is hi + lo; the stored pair stays a pair
        if (!sum_like(st->op[o])) continue;
        double *hi = out + (size_t)o * N;
        const double *lo = out + ((size_t)st->n_out + o) * N;
        for (size_t i = 0; i < N; i++) hi[i] = hi[i] + lo[i];
    }
    if (info) { info[0] = (double)st->samples; info[1] = st->el_hi; info[2] = st->el_lo; info[3] = st->t_first; info[4] = st->t_last; }
    return 0;
}

int sx_stats_describe(const sx_handle *h, int32_t *source, int32_t *n_out, int32_t *op, double *threshold) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    const StatsState *st = sstate(h);
    const int n = st ? st->n_out : 0;
    if (n_out) *n_out = n;
    if (n == 0) return 0;
    if (source) *source = st->source;
    for (int o = 0; o < n; o++) {
        if (op) op[o] = st->op[o];
        if (threshold) threshold[o] = st->thr[o];
    }
    return 0;
}

// blob: [magic, N, source, n_terms, n_out, samples, elapsed hi, lo, first time, last time][coef [n_terms]][terms [n_terms][11]][op [n_out]]
// [threshold [n_out]][acc [n_out][2][N]]
int sx_stats_state_size(const sx_handle *h, int64_t *n_doubles) {
    clear_error();
    if (!h || !n_doubles) { set_error("null argument"); return 1; }
    const StatsState *st = sstate(h);
    *n_doubles = st && st->n_out ? STAT_HDR + (int64_t)(1 + RED_TERM_W) * st->n_terms + 2 * st->n_out + 2 * (int64_t)st->n_out * h->N : 0;
    return 0;
}

int sx_stats_get_state(sx_handle *h, double *out) {
    clear_error();
    if (!h || !out) { set_error("null argument"); return 1; }
    StatsState *st = sstate(h);
    if (!st || st->n_out == 0) { set_error("sx_stats_get_state: the handle has no statistics set"); return 1; }
    double *p = out;
    *p++ = STAT_MAGIC; *p++ = (double)h->N; *p++ = (double)st->source; *p++ = (double)st->n_terms; *p++ = (double)st->n_out;
    *p++ = (double)st->samples; *p++ = st->el_hi; *p++ = st->el_lo; *p++ = st->t_first; *p++ = st->t_last;
    for (int t = 0; t < st->n_terms; t++) *p++ = st->coef[t];
    for (size_t q = 0; q < st->terms.size(); q++) *p++ = (double)st->terms[q];
    for (int o = 0; o < st->n_out; o++) *p++ = (double)st->op[o];
    for (int o = 0; o < st->n_out; o++) *p++ = st->thr[o];
    HIPCHK(hipMemcpyAsync(p, st->d_acc, sizeof(double) * 2 * st->n_out * (size_t)h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return error_status();
}

int sx_stats_set_state(sx_handle *h, const double *in, int64_t n_doubles) {
    clear_error();
    if (!h || !in) { set_error("null argument"); return 1; }
    const char *bad = "sx_stats_set_state: the blob does not belong to a handle with these dimensions";
    if (n_doubles < STAT_HDR || in[0] != STAT_MAGIC || in[1] != (double)h->N) { set_error(bad); return 1; }
    if (!(in[3] >= 0.0 && in[3] <= RED_TERMS) || !(in[4] >= 1.0 && in[4] <= RED_OUT) || !(in[5] >= 0.0 && in[5] <= 9.0e15)) { set_error(bad); return 1; }
    const int source = (int)in[2], n_terms = (int)in[3], n_out = (int)in[4];
    const int64_t samples = (int64_t)in[5];
    if ((double)source != in[2] || (double)n_terms != in[3] || (double)n_out != in[4] || (double)samples != in[5]) { set_error(bad); return 1; }
    if (n_doubles != STAT_HDR + (int64_t)(1 + RED_TERM_W) * n_terms + 2 * n_out + 2 * (int64_t)n_out * h->N) { set_error(bad); return 1; }
    const double *coef = in + STAT_HDR, *pt = coef + n_terms, *po = pt + (size_t)n_terms * RED_TERM_W, *thr = po + n_out, *raw = thr + n_out;
    std::vector<int32_t> terms((size_t)n_terms * RED_TERM_W);
    int32_t op[RED_OUT] = {};
    for (size_t q = 0; q < terms.size(); q++) {
        if (!(pt[q] >= -2147483648.0 && pt[q] <= 2147483647.0) || (double)(int32_t)pt[q] != pt[q]) { set_error(bad); return 1; }
        terms[q] = (int32_t)pt[q];
    }
    for (int o = 0; o < n_out; o++) {
        if (!(po[o] >= 0.0 && po[o] <= 3.0) || (double)(int32_t)po[o] != po[o]) { set_error(bad); return 1; }
        op[o] = (int32_t)po[o];
    }
    if (!std::isfinite(in[6]) || !std::isfinite(in[7]) || (samples > 0 && (!std::isfinite(in[8]) || !std::isfinite(in[9])))) { set_error(bad); return 1; }
    int32_t planes[RED_PLANES][2] = {}, n_planes = 0;
    if (!stat_args_ok(h, "sx_stats_set_state", source, n_terms, coef, terms.data(), n_out, op, thr, planes, &n_planes)) return 1;
    if (!stat_install(h, "sx_stats_set_state", source, n_terms, coef, terms.data(), n_out, op, thr, planes, n_planes, raw)) return 1;
    StatsState *st = sstate(h);
    st->samples = samples; st->el_hi = in[6]; st->el_lo = in[7];
    if (samples > 0) { st->t_first = in[8]; st->t_last = in[9]; }
    return 0;
}

}  // extern "C"
