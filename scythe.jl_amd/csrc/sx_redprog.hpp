// What the entry points that evaluate a field program at every gridpoint of a tile share - sx_reduce, sx_extrema, sx_distribution,
// sx_stats_*, sx_project and sx_derive (sx_<name>.hip): the program as the kernels read it and its acceptance, the loads of the planes it names and its outputs at one point, the scan table of a handle (work list and weights) and the choice of the kernel
// instantiation.  The walk of a ring piece stays written out in each kernel: as a helper that takes the body as a lambda, the
// program and the accumulators the body captures went to scratch.
#pragma once
#include "sx_internal.hpp"
#include <cstring>
#include <type_traits>

namespace sx {

constexpr int RED_T = 256;          // threads per workgroup of the scan kernels
constexpr int RED_ITERS = 32;       // strides of a workgroup over its piece of a ring: pieces per ring = ceil(strides / RED_ITERS)
constexpr int RED_TERMS = 64, RED_OUT = 16, RED_PLANES = 16, RED_FACTORS = 4, RED_TERM_W = 11;

struct RedProg {
    double coef[RED_TERMS];
    int8_t p[RED_TERMS], nf[RED_TERMS];
    uint8_t f[RED_TERMS][RED_FACTORS];      // plane of each factor
    uint8_t start[RED_OUT + 1];             // terms of output o: [start[o], start[o + 1])
    uint8_t pvar[RED_PLANES], pslot[RED_PLANES];   // 0-based variable, slot
    int n_planes, n_out;
};

struct RedItem { int ring, lam0, nlam, pad; };

// the planes of the program at one point, widened to fp64 (a derivative slot is read in the type it is stored in)
template <class ST>
__device__ inline void red_load_planes(const Planes<ST> &P, int V, int64_t N, int64_t pt, const RedProg &g, double (&val)[RED_PLANES]) {
#pragma unroll
    for (int j = 0; j < RED_PLANES; j++) {
        val[j] = 0.0;
        if (j < g.n_planes) {
            const int v = g.pvar[j], s = g.pslot[j];
            val[j] = s == 0 ? P.val[(int64_t)v * N + pt] : (double)P.der[((int64_t)(s - 1) * V + v) * N + pt];
        }
    }
}

// W consecutive points per lane: one 16-byte access of an fp64 plane (8 of an fp32-stored one) where W = 2
template <int W> struct StatVec;
template <> struct StatVec<1> { using d = double; using f = float; };
template <> struct StatVec<2> { using d = double2; using f = float2; };
__device__ inline double stat_lane(double v, int) { return v; }
__device__ inline double stat_lane(float v, int) { return (double)v; }
__device__ inline double stat_lane(const double2 &v, int k) { return k ? v.y : v.x; }
__device__ inline double stat_lane(const float2 &v, int k) { return (double)(k ? v.y : v.x); }
__device__ inline void stat_pack(double &o, const double (&a)[1]) { o = a[0]; }
__device__ inline void stat_pack(double2 &o, const double (&a)[2]) { o = make_double2(a[0], a[1]); }

// red_load_planes W points wide (k_stats, k_project): the planes of the program at W consecutive points from pt (a multiple of W), one access per plane
template <class ST, int W>
__device__ inline void stat_load_planes(const Planes<ST> &P, int V, int64_t N, int64_t pt, const RedProg &g, double (&val0)[RED_PLANES],
                                        double (&val1)[RED_PLANES]) {
    using VD = typename StatVec<W>::d;
    using VS = typename std::conditional<std::is_same<ST, float>::value, typename StatVec<W>::f, VD>::type;
#pragma unroll
    for (int j = 0; j < RED_PLANES; j++) {
        val0[j] = val1[j] = 0.0;
        if (j < g.n_planes) {
            const int v = g.pvar[j], s = g.pslot[j];
            if (s == 0) {
                const VD x = *reinterpret_cast<const VD *>(P.val + (int64_t)v * N + pt);
                val0[j] = stat_lane(x, 0);
                if (W == 2) val1[j] = stat_lane(x, 1);
            } else {
                const VS x = *reinterpret_cast<const VS *>(P.der + ((int64_t)(s - 1) * V + v) * N + pt);
                val0[j] = stat_lane(x, 0);
                if (W == 2) val1[j] = stat_lane(x, 1);
            }
        }
    }
}

// the powers of r a term may name: r, r^2, 1 / r, 1 / r^2
struct RedPow { double r, rr, ri, rri; };
__host__ __device__ inline RedPow red_pow(double r) {
    const double rr = r * r;
    return RedPow{r, rr, 1.0 / r, 1.0 / rr};
}

// term t at a point: coef r^p prod field, the factors in the program's order (also on the host: sx_project_point)
__host__ __device__ inline double red_term(const RedProg &g, int t, const double (&val)[RED_PLANES], const RedPow &pw) {
    const int p = g.p[t], nf = g.nf[t];
    const double r = pw.r, rr = pw.rr, ri = pw.ri, rri = pw.rri;      // values, so that the choice below compiles to selects, not branches
    double x = g.coef[t];
    if (p != 0) x *= p == 1 ? r : p == 2 ? rr : p == -1 ? ri : rri;
#pragma unroll
    for (int f = 0; f < RED_FACTORS; f++)
        if (f < nf) x *= val[g.f[t][f]];
    return x;
}

// output o at a point: the sum of its terms in term order, plain fp64 (0 at o >= n_out: no terms)
__host__ __device__ __forceinline__ double red_output(const RedProg &g, int o, const double (&val)[RED_PLANES], const RedPow &pw) {
    double q = 0.0;
    for (int t = g.start[o]; t < g.start[o + 1]; t++) q += red_term(g, t, val, pw);
    return q;
}
// ... at the W points of stat_load_planes: one pass over the terms serves both points
template <int W>
__device__ __forceinline__ void red_output(const RedProg &g, int o, const double (&val0)[RED_PLANES], const double (&val1)[RED_PLANES], const RedPow &pw0,
                                           const RedPow &pw1, double (&q)[W]) {
    q[0] = 0.0;
    if constexpr (W == 2) q[1] = 0.0;
    for (int t = g.start[o]; t < g.start[o + 1]; t++) {
        q[0] += red_term(g, t, val0, pw0);
        if constexpr (W == 2) q[1] += red_term(g, t, val1, pw1);
    }
}

// the double-double sums of sx_reduce and sx_distribution: (hi, lo) += x, the rounding error of the sum kept in lo (Knuth's two-sum: no ordering of |hi|, |x| assumed)
__device__ inline void dd_add(double &hi, double &lo, double x) {
    const double s = hi + x, b = s - hi;
    lo += (hi - (s - b)) + (x - b);
    hi = s;
}
__device__ inline void dd_add(double &hi, double &lo, double xh, double xl) {
    dd_add(hi, lo, xh);
    lo += xl;
}

// the work list: ring pieces (grids with an azimuth) or whole rings; first [nrings + 1] = first piece of each ring.  A function of the
// grid alone.
inline void red_items(const sx_handle *h, std::vector<RedItem> &items, std::vector<int> &first) {
    items.clear();
    first.assign(h->nrings + 1, 0);
    const int G = RED_T / h->nz;         // lambdas per stride (nz <= 256: sx_create)
    for (int i = 0; i < h->nrings; i++) {
        first[i] = (int)items.size();
        const int L = h->hL[i];
        const int strides = (L + G - 1) / G, pieces = h->has_l ? (strides + RED_ITERS - 1) / RED_ITERS : 1;
        for (int c = 0; c < pieces; c++) {
            const int l0 = (int)((int64_t)L * c / pieces), l1 = (int)((int64_t)L * (c + 1) / pieces);
            items.push_back(RedItem{i, l0, l1 - l0, 0});
        }
    }
    first[h->nrings] = (int)items.size();
}

// the program as the kernels read it, from one that sx_reduce_planes has passed: terms by output (their order within an output
// kept), factors as plane numbers
inline void red_pack(RedProg &prog, const int32_t (*planes)[2], int n_planes, int n_terms, const double *coef, const int32_t *terms, int n_out) {
    std::memset(&prog, 0, sizeof(prog));
    prog.n_planes = n_planes; prog.n_out = n_out;
    for (int j = 0; j < n_planes; j++) { prog.pvar[j] = (uint8_t)(planes[j][0] - 1); prog.pslot[j] = (uint8_t)planes[j][1]; }
    int k = 0;
    for (int o = 0; o < n_out; o++) {
        prog.start[o] = (uint8_t)k;
        for (int t = 0; t < n_terms; t++) {
            const int32_t *q = terms + (size_t)t * RED_TERM_W;
            if (q[0] != o) continue;
            prog.coef[k] = coef[t]; prog.p[k] = (int8_t)q[1]; prog.nf[k] = (int8_t)q[2];
            for (int f = 0; f < q[2]; f++) {
                int j = 0;
                while (planes[j][0] != q[3 + f] || planes[j][1] != q[3 + RED_FACTORS + f]) j++;
                prog.f[k][f] = (uint8_t)j;
            }
            k++;
        }
    }
    for (int o = n_out; o <= RED_OUT; o++) prog.start[o] = (uint8_t)k;
}

// bytes a scan kernel reads: the planes named x N x their element size
inline double red_bytes(const sx_handle *h, int source, const int32_t (*planes)[2], int n_planes) {
    double b = 0;
    for (int j = 0; j < n_planes; j++) b += (double)h->N * (source == SX_REDUCE_PHYSICAL && h->f32 && planes[j][1] > 0 ? 4.0 : 8.0);
    return b;
}

// the null-coef refusal in who's name; red_accept: what sx_reduce_planes refuses, then that, and the planes of the program on
// success; red_program: red_accept + red_pack, for the callers that launch at once
inline bool red_coef_ok(const char *who, int n_terms, const double *coef) {
    if (n_terms > 0 && !coef) set_error(std::string(who) + ": null coef with n_terms > 0");
    return n_terms <= 0 || coef;
}
inline bool red_accept(const char *who, const sx_grid_desc *gd, int source, int n_terms, const double *coef, const int32_t *terms, int n_out,
                       int32_t (*planes)[2], int32_t *n_planes) {
    return !sx_reduce_planes(gd, source, n_terms, terms, n_out, &planes[0][0], n_planes) && red_coef_ok(who, n_terms, coef);
}
inline bool red_program(const char *who, const sx_grid_desc *gd, int source, int n_terms, const double *coef, const int32_t *terms, int n_out,
                        int32_t (*planes)[2], int32_t *n_planes, RedProg &prog) {
    if (!red_accept(who, gd, source, n_terms, coef, terms, n_out, planes, n_planes)) return false;
    red_pack(prog, planes, *n_planes, n_terms, coef, terms, n_out);
    return true;
}

// The scan table: work list and quadrature weights, functions of the grid alone, one copy per handle (DIAG_SCAN), fetched per call.
struct ScanGrid : DiagState {
    std::vector<RedItem> items;     // the work list on the host (sx_stats: the longest piece)
    DevBuf<RedItem> d_items;        // ring pieces (grids with an azimuth) or whole rings
    DevBuf<int> d_first;            // [nrings + 1] first piece of each ring
    DevBuf<double> d_wrl, d_wz;     // w_r w_l per ring, w_z per level; d_wrl is set last: it is there when both are
    int n_items = 0;
};
// made on first use; the weights when a caller first asks for them.  Null, the error set in who's name, when an upload failed
inline ScanGrid *scan_grid(sx_handle *h, const char *who, bool weights) {
    ScanGrid *sg = diag_state<ScanGrid>(h, DIAG_SCAN);
    if (sg && (!weights || sg->d_wrl)) return sg;
    const std::string err = std::string(who) + ": hipMalloc / hipMemcpy of the work list failed";
    if (!sg) {
        std::unique_ptr<ScanGrid> made(new ScanGrid());
        std::vector<int> first;
        red_items(h, made->items, first);
        made->n_items = (int)made->items.size();
        if (!made->d_items.upload(made->items, err.c_str()) || !made->d_first.upload(first, err.c_str())) return nullptr;
        h->diag[DIAG_SCAN] = std::move(made);
        sg = diag_state<ScanGrid>(h, DIAG_SCAN);
    }
    if (weights) {
        std::vector<double> wr(h->nrings), wl(h->nrings), wz(h->nz, 1.0), wrl(h->nrings);
        reduce_weights(eval_geom_of(h), wr.data(), wl.data(), wz.data());
        for (int i = 0; i < h->nrings; i++) wrl[i] = wr[i] * wl[i];
        if (!sg->d_wz.upload(wz, err.c_str()) || !sg->d_wrl.upload(wrl, err.c_str())) return nullptr;
    }
    return sg;
}

// The kernel instantiation of a call.  The state (SX_REDUCE_STATE: var_np1) is always fp64; the derivative slots of `physical` are
// fp32 on an f32 handle.  Grids with an azimuth walk ring pieces (RINGS).  f(double() or float(), std::true_type or false_type, planes)
template <class F>
inline void scan_dispatch(const sx_handle *h, int source, F &&f) {
    double *base = source == SX_REDUCE_STATE ? h->d_np1 : h->d_phys;
    auto geometry = [&](auto st) {
        const auto P = planes_of<decltype(st)>(base, h->V, h->N);
        if (h->has_l) f(st, std::true_type(), P);
        else f(st, std::false_type(), P);
    };
    if (source == SX_REDUCE_STATE || !h->f32) geometry(double());
    else geometry(float());
}
// workgroups of a flat launch: RED_T lanes, W points each
inline unsigned scan_flat_blocks(const sx_handle *h, int W = 1) { return (unsigned)((h->N + (int64_t)RED_T * W - 1) / ((int64_t)RED_T * W)); }

// ---- what sx_project and sx_derive share: a kernel on the source's stream writes the var_np1 planes of a companion handle, whose own
// forward chain then runs on its stream
struct CompanionWrite : DiagState {
    hipEvent_t done = nullptr;        // recorded on the source's stream behind the kernel; the destination's stream waits on it
    ~CompanionWrite() override { if (done) hipEventDestroy(done); }
};
// the state of entry point `which` of src with its event, made on first use; null with the error set
inline CompanionWrite *companion_write_state(sx_handle *src, int which) {
    if (!src->diag[which]) src->diag[which].reset(new CompanionWrite());
    CompanionWrite *st = diag_state<CompanionWrite>(src, which);
    if (!st->done) HIPCHK(hipEventCreateWithFlags(&st->done, hipEventDisableTiming));
    return error_status() ? nullptr : st;
}
// the handle's grid with what companion_pair_ok compares beyond desc_of
inline sx_grid_desc companion_desc(const sx_handle *h) {
    sx_grid_desc gd = desc_of(h);
    gd.ring_uniform_L = h->uniform_L; gd.zmin = h->zmin; gd.zmax = h->zmax;
    return gd;
}
// both one-tile patches on the same grid (b_zDim may differ: the destination truncates as it says), or the refusal in who's name
inline bool companion_pair_ok(const char *who, const sx_grid_desc *src, const sx_grid_desc *dst) {
    if (src->tile_cell0 != 0 || src->tile_num_cells != src->num_cells || dst->tile_cell0 != 0 || dst->tile_num_cells != dst->num_cells) {
        set_error(std::string(who) + ": source and destination must be one-tile patches");
        return false;
    }
    const EvalGeom gs = desc_geom(src), gd = desc_geom(dst);
    const char *differs = src->geometry != dst->geometry ? "geometry" : src->xmin != dst->xmin ? "xmin" : src->xmax != dst->xmax ? "xmax" :
                          src->num_cells != dst->num_cells ? "num_cells" : gs.uniform_L != gd.uniform_L ? "ring table" :
                          gs.has_z && gs.nz != gd.nz ? "zDim" : gs.has_z && gs.zmin != gd.zmin ? "zmin" : gs.has_z && gs.zmax != gd.zmax ? "zmax" : nullptr;
    if (differs) set_error(std::string(who) + ": the destination's grid differs from the source's in " + differs);
    return !differs;
}
// behind the kernel: the event hand-over, then the destination's own forward chain, every variable - what sx_spectral_transform +
// sx_spline_transform launch; returns after completion
inline int companion_transform(sx_handle *src, sx_handle *dst, CompanionWrite *st) {
    HIPCHK(hipEventRecord(st->done, src->stream));
    HIPCHK(hipStreamWaitEvent(dst->stream, st->done, 0));
    if (error_status()) return 1;
    dst->diag_dirty = false;
    launch_fl_forward(dst);
    launch_sb(dst);
    launch_solve(dst);
    HIPCHK(hipStreamSynchronize(dst->stream));
    return error_status();
}

}  // namespace sx
