// sx_reduce / sx_reduce_weights / sx_reduce_planes: integrals and azimuthal means of field products (include/scythe_hip.h).
//
// Two stages.  k_reduce forms the azimuthal sums S[ring][level][output] = sum_lambda integrand: a workgroup takes one piece of one ring
// (a run of lambdas, all levels), its threads take consecutive points - z innermost, so a thread keeps ONE level and strides over the
// lambdas - read every plane the program names once, evaluate all terms from registers and add them to one double-double accumulator
// per output; the workgroup then adds, per level and in lambda order, the accumulators of the threads that share the level.  Grids
// without an azimuth (L = 1) have nothing to sum: there a workgroup takes 256 consecutive points and writes their integrands.
// k_reduce_final adds the pieces of a ring in order and divides by L (SX_REDUCE_AZIMUTH), or forms the weighted sum over rings and
// levels (SX_REDUCE_DOMAIN: a fixed number of workgroups per output, fixed strides, a fixed tree, then the workgroups' sums in order).  Nothing is added atomically: which lane adds
// what, and in which order, follows from the grid and the program alone, so two calls on the same data agree bitwise; and every sum is
// double-double, so the rounding error is that of the terms and does not grow with the point count.
//
// The program is a kernel ARGUMENT (constant memory, scalar loads: its indices are uniform), terms sorted by output so that the
// accumulators are indexed statically.
#include "sx_redprog.hpp"
#include <algorithm>
#include <cstring>

namespace sx {

constexpr int RED_TF = 1024;        // threads per workgroup of k_reduce_final's domain sum
// RED_T, RED_ITERS, the limits, RedProg, RedItem, the scan table (work list, weights), the plane loads and dd_add: sx_redprog.hpp

struct ReduceState : DiagState {
    DevBuf<double2> d_part;         // [piece][output][level] (hi, lo)
    DevBuf<double2> d_part2;        // [RED_OUT][blocks2] sums of the domain kind's first level
    int blocks2 = 1;                // workgroups per output of k_reduce_domain: 4 (piece, level) entries per thread, at most 64
    DevBuf<double> d_out;
};

// One point: load the planes, evaluate the terms.  pt < N is the caller's business.
template <class ST>
__device__ inline void reduce_point(const Planes<ST> &P, int V, int64_t N, int64_t pt, double r, const RedProg &g, double (&hi)[RED_OUT],
                                    double (&lo)[RED_OUT]) {
    double val[RED_PLANES];
    red_load_planes<ST>(P, V, N, pt, g, val);
    const RedPow pw = red_pow(r);
#pragma unroll
    for (int o = 0; o < RED_OUT; o++) {
        for (int t = g.start[o]; t < g.start[o + 1]; t++) {       // empty at o >= n_out
            const double x = red_term(g, t, val, pw);
            dd_add(hi[o], lo[o], x);
        }
    }
}

// RINGS: grid = pieces; a thread's level is tid % nz, its first lambda lam0 + tid / nz, its stride RED_T / nz lambdas.
// !RINGS (every ring has one lambda): grid = ceil(N / RED_T); thread = point; piece = ring.   part [piece][output][level]
template <class ST, bool RINGS>
__global__ __launch_bounds__(RED_T) void k_reduce(Planes<ST> P, int V, int64_t N, int nz, const RedItem *__restrict__ items,
                                                  const int64_t *__restrict__ pstart, const double *__restrict__ rh, RedProg g,
                                                  double2 *__restrict__ part) {
    __shared__ double s_hi[RED_T], s_lo[RED_T];
    const int tid = threadIdx.x;
    double hi[RED_OUT], lo[RED_OUT];
#pragma unroll
    for (int o = 0; o < RED_OUT; o++) hi[o] = lo[o] = 0.0;
    if (RINGS) {
        const RedItem it = items[blockIdx.x];
        const int G = RED_T / nz, z = tid % nz, gl = tid / nz;
        const int64_t h0 = pstart[it.ring];
        const double r = rh[h0];
        if (gl < G)
            for (int l = it.lam0 + gl; l < it.lam0 + it.nlam; l += G) reduce_point<ST>(P, V, N, (h0 + l) * nz + z, r, g, hi, lo);
#pragma unroll
        for (int o = 0; o < RED_OUT; o++) {
            if (o >= g.n_out) continue;
            s_hi[tid] = hi[o]; s_lo[tid] = lo[o];
            __syncthreads();
            if (tid < nz) {
                double a = s_hi[tid], b = s_lo[tid];
                for (int k = 1; k < G; k++) dd_add(a, b, s_hi[k * nz + tid], s_lo[k * nz + tid]);
                part[((int64_t)blockIdx.x * g.n_out + o) * nz + tid] = make_double2(a, b);
            }
            __syncthreads();
        }
    } else {
        const int64_t pt = (int64_t)blockIdx.x * RED_T + tid;
        if (pt >= N) return;
        const int64_t ring = pt / nz;
        const int z = (int)(pt - ring * nz);
        reduce_point<ST>(P, V, N, pt, rh[ring], g, hi, lo);
#pragma unroll
        for (int o = 0; o < RED_OUT; o++) {
            if (o < g.n_out) part[((int64_t)ring * g.n_out + o) * nz + z] = make_double2(hi[o], lo[o]);
        }
    }
}

// SX_REDUCE_AZIMUTH: thread = (ring, level, output), the ring fastest as in out; the ring's pieces in order, then / L
__global__ void k_reduce_mean(const double2 *__restrict__ part, const int *__restrict__ first, const int *__restrict__ L, int nrings, int nz,
                              int n_out, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)nrings * nz * n_out) return;
    const int ring = (int)(e % nrings), z = (int)(e / nrings % nz), o = (int)(e / nrings / nz);
    double a = 0.0, b = 0.0;
    for (int i = first[ring]; i < first[ring + 1]; i++) {
        const double2 x = part[((int64_t)i * n_out + o) * nz + z];
        dd_add(a, b, x.x, x.y);
    }
    out[e] = (a + b) / (double)L[ring];
}

// SX_REDUCE_DOMAIN, two levels.  k_reduce_domain: grid (n_out, blocks); the (piece, level) entries are dealt to the blocks x RED_TF
// threads of an output in order (thread g takes entries g, g + blocks RED_TF, ...), each ring sum is weighted without a rounding error
// of the product (fma), and a workgroup adds its RED_TF double-double sums in a fixed tree -> part2[output][block].
// k_reduce_domain_sum: thread = output, the blocks in order.  The block count follows from the grid alone (reduce_state).
__global__ __launch_bounds__(RED_TF) void k_reduce_domain(const double2 *__restrict__ part, const RedItem *__restrict__ items,
                                                          const double *__restrict__ wrl, const double *__restrict__ wz, int n_items, int nz,
                                                          int n_out, double2 *__restrict__ part2) {
    __shared__ double s_hi[RED_TF], s_lo[RED_TF];
    const int tid = threadIdx.x, o = blockIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t e = (int64_t)blockIdx.y * RED_TF + tid; e < (int64_t)n_items * nz; e += (int64_t)gridDim.y * RED_TF) {
        const int i = (int)(e / nz), z = (int)(e - (int64_t)i * nz);
        const double2 x = part[((int64_t)i * n_out + o) * nz + z];
        const double w = wrl[items[i].ring] * wz[z];
        const double ph = w * x.x, pl = fma(w, x.x, -ph) + w * x.y;
        dd_add(a, b, ph, pl);
    }
    s_hi[tid] = a; s_lo[tid] = b;
    __syncthreads();
    for (int s = RED_TF / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            dd_add(a, b, s_hi[tid + s], s_lo[tid + s]);
            s_hi[tid] = a; s_lo[tid] = b;
        }
        __syncthreads();
    }
    if (tid == 0) part2[(int64_t)o * gridDim.y + blockIdx.y] = make_double2(a, b);
}

__global__ void k_reduce_domain_sum(const double2 *__restrict__ part2, int blocks, int n_out, double *__restrict__ out) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_out) return;
    double a = 0.0, b = 0.0;
    for (int k = 0; k < blocks; k++) dd_add(a, b, part2[(int64_t)o * blocks + k].x, part2[(int64_t)o * blocks + k].y);
    out[o] = a + b;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// the second level of the domain kind: its size follows from the work list (sg: the handle's scan table)
static ReduceState *reduce_state(sx_handle *h, const ScanGrid *sg) {
    if (h->diag[DIAG_REDUCE]) return diag_state<ReduceState>(h, DIAG_REDUCE);
    std::unique_ptr<ReduceState> st(new ReduceState());
    st->blocks2 = (int)std::min<int64_t>(64, std::max<int64_t>(1, ((int64_t)sg->n_items * h->nz + 4 * RED_TF - 1) / (4 * RED_TF)));
    if (!st->d_part2.upload(std::vector<double2>((size_t)RED_OUT * st->blocks2), "sx_reduce: hipMalloc / hipMemcpy of the work list failed"))
        return nullptr;
    h->diag[DIAG_REDUCE] = std::move(st);
    return diag_state<ReduceState>(h, DIAG_REDUCE);
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_reduce_weights(const sx_grid_desc *gd, double *w_r, double *w_l, double *w_z) {
    clear_error();
    if (!desc_ok(gd, "sx_reduce_weights")) return 1;
    const EvalGeom g = desc_geom(gd);
    if (g.has_z && (g.nz < 4 || !(g.zmax > g.zmin))) { set_error("invalid vertical grid (need zDim >= 4, zmax > zmin)"); return 1; }
    reduce_weights(g, w_r, w_l, w_z);
    return 0;
}

int sx_reduce_planes(const sx_grid_desc *gd, int32_t source, int32_t n_terms, const int32_t *terms, int32_t n_out, int32_t *planes,
                     int32_t *n_planes) {
    clear_error();
    if (!desc_ok(gd, "sx_reduce_planes")) return 1;
    if (source != SX_REDUCE_PHYSICAL && source != SX_REDUCE_STATE) { set_error("sx_reduce: source must be SX_REDUCE_PHYSICAL or SX_REDUCE_STATE"); return 1; }
    if (n_terms < 0 || n_terms > RED_TERMS) { set_error("sx_reduce: n_terms must be 0 .. 64"); return 1; }
    if (n_out < 0 || n_out > RED_OUT) { set_error("sx_reduce: n_out must be 0 .. 16"); return 1; }
    if (n_terms > 0 && !terms) { set_error("sx_reduce: null terms with n_terms > 0"); return 1; }
    const int D = gd->geometry == SX_GEOM_R ? 3 : gd->geometry == SX_GEOM_RLZ ? 7 : 5;
    int32_t found[RED_PLANES][2];
    int nfound = 0;
    bool neg_p = false;
    for (int t = 0; t < n_terms; t++) {
        const int32_t *q = terms + (size_t)t * RED_TERM_W;
        const std::string at = "sx_reduce: term " + std::to_string(t) + ": ";
        if (q[0] < 0 || q[0] >= n_out) { set_error(at + "out = " + std::to_string(q[0]) + " is not in [0, n_out)"); return 1; }
        if (q[1] < -2 || q[1] > 2) { set_error(at + "r_power = " + std::to_string(q[1]) + " is not in [-2, 2]"); return 1; }
        if (q[2] < 0 || q[2] > RED_FACTORS) { set_error(at + "n_factors = " + std::to_string(q[2]) + " is not in [0, 4]"); return 1; }
        neg_p = neg_p || q[1] < 0;
        for (int f = 0; f < q[2]; f++) {
            const int32_t var = q[3 + f], slot = q[3 + RED_FACTORS + f];
            if (var < 1 || var > gd->nvars) { set_error(at + "var = " + std::to_string(var) + " is 1-based and at most nvars"); return 1; }
            if (slot < 0 || slot >= D) { set_error(at + "slot = " + std::to_string(slot) + " is not a derivative slot of the geometry"); return 1; }
            if (source == SX_REDUCE_STATE && slot != 0) { set_error(at + "SX_REDUCE_STATE holds the values only (slot 0)"); return 1; }
            int j = 0;
            while (j < nfound && (found[j][0] != var || found[j][1] != slot)) j++;
            if (j == nfound) {
                if (nfound == RED_PLANES) { set_error("sx_reduce: the program names more than 16 distinct (var, slot) planes"); return 1; }
                found[nfound][0] = var; found[nfound][1] = slot;
                nfound++;
            }
        }
    }
    if (neg_p) {
        const double DX = (gd->xmax - gd->xmin) / gd->num_cells;
        for (int i = 0; i < MUBAR * gd->tile_num_cells; i++)
            if (gd->xmin + DX * (gd->tile_cell0 + i / MUBAR + 0.5 + gauss_offset(i % MUBAR)) == 0.0) {
                set_error("sx_reduce: a negative r_power on a tile with a gridpoint at r == 0");
                return 1;
            }
    }
    if (planes) std::memcpy(planes, found, sizeof(int32_t) * 2 * nfound);
    if (n_planes) *n_planes = nfound;
    return 0;
}

int sx_reduce(sx_handle *h, int32_t kind, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_out,
              double *out) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    if (kind != SX_REDUCE_DOMAIN && kind != SX_REDUCE_AZIMUTH) { set_error("sx_reduce: kind must be SX_REDUCE_DOMAIN or SX_REDUCE_AZIMUTH"); return 1; }
    const sx_grid_desc gd = desc_of(h);
    int32_t planes[RED_PLANES][2], n_planes = 0;
    RedProg prog;
    if (!red_program("sx_reduce", &gd, source, n_terms, coef, terms, n_out, planes, &n_planes, prog)) return 1;
    if (n_out > 0 && !out) { set_error("sx_reduce: null out with n_out > 0"); return 1; }
    if (n_out == 0) return 0;
    ScanGrid *sg = scan_grid(h, "sx_reduce", true);
    ReduceState *st = sg ? reduce_state(h, sg) : nullptr;
    if (!st) return 1;

    const size_t n_res = kind == SX_REDUCE_AZIMUTH ? (size_t)h->nrings * h->nz * n_out : (size_t)n_out;
    if (!st->d_part.grow((size_t)sg->n_items * n_out * h->nz, "sx_reduce") || !st->d_out.grow(n_res, "sx_reduce")) return 1;
    {
        TimedLaunch scope(h, "k_reduce", red_bytes(h, source, planes, n_planes));
        scan_dispatch(h, source, [&](auto st_t, auto rings, auto P) {
            constexpr bool RINGS = decltype(rings)::value;
            hipLaunchKernelGGL((k_reduce<decltype(st_t), RINGS>), dim3(RINGS ? (unsigned)sg->n_items : scan_flat_blocks(h)), dim3(RED_T), 0, h->stream, P,
                               h->V, h->N, h->nz, sg->d_items, h->d_pstart, h->d_r, prog, st->d_part);
        });
    }
    {
        TimedLaunch scope(h, "k_reduce_final", 0.0);
        if (kind == SX_REDUCE_AZIMUTH)
            hipLaunchKernelGGL(k_reduce_mean, grid1((int64_t)n_res, 256), dim3(256), 0, h->stream, st->d_part, sg->d_first, h->d_L, h->nrings, h->nz,
                               n_out, st->d_out);
        else {
            hipLaunchKernelGGL(k_reduce_domain, dim3((unsigned)n_out, (unsigned)st->blocks2), dim3(RED_TF), 0, h->stream, st->d_part, sg->d_items,
                               sg->d_wrl, sg->d_wz, sg->n_items, h->nz, n_out, st->d_part2);
            hipLaunchKernelGGL(k_reduce_domain_sum, dim3(1), dim3(64), 0, h->stream, st->d_part2, st->blocks2, n_out, st->d_out);
        }
    }
    std::vector<double> res(n_res);      // held back until the call has succeeded: a failed call writes nothing to out
    HIPCHK(hipMemcpyAsync(res.data(), st->d_out, sizeof(double) * n_res, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (error_status()) return 1;
    std::memcpy(out, res.data(), sizeof(double) * n_res);
    return 0;
}

}  // extern "C"
