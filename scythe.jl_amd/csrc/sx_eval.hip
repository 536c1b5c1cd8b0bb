// sx_evaluate / sx_eval_basis: the spectral state sampled at arbitrary points (include/scythe_hip.h).
//
// u(r, lambda, z) = sum A[zm, blk, node] phi_node(r) F_blk(lambda) C_zm(z).  The host forms, per point, what depends on r and z
// (the 4 radial weights of phi, phi', phi'', the wavenumber cap, the vertical weight rows: eval_radial_pt /
// eval_vert_weights of sx_setup.cpp, the functions sx_eval_basis returns) and sorts the points by radial cell; the kernel does the
// sum over A.  That sum reads 4 node rows x (2 kcap + 1) blocks x b_zDim modes per (point, variable) - 2 MB per point at the bench
// grid - so a workgroup takes up to EVAL_P points of ONE cell and loads each A element once for all of them: threads stride over the
// (zm, blk) columns of the [node][col] array (coalesced), every point's 7 slot sums stay in registers, and the workgroup reduces
// them at the end (shuffles within a wave, LDS across waves).  The column a thread sums and the order of the reduction depend on
// nothing but the grid, so a point's result does not depend on which points share its batch or its call.
#include "sx_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>

namespace sx {

constexpr int EVAL_P = 8;          // points per workgroup (their slot sums are registers: 7 x EVAL_P doubles per thread)
constexpr int EVAL_T = 256;        // threads per workgroup
constexpr int EVAL_CT = 2;         // columns per thread in flight: a point's radial weights are read from LDS once per EVAL_CT columns
constexpr int EVAL_CHUNK = 16384;  // points per launch (bounds the device scratch)
constexpr size_t EVAL_LDS_MAX = 64 * 1024;

struct EvalPt {          // one point as the kernel reads it (sorted by cell)
    double wr[12];       // [3][4] phi, phi', phi'' at nodes cell .. cell + 3
    double lh, ll;       // lambda reduced to [-pi, pi] in extended precision, as a double and the remainder
    int cell, kcap, zi, orig;   // patch row of the first node; wavenumber cap; row of the vertical weight table; index in the chunk
};

struct EvalSlots { int s[7]; };     // u r rr l ll z zz -> slot of `physical`, -1 = the geometry has none

struct EvalState : DiagState {
    EvalClasses cls;
    DevBuf<EvalPt> d_pts;
    DevBuf<int2> d_batch;
    DevBuf<double> d_wz, d_res;
};

// 2 pi as a double and the remainder, for the reduction of k lambda
#define SX_TWO_PI_HI 6.283185307179586
#define SX_TWO_PI_LO 2.4492935982947064e-16

// cos(k lambda), sin(k lambda) for lambda = lh + ll: the product k lh is split exactly (fma), reduced by a multiple of 2 pi (exact: the
// difference is small and fits a double), and what is left over enters to first order - the Float64 product k * lambda alone loses k ulp
__device__ inline double2 eval_cs(int k, double lh, double ll) {
    const double kd = (double)k;
    const double p = kd * lh, e = fma(kd, lh, -p);
    const double n = rint(p * (1.0 / SX_TWO_PI_HI));
    const double y = fma(-n, SX_TWO_PI_HI, p);
    const double t = e + kd * ll - n * SX_TWO_PI_LO;
    double s, c;
    sincos(y, &s, &c);
    return make_double2(c - t * s, s + t * c);
}

// grid (batches, V).  LDS (doubles): cs [P][csw] double2 | zw [P][3][Zb] | wr [P][12] | red [4][P][7] | kcap [P] int
__global__ __launch_bounds__(EVAL_T) void k_evaluate(const double *__restrict__ A, int64_t C, const EvalPt *__restrict__ pts,
                                                     const int2 *__restrict__ batches, const double *__restrict__ wz,
                                                     const int *__restrict__ vcls, int ncls, int Zb, int K2, int has_l, int csw, int P,
                                                     int kmin, int kband, EvalSlots slots, double *__restrict__ res, int64_t nres, int V) {
    extern __shared__ double lds[];
    double2 *cs = reinterpret_cast<double2 *>(lds);
    double *zw = lds + (size_t)2 * P * csw;
    double *wr = zw + (size_t)P * 3 * Zb;
    double *red = wr + (size_t)P * 12;
    int *kc = reinterpret_cast<int *>(red + 4 * EVAL_P * 7);
    const int tid = threadIdx.x, v = blockIdx.y;
    const int2 bt = batches[blockIdx.x];
    const int start = bt.x, np = bt.y;
    const int cell = pts[start].cell;
    const int cls = vcls[v];

    for (int i = tid; i < np * 12; i += EVAL_T) wr[i] = pts[start + i / 12].wr[i % 12];
    for (int i = tid; i < np * 3 * Zb; i += EVAL_T) {
        const int p = i / (3 * Zb), j = i - p * 3 * Zb;
        zw[i] = wz[((size_t)pts[start + p].zi * ncls + cls) * 3 * Zb + j];
    }
    int kmaxb = 0;
    for (int p = 0; p < np; p++) kmaxb = max(kmaxb, pts[start + p].kcap);
    kmaxb = min(kmaxb, kband);                        // the band kmin <= k <= kband (sx_evaluate: 0, kDim)
    if (tid < np) kc[tid] = pts[start + tid].kcap;
    for (int i = tid; i < np * csw; i += EVAL_T) {
        const int p = i / csw, k = i - p * csw;
        if (k <= pts[start + p].kcap) cs[i] = eval_cs(k, pts[start + p].lh, pts[start + p].ll);
    }
    __syncthreads();

    double acc[EVAL_P][7];
#pragma unroll
    for (int p = 0; p < EVAL_P; p++)
#pragma unroll
        for (int m = 0; m < 7; m++) acc[p][m] = 0.0;

    const double *__restrict__ Av = A + (int64_t)cell * C + (int64_t)v * Zb * K2;
    const int ncol = Zb * K2, q = EVAL_T / K2, rem = EVAL_T % K2;
    const int live = has_l ? 2 * kmaxb + 1 : 0;       // last live block
    int zm = tid / K2, blk = tid % K2;
    for (int col0 = tid; col0 < ncol; col0 += EVAL_T * EVAL_CT) {
        double a[EVAL_CT][4];
        int czm[EVAL_CT], cblk[EVAL_CT];
        bool on[EVAL_CT];
#pragma unroll
        for (int c = 0; c < EVAL_CT; c++) {
            const int col = col0 + c * EVAL_T;
            czm[c] = zm; cblk[c] = blk;
            on[c] = col < ncol && blk <= live && blk != 1 && (blk >> 1) >= kmin;
#pragma unroll
            for (int j = 0; j < 4; j++) a[c][j] = on[c] ? Av[(int64_t)j * C + col] : 0.0;
            zm += q; blk += rem;
            if (blk >= K2) { blk -= K2; zm++; }
        }
#pragma unroll
        for (int p = 0; p < EVAL_P; p++) {
            if (p >= np) break;
            double w[12];
#pragma unroll
            for (int j = 0; j < 12; j++) w[j] = wr[p * 12 + j];
            const int kcp = kc[p];
#pragma unroll
            for (int c = 0; c < EVAL_CT; c++) {
                if (!on[c] || cblk[c] > 2 * kcp + 1) continue;
                const double s0 = fma(w[3], a[c][3], fma(w[2], a[c][2], fma(w[1], a[c][1], w[0] * a[c][0])));
                const double s1 = fma(w[7], a[c][3], fma(w[6], a[c][2], fma(w[5], a[c][1], w[4] * a[c][0])));
                const double s2 = fma(w[11], a[c][3], fma(w[10], a[c][2], fma(w[9], a[c][1], w[8] * a[c][0])));
                // F_blk and its lambda derivatives: block 0 is 1; Re k: 2 cos, -2 k sin, -2 k^2 cos; Im k: -2 sin, -2 k cos, 2 k^2 sin
                const int k = cblk[c] >> 1;
                const double2 t = cs[p * csw + k];
                const double kd = (double)k;
                const double x = (cblk[c] & 1) ? -t.y : t.x, y = (cblk[c] & 1) ? -t.x : -t.y;
                const double F0 = cblk[c] == 0 ? 1.0 : 2.0 * x, F1 = 2.0 * kd * y, F2 = -(kd * kd) * F0;
                const double z0 = zw[(p * 3 + 0) * Zb + czm[c]], z1 = zw[(p * 3 + 1) * Zb + czm[c]], z2 = zw[(p * 3 + 2) * Zb + czm[c]];
                const double f0 = F0 * z0;
                acc[p][0] = fma(s0, f0, acc[p][0]);
                acc[p][1] = fma(s1, f0, acc[p][1]);
                acc[p][2] = fma(s2, f0, acc[p][2]);
                acc[p][3] = fma(s0, F1 * z0, acc[p][3]);
                acc[p][4] = fma(s0, F2 * z0, acc[p][4]);
                acc[p][5] = fma(s0, F0 * z1, acc[p][5]);
                acc[p][6] = fma(s0, F0 * z2, acc[p][6]);
            }
        }
    }

    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int p = 0; p < EVAL_P; p++)
#pragma unroll
        for (int m = 0; m < 7; m++) {
            double x = acc[p][m];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
            if (lane == 0) red[(wave * EVAL_P + p) * 7 + m] = x;
        }
    __syncthreads();
    if (tid < np * 7) {
        const int p = tid / 7, m = tid - p * 7, d = slots.s[m];
        if (d >= 0) {
            double x = red[p * 7 + m];
            for (int w = 1; w < EVAL_T / 64; w++) x += red[(w * EVAL_P + p) * 7 + m];
            res[((int64_t)d * V + v) * nres + pts[start + p].orig] = x;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// what both entry points (and sx_parcels_set, sx_harmonics) refuse; coordinates r[, lambda][, z]
static const char *const NOT_FINITE = "a coordinate is NaN or Inf";

bool eval_radius_ok(const EvalGeom &g, double r, std::string &why) {
    if (!std::isfinite(r)) { why = NOT_FINITE; return false; }
    if (!(r >= g.tile_lo() && r <= g.tile_hi())) {
        why = "r = " + std::to_string(r) + " outside the tile's extent [" + std::to_string(g.tile_lo()) + ", " + std::to_string(g.tile_hi()) + "]";
        return false;
    }
    return true;
}

bool eval_height_ok(const EvalGeom &g, double z, std::string &why) {
    if (!std::isfinite(z)) { why = NOT_FINITE; return false; }
    if (g.has_z && !(z >= g.zmin && z <= g.zmax)) {
        why = "z = " + std::to_string(z) + " outside [" + std::to_string(g.zmin) + ", " + std::to_string(g.zmax) + "]";
        return false;
    }
    return true;
}

static bool eval_point_ok(const EvalGeom &g, double r, double lam, double z, std::string &why) {
    if (!std::isfinite(r) || !std::isfinite(lam) || !std::isfinite(z)) { why = NOT_FINITE; return false; }      // before any range
    return eval_radius_ok(g, r, why) && eval_height_ok(g, z, why);
}

// every point of pts [n_coord][n] lies in the tile; a refusal reads "<who>: <noun> i: <why>"
bool eval_points_ok(const sx_handle *h, const double *pts, int64_t n, const char *who, const char *noun) {
    const EvalGeom g = eval_geom_of(h);
    std::string why;
    for (int64_t i = 0; i < n; i++) {
        const double lam = h->has_l ? pts[n + i] : 0.0, z = h->has_z ? pts[(int64_t)(h->ncoord - 1) * n + i] : 0.0;
        if (!eval_point_ok(g, pts[i], lam, z, why)) { set_error(std::string(who) + ": " + noun + " " + std::to_string(i) + ": " + why); return false; }
    }
    return true;
}

double wrap_lambda(double lam) {
    const double l = (double)remainderl((long double)lam, 8.0L * atanl(1.0L));
    return l <= -M_PI ? M_PI : l;
}

static EvalState *eval_state(sx_handle *h) {
    if (h->diag[DIAG_EVAL]) return diag_state<EvalState>(h, DIAG_EVAL);
    std::unique_ptr<EvalState> st(new EvalState());
    EvalClasses &k = st->cls;
    k.vcls.assign(h->V, 0);
    std::string err;
    if (h->has_z) {
        for (int v = 0; v < h->V; v++) {
            int found = -1;
            for (size_t c = 0; c < k.vert.size(); c++)
                if (k.vert[c].bcb == h->bcb[v] && k.vert[c].bct == h->bct[v]) found = (int)c;
            if (found < 0) {
                EvalVert ev;
                if (!build_eval_vert(h->zmin, h->zmax, h->nz, h->Zb, h->bcb[v], h->bct[v], ev, err)) { set_error(err); return nullptr; }
                k.vert.push_back(ev);
                found = (int)k.vert.size() - 1;
            }
            k.vcls[v] = found;
        }
    }
    std::vector<double> w3;             // W[0 .. 2] of every class, rounded once
    for (const EvalVert &ev : k.vert)
        for (int m = 0; m < 3; m++)
            for (long double x : ev.W[m]) w3.push_back((double)x);
    if (!k.d_vcls.upload(k.vcls, "sx_evaluate: hipMalloc of the scratch failed") || (!w3.empty() && !k.d_w3.upload(w3, "eval_classes: hipMalloc of the vertical operators failed")))
        return nullptr;
    h->diag[DIAG_EVAL] = std::move(st);
    return diag_state<EvalState>(h, DIAG_EVAL);
}

// the vertical classes and the per-variable class table, for sx_harmonics, sx_spectrum and sx_parcels_set as well
const EvalClasses *eval_classes(sx_handle *h) {
    EvalState *st = eval_state(h);
    return st ? &st->cls : nullptr;
}

static size_t eval_lds_bytes(int P, int csw, int Zb) {
    return sizeof(double) * ((size_t)2 * P * csw + (size_t)P * 3 * Zb + (size_t)P * 12 + 4 * EVAL_P * 7) + sizeof(int) * EVAL_P;
}

// one launch: the points [p0, p0 + n) of the call
// bytes: the A traffic of the call so far, this launch's added (its batches x 4 rows x live columns)
static bool eval_chunk(sx_handle *h, EvalState *st, const EvalGeom &g, const double *points, int64_t n_all, int64_t p0, int n, int flags,
                       int kmin, int kband, double *out, double &bytes) {
    const std::vector<EvalVert> &vert = st->cls.vert;
    const int ncls = std::max<int>(1, (int)vert.size()), Zb = h->has_z ? h->Zb : 1;
    const long double two_pi = 8.0L * atanl(1.0L);
    std::vector<EvalPt> pts(n);
    std::vector<double> wz;
    std::unordered_map<uint64_t, int> zrow;
    if (!h->has_z) wz = {1.0, 0.0, 0.0};
    for (int i = 0; i < n; i++) {
        const double r = points[p0 + i];
        const double lam = h->has_l ? points[n_all + p0 + i] : 0.0;
        const double z = h->has_z ? points[(int64_t)(h->ncoord - 1) * n_all + p0 + i] : 0.0;
        EvalPt &e = pts[i];
        eval_radial_pt(g, r, flags, e.wr, e.cell, e.kcap);
        const long double lr = remainderl((long double)lam, two_pi);
        e.lh = (double)lr;
        e.ll = (double)(lr - (long double)e.lh);
        e.orig = i;
        e.zi = 0;
        if (h->has_z) {
            uint64_t key;
            const double zk = z == 0.0 ? 0.0 : z;      // -0.0 and 0.0 are one level
            std::memcpy(&key, &zk, sizeof(key));
            auto it = zrow.find(key);
            if (it == zrow.end()) {
                const int row = (int)zrow.size();
                zrow.emplace(key, row);
                wz.resize((size_t)(row + 1) * ncls * 3 * Zb);
                for (int c = 0; c < ncls; c++) eval_vert_weights(vert[c], h->zmin, h->zmax, h->nz, Zb, z, &wz[((size_t)row * ncls + c) * 3 * Zb]);
                e.zi = row;
            } else {
                e.zi = it->second;
            }
        }
    }
    // by cell; within a cell the caller's order
    std::stable_sort(pts.begin(), pts.end(), [](const EvalPt &a, const EvalPt &b) { return a.cell < b.cell; });
    const int csw = h->kDim + 1;
    int P = EVAL_P;
    while (P > 1 && eval_lds_bytes(P, csw, Zb) > EVAL_LDS_MAX) P--;
    if (eval_lds_bytes(P, csw, Zb) > EVAL_LDS_MAX) { set_error("sx_evaluate: the wavenumber table of one point does not fit the LDS (kDim too large)"); return false; }
    std::vector<int2> batches;
    double cols = 0;
    for (int i = 0; i < n;) {
        int j = i, kmax = 0;
        while (j < n && j - i < P && pts[j].cell == pts[i].cell) kmax = std::max(kmax, pts[j++].kcap);
        batches.push_back(make_int2(i, j - i));
        const int khi = std::min(kmax, kband);                       // live blocks: k = 0 is one, every k >= 1 two
        cols += (double)Zb * (h->has_l ? (kmin > 0 ? std::max(0, 2 * (khi - kmin + 1)) : 2 * khi + 1) : 1);
        i = j;
    }
    bytes += 8.0 * 4.0 * cols * h->V;
    const size_t nres = (size_t)n * h->V * h->D;
    const char *who = "sx_evaluate";
    if (!st->d_pts.grow(pts.size(), who) || !st->d_batch.grow(batches.size(), who) || !st->d_wz.grow(wz.size(), who) || !st->d_res.grow(nres, who))
        return false;
    HIPCHK(hipMemcpyAsync(st->d_pts, pts.data(), sizeof(EvalPt) * pts.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(st->d_batch, batches.data(), sizeof(int2) * batches.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(st->d_wz, wz.data(), sizeof(double) * wz.size(), hipMemcpyHostToDevice, h->stream));
    if (error_status()) return false;
    EvalSlots sl;
    for (int m = 0; m < 7; m++) sl.s[m] = h->slot[m];
    {
        TimedLaunch scope(h, "k_evaluate", bytes);
        hipLaunchKernelGGL(k_evaluate, dim3((unsigned)batches.size(), (unsigned)h->V), dim3(EVAL_T), eval_lds_bytes(P, csw, Zb), h->stream, h->d_A,
                           h->C, st->d_pts, st->d_batch, st->d_wz, st->cls.d_vcls, ncls, Zb, h->K2, h->has_l, csw, P, kmin, kband, sl, st->d_res, (int64_t)n, h->V);
    }
    std::vector<double> res(nres);
    HIPCHK(hipMemcpyAsync(res.data(), st->d_res, sizeof(double) * nres, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (error_status()) return false;
    for (int q = 0; q < h->V * h->D; q++) std::memcpy(out + (int64_t)q * n_all + p0, res.data() + (size_t)q * n, sizeof(double) * n);
    return true;
}

}  // namespace sx

using namespace sx;

extern "C" {

static int evaluate_band(sx_handle *h, const double *points, int64_t n_points, int32_t flags, int kmin, int kband, double *out) {
    if (n_points < 0) { set_error("sx_evaluate: n_points is negative"); return 1; }
    if (flags != SX_EVAL_RING_K && flags != SX_EVAL_ALL_K) { set_error("sx_evaluate: flags must be SX_EVAL_RING_K or SX_EVAL_ALL_K"); return 1; }
    if (n_points == 0) return 0;
    if (!points || !out) { set_error("sx_evaluate: null argument"); return 1; }
    if (!eval_points_ok(h, points, n_points, "sx_evaluate", "point")) return 1;
    const EvalGeom g = eval_geom_of(h);
    EvalState *st = eval_state(h);
    if (!st) return 1;
    flush_diag(h);
    // the results of every launch are held back until all of them have succeeded: a failed call writes nothing to out
    std::vector<double> tmp((size_t)n_points * h->V * h->D);
    double bytes = 0;
    for (int64_t p0 = 0; p0 < n_points; p0 += EVAL_CHUNK)
        if (!eval_chunk(h, st, g, points, n_points, p0, (int)std::min<int64_t>(EVAL_CHUNK, n_points - p0), flags, kmin, kband, tmp.data(), bytes)) return 1;
    std::memcpy(out, tmp.data(), sizeof(double) * tmp.size());
    return error_status();
}

int sx_evaluate(sx_handle *h, const double *points, int64_t n_points, int32_t flags, double *out) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    return evaluate_band(h, points, n_points, flags, 0, h->kDim, out);
}

int sx_evaluate_band(sx_handle *h, const double *points, int64_t n_points, int32_t flags, int32_t kmin, int32_t kmax, double *out) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    if (kmin < 0 || kmax < kmin) { set_error("sx_evaluate_band: need 0 <= kmin <= kmax"); return 1; }
    return evaluate_band(h, points, n_points, flags, kmin, std::min<int>(kmax, h->kDim), out);
}

int sx_eval_basis(const sx_grid_desc *gd, int32_t var, const double *point, int32_t flags, int32_t *node0, double *w_r, int32_t *kcap,
                  double *w_z) {
    clear_error();
    if (!point) { set_error("sx_eval_basis: null argument"); return 1; }
    if (!desc_ok(gd, "sx_eval_basis")) return 1;
    if (var < 1 || var > gd->nvars) { set_error("sx_eval_basis: var is 1-based and at most nvars"); return 1; }
    if (flags != SX_EVAL_RING_K && flags != SX_EVAL_ALL_K) { set_error("sx_eval_basis: flags must be SX_EVAL_RING_K or SX_EVAL_ALL_K"); return 1; }
    const EvalGeom g = desc_geom(gd);
    if (g.has_z && (g.nz < 4 || g.Zb > g.nz || !(g.zmax > g.zmin))) { set_error("invalid vertical grid (need zDim >= 4, b_zDim <= zDim, zmax > zmin)"); return 1; }
    const double r = point[0], lam = g.has_l ? point[1] : 0.0, z = g.has_z ? point[1 + g.has_l] : 0.0;
    std::string why;
    if (!eval_point_ok(g, r, lam, z, why)) { set_error("sx_eval_basis: " + why); return 1; }
    int n0, kc;
    double w[12];
    eval_radial_pt(g, r, flags, w, n0, kc);
    if (node0) *node0 = n0;
    if (w_r) std::memcpy(w_r, w, sizeof(w));
    if (kcap) *kcap = kc;
    if (g.has_z && w_z) {
        // the class's extended-precision operators are built per call (the projection and two N x N x Zb products, O(N^3)): fine
        // for a helper that checks weights; sx_evaluate builds them once per handle
        EvalVert ev;
        std::string err;
        const int bcb = gd->bcb ? gd->bcb[var - 1] : SX_BC_R0, bct = gd->bct ? gd->bct[var - 1] : SX_BC_R0;
        if (!build_eval_vert(g.zmin, g.zmax, g.nz, g.Zb, bcb, bct, ev, err)) { set_error(err); return 1; }
        eval_vert_weights(ev, g.zmin, g.zmax, g.nz, g.Zb, z, w_z);
    }
    return 0;
}

}  // extern "C"
