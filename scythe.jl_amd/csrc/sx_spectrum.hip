// sx_spectrum / sx_spectrum_check: azimuthal power and cross spectra of the state (include/scythe_hip.h).
//
// P_k(ring, level) = eps_k (a[2k] b[2k] + a[2k + 1] b[2k + 1]) with a[blk], b[blk] the per-block harmonics of two planes at the ring's
// radius and the level's height - what sx_harmonics returns there.  k_spectrum forms them the way k_harmonics does (stage 1: the
// radial fma chain straight into the B operand of v_mfma_f64_16x16x4; stage 2: 16-height tiles of the vertical weight table from
// LDS), but the 16 x 16 result tiles never leave the registers: each lane multiplies its a and b entries, weights the product with
// w_z[level] and adds it to a double-double sum per block.  Stage 1 and stage 2 are a second copy of k_harmonics' (spec_radial,
// spec_vertical): lifted into functions shared by both kernels they moved k_harmonics' register counts, so k_harmonics keeps its text.
// Order of a sum: the lane's 4 heights of a tile, then the 4 lanes that share the block (kk = 0 .. 3), then the height tiles; then the
// block pair (2k, 2k + 1), then eps_k.  SX_SPEC_RING rounds hi + lo once; SX_SPEC_DOMAIN leaves (hi, lo) per (ring, k, pair) to
// k_spectrum_final, which adds the rings times 2 pi w_r: 16 k's x 16 ring strides per workgroup, a stride's rings in order, the 16
// strides in a fixed tree.  Nothing is added atomically; a workgroup belongs to one pair, so a pair's bytes do not depend on the others.
#include "sx_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

constexpr int SPEC_T = 256;           // 4 waves x 16 blocks
constexpr int SPEC_PAIRS = 16;
constexpr int SPEC_SEG = 16;          // ring strides of k_spectrum_final

struct SpecProg {        // the pairs as the kernel reads them: 0-based variable, radial weight set, vertical row of either plane
    int va[SPEC_PAIRS], da[SPEC_PAIRS], ra[SPEC_PAIRS], vb[SPEC_PAIRS], db[SPEC_PAIRS], rb[SPEC_PAIRS], same[SPEC_PAIRS];
};

struct SpecState : DiagState {
    DevBuf<RadialPt> d_pts;         // [nrings] the rings of the tile
    DevBuf<double> d_wz;            // [cls][height tile][row 3][Zp][16]: height_tiles at the level heights
    DevBuf<double> d_wlev;          // [nht 16] w_z per level, zero-padded
    DevBuf<double> d_wring;         // [nrings] 2 pi w_r
    DevBuf<double2> d_part;         // [pair][ring][k] (hi, lo), domain kind
    DevBuf<double> d_out;
    int nht = 1;
    std::vector<int> kcap;          // host copy, for sx_kernel_bytes
};

typedef double spec_d4 __attribute__((ext_vector_type(4)));

// (hi, lo) += (xh, xl), two-sum of the high parts (no ordering assumed), the low parts added
__device__ inline void spec_dd_add(double &hi, double &lo, double xh, double xl) {
    const double s = hi + xh, b = s - hi;
    lo += ((hi - (s - b)) + (xh - b)) + xl;
    hi = s;
}

// stage 1 of k_harmonics for the planes of a pair: ba[ks] = sum_{j < 4} wa[j] A[cell + j][va, zm = 4 ks + kk, blk], and with TWO bb
// likewise from wb and vb in the same loop (the two share the offsets of their loads).  Every lane loads: a lane whose block or mode
// is switched off reads block 0 / the last mode, which exist, and selects 0.0 - a conditional load would put each load into a basic
// block of its own, all of them ahead of the first fma, and every loaded value of both planes would be alive at once.
template <int KS, bool TWO>
__device__ inline void spec_radial(const double *__restrict__ Aa, const double *__restrict__ Ab, int64_t C, int K2, int Zb, int kk, bool on,
                                   const double (&wa)[4], const double (&wb)[4], double (&ba)[KS], double (&bb)[KS]) {
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
        const int zm = 4 * ks + kk;
        const bool ld = on && zm < Zb;
        double a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t o = (int64_t)j * C + (int64_t)min(zm, Zb - 1) * K2;
            const double xa = Aa[o], xb = TWO ? Ab[o] : 0.0;
            a[j] = ld ? xa : 0.0;
            b[j] = ld ? xb : 0.0;
        }
        ba[ks] = fma(wa[3], a[3], fma(wa[2], a[2], fma(wa[1], a[1], wa[0] * a[0])));
        if (TWO) bb[ks] = fma(wb[3], b[3], fma(wb[2], b[2], fma(wb[1], b[1], wb[0] * b[0])));
    }
}

// stage 2 of k_harmonics: 16 heights x 16 blocks; the lane gets heights kk + 4 r, r < 4, of block n
template <int KS>
__device__ inline spec_d4 spec_vertical(const double *row, int lane, int Zb, const double (&b)[KS]) {
    spec_d4 acc = spec_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
        if (4 * ks < Zb) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(row[ks * 64 + lane], b[ks], acc, 0, 0, 0);
    return acc;
}

// grid (tile rings, ceil(KO / 64), pairs).  KS: K steps of 4 modes held in registers (4 KS >= b_zDim).  KO = 2 (kDim + 1).
// DOMAIN: part [pair][ring][k] (hi, lo); else out [pair][ring][k] = hi + lo.
template <int KS, bool DOMAIN>
__global__ __launch_bounds__(SPEC_T) void k_spectrum(const double *__restrict__ A, int64_t C, const RadialPt *__restrict__ pts,
                                                     const double *__restrict__ wz, const double *__restrict__ wlev,
                                                     const int *__restrict__ vcls, int nht, int Zb, int K2, int KO, int has_l,
                                                     SpecProg prog, double *__restrict__ out, double2 *__restrict__ part) {
    __shared__ double tile[2 * KS * 4 * 16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, kk = lane >> 4;
    const int ring = blockIdx.x, pr = blockIdx.z, Zp = (Zb + 3) & ~3;
    const int va = prog.va[pr], vb = prog.vb[pr], ra = prog.ra[pr], rb = prog.rb[pr];
    const bool same = prog.same[pr] != 0;
    const RadialPt *__restrict__ pt = pts + ring;
    const int cell = pt->cell, live = has_l ? 2 * pt->kcap + 1 : 0;
    const int blk = (blockIdx.y * 4 + wave) * 16 + n;
    const bool on = blk < K2 && blk <= live && blk != 1;       // block 1 is the padding block: never read
    double wa[4], wb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { wa[j] = pt->wr[prog.da[pr] * 4 + j]; wb[j] = pt->wr[prog.db[pr] * 4 + j]; }

    double ba[KS], bb[KS];
    const double *__restrict__ Ar = A + (int64_t)cell * C + (on ? blk : 0);     // a switched-off lane reads block 0 and drops it
    if (same) spec_radial<KS, false>(Ar + (int64_t)va * Zb * K2, Ar, C, K2, Zb, kk, on, wa, wb, ba, bb);
    else spec_radial<KS, true>(Ar + (int64_t)va * Zb * K2, Ar + (int64_t)vb * Zb * K2, C, K2, Zb, kk, on, wa, wb, ba, bb);

    const int ca = vcls[va], cb = vcls[vb];
    const bool share = ca == cb && ra == rb;                    // one operator row serves both planes
    const double *__restrict__ wza = wz + ((size_t)ca * nht * 3 + ra) * Zp * 16, *__restrict__ wzb = wz + ((size_t)cb * nht * 3 + rb) * Zp * 16;
    const double *tb = share ? tile : tile + KS * 64;
    double H = 0.0, Lo = 0.0;
    for (int ht = 0; ht < nht; ht++) {
        __syncthreads();
        for (int i = tid; i < Zp * 16; i += SPEC_T) {
            tile[i] = wza[(size_t)ht * 3 * Zp * 16 + i];
            if (!share) tile[KS * 64 + i] = wzb[(size_t)ht * 3 * Zp * 16 + i];
        }
        __syncthreads();
        const spec_d4 xa = spec_vertical<KS>(tile, lane, Zb, ba);
        spec_d4 xb = xa;
        if (!same) xb = spec_vertical<KS>(tb, lane, Zb, bb);
        // the lane's 4 heights: w_z a b with the rounding errors of both products kept (padded heights have w_z = 0)
        double th = 0.0, tl = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double w = wlev[ht * 16 + kk + 4 * r];
            const double p = xa[r] * xb[r], pe = fma(xa[r], xb[r], -p);
            const double q = w * p, ql = fma(w, p, -q) + w * pe;
            spec_dd_add(th, tl, q, ql);
        }
        // the 4 lanes that share the block, kk = 0 .. 3 in order (every lane of the column ends with the same sum)
        double ch = __shfl(th, n), cl = __shfl(tl, n);
#pragma unroll
        for (int k = 1; k < 4; k++) {
            const double xh = __shfl(th, n + 16 * k), xl = __shfl(tl, n + 16 * k);
            spec_dd_add(ch, cl, xh, xl);
        }
        spec_dd_add(H, Lo, ch, cl);
    }
    // the block pair (2k, 2k + 1) sits in neighbouring lanes; eps_k
    const double ph = __shfl_xor(H, 1), pl = __shfl_xor(Lo, 1);
    spec_dd_add(H, Lo, ph, pl);
    const double eps = blk < 2 ? 1.0 : 2.0;
    if (kk == 0 && !(n & 1) && blk < KO) {
        const int64_t e = ((int64_t)pr * gridDim.x + ring) * (KO >> 1) + (blk >> 1);
        if (DOMAIN) part[e] = on ? make_double2(eps * H, eps * Lo) : make_double2(0.0, 0.0);
        else out[e] = on ? eps * (H + Lo) : 0.0;                  // k > kmax[ring]: exact zeros
    }
}

// SX_SPEC_DOMAIN: grid (ceil(K / 16), pairs), 256 threads = 16 k's x 16 ring strides.  Stride s adds rings s, s + 16, ... in order,
// each times 2 pi w_r without a rounding error of the product (fma); the strides are added in a fixed tree.  out [pair][k].
__global__ __launch_bounds__(SPEC_T) void k_spectrum_final(const double2 *__restrict__ part, const double *__restrict__ wring, int nrings,
                                                           int K, double *__restrict__ out) {
    __shared__ double s_hi[SPEC_T], s_lo[SPEC_T];
    const int tid = threadIdx.x, k = blockIdx.x * 16 + (tid & 15), seg = tid >> 4, pr = blockIdx.y;
    double a = 0.0, b = 0.0;
    if (k < K)
        for (int ring = seg; ring < nrings; ring += SPEC_SEG) {
            const double2 x = part[((int64_t)pr * nrings + ring) * K + k];
            const double w = wring[ring];
            const double ph = w * x.x, pl = fma(w, x.x, -ph) + w * x.y;
            spec_dd_add(a, b, ph, pl);
        }
    s_hi[tid] = a; s_lo[tid] = b;
    __syncthreads();
    for (int s = SPEC_SEG / 2; s >= 1; s >>= 1) {
        if (seg < s) {
            spec_dd_add(a, b, s_hi[tid + 16 * s], s_lo[tid + 16 * s]);
            s_hi[tid] = a; s_lo[tid] = b;
        }
        __syncthreads();
    }
    if (seg == 0 && k < K) out[(int64_t)pr * K + k] = a + b;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// the rings, the level table and the weights: functions of the grid alone, made once per handle
static SpecState *spec_state(sx_handle *h, const std::vector<EvalVert> &vert) {
    if (h->diag[DIAG_SPEC]) return diag_state<SpecState>(h, DIAG_SPEC);
    std::unique_ptr<SpecState> st(new SpecState());
    const EvalGeom g = eval_geom_of(h);
    const int Zb = h->has_z ? h->Zb : 1, nz = h->has_z ? h->nz : 1;
    st->nht = (nz + 15) / 16;
    std::vector<RadialPt> pts(h->nrings);
    st->kcap.resize(h->nrings);
    for (int i = 0; i < h->nrings; i++) {
        eval_radial_pt(g, ring_radius(h->xmin, h->DX, h->cell0, i), SX_EVAL_RING_K, pts[i].wr, pts[i].cell, pts[i].kcap);
        st->kcap[i] = pts[i].kcap;
        pts[i].orig = pts[i].pad = 0;
    }
    std::vector<double> lev;
    for (int zj = 0; h->has_z && zj < nz; zj++) lev.push_back(level_height(h->zmin, h->zmax, h->nz, zj));
    const std::vector<double> wz = height_tiles(vert, lev.data(), nz, h->zmin, h->zmax, h->nz, Zb);
    std::vector<double> wr(h->nrings), wl(h->nrings), wlev((size_t)st->nht * 16, 0.0), wring(h->nrings);
    wlev[0] = 1.0;                                             // without a vertical: one level of weight 1
    reduce_weights(g, wr.data(), wl.data(), wlev.data());
    for (int i = 0; i < h->nrings; i++) wring[i] = wr[i] * (wl[i] * (double)h->hL[i]);      // 2 pi = w_l L (1 without an azimuth)
    const char *err = "sx_spectrum: hipMalloc / hipMemcpy of the tables failed";
    if (!st->d_pts.upload(pts, err) || !st->d_wz.upload(wz, err) || !st->d_wlev.upload(wlev, err) || !st->d_wring.upload(wring, err)) return nullptr;
    h->diag[DIAG_SPEC] = std::move(st);
    return diag_state<SpecState>(h, DIAG_SPEC);
}

struct SpecLaunch {
    const int *vcls;
    int Zb, KO, n_pairs;
    SpecProg prog;
};

template <int KS>
static void spec_launch_ks(sx_handle *h, SpecState *st, const SpecLaunch &a, bool domain) {
    const dim3 grid((unsigned)h->nrings, (unsigned)((a.KO + 63) / 64), (unsigned)a.n_pairs);
    if (domain)
        hipLaunchKernelGGL((k_spectrum<KS, true>), grid, dim3(SPEC_T), 0, h->stream, h->d_A, h->C, st->d_pts, st->d_wz, st->d_wlev, a.vcls,
                           st->nht, a.Zb, h->K2, a.KO, h->has_l, a.prog, st->d_out, st->d_part);
    else
        hipLaunchKernelGGL((k_spectrum<KS, false>), grid, dim3(SPEC_T), 0, h->stream, h->d_A, h->C, st->d_pts, st->d_wz, st->d_wlev, a.vcls,
                           st->nht, a.Zb, h->K2, a.KO, h->has_l, a.prog, st->d_out, st->d_part);
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_spectrum_check(const sx_grid_desc *gd, int32_t n_pairs, const int32_t *pairs) {
    clear_error();
    if (!desc_ok(gd, "sx_spectrum_check")) return 1;
    if (n_pairs < 0 || n_pairs > SPEC_PAIRS) { set_error("sx_spectrum: n_pairs must be 0 .. 16"); return 1; }
    if (n_pairs > 0 && !pairs) { set_error("sx_spectrum: null pairs with n_pairs > 0"); return 1; }
    const bool has_z = gd->geometry == SX_GEOM_RZ || gd->geometry == SX_GEOM_RLZ;
    if (has_z && (gd->b_zDim > 0 ? gd->b_zDim : default_bzdim(gd->zDim)) > 128) { set_error("sx_spectrum: b_zDim above 128 is not supported"); return 1; }
    for (int p = 0; p < n_pairs; p++)
        for (int s = 0; s < 2; s++) {
            const int32_t var = pairs[4 * p + 2 * s], slot = pairs[4 * p + 2 * s + 1];
            const std::string at = "sx_spectrum: pair " + std::to_string(p) + (s ? ", plane b: " : ", plane a: ");
            if (var < 1 || var > gd->nvars) { set_error(at + "var = " + std::to_string(var) + " is 1-based and at most nvars"); return 1; }
            if (slot < 0 || slot > 4) { set_error(at + "slot = " + std::to_string(slot) + " is none of the 5 slots u, r, rr, z, zz (0 .. 4)"); return 1; }
            if (slot > 2 && !has_z) { set_error(at + "slot = " + std::to_string(slot) + " (z, zz): the grid has no vertical"); return 1; }
        }
    return 0;
}

int sx_spectrum(sx_handle *h, int32_t kind, int32_t n_pairs, const int32_t *pairs, double *out) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    if (kind != SX_SPEC_RING && kind != SX_SPEC_DOMAIN) { set_error("sx_spectrum: kind must be SX_SPEC_RING or SX_SPEC_DOMAIN"); return 1; }
    const sx_grid_desc gd = desc_of(h);
    if (sx_spectrum_check(&gd, n_pairs, pairs)) return 1;
    if (n_pairs == 0) return 0;
    if (!out) { set_error("sx_spectrum: null out with n_pairs > 0"); return 1; }
    const EvalClasses *cls = eval_classes(h);
    if (!cls) return 1;
    SpecState *st = spec_state(h, cls->vert);
    if (!st) return 1;
    flush_diag(h);

    static const int RAD[5] = {0, 1, 2, 0, 0}, ROW[5] = {0, 0, 0, 1, 2};      // slot u, r, rr, z, zz -> radial weights, vertical row
    SpecLaunch a;
    std::memset(&a.prog, 0, sizeof(a.prog));
    a.vcls = cls->d_vcls;
    a.Zb = h->has_z ? h->Zb : 1;
    a.KO = 2 * (h->kDim + 1);
    a.n_pairs = n_pairs;
    std::vector<bool> plane((size_t)h->V * 5, false);
    for (int p = 0; p < n_pairs; p++) {
        const int32_t *q = pairs + 4 * p;
        a.prog.va[p] = (q[0] - 1); a.prog.da[p] = RAD[q[1]]; a.prog.ra[p] = ROW[q[1]];
        a.prog.vb[p] = (q[2] - 1); a.prog.db[p] = RAD[q[3]]; a.prog.rb[p] = ROW[q[3]];
        a.prog.same[p] = q[0] == q[2] && q[1] == q[3];
        plane[(size_t)(q[0] - 1) * 5 + q[1]] = plane[(size_t)(q[2] - 1) * 5 + q[3]] = true;
    }
    const int K = h->kDim + 1;
    const bool domain = kind == SX_SPEC_DOMAIN;
    const size_t n_ring = (size_t)K * h->nrings * n_pairs, n_res = domain ? (size_t)K * n_pairs : n_ring;
    if (!st->d_out.grow(n_res, "sx_spectrum") || (domain && !st->d_part.grow(n_ring, "sx_spectrum"))) return 1;
    // the A traffic: every distinct (var, slot) plane reads 4 rows x b_zDim x (2 kmax + 1) doubles per ring
    const double n_planes = (double)std::count(plane.begin(), plane.end(), true);
    double a_bytes = 0;
    for (int i = 0; i < h->nrings; i++) a_bytes += n_planes * 8.0 * 4.0 * a.Zb * (h->has_l ? 2 * st->kcap[i] + 1 : 1);

    {
        TimedLaunch scope(h, "k_spectrum", a_bytes);
        if (a.Zb <= 16) spec_launch_ks<4>(h, st, a, domain);
        else if (a.Zb <= 48) spec_launch_ks<12>(h, st, a, domain);
        else spec_launch_ks<32>(h, st, a, domain);
    }
    if (domain) {
        {
            TimedLaunch scope(h, "k_spectrum_final", 0.0);
            hipLaunchKernelGGL(k_spectrum_final, dim3((unsigned)((K + 15) / 16), (unsigned)n_pairs), dim3(SPEC_T), 0, h->stream, st->d_part,
                               st->d_wring, h->nrings, K, st->d_out);
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
