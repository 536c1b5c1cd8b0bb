// sx_harmonics: the azimuthal harmonics c_k(r, z) of the spectral state at arbitrary radii and heights (include/scythe_hip.h).
//
// The A coefficients already are the decomposition: block 2k / 2k + 1 holds the real / imaginary part of wavenumber k, so
//   c_k(r, z) = sum_node sum_zm (A[zm, 2k, node] + i A[zm, 2k + 1, node]) phi_node(r) Wz[zm](z)
// is a radial spline evaluation times a vertical operator row - no Fourier transform, nothing but A is read.  The host forms what
// depends on r (the 4 radial weights of phi, phi', phi'' and the wavenumber cap: eval_radial_pt, the function sx_evaluate
// uses) and on z (the rows of the vertical operator, packed by height_tiles), the kernel does the two sums:
//   stage 1, radial    s_d[zm][blk] = sum_{j < 4} w_d[j] A[cell + j][v, zm, blk]          d = phi, phi', phi''
//   stage 2, vertical  out_slot[zj][blk] = sum_zm Wz_row[zj][zm] s_d[zm][blk]             a (n_z x b_zDim) (b_zDim x K2) product
// A wave owns 16 blocks of one (radius, variable).  Stage 1 leaves s_d in registers in the B-operand layout of
// v_mfma_f64_16x16x4 (lane = (zm & 3) * 16 + block: the layout k_colmat_mfma reads its coefficient rows in, 16 blocks = one 128-byte
// line per zm), stage 2 multiplies it by 16-height tiles of the weight table, which the workgroup stages through LDS, and stores the
// 16 x 16 result tile as 128-byte lines.  Heights and modes are zero-padded to the tile: every shape runs the same instructions.
// One radius per workgroup row: which lane sums what, and in which order, depends on the grid, the heights and the mask alone.
#include "sx_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

constexpr int HARM_T = 256;                         // 4 waves x 16 blocks
constexpr size_t HARM_SCRATCH = (size_t)256 << 20;  // device result bytes per launch aimed at (one radius always fits)

struct HarmState : DiagState {
    DevBuf<RadialPt> d_pts;         // the radii of a launch, sorted by cell
    DevBuf<double> d_wz, d_res;
};

typedef double harm_d4 __attribute__((ext_vector_type(4)));

// grid (ceil(KO / 64), radii of the chunk, V).  KS: K steps of 4 modes held in registers (4 KS >= b_zDim); DR: phi' and phi'' too.
// wz [cls][height tile][row 3][Zp][16 heights], Zp = b_zDim rounded up to 4: a tile is one contiguous piece, and the A operand of
// K step ks, row `row` is tile[row Zp 16 + 64 ks + lane].  res [slot][v][radius][height][KO].
template <int KS, bool DR>
__global__ __launch_bounds__(HARM_T) void k_harmonics(const double *__restrict__ A, int64_t C, const RadialPt *__restrict__ pts,
                                                      const double *__restrict__ wz, const int *__restrict__ vcls, int nht, int Zb,
                                                      int K2, int KO, int has_l, int mask, int nz, int nrc, int V,
                                                      double *__restrict__ res) {
    constexpr int ND = DR ? 3 : 1;
    __shared__ double tile[3 * KS * 4 * 16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, kk = lane >> 4;
    const int v = blockIdx.z, Zp = (Zb + 3) & ~3;
    const RadialPt *__restrict__ pt = pts + blockIdx.y;
    const int cell = pt->cell, live = has_l ? 2 * pt->kcap + 1 : 0, orig = pt->orig;
    const int blk = (blockIdx.x * 4 + wave) * 16 + n;
    const bool on = blk < K2 && blk <= live && blk != 1;       // block 1 is the padding block: never read
    double w[ND][4];
#pragma unroll
    for (int d = 0; d < ND; d++)
#pragma unroll
        for (int j = 0; j < 4; j++) w[d][j] = pt->wr[d * 4 + j];

    // stage 1: the radial sums of this lane's (zm = 4 ks + kk, blk), the fma chain of k_evaluate
    double b[ND][KS];
    const double *__restrict__ Av = A + (int64_t)cell * C + (int64_t)v * Zb * K2 + blk;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
        const int zm = 4 * ks + kk;
        const bool ld = on && zm < Zb;
        double a[4];
#pragma unroll
        for (int j = 0; j < 4; j++) a[j] = ld ? Av[(int64_t)j * C + (int64_t)zm * K2] : 0.0;
#pragma unroll
        for (int d = 0; d < ND; d++) b[d][ks] = fma(w[d][3], a[3], fma(w[d][2], a[2], fma(w[d][1], a[1], w[d][0] * a[0])));
    }

    // stage 2: 16 heights x 16 blocks per slot on the matrix cores, K = b_zDim in steps of 4
    const double *__restrict__ wzc = wz + (size_t)vcls[v] * nht * 3 * Zp * 16;
    for (int ht = 0; ht < nht; ht++) {
        __syncthreads();
        // only the rows the mask needs (row 0: u, r, rr; row 1: z; row 2: zz), each at its fixed place in the tile
        for (int row = 0; row < 3; row++)
            if (mask & (row == 0 ? 7 : 4 << row))
                for (int i = tid; i < Zp * 16; i += HARM_T) tile[row * Zp * 16 + i] = wzc[((size_t)ht * 3 + row) * Zp * 16 + i];
        __syncthreads();
        int si = 0;
#pragma unroll
        for (int s = 0; s < 5; s++) {
            if (!((mask >> s) & 1)) continue;
            if (DR || (s != 1 && s != 2)) {
                const int row = s < 3 ? 0 : s - 2, d = DR ? (s == 1 ? 1 : s == 2 ? 2 : 0) : 0;
                harm_d4 acc = harm_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int ks = 0; ks < KS; ks++)
                    if (4 * ks < Zb) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(tile[row * Zp * 16 + ks * 64 + lane], b[d][ks], acc, 0, 0, 0);
                if (blk < KO) {
                    double *__restrict__ dst = res + ((((int64_t)si * V + v) * nrc + orig) * nz) * KO + blk;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int zj = ht * 16 + kk + 4 * r;
                        if (zj < nz) dst[(int64_t)zj * KO] = on ? acc[r] : 0.0;      // k > kcap, Im c_0: exact zeros
                    }
                }
            }
            si++;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct HarmLaunch {
    const double *wz;
    const int *vcls;
    int nht, Zb, KO, mask, nslots, nz;
};

template <int KS>
static void harm_launch_ks(sx_handle *h, HarmState *st, const HarmLaunch &a, int nrc) {
    const dim3 grid((unsigned)((a.KO + 63) / 64), (unsigned)nrc, (unsigned)h->V);
    if (a.mask & 6)
        hipLaunchKernelGGL((k_harmonics<KS, true>), grid, dim3(HARM_T), 0, h->stream, h->d_A, h->C, st->d_pts, a.wz, a.vcls, a.nht, a.Zb,
                           h->K2, a.KO, h->has_l, a.mask, a.nz, nrc, h->V, st->d_res);
    else
        hipLaunchKernelGGL((k_harmonics<KS, false>), grid, dim3(HARM_T), 0, h->stream, h->d_A, h->C, st->d_pts, a.wz, a.vcls, a.nht, a.Zb,
                           h->K2, a.KO, h->has_l, a.mask, a.nz, nrc, h->V, st->d_res);
}

// one launch: the radii [r0, r0 + n) of the call; tmp [KO, nz, n_r, V, nslots] column-major
// bytes: the A traffic of the call so far, this launch's added (4 rows x b_zDim x (2 kcap + 1) per radius and variable)
static bool harm_chunk(sx_handle *h, HarmState *st, const EvalGeom &g, const double *radii, int n_all, int r0, int n, int flags,
                       const HarmLaunch &a, double *tmp, double &bytes) {
    std::vector<RadialPt> pts(n);
    for (int i = 0; i < n; i++) {
        RadialPt &e = pts[i];
        eval_radial_pt(g, radii[r0 + i], flags, e.wr, e.cell, e.kcap);
        e.orig = i;
        e.pad = 0;
        bytes += 8.0 * 4.0 * a.Zb * (h->has_l ? 2 * e.kcap + 1 : 1) * h->V;
    }
    // by cell (neighbouring workgroups then read the same 4 rows); within a cell the caller's order
    std::stable_sort(pts.begin(), pts.end(), [](const RadialPt &x, const RadialPt &y) { return x.cell < y.cell; });
    HIPCHK(hipMemcpyAsync(st->d_pts, pts.data(), sizeof(RadialPt) * n, hipMemcpyHostToDevice, h->stream));
    if (error_status()) return false;
    {
        TimedLaunch scope(h, "k_harmonics", bytes);
        if (a.Zb <= 16) harm_launch_ks<4>(h, st, a, n);
        else if (a.Zb <= 48) harm_launch_ks<12>(h, st, a, n);
        else harm_launch_ks<32>(h, st, a, n);
    }
    // device [slot][v][radius of the chunk][height][KO]: per (slot, v) one contiguous piece of the caller's array
    const size_t piece = (size_t)n * a.nz * a.KO;
    for (int q = 0; q < a.nslots * h->V; q++)
        HIPCHK(hipMemcpyAsync(tmp + ((size_t)q * n_all + r0) * a.nz * a.KO, st->d_res + (size_t)q * piece, sizeof(double) * piece,
                              hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));       // pts is reused by the next chunk
    return !error_status();
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_harmonics(sx_handle *h, const double *radii, int32_t n_r, const double *heights, int32_t n_z, int32_t flags, int32_t slot_mask,
                 double *out) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    if (n_r < 0 || n_z < 0) { set_error("sx_harmonics: n_r or n_z is negative"); return 1; }
    if (flags != SX_EVAL_RING_K && flags != SX_EVAL_ALL_K) { set_error("sx_harmonics: flags must be SX_EVAL_RING_K or SX_EVAL_ALL_K"); return 1; }
    const int allowed = h->has_z ? 31 : 7;
    if (slot_mask == 0 || (slot_mask & ~allowed)) {
        set_error(h->has_z ? "sx_harmonics: slot_mask must name at least one of the 5 slots u, r, rr, z, zz (bits 0..4)"
                           : "sx_harmonics: slot_mask must name at least one of u, r, rr (bits 0..2): the grid has no vertical");
        return 1;
    }
    if (!h->has_z && (heights || n_z != 0)) { set_error("sx_harmonics: the grid has no vertical: heights must be NULL and n_z 0"); return 1; }
    if (h->has_z && n_z > 0 && !heights) { set_error("sx_harmonics: null argument"); return 1; }
    if (h->Zb > 128) { set_error("sx_harmonics: b_zDim above 128 is not supported"); return 1; }
    const EvalGeom g = eval_geom_of(h);
    std::string why;
    for (int i = 0; i < n_z; i++)
        if (!eval_height_ok(g, heights[i], why)) { set_error("sx_harmonics: height " + std::to_string(i) + ": " + why); return 1; }
    if (n_r > 0 && !radii) { set_error("sx_harmonics: null argument"); return 1; }
    for (int i = 0; i < n_r; i++)
        if (!eval_radius_ok(g, radii[i], why)) { set_error("sx_harmonics: radius " + std::to_string(i) + ": " + why); return 1; }
    const int nz = h->has_z ? n_z : 1;
    if (n_r == 0 || nz == 0) return 0;
    if (!out) { set_error("sx_harmonics: null argument"); return 1; }
    const EvalClasses *cls = eval_classes(h);
    if (!cls) return 1;
    if (!h->diag[DIAG_HARM]) h->diag[DIAG_HARM].reset(new HarmState());
    HarmState *st = diag_state<HarmState>(h, DIAG_HARM);
    flush_diag(h);

    HarmLaunch a;
    a.Zb = h->has_z ? h->Zb : 1;
    a.KO = 2 * (h->kDim + 1);
    a.mask = slot_mask;
    a.nslots = __builtin_popcount((unsigned)slot_mask);
    a.nz = nz;
    a.nht = (nz + 15) / 16;
    // the height weight table, once per call
    const std::vector<double> wz = height_tiles(cls->vert, heights, nz, h->zmin, h->zmax, h->nz, a.Zb);
    const size_t per_r = (size_t)a.nslots * h->V * nz * a.KO;
    // radii per launch: the scratch bound, and the y extent of a grid
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n_r, HARM_SCRATCH / (per_r * sizeof(double)), (size_t)32768}));
    const char *who = "sx_harmonics";
    if (!st->d_pts.grow((size_t)chunk, who) || !st->d_wz.grow(wz.size(), who) || !st->d_res.grow(per_r * chunk, who)) return 1;
    HIPCHK(hipMemcpyAsync(st->d_wz, wz.data(), sizeof(double) * wz.size(), hipMemcpyHostToDevice, h->stream));
    if (error_status()) return 1;
    a.wz = st->d_wz;
    a.vcls = cls->d_vcls;
    // the results of every launch are held back until all of them have succeeded: a failed call writes nothing to out
    std::vector<double> tmp(per_r * n_r);
    double bytes = 0;
    for (int r0 = 0; r0 < n_r; r0 += chunk)
        if (!harm_chunk(h, st, g, radii, n_r, r0, std::min(chunk, n_r - r0), flags, a, tmp.data(), bytes)) return 1;
    std::memcpy(out, tmp.data(), sizeof(double) * tmp.size());
    return error_status();
}

}  // extern "C"
