// HIP kernels (gfx950) for the Scythe.jl spectral-transform time-stepping path: transforms, banded solve, pack and check kernels
// and their launchers.  The equation sets are in sx_physics.hip.
//
// Device data layout:
//   spectral   A, B     [radial node m][col]            col = (v * Zb + zm) * K2 + blk   (blk fastest)
//                       blk = 0: k = 0;  1: unused (zero);  2k: Re k;  2k+1: Im k   => (Re, Im) pairs are 16-B aligned
//   Az                  [tile node j][v][sz][z][blk]    sz = value, d/dz, d2/dz2 (z already inverted)
//   physical            [slot][v][point]                point = (pstart[ring] + l) * nz + z   (reference layout)
//   var_np1, expdot_*   [v][point]
//   Fl                  [ring][v][z][blk]               ring spectra of var_np1
//   Bz                  [tile node j][v][z][blk]        radial inner products before the vertical transform
// The radial node is the slowest index of every spectral array so that (a) the banded solve runs one lane per
// right-hand side with perfectly coalesced rows, (b) radial evaluation / inner products stream whole rows,
// (c) a tile's halo (3 nodes) is one contiguous block.
#include "sx_internal.hpp"
#include <cmath>

namespace sx {

constexpr int ZC = 16;   // z-levels per workgroup in the ring kernels: 16 * 8 B = one 128-B line per (ring point)

// ------------------------------------------------------------------------------------------------ vertical transforms
// Dense Chebyshev collocation products on spectral-sized data, one "job" per (variable, operator):
//   out[row][job.out_off + o*K2 + blk] = sum_i M[job.mat_off + o*n_in + i] * in[row0 + row][job.in_off + i*K2 + blk]
// inverse: in = A rows, M = Mz[v][sz] (b -> value / d/dz / d2/dz2 incl. BC projection), out = Az
// forward: in = Bz rows, M = CB (values -> truncated b), out = B
// Workgroup = 64 wavenumber blocks x 4 output groups; the input tile sits in LDS, the operator entries are
// wave-uniform (scalar loads), every thread accumulates 4 outputs per pass over the input.
__global__ void __launch_bounds__(256)
k_colmat(const double *__restrict__ in, double *__restrict__ out, const double *__restrict__ mats,
         const ColJob *__restrict__ jobs, int n_in, int n_out, int K2, int64_t in_row, int64_t out_row, int row0) {
    extern __shared__ double As[];
    const int lane = threadIdx.x;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.y);     // blockDim.x == 64: one wave per g => operator
    const int blk = blockIdx.x * 64 + lane;                         // entries become scalar loads
    const ColJob job = jobs[blockIdx.y];
    const double *src = in + (int64_t)(row0 + blockIdx.z) * in_row + job.in_off;
    double *dst = out + (int64_t)blockIdx.z * out_row + job.out_off;
    const double *M = mats + job.mat_off;
    const bool ok = blk < K2;
    for (int i = g; i < n_in; i += 4) As[i * 64 + lane] = ok ? src[(int64_t)i * K2 + blk] : 0.0;
    __syncthreads();
    for (int o0 = g * 4; o0 < n_out; o0 += 16) {
        const double *m0 = M + (int64_t)o0 * n_in;
        const double *m1 = M + (int64_t)min(o0 + 1, n_out - 1) * n_in;
        const double *m2 = M + (int64_t)min(o0 + 2, n_out - 1) * n_in;
        const double *m3 = M + (int64_t)min(o0 + 3, n_out - 1) * n_in;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int i = 0; i < n_in; i++) {
            const double x = As[i * 64 + lane];
            a0 += m0[i] * x;
            a1 += m1[i] * x;
            a2 += m2[i] * x;
            a3 += m3[i] * x;
        }
        if (ok) {
            dst[(int64_t)o0 * K2 + blk] = a0;
            if (o0 + 1 < n_out) dst[(int64_t)(o0 + 1) * K2 + blk] = a1;
            if (o0 + 2 < n_out) dst[(int64_t)(o0 + 2) * K2 + blk] = a2;
            if (o0 + 3 < n_out) dst[(int64_t)(o0 + 3) * K2 + blk] = a3;
        }
    }
}

// The same product on the f64 matrix cores for n_out a multiple of 16 (zDim 32 / 64 / 128): wave = (16 wavenumber blocks) x
// all n_out outputs, K = n_in in steps of 4.  B comes straight from the A-coefficient rows (16 consecutive blocks = one
// 128-byte line per k), the operator fragments are shared by every wave of the launch (L1 / L2 resident), the result
// tile is stored as 128-byte lines: no LDS, no barrier, and the scalar operator loads of k_colmat (its limiter) are gone.
typedef double colmat_d4 __attribute__((ext_vector_type(4)));

// CT = column tiles (16 wavenumber blocks each) per wave: a tile's operator fragments are fetched once per wave and row tile
// and serve CT column tiles.  At 128 levels every wave pulls the whole 87 KB operator through L2 (6.7 GB per step at config 5
// with CT = 1, three times the kernel's HBM bytes): CT = 2 there.
template <int MT, class OT = double, int CT = 1>          // n_out / 16; OT = float: the fp32 spectral-intermediate mode (storage_f32 = 2)
__global__ void __launch_bounds__(256)
k_colmat_mfma(const double *__restrict__ in, OT *__restrict__ out, const double *__restrict__ mats,
              const ColJob *__restrict__ jobs, int n_in, int K2, int64_t in_row, int64_t out_row, int row0) {
    constexpr int n_out = MT * 16;
    constexpr int KSTEPS = MT * 4;          // K = n_in <= n_out in steps of 4, fully unrolled (rows beyond n_in contribute zeros)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = lane & 15, kk = lane >> 4;
    const int blk0 = (blockIdx.x * 4 + wave) * 16 * CT;
    if (blk0 >= K2) return;
    const ColJob job = jobs[blockIdx.y];
    const double *src = in + (int64_t)(row0 + blockIdx.z) * in_row + job.in_off;
    OT *dst = out + (int64_t)blockIdx.z * out_row + job.out_off;
    const double *MTr = mats + job.mat_off;                // operator transposed: [n_in][n_out]
    // Every B element (coefficient row k, block n) of this wave is requested before the first MFMA, and each tile's operator
    // fragments (L2-resident) before that tile's chain: with the loads inside the K loop every step of 4 waited for its own
    // round trip (11 in a row at b_zDim 43).
    double b[CT][KSTEPS];
#pragma unroll
    for (int c = 0; c < CT; c++) {
        const int blk = min(blk0 + c * 16 + n, K2 - 1);
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) {
            const int k = 4 * ks + kk;
            b[c][ks] = (k < n_in) ? src[(int64_t)k * K2 + blk] : 0.0;
        }
    }
#pragma unroll
    for (int t = 0; t < MT; t++) {
        double a[KSTEPS];
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) {
            const int k = 4 * ks + kk;
            a[ks] = (k < n_in) ? MTr[(int64_t)k * n_out + t * 16 + n] : 0.0;      // A[m = lane & 15][k], 128-byte rows
        }
#pragma unroll
        for (int c = 0; c < CT; c++) {
            colmat_d4 acc = colmat_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ks++)
                if (4 * ks < n_in) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b[c][ks], acc, 0, 0, 0);
            if (blk0 + c * 16 + n < K2) {
#pragma unroll
                for (int r = 0; r < 4; r++) dst[(int64_t)(t * 16 + kk + 4 * r) * K2 + blk0 + c * 16 + n] = (OT)acc[r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ radial + azimuthal inverse
// One workgroup per (z-chunk, variable, ring): radial evaluation (4 rows of Az), phase reference, truncated inverse
// DFT with lambda-derivatives, stores straight into the reference physical layout (z innermost => 128-B lines).
template <class ST>
__global__ void __launch_bounds__(256)
k_rl_inverse(const double *__restrict__ Az, Planes<ST> phys, const double *__restrict__ phi,
             const int *__restrict__ Lr, const int *__restrict__ kmaxr, const int64_t *__restrict__ pstart,
             const int64_t *__restrict__ twoff, const double2 *__restrict__ tw, const int64_t *__restrict__ phoff,
             const double2 *__restrict__ ph, int V, int nz, int nsz, int K2, int nrings, int64_t N, int64_t azrow,
             int s_u, int s_r, int s_rr, int s_l, int s_ll, int s_z, int s_zz, int has_l, int cstride,
             const int *__restrict__ slotmask) {
    extern __shared__ double sm[];
    const int ring = blockIdx.z, v = blockIdx.y, z0 = blockIdx.x * ZC;
    const int mask = slotmask[v];
    const int zc = min(ZC, nz - z0);
    const int L = Lr[ring], km = has_l ? kmaxr[ring] : 0;
    const int j0 = ring / MUBAR;
    double *cR = sm, *cI = sm + (size_t)ZC * cstride;
    const double2 *twr = tw + twoff[ring];
    const double2 *phr = ph + phoff[ring];
    const int64_t p0 = pstart[ring];
    const int tid = threadIdx.x;

    for (int q = 0; q < 5; q++) {
        // coefficient line q: (sz, d) = (0,0) (0,1) (0,2) (1,0) (2,0)
        const int sz = q < 3 ? 0 : q - 2, d = q < 3 ? q : 0;
        if (sz >= nsz) break;
        const int slot0 = (q == 0) ? s_u : (q == 1) ? s_r : (q == 2) ? s_rr : (q == 3) ? s_z : s_zz;
        const bool need0 = (mask >> slot0) & 1;
        const bool needl = (q == 0) && has_l && ((mask >> s_l) & 1), needll = (q == 0) && has_l && ((mask >> s_ll) & 1);
        if (!need0 && !needl && !needll) continue;
        const double *p = phi + ((int64_t)d * nrings + ring) * 4;
        const double f0 = p[0], f1 = p[1], f2 = p[2], f3 = p[3];
        __syncthreads();
        for (int e = tid; e < zc * (km + 1); e += blockDim.x) {
            const int k = e % (km + 1), zz = e / (km + 1);
            const double *a = Az + (int64_t)j0 * azrow + (((int64_t)v * nsz + sz) * nz + (z0 + zz)) * K2;
            double cr, ci = 0.0;
            if (k == 0) {
                cr = f0 * a[0] + f1 * a[azrow] + f2 * a[2 * azrow] + f3 * a[3 * azrow];
            } else {
                const int b = 2 * k;
                cr = f0 * a[b] + f1 * a[azrow + b] + f2 * a[2 * azrow + b] + f3 * a[3 * azrow + b];
                ci = f0 * a[b + 1] + f1 * a[azrow + b + 1] + f2 * a[2 * azrow + b + 1] + f3 * a[3 * azrow + b + 1];
                const double2 w = phr[k];          // e^{+i k off}
                const double tr = cr * w.x - ci * w.y;
                ci = cr * w.y + ci * w.x;
                cr = 2.0 * tr;
                ci = 2.0 * ci;
            }
            cR[zz * cstride + k] = cr;
            cI[zz * cstride + k] = ci;
        }
        __syncthreads();
        const bool lamder = needl || needll;
        for (int o = tid; o < L * zc; o += blockDim.x) {
            const int zz = o % zc, l = o / zc;
            const double *r = cR + zz * cstride, *im = cI + zz * cstride;
            double a0 = r[0], a1 = 0.0, a2 = 0.0;
            int idx = 0;
            for (int k = 1; k <= km; k++) {
                idx += l;
                if (idx >= L) idx -= L;
                const double2 t = twr[idx];
                const double val = r[k] * t.x - im[k] * t.y;
                a0 += val;
                if (lamder) {
                    a1 -= k * (im[k] * t.x + r[k] * t.y);
                    a2 -= (double)k * k * val;
                }
            }
            const int64_t pt = (p0 + l) * nz + z0 + zz;
            if (need0) {
                if (slot0 == 0) phys.val[(int64_t)v * N + pt] = a0;
                else phys.der[((int64_t)(slot0 - 1) * V + v) * N + pt] = (ST)a0;
            }
            if (needl) phys.der[((int64_t)(s_l - 1) * V + v) * N + pt] = (ST)a1;
            if (needll) phys.der[((int64_t)(s_ll - 1) * V + v) * N + pt] = (ST)a2;
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward azimuthal
// Fl[ring][v][z][blk] = (1/L) sum_l var_np1[v][(pstart + l) nz + z] e^{-ik lambda_l}
__global__ void __launch_bounds__(256)
k_fl_forward(const double *__restrict__ np1, double *__restrict__ Fl, const int *__restrict__ Lr,
             const int *__restrict__ kmaxr, const int64_t *__restrict__ pstart, const int64_t *__restrict__ twoff,
             const double2 *__restrict__ tw, const int64_t *__restrict__ phoff, const double2 *__restrict__ ph, int V,
             int nz, int K2, int64_t N, int has_l, int xstride) {
    extern __shared__ double sm[];
    const int ring = blockIdx.z, v = blockIdx.y, z0 = blockIdx.x * ZC;
    const int zc = min(ZC, nz - z0);
    const int L = Lr[ring], km = has_l ? kmaxr[ring] : 0;
    const double2 *twr = tw + twoff[ring];
    const double2 *phr = ph + phoff[ring];
    const int64_t p0 = pstart[ring];
    const int tid = threadIdx.x;
    for (int o = tid; o < L * zc; o += blockDim.x) {
        const int zz = o % zc, l = o / zc;
        sm[zz * xstride + l] = np1[(int64_t)v * N + (p0 + l) * nz + z0 + zz];
    }
    __syncthreads();
    const double inv = 1.0 / L;
    for (int e = tid; e < zc * (km + 1); e += blockDim.x) {
        const int k = e % (km + 1), zz = e / (km + 1);
        const double *x = sm + zz * xstride;
        double sr = 0.0, si = 0.0;
        int idx = 0;
        for (int l = 0; l < L; l++) {
            const double2 t = twr[idx];
            sr += x[l] * t.x;
            si -= x[l] * t.y;
            idx += k;
            if (idx >= L) idx -= L;
        }
        double *out = Fl + (((int64_t)ring * V + v) * nz + z0 + zz) * K2;
        if (k == 0) {
            out[0] = sr * inv;
        } else {
            const double2 w = phr[k];              // multiply by e^{-i k off}
            out[2 * k] = (sr * w.x + si * w.y) * inv;
            out[2 * k + 1] = (si * w.x - sr * w.y) * inv;
        }
    }
}

// ------------------------------------------------------------------------------------------------ radial inner products
// Bz[j][e] = sum over the rings of cells j-3..j of wq * phi0 * Fl[ring][e],   e = (v, z, blk) flattened
__global__ void k_sb(const double *__restrict__ Fl, double *__restrict__ Bz, const double *__restrict__ phi,
                     const double *__restrict__ wq, int ncells, int64_t plane) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (e >= plane) return;
    double s = 0.0;
    for (int c = max(0, j - 3); c <= min(ncells - 1, j); c++) {
        const int jj = j - c;
        for (int mu = 0; mu < MUBAR; mu++) {
            const int ring = c * MUBAR + mu;
            s += wq[ring] * phi[(int64_t)ring * 4 + jj] * Fl[(int64_t)ring * plane + e];
        }
    }
    Bz[(int64_t)j * plane + e] = s;
}

// ------------------------------------------------------------------------------------------------ radial inner products + vertical forward
// Fused k_sb + vertical forward transform (RZ / RLZ): the [z][64 blocks] tile of radial inner products of node j stays in
// LDS and is contracted with CB right away, so Bz never goes to HBM.
//   B[j][v][zm][blk] = sum_z CB[zm][z] * sum_{rings of cells j-3..j} wq * phi0 * Fl[ring][v][z][blk]
__global__ void __launch_bounds__(256)
k_sbz(const double *__restrict__ Fl, double *__restrict__ B, const double *__restrict__ phi, const double *__restrict__ wq,
      const double *__restrict__ CB, int ncells, int V, int nz, int Zb, int K2, int64_t C) {
    extern __shared__ double As[];          // [nz][64]
    const int lane = threadIdx.x;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int blk = blockIdx.x * 64 + lane;
    const int v = blockIdx.y, j = blockIdx.z;
    const bool ok = blk < K2;
    const int64_t plane = (int64_t)V * nz * K2;
    const int c0 = max(0, j - 3), c1 = min(ncells - 1, j);
    for (int z = g; z < nz; z += 4) {
        double s = 0.0;
        if (ok) {
            const int64_t e = ((int64_t)v * nz + z) * K2 + blk;
            for (int c = c0; c <= c1; c++) {
                const int jj = j - c;
#pragma unroll
                for (int mu = 0; mu < MUBAR; mu++) {
                    const int ring = c * MUBAR + mu;
                    s += wq[ring] * phi[(int64_t)ring * 4 + jj] * Fl[(int64_t)ring * plane + e];
                }
            }
        }
        As[z * 64 + lane] = s;
    }
    __syncthreads();
    double *dst = B + (int64_t)j * C + (int64_t)v * Zb * K2;
    for (int o0 = g * 4; o0 < Zb; o0 += 16) {
        const double *m0 = CB + (int64_t)o0 * nz;
        const double *m1 = CB + (int64_t)min(o0 + 1, Zb - 1) * nz;
        const double *m2 = CB + (int64_t)min(o0 + 2, Zb - 1) * nz;
        const double *m3 = CB + (int64_t)min(o0 + 3, Zb - 1) * nz;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int i = 0; i < nz; i++) {
            const double x = As[i * 64 + lane];
            a0 += m0[i] * x;
            a1 += m1[i] * x;
            a2 += m2[i] * x;
            a3 += m3[i] * x;
        }
        if (ok) {
            dst[(int64_t)o0 * K2 + blk] = a0;
            if (o0 + 1 < Zb) dst[(int64_t)(o0 + 1) * K2 + blk] = a1;
            if (o0 + 2 < Zb) dst[(int64_t)(o0 + 2) * K2 + blk] = a2;
            if (o0 + 3 < Zb) dst[(int64_t)(o0 + 3) * K2 + blk] = a3;
        }
    }
}

// Sliding-window form of k_sbz for zDim = NZ (multiple of 8): a workgroup walks a run of consecutive radial cells for
// one (variable, 64 wavenumber blocks) and keeps the partial inner products of the 4 nodes a cell touches in registers,
// so every Fl value enters the CU once (k_sbz re-reads it for each of its 4 nodes: 4x the L2 -> L1 traffic, which is
// what bounds it).  Node c is complete once cell c has been added (cells c-3..c); its [NZ][64] tile then goes through
// LDS into the vertical contraction with CB.  A segment starts 3 cells early to warm up its first nodes.
// Summation order per node (cells ascending, mish points ascending) is the same as k_sbz's.
#ifdef SX_PHASES
__device__ long long *g_sbw_dbg = nullptr;     // [workgroup][8]: cycles in load+accumulate, barrier 1, LDS write + barrier 2, contraction + stores; cells; total
#define SBW_T0() long long st_ = (long long)__builtin_readcyclecounter(); const long long st0_ = st_; long long sacc_[4] = {0, 0, 0, 0}; int scells_ = 0
#define SBW_LAP(i) do { const long long n_ = (long long)__builtin_readcyclecounter(); sacc_[i] += n_ - st_; st_ = n_; } while (0)
#define SBW_END() do { if (threadIdx.x == 0 && g_sbw_dbg) { long long *d_ = g_sbw_dbg + ((int64_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8; \
        d_[0] = sacc_[0]; d_[1] = sacc_[1]; d_[2] = sacc_[2]; d_[3] = sacc_[3]; d_[4] = scells_; d_[5] = (long long)__builtin_readcyclecounter() - st0_; } } while (0)
#else
#define SBW_T0() do { } while (0)
#define SBW_LAP(i) do { } while (0)
#define SBW_END() do { } while (0)
#endif

template <int NZ, bool PREFETCH>
__global__ void __launch_bounds__(512, 2)       // second argument: waves per SIMD (one 512-thread workgroup per CU)
k_sbw(const double *__restrict__ Fl, double *__restrict__ B, const double *__restrict__ phi, const double *__restrict__ wq,
      const double *__restrict__ CB, int ncells, int V, int Zb, int K2, int64_t C, int cps) {
    constexpr int ZPT = NZ / 8;
    __shared__ double As[NZ * 64];
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int blk = blockIdx.x * 64 + lane;
    const int v = blockIdx.y;
    const bool ok = blk < K2;
    const int ca = blockIdx.z * cps, cb = min(ca + cps, ncells);
    const int cend = (cb == ncells) ? ncells + 3 : cb;          // the last segment also owns the 3 trailing nodes
    const int cstart = max(0, ca - 3);
    const int64_t plane = (int64_t)V * NZ * K2;
    const double *base = Fl + ((int64_t)v * NZ + g) * K2 + (ok ? blk : 0);
    double *dst0 = B + (int64_t)v * Zb * K2 + blk;
    double acc[4][ZPT];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < ZPT; i++) acc[q][i] = 0.0;
    // The ring spectra of cell c + 1 are requested as soon as cell c has been accumulated, BEFORE its node is contracted: the
    // loads then fly during the LDS contraction instead of starting after it (a workgroup used to have at most ~11 loads
    // per wave in flight and none at all during the contraction; read once: non-temporal, the caches stay with B and the
    // history).
    double xn[PREFETCH ? MUBAR : 1][ZPT];
    auto fetch = [&](int c) {
        if (!PREFETCH || c < cstart || c >= cend || c >= ncells) return;
#pragma unroll
        for (int mu = 0; mu < MUBAR; mu++) {
            const double *src = base + (int64_t)(c * MUBAR + mu) * plane;
#pragma unroll
            for (int i = 0; i < ZPT; i++) xn[mu][i] = __builtin_nontemporal_load(src + (int64_t)(8 * i) * K2);
        }
    };
    fetch(cstart);
    SBW_T0();
    for (int c4 = cstart & ~3; c4 < cend; c4 += 4) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int c = c4 + u;
            if (c < cstart || c >= cend) continue;
#ifdef SX_PHASES
            scells_++;
#endif
            if (c < ncells) {
#pragma unroll
                for (int mu = 0; mu < MUBAR; mu++) {
                    const int ring = c * MUBAR + mu;
                    const double w = wq[ring];
                    const double w0 = w * phi[(int64_t)ring * 4], w1 = w * phi[(int64_t)ring * 4 + 1];
                    const double w2 = w * phi[(int64_t)ring * 4 + 2], w3 = w * phi[(int64_t)ring * 4 + 3];
                    double x[ZPT];
                    if (PREFETCH) {
#pragma unroll
                        for (int i = 0; i < ZPT; i++) x[i] = xn[mu][i];
                    } else {
                        const double *src = base + (int64_t)ring * plane;
#pragma unroll
                        for (int i = 0; i < ZPT; i++) x[i] = __builtin_nontemporal_load(src + (int64_t)(8 * i) * K2);
                    }
#pragma unroll
                    for (int i = 0; i < ZPT; i++) {
                        acc[u][i] += w0 * x[i];
                        acc[(u + 1) & 3][i] += w1 * x[i];
                        acc[(u + 2) & 3][i] += w2 * x[i];
                        acc[(u + 3) & 3][i] += w3 * x[i];
                    }
                }
                fetch(c + 1);           // in flight while node c goes through LDS and the vertical contraction
            }
            SBW_LAP(0);
            if (c >= ca) {                      // node c is complete: vertical forward transform and store
                __syncthreads();                // the previous node's tile has been consumed
                SBW_LAP(1);
#pragma unroll
                for (int i = 0; i < ZPT; i++) As[(g + 8 * i) * 64 + lane] = acc[u][i];
                __syncthreads();
                SBW_LAP(2);
                double *dst = dst0 + (int64_t)c * C;
                for (int o0 = g * 4; o0 < Zb; o0 += 32) {
                    const double *m0 = CB + (int64_t)o0 * NZ;
                    const double *m1 = CB + (int64_t)min(o0 + 1, Zb - 1) * NZ;
                    const double *m2 = CB + (int64_t)min(o0 + 2, Zb - 1) * NZ;
                    const double *m3 = CB + (int64_t)min(o0 + 3, Zb - 1) * NZ;
                    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 8
                    for (int i = 0; i < NZ; i++) {
                        const double xx = As[i * 64 + lane];
                        a0 += m0[i] * xx;
                        a1 += m1[i] * xx;
                        a2 += m2[i] * xx;
                        a3 += m3[i] * xx;
                    }
                    if (ok) {
                        dst[(int64_t)o0 * K2] = a0;
                        if (o0 + 1 < Zb) dst[(int64_t)(o0 + 1) * K2] = a1;
                        if (o0 + 2 < Zb) dst[(int64_t)(o0 + 2) * K2] = a2;
                        if (o0 + 3 < Zb) dst[(int64_t)(o0 + 3) * K2] = a3;
                    }
                }
                SBW_LAP(3);
            }
#pragma unroll
            for (int i = 0; i < ZPT; i++) acc[u][i] = 0.0;      // the slot now belongs to node c + 4
        }
    }
    SBW_END();
}

// The same with the vertical contraction on the f64 matrix cores and the next cell's ring spectra in flight meanwhile
// (zDim 64 / 32; b_zDim <= 64).  Phase stamps of k_sbw (profiles/r02/phases_sbw.txt): 57 % of a workgroup's time was the
// contraction - 11,000 cycles per node against ~1,500 of arithmetic: its operator entries arrive as scalar loads, two
// dependent batches per 8 terms, and with 43 output rows over 8 waves x 4 rows three waves ran a second pass while five
// waited.  Here the operator lives in LDS in MFMA-fragment order for the whole kernel: wave w owns column tile w & 3 (16 wavenumber blocks)
// and the row tiles of its half (w < 4: the first ceil(MT / 2) tiles of 16 modes, else the rest), 16 K-steps of
// v_mfma_f64_16x16x4_f64 per tile with B = the node's [level][block] tile in LDS (row stride 80 doubles: the 4 levels a
// K-step reads fall in disjoint bank halves).  One 512-thread workgroup per CU; the grid is one round.
// Summation order differs from k_sbw / k_sbz (K in blocks of 4): results agree to rounding, not bitwise.
// BW = wavenumber blocks per workgroup: 64 (zDim 32 / 64), or 32 for zDim 128, where the operator fragments (6 row tiles x
// 32 K steps = 96 KB) and the node tile (128 levels x 32 blocks) have to share the 160 KB; then wave w owns column tile
// w & 1 and the row tiles (w >> 1), (w >> 1) + 4.
template <int NZ, int BW = 64, int THREADS = 512, class FT = double>      // FT = float: fp32-stored ring spectra (storage_f32 = 2)
__global__ void __launch_bounds__(THREADS, 2)
k_sbw_mfma(const FT *__restrict__ Fl, double *__restrict__ B, const double *__restrict__ phi, const double *__restrict__ wq,
           const double *__restrict__ CB, int ncells, int V, int Zb, int K2, int64_t C, int cps) {
    constexpr int NG = THREADS / BW;                  // level groups: thread = (group g, block lb), levels z = g + NG i
    constexpr int ZPT = NZ / NG, KS = NZ / 4, LS = BW + 16;      // LS: the 4 levels a K step reads fall in disjoint bank halves
    constexpr int MTMAX = BW == 64 ? 4 : 6;           // row tiles of 16 modes: b_zDim <= 64 / <= 96
    __shared__ double As[NZ * LS];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lb = threadIdx.x & (BW - 1);
    const int g = BW == 64 ? wv : (int)(threadIdx.x / BW);
    const int blk = blockIdx.x * BW + lb;
    const int v = blockIdx.y;
    const bool ok = blk < K2;
    const int ca = blockIdx.z * cps, cb = min(ca + cps, ncells);
    const int cend = (cb == ncells) ? ncells + 3 : cb;          // the last segment also owns the 3 trailing nodes
    const int cstart = max(0, ca - 3);
    const int64_t plane = (int64_t)V * NZ * K2;
    const FT *base = Fl + ((int64_t)v * NZ + g) * K2 + (ok ? blk : 0);
    // operator fragments: A[m][k] = CB[m][k], lane supplies m = 16 mt + (lane & 15), k = 4 js + (lane >> 4)
    const int MT = (Zb + 15) / 16, mhalf = (MT + 1) / 2;
    // this wave's column tile nt and row tiles mt0, mt1 (nmt of them)
    const int nt = BW == 64 ? (wv & 3) : (wv & 1);
    const int mt0 = BW == 64 ? (wv < 4 ? 0 : mhalf) : (wv >> 1);
    const int mt1 = BW == 64 ? mt0 + 1 : mt0 + THREADS / 128;      // BW = 32: two column tiles, the waves of a column tile share the row tiles
    const int nmt = BW == 64 ? (wv < 4 ? mhalf : MT - mhalf) : (mt0 >= MT ? 0 : mt1 < MT ? 2 : 1);
    const int n = lane & 15, kk = lane >> 4;
    // (kept in LDS in fragment order [row tile][K step][lane]: a conflict-free 8-byte read per MFMA; in registers the two
    // tiles' 64 VGPRs pushed the kernel into spills)
    __shared__ double Af[MTMAX * KS * 64];
    for (int e = threadIdx.x; e < MT * KS * 64; e += blockDim.x) {
        const int l = e & 63, js = (e >> 6) % KS, mt = e / (64 * KS);
        const int m = mt * 16 + (l & 15);
        Af[e] = (m < Zb) ? CB[(int64_t)m * NZ + 4 * js + (l >> 4)] : 0.0;
    }
    const double *af0 = Af + (size_t)(nmt > 0 ? mt0 : 0) * KS * 64 + lane, *af1 = Af + (size_t)(nmt > 1 ? mt1 : 0) * KS * 64 + lane;
    double acc[4][ZPT];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < ZPT; i++) acc[q][i] = 0.0;
    FT xn[MUBAR][ZPT];
    auto fetch = [&](int c) {
        if (c < cstart || c >= cend || c >= ncells) return;
#pragma unroll
        for (int mu = 0; mu < MUBAR; mu++) {
            const FT *src = base + (int64_t)(c * MUBAR + mu) * plane;
#pragma unroll
            for (int i = 0; i < ZPT; i++) xn[mu][i] = __builtin_nontemporal_load(src + (int64_t)(NG * i) * K2);
        }
    };
    fetch(cstart);
    SBW_T0();
    for (int c4 = cstart & ~3; c4 < cend; c4 += 4) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int c = c4 + u;
            if (c < cstart || c >= cend) continue;
#ifdef SX_PHASES
            scells_++;
#endif
            if (c < ncells) {
#pragma unroll
                for (int mu = 0; mu < MUBAR; mu++) {
                    const int ring = c * MUBAR + mu;
                    const double w = wq[ring];
                    const double w0 = w * phi[(int64_t)ring * 4], w1 = w * phi[(int64_t)ring * 4 + 1];
                    const double w2 = w * phi[(int64_t)ring * 4 + 2], w3 = w * phi[(int64_t)ring * 4 + 3];
#pragma unroll
                    for (int i = 0; i < ZPT; i++) {
                        const double xv = (double)xn[mu][i];
                        acc[u][i] += w0 * xv;
                        acc[(u + 1) & 3][i] += w1 * xv;
                        acc[(u + 2) & 3][i] += w2 * xv;
                        acc[(u + 3) & 3][i] += w3 * xv;
                    }
                }
                fetch(c + 1);           // in flight while node c goes through LDS and the matrix cores
            }
            SBW_LAP(0);
            if (c >= ca) {                      // node c is complete: vertical forward transform and store
                __syncthreads();                // the previous node's tile has been consumed
                SBW_LAP(1);
#pragma unroll
                for (int i = 0; i < ZPT; i++) As[(g + NG * i) * LS + lb] = acc[u][i];
                __syncthreads();
                SBW_LAP(2);
                colmat_d4 o0 = {0.0, 0.0, 0.0, 0.0}, o1 = o0;
                const double *xb = As + kk * LS + nt * 16 + n;
                if (nmt > 0) {
#pragma unroll
                    for (int js = 0; js < KS; js++) {
                        const double b = xb[(4 * js) * LS];
                        o0 = __builtin_amdgcn_mfma_f64_16x16x4f64(af0[js * 64], b, o0, 0, 0, 0);
                        if (nmt > 1) o1 = __builtin_amdgcn_mfma_f64_16x16x4f64(af1[js * 64], b, o1, 0, 0, 0);
                    }
                }
                // D[row = kk + 4 r][col = n]
                const int col = blockIdx.x * BW + nt * 16 + n;
                if (col < K2) {
                    double *dst = B + (int64_t)c * C + (int64_t)v * Zb * K2 + col;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int m0 = mt0 * 16 + kk + 4 * r, m1 = mt1 * 16 + kk + 4 * r;
                        if (nmt > 0 && m0 < Zb) dst[(int64_t)m0 * K2] = o0[r];
                        if (nmt > 1 && m1 < Zb) dst[(int64_t)m1 * K2] = o1[r];
                    }
                }
                SBW_LAP(3);
            }
#pragma unroll
            for (int i = 0; i < ZPT; i++) acc[u][i] = 0.0;      // the slot now belongs to node c + 4
        }
    }
    SBW_END();
}

// The vertical contraction of k_sbw_mfma on its own, over the node spectra k_fl_forward_cells leaves (sx_fft.hip): a workgroup walks a
// run of nodes for one (variable, BW wavenumber blocks); per node it reads the [NZ levels][BW] tile once - where the node is one of
// the first three of a forward segment behind the first, plus the previous segment's open partial, the earlier segment first -
// and contracts it with CB on the f64 matrix cores exactly as k_sbw_mfma does (operator fragments in LDS, same K order), into
// d_Btile's layout.  The next node's tile is requested before the current one is contracted.
template <int NZ, int BW = 64, int THREADS = 512>
__global__ void __launch_bounds__(THREADS, 2)
k_nodes_z(const double *__restrict__ Fn, const double *__restrict__ Fe, double *__restrict__ B, const double *__restrict__ CB,
          int nbt, int V, int Zb, int K2, int64_t C, int S, int fsegs, int nps) {
    constexpr int NG = THREADS / BW;
    constexpr int ZPT = NZ / NG, KS = NZ / 4, LS = BW + 16;
    constexpr int MTMAX = BW == 64 ? 4 : 6;
    __shared__ double As[NZ * LS];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lb = threadIdx.x & (BW - 1);
    const int g = BW == 64 ? wv : (int)(threadIdx.x / BW);
    const int blk = blockIdx.x * BW + lb;
    const int v = blockIdx.y;
    const bool ok = blk < K2;
    const int na = blockIdx.z * nps, nb = min(na + nps, nbt);
    const int64_t plane = (int64_t)V * NZ * K2;
    const int64_t base = ((int64_t)v * NZ + g) * K2 + (ok ? blk : 0);
    const int MT = (Zb + 15) / 16, mhalf = (MT + 1) / 2;
    const int nt = BW == 64 ? (wv & 3) : (wv & 1);
    const int mt0 = BW == 64 ? (wv < 4 ? 0 : mhalf) : (wv >> 1);
    const int mt1 = BW == 64 ? mt0 + 1 : mt0 + THREADS / 128;
    const int nmt = BW == 64 ? (wv < 4 ? mhalf : MT - mhalf) : (mt0 >= MT ? 0 : mt1 < MT ? 2 : 1);
    const int n = lane & 15, kk = lane >> 4;
    __shared__ double Af[MTMAX * KS * 64];               // operator fragments [row tile][K step][lane], as in k_sbw_mfma
    for (int e = threadIdx.x; e < MT * KS * 64; e += blockDim.x) {
        const int l = e & 63, js = (e >> 6) % KS, mt = e / (64 * KS);
        const int m = mt * 16 + (l & 15);
        Af[e] = (m < Zb) ? CB[(int64_t)m * NZ + 4 * js + (l >> 4)] : 0.0;
    }
    const double *af0 = Af + (size_t)(nmt > 0 ? mt0 : 0) * KS * 64 + lane, *af1 = Af + (size_t)(nmt > 1 ? mt1 : 0) * KS * 64 + lane;
    double xn[ZPT], en[ZPT];
    // node nd is node j of forward segment sg; j < 3 behind the first segment: the previous segment's open partial j belongs to it
    auto fetch = [&](int nd) {
        if (nd >= nb) return;
        const int sg = min(nd / S, fsegs - 1), j = nd - sg * S;
        const double *src = Fn + (int64_t)nd * plane + base;
#pragma unroll
        for (int i = 0; i < ZPT; i++) xn[i] = src[(int64_t)(NG * i) * K2];
        if (sg > 0 && j < 3) {                             // workgroup-uniform
            const double *es = Fe + (int64_t)((sg - 1) * 3 + j) * plane + base;
#pragma unroll
            for (int i = 0; i < ZPT; i++) en[i] = es[(int64_t)(NG * i) * K2];
#pragma unroll
            for (int i = 0; i < ZPT; i++) xn[i] = en[i] + xn[i];
        }
    };
    fetch(na);
    for (int c = na; c < nb; c++) {
        __syncthreads();                // the previous node's tile has been consumed (first node: the operator fragments are in place)
#pragma unroll
        for (int i = 0; i < ZPT; i++) As[(g + NG * i) * LS + lb] = xn[i];
        __syncthreads();
        fetch(c + 1);                   // in flight while node c goes through the matrix cores
        colmat_d4 o0 = {0.0, 0.0, 0.0, 0.0}, o1 = o0;
        const double *xb = As + kk * LS + nt * 16 + n;
        if (nmt > 0) {
#pragma unroll
            for (int js = 0; js < KS; js++) {
                const double b = xb[(4 * js) * LS];
                o0 = __builtin_amdgcn_mfma_f64_16x16x4f64(af0[js * 64], b, o0, 0, 0, 0);
                if (nmt > 1) o1 = __builtin_amdgcn_mfma_f64_16x16x4f64(af1[js * 64], b, o1, 0, 0, 0);
            }
        }
        // D[row = kk + 4 r][col = n]
        const int col = blockIdx.x * BW + nt * 16 + n;
        if (col < K2) {
            double *dst = B + (int64_t)c * C + (int64_t)v * Zb * K2 + col;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int m0 = mt0 * 16 + kk + 4 * r, m1 = mt1 * 16 + kk + 4 * r;
                if (nmt > 0 && m0 < Zb) dst[(int64_t)m0 * K2] = o0[r];
                if (nmt > 1 && m1 < Zb) dst[(int64_t)m1 * K2] = o1[r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ B -> A banded SPD solve
// One lane per right-hand side (column); rows are contiguous across lanes so every load/store is coalesced.
// a = Gamma^T (L L^T)^-1 Gamma b with L banded (half-bandwidth 3) plus, for PERIODIC, three dense last rows.
// A wave covers 64 consecutive wavenumber blocks of one (variable, z-mode): its boundary-condition class is
// wave-uniform, so the factor entries are scalar loads. The k = 0 column (its own class) is handled by one extra
// block per (variable, z-mode) in which only lane 0 works.
// scalar / pair arithmetic so that one kernel body serves a lane that owns one column (k = 0) or the (Re, Im) pair of a
// wavenumber (two independent right-hand sides moved as one 16-byte access)
struct S1 { double x; };
struct S2 { double x, y; };
__device__ __forceinline__ S1 ld(const double *p, S1 *) { return S1{p[0]}; }
__device__ __forceinline__ S2 ld(const double *p, S2 *) { const double2 v = *reinterpret_cast<const double2 *>(p); return S2{v.x, v.y}; }
__device__ __forceinline__ void st(double *p, S1 v) { p[0] = v.x; }
__device__ __forceinline__ void st(double *p, S2 v) { *reinterpret_cast<double2 *>(p) = make_double2(v.x, v.y); }
__device__ __forceinline__ S1 operator+(S1 a, S1 b) { return S1{a.x + b.x}; }
__device__ __forceinline__ S2 operator+(S2 a, S2 b) { return S2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ S1 operator-(S1 a, S1 b) { return S1{a.x - b.x}; }
__device__ __forceinline__ S2 operator-(S2 a, S2 b) { return S2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ S1 operator*(double c, S1 a) { return S1{c * a.x}; }
__device__ __forceinline__ S2 operator*(double c, S2 a) { return S2{c * a.x, c * a.y}; }
__device__ __forceinline__ S1 zero(S1 *) { return S1{0.0}; }
__device__ __forceinline__ S2 zero(S2 *) { return S2{0.0, 0.0}; }

// row m of the right-hand side from the LDS offset table: first source + (second source if the global table has one)
template <class T>
__device__ __forceinline__ T brow2(const double *__restrict__ B, const int64_t *sofs, int m, int64_t col) {
    const T x = ld(B + sofs[m * 4 + 0] + col, (T *)nullptr), y = ld(B + sofs[m * 4 + 1] + col, (T *)nullptr);
    return x + (sofs[m * 4 + 1] != sofs[m * 4 + 0] ? 1.0 : 0.0) * y;
}

// Row m of the right-hand side is Bsrc[boffA[m] + col] (+ Bsrc[boffB[m] + col] where a second tile overlaps, boffB >= 0);
// row m of the solution goes to A[aoffA[m] + col] and, in the final sweep, also to A[aoffB[m] + col] if aoffB >= 0.
// SOLVE_U rows per batch: 8 when the launch fills the chip (single-tile solve: bandwidth-bound, A/B 750 -> 755 steps/s),
// 16 for the transposed multi-GPU solve, whose few waves are latency-bound (8 there: 0.058 -> 0.098 ms)
template <class T, bool LINEAR, int SOLVE_U>
__device__ __forceinline__ void solve_columns(const double *__restrict__ Bsrc, const int64_t *__restrict__ boffA,
                                              const int64_t *__restrict__ boffB, double *__restrict__ A,
                                              const int64_t *__restrict__ aoffA, const int64_t *__restrict__ aoffB,
                                              const int *__restrict__ cmeta, const double *__restrict__ gl,
                                              const double *__restrict__ gr, const double *__restrict__ Lband,
                                              const double *__restrict__ Ldinv, const double *__restrict__ Larrow, int nb, int c,
                                              int64_t col, int64_t stride, bool active) {
    const int n = cmeta[c * 4 + 0], per = cmeta[c * 4 + 1], rl = cmeta[c * 4 + 2], rr = cmeta[c * 4 + 3];
    const double *Lb = Lband + (int64_t)c * nb * 4;
    const double *Ld = Ldinv + (int64_t)c * nb;
    // The factor rows (l0, l1, l2, 1 / diagonal) of this boundary-condition class go to LDS once per workgroup: as scalar
    // loads from memory they could not be fetched a batch ahead (16 rows x 5 doubles exceed the scalar registers), and
    // every couple of rows waited ~500 cycles for its own scalar load - the whole run time of the kernel.
    extern __shared__ double sfac[];              // [nb][4] factor rows, then (not LINEAR) [nb][4] row offsets
    int64_t *sofs = reinterpret_cast<int64_t *>(sfac + (size_t)nb * 4);
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const double4 l4 = *reinterpret_cast<const double4 *>(Lb + (int64_t)e * 4);
        *reinterpret_cast<double4 *>(sfac + (size_t)e * 4) = make_double4(l4.x, l4.y, l4.z, Ld[e]);
    }
    if (!LINEAR)
        for (int e = threadIdx.x; e < nb; e += blockDim.x) {
            const int64_t o1 = boffA[e], o2 = boffB[e], a1 = aoffA[e], a2 = aoffB[e];
            // no second source / destination: repeat the first (its contribution is masked, the store is idempotent)
            sofs[e * 4 + 0] = o1; sofs[e * 4 + 1] = o2 >= 0 ? o2 : o1; sofs[e * 4 + 2] = a1; sofs[e * 4 + 3] = a2 >= 0 ? a2 : a1;
        }
    __syncthreads();
    if (!active) return;
    const double *La = Larrow + (int64_t)c * 3 * nb;
    const double *g_l = gl + c * 6, *g_r = gr + c * 6;
    T *tp = nullptr;
    // LINEAR: one contiguous [row][col] array on each side (row offset = m * stride), no offset tables to fetch
#define BROW(m) (LINEAR ? ld(Bsrc + (int64_t)(m) * stride + col, tp) : brow2<T>(Bsrc, sofs, (m), col))
#define AROW(m) ld(A + (LINEAR ? (int64_t)(m) * stride : sofs[(m) * 4 + 2]) + col, tp)
#define ASET(m, val) st(A + (LINEAR ? (int64_t)(m) * stride : sofs[(m) * 4 + 2]) + col, (val))
#define AFIN(m, val)                                                     \
    do {                                                                 \
        const T v_ = (val);                                              \
        st(A + (LINEAR ? (int64_t)(m) * stride : sofs[(m) * 4 + 2]) + col, v_);   \
        if (!LINEAR) st(A + sofs[(m) * 4 + 3] + col, v_);   /* no second destination: the same address again */ \
    } while (0)
    if (!per) {
        // forward substitution; the free unknown i lives in row rl + i of A
        T y1 = zero(tp), y2 = zero(tp), y3 = zero(tp);     // y[i-1], y[i-2], y[i-3]
        T bl0 = zero(tp), bl1 = zero(tp), br0 = zero(tp), br1 = zero(tp);
        for (int q = 0; q < rl; q++) { const T bq = BROW(q); bl0 = bl0 + g_l[q * 2] * bq; bl1 = bl1 + g_l[q * 2 + 1] * bq; }
        for (int q = 0; q < rr; q++) { const T bq = BROW(nb - 1 - q); br0 = br0 + g_r[q * 2] * bq; br1 = br1 + g_r[q * 2 + 1] * bq; }
        // Full batches of SOLVE_U rows run without any control flow (row index tests are selects), so the compiler hoists the
        // wave-uniform factor loads of a whole batch in front of its dependent multiply-adds; with a branch per row every row
        // waited for its own scalar loads (~700 cycles per row, the whole kernel).  The remainder rows take the simple loop.
        // interior rows: nothing but the three-term recurrence (7 multiply / add per column and row); the boundary-condition
        // contributions only touch the first and last two rows, which take the general form outside the batches
        auto fwd_plain = [&](int i, T s) {
            const double4 l = *reinterpret_cast<const double4 *>(sfac + (size_t)i * 4);
            s = s - (l.z * y1 + l.y * y2 + l.x * y3);
            s = l.w * s;
            y3 = y2; y2 = y1; y1 = s;
            ASET(rl + i, s);
        };
        auto fwd_edge = [&](int i, T s) {
            if (i == 0) s = s + bl0;
            if (i == 1) s = s + bl1;
            if (i == n - 1) s = s + br0;
            if (i == n - 2) s = s + br1;
            fwd_plain(i, s);
        };
        const int f_lo = min(2, n), f_hi = max(f_lo, n - 2);                      // interior rows [f_lo, f_hi)
        const int f_full = f_lo + ((f_hi - f_lo) / SOLVE_U) * SOLVE_U;
        for (int i = 0; i < f_lo; i++) fwd_edge(i, BROW(rl + i));
        // The rows of batch b + 1 are requested BEFORE batch b is computed and stored: the memory counter of this hardware
        // retires loads and stores in issue order, so a load issued after a batch's stores would also wait for those
        // stores to complete (and its own latency would be exposed once per batch).
        {
            T rhs[SOLVE_U], nxt[SOLVE_U];
            if (f_lo < f_full) {
#pragma unroll
                for (int u = 0; u < SOLVE_U; u++) rhs[u] = BROW(rl + f_lo + u);
            }
            for (int i0 = f_lo; i0 < f_full; i0 += SOLVE_U) {
                const bool more = i0 + SOLVE_U < f_full;
#pragma unroll
                for (int u = 0; u < SOLVE_U; u++) nxt[u] = BROW(rl + (more ? i0 + SOLVE_U + u : i0 + u));
#pragma unroll
                for (int u = 0; u < SOLVE_U; u++) fwd_plain(i0 + u, rhs[u]);
#pragma unroll
                for (int u = 0; u < SOLVE_U; u++) rhs[u] = nxt[u];
            }
        }
        for (int i = f_full; i < n; i++) fwd_edge(i, BROW(rl + i));
        // back substitution
        T x1 = zero(tp), x2 = zero(tp), x3 = zero(tp);     // x[i+1], x[i+2], x[i+3]
        T xl0 = zero(tp), xl1 = zero(tp), xr0 = zero(tp), xr1 = zero(tp);
        auto bwd_plain = [&](int i, T s) {                 // rows i <= n - 4: all three super-diagonal terms exist
            s = s - (sfac[(size_t)(i + 1) * 4 + 2] * x1 + sfac[(size_t)(i + 2) * 4 + 1] * x2 + sfac[(size_t)(i + 3) * 4 + 0] * x3);
            s = sfac[(size_t)i * 4 + 3] * s;
            x3 = x2; x2 = x1; x1 = s;
            AFIN(rl + i, s);
        };
        auto bwd_edge = [&](int i, T s) {
            if (i + 1 < n) s = s - Lb[(int64_t)(i + 1) * 4 + 2] * x1;
            if (i + 2 < n) s = s - Lb[(int64_t)(i + 2) * 4 + 1] * x2;
            if (i + 3 < n) s = s - Lb[(int64_t)(i + 3) * 4 + 0] * x3;
            s = Ld[i] * s;
            x3 = x2; x2 = x1; x1 = s;
            AFIN(rl + i, s);
            if (i == n - 1) xr0 = s;
            if (i == n - 2) xr1 = s;
            if (i == 1) xl1 = s;
            if (i == 0) xl0 = s;
        };
        int ib = n - 1;
        for (; ib >= max(n - 3, 0); ib--) bwd_edge(ib, AROW(rl + ib));               // last three rows
        {                                                                            // interior rows down to row 2
            T rhs[SOLVE_U], nxt[SOLVE_U];
            if (ib >= SOLVE_U + 1) {
#pragma unroll
                for (int u = 0; u < SOLVE_U; u++) rhs[u] = AROW(rl + ib - u);
            }
            for (; ib >= SOLVE_U + 1; ib -= SOLVE_U) {
                const bool more = ib - SOLVE_U >= SOLVE_U + 1;
#pragma unroll
                for (int u = 0; u < SOLVE_U; u++) nxt[u] = AROW(rl + (more ? ib - SOLVE_U - u : ib - u));
#pragma unroll
                for (int u = 0; u < SOLVE_U; u++) bwd_plain(ib - u, rhs[u]);
#pragma unroll
                for (int u = 0; u < SOLVE_U; u++) rhs[u] = nxt[u];
            }
        }
        for (; ib >= 0; ib--) bwd_edge(ib, AROW(rl + ib));
        for (int q = 0; q < rl; q++) AFIN(q, g_l[q * 2] * xl0 + g_l[q * 2 + 1] * xl1);
        for (int q = 0; q < rr; q++) AFIN(nb - 1 - q, g_r[q * 2] * xr0 + g_r[q * 2 + 1] * xr1);
    } else {
        // periodic: unknown i <-> row i + 1; rows 0, nb-2, nb-1 fold onto unknowns n-1, 0, 1
        T y1 = zero(tp), y2 = zero(tp), y3 = zero(tp);
        T acc0 = zero(tp), acc1 = zero(tp), acc2 = zero(tp);        // arrow-row dot products
        for (int i = 0; i < n - 3; i++) {
            T s = BROW(i + 1);
            if (i == 0) s = s + BROW(nb - 2);
            if (i == 1) s = s + BROW(nb - 1);
            const double *l = Lb + (int64_t)i * 4;
            s = s - (l[2] * y1 + l[1] * y2 + l[0] * y3);
            s = Ld[i] * s;
            y3 = y2; y2 = y1; y1 = s;
            ASET(i + 1, s);
            acc0 = acc0 + La[i] * s;
            acc1 = acc1 + La[nb + i] * s;
            acc2 = acc2 + La[2 * nb + i] * s;
        }
        const T t0 = (1.0 / La[n - 3]) * (BROW(n - 2) - acc0);
        const T t1 = (1.0 / La[nb + n - 2]) * (BROW(n - 1) - acc1 - La[nb + n - 3] * t0);
        const T t2 = (1.0 / La[2 * nb + n - 1]) * (BROW(n) + BROW(0) - acc2 - La[2 * nb + n - 3] * t0 - La[2 * nb + n - 2] * t1);
        // back substitution of the dense 3x3 corner
        const T u2 = (1.0 / La[2 * nb + n - 1]) * t2;
        const T u1 = (1.0 / La[nb + n - 2]) * (t1 - La[2 * nb + n - 2] * u2);
        const T u0 = (1.0 / La[n - 3]) * (t0 - La[nb + n - 3] * u1 - La[2 * nb + n - 3] * u2);
        AFIN(n - 2, u0);
        AFIN(n - 1, u1);
        AFIN(n, u2);
        T x1 = zero(tp), x2 = zero(tp), x3 = zero(tp);
        T first0 = zero(tp), first1 = zero(tp);
        for (int i = n - 4; i >= 0; i--) {
            T s = AROW(i + 1);
            if (i + 1 < n - 3) s = s - Lb[(int64_t)(i + 1) * 4 + 2] * x1;
            if (i + 2 < n - 3) s = s - Lb[(int64_t)(i + 2) * 4 + 1] * x2;
            if (i + 3 < n - 3) s = s - Lb[(int64_t)(i + 3) * 4 + 0] * x3;
            s = s - (La[i] * u0 + La[nb + i] * u1 + La[2 * nb + i] * u2);
            s = Ld[i] * s;
            x3 = x2; x2 = x1; x1 = s;
            AFIN(i + 1, s);
            if (i == 0) first0 = s;
            if (i == 1) first1 = s;
        }
        AFIN(0, u2);            // a_{-1} = a_{n-1}
        AFIN(nb - 2, first0);   // a_{n}  = a_0
        AFIN(nb - 1, first1);   // a_{n+1} = a_1
    }
#undef BROW
#undef AROW
#undef ASET
#undef AFIN
}

// One lane per wavenumber: the (Re, Im) columns of a wavenumber k >= 1 form one 16-byte aligned pair and share a
// boundary-condition class, so a lane solves both with double2 loads/stores; rows are contiguous across lanes, so every
// access is coalesced. The k = 0 column (own class, single column) is handled by one extra block per (variable,
// z-mode) in which only lane 0 works.
// PAIR = false: one column per lane (twice the waves, half the dependent arithmetic per row): used when the launch has too
// few wavenumbers to occupy the chip - the transposed solve of a multi-GPU run - where the kernel time is the latency
// of one wave's row recurrence.
template <bool LINEAR, bool PAIR = true, int SOLVE_U = LINEAR ? 8 : 16>
__global__ void __launch_bounds__(64)
k_solve(const double *__restrict__ Bsrc, const int64_t *__restrict__ boffA, const int64_t *__restrict__ boffB,
        double *__restrict__ A, const int64_t *__restrict__ aoffA, const int64_t *__restrict__ aoffB,
        const int *__restrict__ cls, const int *__restrict__ cmeta, const double *__restrict__ gl,
        const double *__restrict__ gr, const double *__restrict__ Lband, const double *__restrict__ Ldinv,
        const double *__restrict__ Larrow, int nb, int Zb, int K2, int vz0, int64_t stride) {
    const int vz = blockIdx.y;                      // local (v, zm) group; vz0 + vz is the patch-level group
    const int v = (vz0 + vz) / Zb;
    const bool k0 = (blockIdx.x == gridDim.x - 1);  // the last block in x handles the k = 0 column
    // every lane takes part in staging the factor rows; lanes without a column leave after that (`active`)
    if (k0) {
        solve_columns<S1, LINEAR, SOLVE_U>(Bsrc, boffA, boffB, A, aoffA, aoffB, cmeta, gl, gr, Lband, Ldinv, Larrow, nb, cls[v * 2 + 0],
                                  (int64_t)vz * K2, stride, threadIdx.x == 0);
    } else if (PAIR) {
        const int k = 1 + blockIdx.x * 64 + threadIdx.x;      // wavenumber; its columns are blocks 2k and 2k + 1
        const bool act = 2 * k + 1 < K2;
        solve_columns<S2, LINEAR, SOLVE_U>(Bsrc, boffA, boffB, A, aoffA, aoffB, cmeta, gl, gr, Lband, Ldinv, Larrow, nb, cls[v * 2 + 1],
                                  (int64_t)vz * K2 + (act ? 2 * k : 2), stride, act);
    } else {
        const int c = 2 + blockIdx.x * 64 + threadIdx.x;      // column (Re or Im of a wavenumber >= 1)
        const bool act = c < K2;
        solve_columns<S1, LINEAR, SOLVE_U>(Bsrc, boffA, boffB, A, aoffA, aoffB, cmeta, gl, gr, Lband, Ldinv, Larrow, nb, cls[v * 2 + 1],
                                  (int64_t)vz * K2 + (act ? c : 2), stride, act);
    }
}

// Transposed (all-to-all) patch solve, tile side: split the tile's [row][col] arrays by destination column range.
//   pack:   send[soff[d] + j * cw[d] + (col - cs[d])] = B[j][col]
//   unpack: A[(cell0 + j)][col] = recv[soff[d] + j * cw[d] + (col - cs[d])]        d = owner of col's (v, z-mode) group
__global__ void k_a2a_pack(const double *__restrict__ B, double *__restrict__ send, const int *__restrict__ owner,
                           const int64_t *__restrict__ soff, const int64_t *__restrict__ cw, const int64_t *__restrict__ cs,
                           int K2, int64_t C, int unpack, int64_t brow0) {
    const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (col >= C) return;
    const int d = owner[col / K2];
    const int64_t o = soff[d] + (int64_t)j * cw[d] + (col - cs[d]);
    if (unpack) const_cast<double *>(B)[(brow0 + j) * C + col] = send[o];
    else send[o] = B[(brow0 + j) * C + col];
}

__global__ void k_halo_add(double *__restrict__ B, const double *__restrict__ recv, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) B[i] += recv[i];
}

__global__ void k_nan_check(const double *__restrict__ x, int64_t n, int *flag) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int bad = 0;
    for (; i < n; i += stride) bad |= (x[i] != x[i]);
    if (bad) atomicOr(flag, 1);
}

// max |x[v][p]| per variable: the bit pattern of a non-negative double orders like an unsigned integer, and every NaN
// pattern (sign cleared) orders above +Inf - so a NaN anywhere in the field comes out as NaN, as Julia's maximum(abs, x) does
__global__ void k_max_abs(const double *__restrict__ x, int64_t N, unsigned long long *__restrict__ out) {
    const int v = blockIdx.y;
    const double *xv = x + (int64_t)v * N;
    unsigned long long m = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long a = (unsigned long long)__double_as_longlong(xv[i]) & 0x7fffffffffffffffull;
        if (a > m) m = a;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(m, o);
        if (t > m) m = t;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(out + v, m);
}

// ------------------------------------------------------------------------------------------------ launchers

#ifdef SX_PHASES
static long long *g_sbw_buf = nullptr;
static int64_t g_sbw_n = 0;
void sbw_phases_dump() {
    const char *path = getenv("SX_SBW_PHASES_OUT");
    if (!path || !g_sbw_buf) return;
    std::vector<long long> hst((size_t)g_sbw_n * 8);
    hipDeviceSynchronize();
    hipMemcpy(hst.data(), g_sbw_buf, sizeof(long long) * hst.size(), hipMemcpyDeviceToHost);
    FILE *f = fopen(path, "wb");
    if (f) { fwrite(hst.data(), sizeof(long long), hst.size(), f); fclose(f); }
}
#endif

// Rows of Az the vertical inverse fills.  Inside sx_advance (the equation-set mask) on uniform rings the node-space units invert
// vertically inside their FFT kernel (sx_fft.hip, FUSE): Az is then needed only for the nodes the ring-wise inner rings read (cells
// [0, R_in / 3) -> nodes 0 .. R_in / 3 + 2)
int zinv_rows(const sx_handle *h, bool full) {
    return (!full && h->node_mode && fft_fused_zinv(h)) ? (h->R_in > 0 ? std::min(h->nbt, h->R_in / MUBAR + 3) : 0) : h->nbt;
}

// entries of Az the azimuthal inverse reads after launch_zinv(h, full); without a vertical it reads the tile's A rows
double az_count(const sx_handle *h, bool full) {
    return h->has_z ? (double)zinv_rows(h, full) * (full ? h->njobs_zinv_full : h->njobs_zinv_eq) * h->nz * h->K2 : (double)h->nbt * h->C;
}

void launch_zinv(sx_handle *h, bool full) {
    if (!h->has_z || rz_fused(h)) return;          // RZ: the vertical inverse is part of k_rz_inverse (sx_rz.hip)
    const int njobs = full ? h->njobs_zinv_full : h->njobs_zinv_eq;
    const int rows = zinv_rows(h, full);
    TimedLaunch scope(h, "k_zinv", 8.0 * ((double)h->nbt * h->C) * rows / h->nbt + (h->sp32 ? 4.0 : 8.0) * az_count(h, full));   // read the rows' A, write Az
    if (njobs > 0 && rows > 0) {
        const ZinvPlan p = plan_zinv(h->geom, h->nz, h->K2, h->sp32, h->sw);
        dim3 g(p.grid_x, njobs, rows);
        const ColJob *jobs = full ? h->d_jobs_zinv_full : h->d_jobs_zinv_eq;
        const int64_t azrow = (int64_t)h->V * 3 * h->nz * h->K2;
#define ZINV_T(MT, OT, CT) hipLaunchKernelGGL((k_colmat_mfma<MT, OT, CT>), g, dim3(256), 0, h->stream, h->d_A, reinterpret_cast<OT *>(h->d_Az), h->d_MzT, jobs, h->Zb, h->K2, h->C, azrow, h->cell0)
#define ZINV(MT, CT) if (p.f32) ZINV_T(MT, float, CT); else ZINV_T(MT, double, CT); break
        switch (p.kernel) {
        case ZinvKernel::mfma_2_1: ZINV(2, 1);
        case ZinvKernel::mfma_4_1: ZINV(4, 1);
        case ZinvKernel::mfma_4_2: ZINV(4, 2);
        case ZinvKernel::mfma_8_1: ZINV(8, 1);
        case ZinvKernel::mfma_8_2: ZINV(8, 2);
        case ZinvKernel::mfma_8_4: ZINV(8, 4);
        case ZinvKernel::colmat:
            hipLaunchKernelGGL(k_colmat, g, dim3(64, 4), sizeof(double) * 64 * h->Zb, h->stream, h->d_A, h->d_Az, h->d_Mz, jobs,
                               h->Zb, h->nz, h->K2, h->C, azrow, h->cell0);
            break;
        case ZinvKernel::none: break;      // not reached: has_z and not the fused RZ form (above)
        }
#undef ZINV
#undef ZINV_T
    }
}

void launch_rl_inverse(sx_handle *h, bool full) {
    const int *mask = full ? h->d_mask_full : h->d_mask_eq;
    h->node_active = (!full && h->node_mode);
    if (rz_fused(h)) { launch_rz_inverse(h, mask); return; }
    if (h->node_active) {            // sx_advance on uniform rings: node-space transforms + ring-wise inner rings only
        launch_node_fft(h);
        launch_rl_inverse_fft(h, mask, h->R_in);
        return;
    }
    if (fft_path_ok(h)) { launch_rl_inverse_fft(h, mask); return; }
    if (dft_mfma_ok(h)) { launch_rl_inverse_dft(h, mask); return; }
    // write the requested physical planes, read Az
    TimedLaunch scope(h, "k_rl_inverse", (double)h->N * out_plane_bytes(h, full) + (h->sp32 ? 4.0 : 8.0) * az_count(h, full));
    const int cstride = (h->kmax_max + 1) | 1;
    const size_t lds = sizeof(double) * 2 * ZC * cstride;
    if (lds > 64 * 1024) {
        set_error("azimuthal inverse transform: rings with " + std::to_string(h->kmax_max) + " wavenumbers are outside every transform path (power-of-two ring tables up to 512 points, ring lengths that are multiples of 4 up to 5120 points, otherwise kmax <= 255)");
        return;
    }
    const double *az = h->has_z ? h->d_Az : h->d_A + (int64_t)h->cell0 * h->C;
    const int64_t azrow = h->has_z ? (int64_t)h->V * 3 * h->nz * h->K2 : h->C;
    dim3 g((h->nz + ZC - 1) / ZC, h->V, h->nrings);
#define RL_ARGS h->d_phi, h->d_L, h->d_kmax, h->d_pstart, h->d_twoff, h->d_tw, h->d_phoff, h->d_ph, h->V, h->nz, h->nsz, h->K2,   \
                h->nrings, h->N, azrow, h->slot[0], h->slot[1], h->slot[2], h->slot[3], h->slot[4], h->slot[5], h->slot[6],   \
                h->has_l, cstride, mask
    if (h->f32) hipLaunchKernelGGL(k_rl_inverse<float>, g, dim3(256), lds, h->stream, az, planes_of<float>(h->d_phys, h->V, h->N), RL_ARGS);
    else hipLaunchKernelGGL(k_rl_inverse<double>, g, dim3(256), lds, h->stream, az, planes_of<double>(h->d_phys, h->V, h->N), RL_ARGS);
#undef RL_ARGS
}

// the forward pair for the launch's variable window, or off (plan_fwd_cells: sx_plan.cpp)
static CellsPlan cells_plan(const sx_handle *h) {
    if (!h->cells.on) return CellsPlan();
    return plan_fwd_cells(h->geom, h->nz, h->Zb, h->K2, h->V, h->v_cnt, h->ncells, h->sp32, h->uniform_L, h->sw);
}

void launch_fl_forward(sx_handle *h) {
    if (rz_fused(h)) return;                        // RZ: k_rz_forward reads var_np1 itself (no azimuth, nothing to transform)
    if (const CellsPlan cp = cells_plan(h); cp.on) { launch_fl_forward_cells(h, cp); return; }
    if (fft_path_ok(h)) { launch_fl_forward_fft(h); return; }
    if (dft_mfma_ok(h)) { launch_fl_forward_dft(h); return; }
    TimedLaunch scope(h, "k_fl_forward", 8.0 * (double)h->N * h->V + (h->sp32 ? 4.0 : 8.0) * fl_count(h));      // read var_np1, write the spectra
    const int xstride = h->L_max | 1;
    const size_t lds = sizeof(double) * ZC * xstride;
    if (lds > 64 * 1024) {       // the scalar kernel stages a whole ring; longer rings need the matrix-core DFT (lengths that are multiples of 4)
        set_error("azimuthal forward transform: rings of " + std::to_string(h->L_max) + " points are outside every transform path (power-of-two ring tables up to 512 points, ring lengths that are multiples of 4 up to 5120 points, any length up to 511 points)");
        return;
    }
    dim3 g((h->nz + ZC - 1) / ZC, h->V, h->nrings);
    hipLaunchKernelGGL(k_fl_forward, g, dim3(256), lds, h->stream, h->d_np1, h->d_Fl, h->d_L, h->d_kmax, h->d_pstart,
                       h->d_twoff, h->d_tw, h->d_phoff, h->d_ph, h->V, h->nz, h->K2, h->N, h->has_l, xstride);
}

static void launch_nodes_z(sx_handle *h, const CellsPlan &p) {
    TimedLaunch scope(h, "k_sbz", (h->sp32 ? 4.0 : 8.0) * fl_count(h) + 8.0 * ((double)h->nbt * h->C));      // read the spectra, write the tile's B rows
    dim3 g((h->K2 + p.bw - 1) / p.bw, h->v_cnt, p.zsegs);
    const int64_t plane = (int64_t)h->V * h->nz * h->K2, flo = (int64_t)h->v_lo * h->nz * h->K2, blo = (int64_t)h->v_lo * h->Zb * h->K2;
#define NODES_Z(...) hipLaunchKernelGGL((__VA_ARGS__), g, dim3(p.zthreads), 0, h->stream, h->d_Fn + flo, h->d_Fn + (int64_t)h->nbt * plane + flo, \
                                        h->d_Btile + blo, h->d_CB, h->nbt, h->V, h->Zb, h->K2, h->C, p.S, p.segs, p.nps); break
    switch (p.zk) {
    case SbKernel::mfma_32: NODES_Z(k_nodes_z<32>);
    case SbKernel::mfma_64: NODES_Z(k_nodes_z<64>);
    case SbKernel::mfma_64_t256: NODES_Z(k_nodes_z<64, 32, 256>);
    default: NODES_Z(k_nodes_z<128, 32>);
    }
#undef NODES_Z
}

void launch_sb(sx_handle *h) {
    if (const CellsPlan cp = cells_plan(h); cp.on) { launch_nodes_z(h, cp); return; }
    const SbPlan p = plan_sb(h->geom, h->nz, h->Zb, h->K2, h->v_cnt, h->ncells, h->sp32, h->sw);
    if (p.kernel == SbKernel::rz_forward) { launch_rz_forward(h); return; }
    if (p.kernel == SbKernel::refused) { set_error("launch_sb: fp32 ring spectra (storage_f32 = 2) need the matrix-core sliding-window kernel"); return; }
    // k_sbz (fused with the vertical forward transform): read the spectra, write the tile's B rows; k_sb: the same without a vertical
    const double fl = fl_count(h), bz = (double)h->nbt * h->V * h->nz * h->K2;
    TimedLaunch scope(h, h->has_z ? "k_sbz" : "k_sb", h->has_z ? (h->sp32 ? 4.0 : 8.0) * fl + 8.0 * ((double)h->nbt * h->C) : 8.0 * (fl + bz));
    if (p.kernel == SbKernel::sb) {
        const int64_t plane = (int64_t)h->V * h->nz * h->K2;
        dim3 g((unsigned)((plane + 255) / 256), h->nbt);
        hipLaunchKernelGGL(k_sb, g, dim3(p.threads), 0, h->stream, h->d_Fl, h->d_Btile, h->d_phi, h->d_wq, h->ncells, plane);
    } else if (p.kernel == SbKernel::sbz) {
        dim3 g((h->K2 + p.bw - 1) / p.bw, h->V, h->nbt);
        hipLaunchKernelGGL(k_sbz, g, dim3(64, 4), sizeof(double) * 64 * h->nz, h->stream, h->d_Fl, h->d_Btile, h->d_phi, h->d_wq,
                           h->d_CB, h->ncells, h->V, h->nz, h->Zb, h->K2, h->C);
    } else {       // the sliding-window kernels
        dim3 gw((h->K2 + p.bw - 1) / p.bw, h->v_cnt, p.segs);      // variable window: see sx_internal.hpp
        const int64_t flo = (int64_t)h->v_lo * h->nz * h->K2, blo = (int64_t)h->v_lo * h->Zb * h->K2;
#ifdef SX_PHASES
        if (!g_sbw_buf) {
            g_sbw_n = (int64_t)gw.x * gw.y * gw.z;
            hipMalloc(&g_sbw_buf, sizeof(long long) * g_sbw_n * 8);
            hipMemset(g_sbw_buf, 0, sizeof(long long) * g_sbw_n * 8);
            hipMemcpyToSymbol(HIP_SYMBOL(g_sbw_dbg), &g_sbw_buf, sizeof(g_sbw_buf));
        }
#endif
        // FT: how the ring spectra d_Fl are stored (float: storage_f32 = 2)
#define SBW(FT, ...) hipLaunchKernelGGL((__VA_ARGS__), gw, dim3(p.threads), 0, h->stream, reinterpret_cast<const FT *>(h->d_Fl) + flo, h->d_Btile + blo, \
                                        h->d_phi, h->d_wq, h->d_CB, h->ncells, h->V, h->Zb, h->K2, h->C, p.cps); break
        switch (p.kernel) {
        case SbKernel::sbw_32: SBW(double, k_sbw<32, false>);
        case SbKernel::sbw_32_pf: SBW(double, k_sbw<32, true>);
        case SbKernel::sbw_64: SBW(double, k_sbw<64, false>);
        case SbKernel::sbw_64_pf: SBW(double, k_sbw<64, true>);
        case SbKernel::sbw_128: SBW(double, k_sbw<128, false>);
        case SbKernel::mfma_32: SBW(double, k_sbw_mfma<32>);
        case SbKernel::mfma_64: SBW(double, k_sbw_mfma<64>);
        case SbKernel::mfma_64_t256: SBW(double, k_sbw_mfma<64, 32, 256>);
        case SbKernel::mfma_128: SBW(double, k_sbw_mfma<128, 32>);
        case SbKernel::mfma_32_f32: SBW(float, k_sbw_mfma<32, 64, 512, float>);
        case SbKernel::mfma_64_f32: SBW(float, k_sbw_mfma<64, 64, 512, float>);
        case SbKernel::mfma_64_t256_f32: SBW(float, k_sbw_mfma<64, 32, 256, float>);
        case SbKernel::mfma_128_f32: SBW(float, k_sbw_mfma<128, 32, 512, float>);
        default: break;      // the other kernels: above
        }
#undef SBW
    }
}


void launch_solve(sx_handle *h) {
    dim3 g((h->K2 > 1 ? (h->K2 / 2 - 1 + 63) / 64 : 0) + 1, h->V * h->Zb);
    // few right-hand sides (the R grid's one column, RZ grids, small RL patches): LDS-staged parallel cyclic reduction (sx_pcr.hip)
    // instead of one wave's serial recurrence per 64 columns
    const bool contiguous = (h->d_Bsrc == h->d_Bfull);
    const int ngroups = contiguous ? h->v_cnt * h->Zb : h->V * h->Zb;
    const int64_t ncols = (int64_t)ngroups * (h->K2 > 1 ? h->K2 - 1 : 1);
    // contiguous, non-periodic, enough columns to fill the chip: row partitions in one workgroup, y on chip (k_solve_part, sx_iface.hip)
    const bool part = h->part_P && plan_solve_part(h->b_rDim, 0, contiguous, ncols, h->sw) == h->part_P;
    TimedLaunch scope(h, "k_solve", 8.0 * (part ? 2.0 : 4.0) * ((double)h->b_rDim * h->C));      // read B, write y, read y, write A; k_solve_part: B in, A out
    if (part) {
        const int64_t clo = (int64_t)h->v_lo * h->Zb * h->K2;
        launch_solve_part(h, h->d_Bsrc + clo, h->d_A + clo, h->v_lo * h->Zb, ngroups);
        return;
    }
    if (pcr_wanted(h, ncols)) {
        const int64_t clo = contiguous ? (int64_t)h->v_lo * h->Zb * h->K2 : 0;
        launch_solve_pcr(h, contiguous, h->d_Bsrc + clo, h->d_rowoff, h->d_neg1, h->d_A + clo, h->d_aoff, h->d_neg1,
                         contiguous ? h->v_lo * h->Zb : 0, ngroups, h->C);
        return;
    }
    if (contiguous) {   // internal contiguous B: no offset tables needed; the variable window through the base pointers
        const int64_t clo = (int64_t)h->v_lo * h->Zb * h->K2;
        g.y = h->v_cnt * h->Zb;
        hipLaunchKernelGGL(k_solve<true>, g, dim3(64), sizeof(double) * 4 * h->b_rDim, h->stream, h->d_Bsrc + clo, h->d_rowoff, h->d_neg1, h->d_A + clo, h->d_aoff, h->d_neg1,
                           h->d_cls, h->d_cmeta, h->d_gl, h->d_gr, h->d_Lband, h->d_Ldinv, h->d_Larrow, h->b_rDim, h->Zb, h->K2, h->v_lo * h->Zb,
                           h->C);
    }
    else
        hipLaunchKernelGGL(k_solve<false>, g, dim3(64), sizeof(double) * 8 * h->b_rDim, h->stream, h->d_Bsrc, h->d_rowoff, h->d_neg1, h->d_A, h->d_aoff,
                           h->d_neg1, h->d_cls, h->d_cmeta, h->d_gl, h->d_gr, h->d_Lband, h->d_Ldinv, h->d_Larrow, h->b_rDim, h->Zb,
                           h->K2, 0, h->C);
}

// transposed solve: my column groups [g0, g1), right-hand sides from the all-to-all receive buffer, solution rows into
// the all-to-all send buffer (both [tile][row][my columns]; a row shared by two tiles is summed on input, duplicated on output)
void launch_solve_a2a(sx_handle *h, const double *recv, double *send) {
    TimedLaunch scope(h, "k_solve", 8.0 * 4.0 * ((double)h->b_rDim * h->C));      // read B, write y, read y, write A
    const int ng = h->a2a_g1 - h->a2a_g0;
    if (ng > 0 && pcr_wanted(h, (int64_t)ng * (h->K2 > 1 ? h->K2 - 1 : 1))) {
        launch_solve_pcr(h, false, recv, h->d_a2a_offA, h->d_a2a_offB, send, h->d_a2a_offA, h->d_a2a_offB, h->a2a_g0, ng, 0);
        return;
    }
    if (ng > 0) {
        const int bx_pair = (h->K2 > 1 ? (h->K2 / 2 - 1 + 63) / 64 : 0) + 1;
        const bool single = (int64_t)bx_pair * ng < 768 && h->K2 > 2;        // fewer waves than SIMDs: one column per lane
#define A2A_ARGS recv, h->d_a2a_offA, h->d_a2a_offB, send, h->d_a2a_offA, h->d_a2a_offB, h->d_cls, h->d_cmeta, h->d_gl, h->d_gr,      \
                 h->d_Lband, h->d_Ldinv, h->d_Larrow, h->b_rDim, h->Zb, h->K2, h->a2a_g0, (int64_t)0
        if (single) hipLaunchKernelGGL((k_solve<false, false>), dim3((h->K2 - 2 + 63) / 64 + 1, ng), dim3(64), sizeof(double) * 8 * h->b_rDim, h->stream, A2A_ARGS);
        else hipLaunchKernelGGL((k_solve<false, true>), dim3(bx_pair, ng), dim3(64), sizeof(double) * 8 * h->b_rDim, h->stream, A2A_ARGS);
#undef A2A_ARGS
    }
}

void launch_a2a_pack(sx_handle *h, double *buf, int unpack) {
    TimedLaunch scope(h, unpack ? "k_a2a_unpack" : "k_a2a_pack", 0.0);
    dim3 g((unsigned)((h->C + 255) / 256), h->nbt);
    const double *arr = unpack ? h->d_A : h->d_Btile;
    hipLaunchKernelGGL(k_a2a_pack, g, dim3(256), 0, h->stream, arr, buf, h->d_a2a_owner, h->d_a2a_soff, h->d_a2a_cw, h->d_a2a_cs,
                       h->K2, h->C, unpack, (int64_t)(unpack ? h->cell0 : 0));
}

void launch_halo_add(sx_handle *h, const double *recv) {
    TimedLaunch scope(h, "k_halo_add", 0.0);
    const int64_t n = 3 * h->C;
    hipLaunchKernelGGL(k_halo_add, grid1(n, 256), dim3(256), 0, h->stream, h->d_Btile, recv, n);
}

void launch_max_abs(sx_handle *h, unsigned long long *d_out) {
    HIPCHK(hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * h->V, h->stream));
    hipLaunchKernelGGL(k_max_abs, dim3(512, h->V), dim3(256), 0, h->stream, h->d_np1, h->N, d_out);
    HIPCHK(hipGetLastError());
}

void launch_nan_check(sx_handle *h) {
    HIPCHK(hipMemsetAsync(h->d_flag, 0, sizeof(int), h->stream));
    // checkCFL (src/semiimplicit.jl:737-751) scans physical[:, v, 1] right after a tileTransform!.  Here the scan runs
    // over var_np1 = value + ts * tendency of the last step (the initial values before the first step): a NaN in any
    // value propagates into it, and unlike `physical` it is complete after every sx_advance (slot masks and the
    // node-space inverse leave parts of `physical` untouched between outputs).
    const int64_t n = (int64_t)h->V * h->N;
    hipLaunchKernelGGL(k_nan_check, dim3(2048), dim3(256), 0, h->stream, h->d_np1, n, h->d_flag);
    HIPCHK(hipGetLastError());
}

}  // namespace sx
