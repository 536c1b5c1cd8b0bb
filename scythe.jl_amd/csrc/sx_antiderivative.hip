// sx_antiderivative: F(r) = int_{xmin}^{r} w f ds, F(z) = int_{zmin}^{z} f dz' (or from the other end) from the A coefficients, written as
// the A coefficients of another variable (include/scythe_hip.h, "antiderivatives").
//
// Radial.  f = sum_j a_j phi_j; F is projected onto the destination variable's spline space as the model's B -> A projects a field (its
// boundary-condition classes, its l_q filter) but with the exact right-hand side and, with it, the exact Gram matrix in P + eps_q Q
//     b_i = int phi_i F dr = sum_{|j - i| <= 3} Pband[i][j] a_j + m_i sum_{j <= i - 4} c_j a_j          (FROM_LOW; mirrored for FROM_HIGH)
// (sx_setup.cpp forms Pband, c, m in extended precision and hands them over in walk order: step s is row s going up or row nb - 1 - s
// going down, so both origins are one loop).
// k_antiderivative_r: one lane per (z-mode, block) column, 64-lane workgroups; the column index is the fastest in memory, so a wave's row
// access is one coalesced line, and the lanes walk the rows together, so a table row is one address for the wave (k_elliptic's pattern).
// Pass 1 walks the source column: a 7-row window, a fixed fma chain for the band product, and the running sum S += c a of the row that
// leaves the window - serial and in a fixed order per lane - and stores b in the destination column.  Passes 2 and 3 are k_elliptic's
// sweeps over that column, in place as k_solve does: fold with Gamma, L y = Gamma b, L^T x = y, a = Gamma^T x.  The rows of the next batch
// of ANT_U are requested before the arithmetic of the current one in all three passes (k_solve's remedy: DESIGN.md 13 names the cost of
// one exposed round trip per row).  The right-hand side and y each make a global round trip through the destination column; dst's B
// arrays are not touched.  No lane reads what another wrote, nothing is summed across lanes: two calls agree bitwise and a column's
// result does not depend on the launch shape.
//
// Vertical.  A_dst[m][zm][blk] = sum_zm' Z[zm][zm'] A_src[m][zm'][blk], Z = CB T Ic CA_src [Zb][Zb] (sx_setup.cpp).  For one (node row,
// variable) the [Zb][K2] block of A is contiguous, so this is [Zb x Zb] . [Zb x K2] per row:
// k_antiderivative_z<KS>: one wave per (node row, 16 wavenumber blocks) on the f64 matrix cores with k_colmat_mfma's operand scheme - the
// B operand straight from the A row (16 consecutive blocks = one 128-byte line per z-mode), all of it requested before the first MFMA;
// the operator fragments of each 16-row output tile from Z^T (L2 resident, zero-padded to 4 in K and 16 in M, so only the stores are
// guarded at the 16-row edge).  KS = K steps of 4 held in registers: 4, 8 or 16 (b_zDim <= 16, 32, 64).
// k_antiderivative_z_lane: fewer than 16 blocks per z-mode (RZ grids: K2 = 1; R / RL grids have no vertical) or b_zDim > 64: one lane per
// output, the sum in index order.
// Both read the variable's A once and write it once, in a fixed order: two calls agree bitwise.
#include "sx_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

constexpr int ANT_T = 64;       // one wave per workgroup: the recurrences are serial in the rows, the waves spread over the CUs
constexpr int ANT_U = 8;        // rows per batch of loads

struct AntiClsDev {             // Gamma of one boundary-condition class as the kernel reads it
    int n, rl, rr, pad;
    double gl[6], gr[6];        // [q][2] as SplineClass::gl / gr
};

struct AntiRArgs {
    const double *A;            // source A [nb][Cs]
    double *D;                  // destination A [nb][Cd]
    const double *P, *c, *m;    // walk-order tables [nb][7], [nb], [nb]
    const double *F;            // factor rows [2][nb][4]: the k = 0 class, the k >= 1 class
    const AntiClsDev *cls;      // [2]
    int64_t Cs, Cd, col_s, col_d;       // row strides; first column of the source and of the destination variable
    int nb, K2, ncol, high;     // patch rows; blocks per z-mode; columns of one variable; walk downward
};

__global__ __launch_bounds__(ANT_T) void k_antiderivative_r(const AntiRArgs a) {
    const int c = blockIdx.x * ANT_T + threadIdx.x;
    if (c >= a.ncol) return;
    const int nb = a.nb, blk = c % a.K2, k = blk >> 1;
    double *__restrict__ D = a.D + a.col_d + c;
    if (blk == 1) {             // Im c_0: the padding block
        for (int m = 0; m < nb; m++) D[(int64_t)m * a.Cd] = 0.0;
        return;
    }
    // ---- pass 1: the right-hand side, in walk order
    {
        const int64_t ds = a.high ? -a.Cs : a.Cs, dd = a.high ? -a.Cd : a.Cd;
        const double *__restrict__ As = a.A + a.col_s + c + (a.high ? (int64_t)(nb - 1) * a.Cs : 0);
        double *__restrict__ Dw = D + (a.high ? (int64_t)(nb - 1) * a.Cd : 0);
        const double *__restrict__ P = a.P, *__restrict__ cw = a.c, *__restrict__ mw = a.m;
        auto ld = [&](int s) { return s >= 0 && s < nb ? As[(int64_t)s * ds] : 0.0; };
        double w[7], cur[ANT_U], nxt[ANT_U], S = 0.0;
#pragma unroll
        for (int d = 0; d < 7; d++) w[d] = ld(d - 3);
#pragma unroll
        for (int u = 0; u < ANT_U; u++) cur[u] = ld(4 + u);
        for (int s0 = 0; s0 < nb; s0 += ANT_U) {
#pragma unroll
            for (int u = 0; u < ANT_U; u++) nxt[u] = ld(s0 + ANT_U + 4 + u);
#pragma unroll
            for (int u = 0; u < ANT_U; u++) {
                const int s = s0 + u;
                if (s < nb) {
                    double acc = 0.0;
#pragma unroll
                    for (int d = 0; d < 7; d++) acc = fma(P[(int64_t)s * 7 + d], w[d], acc);
                    Dw[(int64_t)s * dd] = fma(mw[s], S, acc);
                    S = fma(s >= 3 ? cw[s - 3] : 0.0, w[0], S);        // the row of step s - 3 leaves the window
#pragma unroll
                    for (int d = 0; d < 6; d++) w[d] = w[d + 1];
                    w[6] = cur[u];
                }
            }
#pragma unroll
            for (int u = 0; u < ANT_U; u++) cur[u] = nxt[u];
        }
    }
    // ---- pass 2: fold with Gamma and L y = Gamma b; y_i stays in row rl + i
    const AntiClsDev *__restrict__ cl = a.cls + (k > 0 ? 1 : 0);
    const int n = cl->n, rl = cl->rl, rr = cl->rr;
    const double4 *__restrict__ F = reinterpret_cast<const double4 *>(a.F) + (k > 0 ? nb : 0);
    double bl0 = 0.0, bl1 = 0.0, br0 = 0.0, br1 = 0.0;
    for (int q = 0; q < rr; q++) {
        const double gm = D[(int64_t)(nb - 1 - q) * a.Cd];
        br0 = fma(cl->gr[q * 2], gm, br0);
        br1 = fma(cl->gr[q * 2 + 1], gm, br1);
    }
    for (int q = 0; q < rl; q++) {
        const double gm = D[(int64_t)q * a.Cd];
        bl0 = fma(cl->gl[q * 2], gm, bl0);
        bl1 = fma(cl->gl[q * 2 + 1], gm, bl1);
    }
    {
        auto ld = [&](int i) { return i < n ? D[(int64_t)(rl + i) * a.Cd] : 0.0; };
        double cur[ANT_U], nxt[ANT_U], y1 = 0.0, y2 = 0.0, y3 = 0.0;
#pragma unroll
        for (int u = 0; u < ANT_U; u++) cur[u] = ld(u);
        for (int i0 = 0; i0 < n; i0 += ANT_U) {
#pragma unroll
            for (int u = 0; u < ANT_U; u++) nxt[u] = ld(i0 + ANT_U + u);
#pragma unroll
            for (int u = 0; u < ANT_U; u++) {
                const int i = i0 + u;
                if (i < n) {
                    double s = cur[u];
                    if (i == 0) s += bl0;
                    if (i == 1) s += bl1;
                    if (i == n - 1) s += br0;
                    if (i == n - 2) s += br1;
                    const double4 l = F[i];
                    double t = fma(-l.z, y1, s);
                    t = fma(-l.y, y2, t);
                    t = fma(-l.x, y3, t);
                    const double y = t * l.w;
                    y3 = y2; y2 = y1; y1 = y;
                    D[(int64_t)(rl + i) * a.Cd] = y;
                }
            }
#pragma unroll
            for (int u = 0; u < ANT_U; u++) cur[u] = nxt[u];
        }
    }
    // ---- pass 3: L^T x = y in place, downward, and the dependent boundary rows a = Gamma^T x
    double xl0 = 0.0, xl1 = 0.0, xr0 = 0.0, xr1 = 0.0;
    {
        auto ld = [&](int i) { return i >= 0 ? D[(int64_t)(rl + i) * a.Cd] : 0.0; };
        double cur[ANT_U], nxt[ANT_U], x1 = 0.0, x2 = 0.0, x3 = 0.0;
        double4 f1 = make_double4(0.0, 0.0, 0.0, 0.0), f2 = f1, f3 = f1;      // factor rows i + 1, i + 2, i + 3
#pragma unroll
        for (int u = 0; u < ANT_U; u++) cur[u] = ld(n - 1 - u);
        for (int i0 = n - 1; i0 >= 0; i0 -= ANT_U) {
#pragma unroll
            for (int u = 0; u < ANT_U; u++) nxt[u] = ld(i0 - ANT_U - u);
#pragma unroll
            for (int u = 0; u < ANT_U; u++) {
                const int i = i0 - u;
                if (i >= 0) {
                    const double4 l = F[i];
                    double t = fma(-f1.z, x1, cur[u]);
                    t = fma(-f2.y, x2, t);
                    t = fma(-f3.x, x3, t);
                    const double x = t * l.w;
                    x3 = x2; x2 = x1; x1 = x;
                    f3 = f2; f2 = f1; f1 = l;
                    D[(int64_t)(rl + i) * a.Cd] = x;
                    if (i == 0) xl0 = x;
                    if (i == 1) xl1 = x;
                    if (i == n - 1) xr0 = x;
                    if (i == n - 2) xr1 = x;
                }
            }
#pragma unroll
            for (int u = 0; u < ANT_U; u++) cur[u] = nxt[u];
        }
    }
    for (int q = 0; q < rl; q++) D[(int64_t)q * a.Cd] = fma(cl->gl[q * 2 + 1], xl1, cl->gl[q * 2] * xl0);
    for (int q = 0; q < rr; q++) D[(int64_t)(nb - 1 - q) * a.Cd] = fma(cl->gr[q * 2 + 1], xr1, cl->gr[q * 2] * xr0);
}

struct AntiZArgs {
    const double *A;            // source A [nb][Cs]
    double *D;                  // destination A [nb][Cd]
    const double *ZT;           // Z^T [Kp][Mp], zero-padded
    int64_t Cs, Cd, col_s, col_d;
    int nb, Zb, K2, Mp;
};

typedef double anti_d4 __attribute__((ext_vector_type(4)));

template <int KS>
__global__ __launch_bounds__(64) void k_antiderivative_z(const AntiZArgs a) {
    const int lane = threadIdx.x, n = lane & 15, kk = lane >> 4;
    const int blk0 = blockIdx.x * 16, Zb = a.Zb, K2 = a.K2;
    const double *__restrict__ src = a.A + (int64_t)blockIdx.y * a.Cs + a.col_s;
    double *__restrict__ dst = a.D + (int64_t)blockIdx.y * a.Cd + a.col_d;
    const double *__restrict__ ZT = a.ZT;
    const int blk = min(blk0 + n, K2 - 1);
    const bool live = blk != 1;                   // Im c_0 is never read: its products are zero
    double b[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
        const int k = 4 * ks + kk;
        b[ks] = (live && k < Zb) ? src[(int64_t)k * K2 + blk] : 0.0;
    }
    const int nt = (Zb + 15) >> 4, nks = (Zb + 3) >> 2;
#pragma unroll 1
    for (int t = 0; t < nt; t++) {
        double z[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ks++) z[ks] = ks < nks ? ZT[(int64_t)(4 * ks + kk) * a.Mp + t * 16 + n] : 0.0;      // Z[m = t 16 + n][k]
        anti_d4 acc = anti_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < KS; ks++)
            if (ks < nks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(z[ks], b[ks], acc, 0, 0, 0);
        if (blk0 + n < K2) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = t * 16 + kk + 4 * r;
                if (row < Zb) dst[(int64_t)row * K2 + blk0 + n] = acc[r];
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_antiderivative_z_lane(const AntiZArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, per = (int64_t)a.Zb * a.K2;
    if (e >= per * a.nb) return;
    const int m = (int)(e / per), zm = (int)((e % per) / a.K2), blk = (int)(e % a.K2);
    const double *__restrict__ src = a.A + (int64_t)m * a.Cs + a.col_s + blk;
    double acc = 0.0;
    if (blk != 1)
        for (int k = 0; k < a.Zb; k++) acc = fma(a.ZT[(int64_t)k * a.Mp + zm], src[(int64_t)k * a.K2], acc);
    a.D[(int64_t)m * a.Cd + a.col_d + (int64_t)zm * a.K2 + blk] = acc;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct AntiState : DiagState {
    // radial tables and their key
    int r_origin = -1, r_weight = -1, bcl0 = -1, bcl = -1, bcr = -1;
    double l_q = 0.0;
    DevBuf<double> d_P, d_c, d_m, d_F;
    DevBuf<AntiClsDev> d_cls;
    // vertical operator and its key
    int z_origin = -1, bcb = -1, bct = -1, Kp = 0, Mp = 0;
    DevBuf<double> d_ZT;
};

static bool anti_same_grid(const sx_handle *s, const sx_handle *d) {
    return s->geom == d->geom && s->xmin == d->xmin && s->xmax == d->xmax && s->nc == d->nc && s->uniform_L == d->uniform_L && s->kDim == d->kDim &&
           s->nz == d->nz && s->Zb == d->Zb && s->zmin == d->zmin && s->zmax == d->zmax;
}

static bool anti_enums_ok(int axis, int origin, int weight, const char *who) {
    if (axis != SX_INT_R && axis != SX_INT_Z) { set_error(std::string(who) + ": axis must be SX_INT_R or SX_INT_Z"); return false; }
    if (origin != SX_INT_FROM_LOW && origin != SX_INT_FROM_HIGH) { set_error(std::string(who) + ": origin must be SX_INT_FROM_LOW or SX_INT_FROM_HIGH"); return false; }
    if (weight != SX_INT_W_ONE && weight != SX_INT_W_R) { set_error(std::string(who) + ": weight must be SX_INT_W_ONE or SX_INT_W_R"); return false; }
    if (axis == SX_INT_Z && weight != SX_INT_W_ONE) { set_error(std::string(who) + ": the vertical antiderivative takes no weight"); return false; }
    return true;
}

static void anti_cls_dev(const SplineClass &sc, AntiClsDev &o) {
    o.n = sc.nfree; o.rl = sc.rl; o.rr = sc.rr; o.pad = 0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 2; j++) { o.gl[i * 2 + j] = sc.gl[i][j]; o.gr[i * 2 + j] = sc.gr[i][j]; }
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_antiderivative(sx_handle *src, int32_t var_src, int32_t axis, int32_t origin, int32_t weight, sx_handle *dst, int32_t var_dst) {
    clear_error();
    const char *who = "sx_antiderivative";
    if (!src || !dst) { set_error("null handle"); return 1; }
    if (!anti_enums_ok(axis, origin, weight, who)) return 1;
    if (var_src < 1 || var_src > src->V || var_dst < 1 || var_dst > dst->V) { set_error("sx_antiderivative: variable index out of range"); return 1; }
    if (dst == src && var_dst == var_src) { set_error("sx_antiderivative: the destination variable is the source variable"); return 1; }
    if (src->ncells != src->nc || dst->ncells != dst->nc) { set_error("sx_antiderivative: source and destination must be one-tile patches"); return 1; }
    if (!anti_same_grid(src, dst)) { set_error("sx_antiderivative: the destination's grid differs from the source's"); return 1; }
    if (axis == SX_INT_Z && !src->has_z) { set_error("sx_antiderivative: SX_INT_Z needs an RZ or RLZ grid"); return 1; }
    const int vs = var_src - 1, vd = var_dst - 1, nb = src->b_rDim;
    if (axis == SX_INT_R) {
        if (dst->bcl0[vd] == SX_BC_PERIODIC || dst->bcl[vd] == SX_BC_PERIODIC || dst->bcr[vd] == SX_BC_PERIODIC) {
            set_error("sx_antiderivative: PERIODIC radial boundary conditions on the destination variable are not supported");
            return 1;
        }
        if (src->has_z && (src->bcb[vs] != dst->bcb[vd] || src->bct[vs] != dst->bct[vd])) {
            set_error("sx_antiderivative: the source variable's vertical boundary conditions differ from the destination variable's");
            return 1;
        }
    } else if (src->bcl[vs] != dst->bcl[vd] || src->bcl0[vs] != dst->bcl0[vd] || src->bcr[vs] != dst->bcr[vd]) {
        set_error("sx_antiderivative: the source variable's radial boundary conditions differ from the destination variable's");
        return 1;
    }
    if (!src->diag[DIAG_ANTIDERIVATIVE]) src->diag[DIAG_ANTIDERIVATIVE].reset(new AntiState());
    AntiState *st = diag_state<AntiState>(src, DIAG_ANTIDERIVATIVE);
    if (axis == SX_INT_R) {
        if (st->r_origin != origin || st->r_weight != weight || st->bcl0 != dst->bcl0[vd] || st->bcl != dst->bcl[vd] || st->bcr != dst->bcr[vd] || st->l_q != dst->l_q || !st->d_F.p) {
            AntiTables t;
            build_antiderivative_tables(src->xmin, src->xmax, src->nc, origin, weight, t);
            std::vector<double> F((size_t)2 * nb * 4, 0.0);
            AntiClsDev cls[2];
            for (int q = 0; q < 2; q++) {
                SplineClass sc;
                std::vector<double> Fq;
                std::string err;
                if (!build_antiderivative_class(src->xmin, src->xmax, src->nc, dst->l_q, q == 0 ? dst->bcl0[vd] : dst->bcl[vd], dst->bcr[vd], sc, Fq, err)) {
                    set_error(std::string(who) + ": " + err);
                    return 1;
                }
                std::copy(Fq.begin(), Fq.end(), F.begin() + (size_t)q * nb * 4);
                anti_cls_dev(sc, cls[q]);
            }
            st->r_origin = -1;      // no key while the tables are replaced
            const char *err = "sx_antiderivative: hipMalloc / copy of the radial tables failed";
            if (!st->d_P.upload(t.P, err) || !st->d_c.upload(t.c, err) || !st->d_m.upload(t.m, err) || !st->d_F.upload(F, err) || !st->d_cls.upload(cls, 2, err)) return 1;
            st->r_origin = origin; st->r_weight = weight; st->bcl0 = dst->bcl0[vd]; st->bcl = dst->bcl[vd]; st->bcr = dst->bcr[vd]; st->l_q = dst->l_q;
        }
    } else if (st->z_origin != origin || st->bcb != src->bcb[vs] || st->bct != src->bct[vs] || !st->d_ZT.p) {
        std::vector<double> ZT;
        std::string err;
        int Kp = 0, Mp = 0;
        if (!build_antiderivative_z(src->zmin, src->zmax, src->nz, src->Zb, src->bcb[vs], src->bct[vs], origin, ZT, Kp, Mp, err)) {
            set_error(std::string(who) + ": " + err);
            return 1;
        }
        st->z_origin = -1;
        if (!st->d_ZT.upload(ZT, "sx_antiderivative: hipMalloc / copy of the vertical operator failed")) return 1;
        st->z_origin = origin; st->bcb = src->bcb[vs]; st->bct = src->bct[vs]; st->Kp = Kp; st->Mp = Mp;
    }
    flush_diag(src);
    if (dst != src) {
        flush_diag(dst);
        HIPCHK(hipStreamSynchronize(dst->stream));      // the destination's own work on its A is complete before another stream writes it
    }
    if (error_status()) return 1;

    const int ncol = src->Zb * src->K2;
    const double live = (double)src->Zb * (src->has_l ? src->K2 - 1 : 1);       // block 1 is never read
    if (axis == SX_INT_R) {
        AntiRArgs a;
        a.A = src->d_A; a.D = dst->d_A;
        a.P = st->d_P; a.c = st->d_c; a.m = st->d_m; a.F = st->d_F; a.cls = st->d_cls;
        a.Cs = src->C; a.Cd = dst->C; a.col_s = (int64_t)vs * ncol; a.col_d = (int64_t)vd * ncol;
        a.nb = nb; a.K2 = src->K2; a.ncol = ncol; a.high = origin == SX_INT_FROM_HIGH;
        // the live source columns in, the destination columns out, and honestly: b and y each go out to the destination column and come
        // back (2 stores + 2 loads of the live columns); the tables [nb][7 + 1 + 1] and the factor rows [2][nb][4]
        TimedLaunch scope(src, "k_antiderivative_r", 8.0 * nb * (live + ncol + 4.0 * live) + 8.0 * nb * (9.0 + 8.0));
        hipLaunchKernelGGL(k_antiderivative_r, grid1(ncol, ANT_T), dim3(ANT_T), 0, src->stream, a);
    } else {
        AntiZArgs a;
        a.A = src->d_A; a.D = dst->d_A; a.ZT = st->d_ZT;
        a.Cs = src->C; a.Cd = dst->C; a.col_s = (int64_t)vs * ncol; a.col_d = (int64_t)vd * ncol;
        a.nb = nb; a.Zb = src->Zb; a.K2 = src->K2; a.Mp = st->Mp;
        TimedLaunch scope(src, "k_antiderivative_z", 2.0 * 8.0 * nb * ncol + 8.0 * src->Zb * src->Zb);      // the columns in and out, the operator
        if (src->K2 >= 16 && src->Zb <= 64) {
            const dim3 g((src->K2 + 15) / 16, nb);
            if (src->Zb <= 16) hipLaunchKernelGGL(k_antiderivative_z<4>, g, dim3(64), 0, src->stream, a);
            else if (src->Zb <= 32) hipLaunchKernelGGL(k_antiderivative_z<8>, g, dim3(64), 0, src->stream, a);
            else hipLaunchKernelGGL(k_antiderivative_z<16>, g, dim3(64), 0, src->stream, a);
        } else {
            hipLaunchKernelGGL(k_antiderivative_z_lane, grid1((int64_t)nb * ncol, 256), dim3(256), 0, src->stream, a);
        }
    }
    HIPCHK(hipStreamSynchronize(src->stream));
    return error_status();
}

int sx_antiderivative_check(const sx_grid_desc *grid, int32_t var_src, int32_t var_dst, int32_t axis, int32_t origin, int32_t weight,
                            int32_t k, const double *a_src, double *a_dst) {
    clear_error();
    const char *who = "sx_antiderivative_check";
    if (!desc_ok(grid, who)) return 1;
    if (!a_src || !a_dst) { set_error("sx_antiderivative_check: null argument"); return 1; }
    if (!anti_enums_ok(axis, origin, weight, who)) return 1;
    if (var_src < 1 || var_src > grid->nvars || var_dst < 1 || var_dst > grid->nvars) { set_error("sx_antiderivative_check: variable index out of range"); return 1; }
    if (grid->tile_cell0 != 0 || grid->tile_num_cells != grid->num_cells) { set_error("sx_antiderivative_check: the descriptor must be a one-tile patch"); return 1; }
    const EvalGeom eg = desc_geom(grid);
    if (k < 0 || k > eg.kDim) { set_error("sx_antiderivative_check: wavenumber out of range"); return 1; }
    if (axis == SX_INT_Z && !eg.has_z) { set_error("sx_antiderivative_check: SX_INT_Z needs an RZ or RLZ grid"); return 1; }
    const int vs = var_src - 1, vd = var_dst - 1;
    auto bc = [](const int32_t *p, int v) { return p ? p[v] : (int)SX_BC_R0; };
    auto bcl0_of = [&](int v) { return grid->bcl_k0 ? grid->bcl_k0[v] : bc(grid->bcl, v); };
    if (axis == SX_INT_R) {
        const int bl = k == 0 ? bcl0_of(vd) : bc(grid->bcl, vd), br = bc(grid->bcr, vd);
        if (bcl0_of(vd) == SX_BC_PERIODIC || bc(grid->bcl, vd) == SX_BC_PERIODIC || br == SX_BC_PERIODIC) {
            set_error("sx_antiderivative_check: PERIODIC radial boundary conditions on the destination variable are not supported");
            return 1;
        }
        if (eg.has_z && (bc(grid->bcb, vs) != bc(grid->bcb, vd) || bc(grid->bct, vs) != bc(grid->bct, vd))) {
            set_error("sx_antiderivative_check: the source variable's vertical boundary conditions differ from the destination variable's");
            return 1;
        }
        SplineClass sc;
        std::vector<double> F;
        std::string err;
        if (!build_antiderivative_class(eg.xmin, eg.xmax, eg.nc, grid->l_q > 0 ? grid->l_q : 2.0, bl, br, sc, F, err)) { set_error(std::string(who) + ": " + err); return 1; }
        AntiTables t;
        build_antiderivative_tables(eg.xmin, eg.xmax, eg.nc, origin, weight, t);
        std::vector<double> tmp(t.nb);
        antiderivative_r_host(t, sc, F.data(), a_src, tmp.data());
        std::copy(tmp.begin(), tmp.end(), a_dst);
        return 0;
    }
    if (bc(grid->bcl, vs) != bc(grid->bcl, vd) || bcl0_of(vs) != bcl0_of(vd) || bc(grid->bcr, vs) != bc(grid->bcr, vd)) {
        set_error("sx_antiderivative_check: the source variable's radial boundary conditions differ from the destination variable's");
        return 1;
    }
    if (eg.nz < 4 || eg.nz > 256 || eg.Zb > eg.nz || eg.Zb < 1 || !(eg.zmax > eg.zmin)) { set_error("sx_antiderivative_check: invalid vertical grid"); return 1; }
    std::vector<double> ZT;
    std::string err;
    int Kp = 0, Mp = 0;
    if (!build_antiderivative_z(eg.zmin, eg.zmax, eg.nz, eg.Zb, bc(grid->bcb, vs), bc(grid->bct, vs), origin, ZT, Kp, Mp, err)) {
        set_error(std::string(who) + ": " + err);
        return 1;
    }
    std::vector<double> tmp(eg.Zb);
    for (int zm = 0; zm < eg.Zb; zm++) {
        double acc = 0.0;
        for (int j = 0; j < eg.Zb; j++) acc = std::fma(ZT[(size_t)j * Mp + zm], a_src[j], acc);
        tmp[zm] = acc;
    }
    std::copy(tmp.begin(), tmp.end(), a_dst);
    return 0;
}

}  // extern "C"
