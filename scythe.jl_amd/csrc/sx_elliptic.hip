// sx_elliptic_solve: streamfunction, velocity potential and other solutions of (lap_h - alpha) psi = f from the A coefficients
// (include/scythe_hip.h, "elliptic inversion").
//
// The state in r is a cubic-B-spline Galerkin expansion and the azimuth is already diagonal - the coefficient blocks are the
// harmonics - so in the weak form, per (wavenumber k, re / im, z-mode) column,
//     K_k x = -Gamma_k g,   a = Gamma_k^T x,   K_k = Gamma_k (S + k^2 T + alpha M) Gamma_k^T   (symmetric positive definite, 7-diagonal)
// with the band matrices S = int J phi' phi', T = int phi phi / r, M = int J phi phi (J = r with an azimuth, 1 without) and the
// right-hand side g a band product of the source columns: M a (field), or, from the two wind components,
//     vorticity   r zeta  = r v_r + v - u_lambda:  g_re = (N + M0) v_re + k M0 u_im,  g_im = (N + M0) v_im - k M0 u_re
//     divergence  r delta = r u_r + u + v_lambda:  g_re = (N + M0) u_re - k M0 v_im,  g_im = (N + M0) u_im + k M0 v_re
// (N = int r phi phi', M0 = int phi phi; c_k = A[2k] + i A[2k + 1]).  The host forms the matrices and, per boundary-condition class
// of the solution variable and wavenumber, the banded Cholesky factor of K_k (sx_setup.cpp, extended precision, rounded once).
//
// k_elliptic: one lane per (z-mode, block) column of the destination variable.  The column index is the fastest in memory, so every
// row access of a wave is one coalesced line; the lanes walk the patch rows together, so a band-matrix row is one address for the
// whole wave.  Per lane: the band products of row m from a 7-row window of the 1 or 2 source columns (the partner block of the same
// wavenumber for vorticity / divergence), folded with Gamma_k; the forward sweep with the factor rows of ITS wavenumber ([k][row][4]:
// a 32-byte vector load per row, neighbouring lanes share it pairwise), the intermediate vector kept in the destination column
// as k_solve does; the back sweep; the boundary rows from Gamma_k^T.  Block 1 (Im c_0) is never read and is written as zero.
// No lane reads what another lane wrote and nothing is summed across lanes: the order of every sum is fixed, two calls agree
// bitwise and a column's result does not depend on the launch shape.
#include "sx_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

constexpr int ELL_T = 64;       // one wave per workgroup: the recurrence is serial in the rows, the waves spread over the CUs

struct EllClsDev {              // Gamma of one boundary-condition class as the kernel reads it
    int n, rl, rr, pad;
    double gl[6], gr[6];        // [q][2] as SplineClass::gl / gr
};

struct EllArgs {
    const double *A;            // source A [nb][Cs]
    double *D;                  // destination A [nb][Cd]
    const double *P, *Q;        // band tables [nb][7]: P times the lane's own block (M, or N + M0), Q times +-k the partner block (M0)
    const double *F;            // factors [kDim + 1][nb][4]
    const EllClsDev *cls;       // [2]: k = 0, k >= 1
    int64_t Cs, Cd, col_p, col_q, col_d;     // row strides; first column of the source variables and of the destination variable
    int nb, K2, ncol, kind;     // patch rows; blocks per z-mode; columns of one variable; SX_ELL_*
};

struct EllState : DiagState {
    bool have_bands = false;
    EllBands bands;
    DevBuf<double> d_M, d_NM0, d_M0, d_F;
    DevBuf<EllClsDev> d_cls;
    double alpha = -1.0;        // the key of d_F / d_cls: alpha and the destination variable's radial boundary conditions
    int bcl0 = -1, bcl = -1, bcr = -1;
};

// the band product of patch row m with the 7 window rows m - 3 .. m + 3 (rows outside the patch are zeros in the window)
__device__ __forceinline__ double ell_row(const double *__restrict__ P, const double *__restrict__ Q, int m, const double (&wp)[7],
                                          const double (&wq)[7], bool useq, double sk) {
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d < 7; d++) acc = fma(P[(int64_t)m * 7 + d], wp[d], acc);
    if (useq) {
        double aq = 0.0;
#pragma unroll
        for (int d = 0; d < 7; d++) aq = fma(Q[(int64_t)m * 7 + d], wq[d], aq);
        acc = fma(sk, aq, acc);
    }
    return acc;
}

__global__ __launch_bounds__(ELL_T) void k_elliptic(const EllArgs a) {
    const int c = blockIdx.x * ELL_T + threadIdx.x;
    if (c >= a.ncol) return;
    const int nb = a.nb, blk = c % a.K2, k = blk >> 1;
    double *__restrict__ D = a.D + a.col_d + c;
    if (blk == 1) {             // Im c_0: the padding block
        for (int m = 0; m < nb; m++) D[(int64_t)m * a.Cd] = 0.0;
        return;
    }
    const EllClsDev *__restrict__ cl = a.cls + (k > 0 ? 1 : 0);
    const int n = cl->n, rl = cl->rl, rr = cl->rr;
    const bool useq = a.kind != SX_ELL_FIELD && k > 0;
    // the sign of the partner term: vorticity +k u_im (re), -k u_re (im); divergence -k v_im (re), +k v_re (im)
    const double sk = ((blk & 1) != 0) == (a.kind == SX_ELL_VORTICITY) ? -(double)k : (double)k;
    const double *__restrict__ Ap = a.A + a.col_p + c;
    const double *__restrict__ Aq = a.A + a.col_q + (c ^ 1);
    const double *__restrict__ P = a.P, *__restrict__ Q = a.Q;
    const double4 *__restrict__ F = reinterpret_cast<const double4 *>(a.F) + (int64_t)k * nb;
    auto ldp = [&](int m) { return m >= 0 && m < nb ? Ap[(int64_t)m * a.Cs] : 0.0; };
    auto ldq = [&](int m) { return useq && m >= 0 && m < nb ? Aq[(int64_t)m * a.Cs] : 0.0; };

    double wp[7], wq[7];
    // what the last rr rows put into the last two free unknowns: needed before the sweep reaches them
    double br0 = 0.0, br1 = 0.0;
    for (int q = 0; q < rr; q++) {
        const int m = nb - 1 - q;
#pragma unroll
        for (int d = 0; d < 7; d++) { wp[d] = ldp(m - 3 + d); wq[d] = ldq(m - 3 + d); }
        const double gm = ell_row(P, Q, m, wp, wq, useq, sk);
        br0 = fma(cl->gr[q * 2], gm, br0);
        br1 = fma(cl->gr[q * 2 + 1], gm, br1);
    }
    // forward: right-hand side row by row, folded with Gamma, and L y = -Gamma g; y_i goes to row rl + i of the destination column
#pragma unroll
    for (int d = 0; d < 7; d++) { wp[d] = ldp(d - 3); wq[d] = ldq(d - 3); }
    double bl0 = 0.0, bl1 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;
    for (int m = 0; m < nb; m++) {
        const double gm = ell_row(P, Q, m, wp, wq, useq, sk);
#pragma unroll
        for (int d = 0; d < 6; d++) { wp[d] = wp[d + 1]; wq[d] = wq[d + 1]; }
        wp[6] = ldp(m + 4);
        wq[6] = ldq(m + 4);
        const int i = m - rl;
        if (i < 0) {
            bl0 = fma(cl->gl[m * 2], gm, bl0);
            bl1 = fma(cl->gl[m * 2 + 1], gm, bl1);
        } else if (i < n) {
            double s = gm;
            if (i == 0) s += bl0;
            if (i == 1) s += bl1;
            if (i == n - 1) s += br0;
            if (i == n - 2) s += br1;
            const double4 l = F[i];
            double t = fma(-l.z, y1, -s);
            t = fma(-l.y, y2, t);
            t = fma(-l.x, y3, t);
            const double y = t * l.w;
            y3 = y2; y2 = y1; y1 = y;
            D[(int64_t)m * a.Cd] = y;
        }
    }
    // back: L^T x = y, in place
    double x1 = 0.0, x2 = 0.0, x3 = 0.0, xl0 = 0.0, xl1 = 0.0, xr0 = 0.0, xr1 = 0.0;
    double4 f1 = make_double4(0.0, 0.0, 0.0, 0.0), f2 = f1, f3 = f1;      // factor rows i + 1, i + 2, i + 3
    for (int i = n - 1; i >= 0; i--) {
        const double4 l = F[i];
        double t = fma(-f1.z, x1, D[(int64_t)(rl + i) * a.Cd]);
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
    // the dependent boundary rows: a = Gamma^T x
    for (int q = 0; q < rl; q++) D[(int64_t)q * a.Cd] = fma(cl->gl[q * 2 + 1], xl1, cl->gl[q * 2] * xl0);
    for (int q = 0; q < rr; q++) D[(int64_t)(nb - 1 - q) * a.Cd] = fma(cl->gr[q * 2 + 1], xr1, cl->gr[q * 2] * xr0);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static std::vector<double> ell_round(const std::vector<long double> &m) { return std::vector<double>(m.begin(), m.end()); }

static bool ell_alpha_ok(double alpha, const char *who) {
    if (std::isfinite(alpha) && alpha >= 0.0) return true;
    set_error(std::string(who) + ": alpha must be finite and >= 0");
    return false;
}

// the factors of every wavenumber of the handle for the boundary conditions (bcl0: k = 0; bcl: k >= 1; bcr), as one [kDim + 1][nb][4]
// table and the two Gamma records
static bool ell_factors(const EllBands &eb, int has_l, double xmin, int kDim, int bcl0, int bcl, int bcr, double alpha, const char *who,
                        std::vector<double> &F, EllClsDev (&cls)[2]) {
    const int nb = eb.nb;
    F.assign((size_t)(kDim + 1) * nb * 4, 0.0);
    for (int q = 0; q < 2; q++) {
        if (q == 1 && kDim == 0) { cls[1] = cls[0]; break; }
        EllClass ec;
        std::string err;
        if (!build_elliptic_class(eb, has_l, xmin, q == 0 ? bcl0 : bcl, bcr, q == 0 ? 0 : 1, q == 0 ? 0 : kDim, alpha, ec, err)) {
            set_error(std::string(who) + ": " + err);
            return false;
        }
        std::copy(ec.L.begin(), ec.L.end(), F.begin() + (size_t)(q == 0 ? 0 : 1) * nb * 4);
        cls[q].n = ec.n; cls[q].rl = ec.rl; cls[q].rr = ec.rr; cls[q].pad = 0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 2; j++) { cls[q].gl[i * 2 + j] = ec.gl[i][j]; cls[q].gr[i * 2 + j] = ec.gr[i][j]; }
    }
    return true;
}

static bool ell_same_grid(const sx_handle *s, const sx_handle *d) {
    return s->geom == d->geom && s->xmin == d->xmin && s->xmax == d->xmax && s->nc == d->nc && s->uniform_L == d->uniform_L && s->kDim == d->kDim &&
           s->nz == d->nz && s->Zb == d->Zb && s->zmin == d->zmin && s->zmax == d->zmax;
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_elliptic_solve(sx_handle *src, int32_t rhs_kind, int32_t var_a, int32_t var_b, double alpha, sx_handle *dst, int32_t var_dst) {
    clear_error();
    const char *who = "sx_elliptic_solve";
    if (!src || !dst) { set_error("null handle"); return 1; }
    if (rhs_kind != SX_ELL_FIELD && rhs_kind != SX_ELL_VORTICITY && rhs_kind != SX_ELL_DIVERGENCE) {
        set_error("sx_elliptic_solve: rhs_kind must be SX_ELL_FIELD, SX_ELL_VORTICITY or SX_ELL_DIVERGENCE");
        return 1;
    }
    const bool two = rhs_kind != SX_ELL_FIELD;
    if (var_a < 1 || var_a > src->V || (two && (var_b < 1 || var_b > src->V)) || var_dst < 1 || var_dst > dst->V) {
        set_error("sx_elliptic_solve: variable index out of range");
        return 1;
    }
    if (dst == src && (var_dst == var_a || (two && var_dst == var_b))) {
        set_error("sx_elliptic_solve: the destination variable is a source variable");
        return 1;
    }
    if (two && !src->has_l) { set_error("sx_elliptic_solve: vorticity / divergence need an RL or RLZ grid"); return 1; }
    if (src->ncells != src->nc || dst->ncells != dst->nc) { set_error("sx_elliptic_solve: source and destination must be one-tile patches"); return 1; }
    if (!ell_same_grid(src, dst)) { set_error("sx_elliptic_solve: the destination's grid differs from the source's"); return 1; }
    const int vd = var_dst - 1, vp = (rhs_kind == SX_ELL_VORTICITY ? var_b : var_a) - 1, vq = (rhs_kind == SX_ELL_VORTICITY ? var_a : two ? var_b : var_a) - 1;
    if (src->has_z)
        for (int v : {var_a - 1, two ? var_b - 1 : var_a - 1})
            if (src->bcb[v] != dst->bcb[vd] || src->bct[v] != dst->bct[vd]) {
                set_error("sx_elliptic_solve: a source variable's vertical boundary conditions differ from the destination variable's");
                return 1;
            }
    if (!ell_alpha_ok(alpha, who)) return 1;
    if (!src->diag[DIAG_ELLIPTIC]) src->diag[DIAG_ELLIPTIC].reset(new EllState());
    EllState *st = diag_state<EllState>(src, DIAG_ELLIPTIC);
    const int nb = src->b_rDim;
    if (!st->have_bands) {
        build_elliptic_bands(src->has_l, src->xmin, src->xmax, src->nc, st->bands);
        std::vector<double> M = ell_round(st->bands.M), N = ell_round(st->bands.N), M0 = ell_round(st->bands.M0), NM0(M.size());
        for (size_t i = 0; i < M.size(); i++) NM0[i] = N[i] + M0[i];
        const char *err = "sx_elliptic_solve: hipMalloc / copy of the band matrices failed";
        if (!st->d_M.upload(M, err) || !st->d_NM0.upload(NM0, err) || !st->d_M0.upload(M0, err)) return 1;
        st->have_bands = true;
    }
    if (st->alpha != alpha || st->bcl0 != dst->bcl0[vd] || st->bcl != dst->bcl[vd] || st->bcr != dst->bcr[vd] || !st->d_F.p) {
        std::vector<double> F;
        EllClsDev cls[2];
        if (!ell_factors(st->bands, src->has_l, src->xmin, src->kDim, dst->bcl0[vd], dst->bcl[vd], dst->bcr[vd], alpha, who, F, cls)) return 1;
        st->alpha = -1.0;       // no key while the tables are replaced
        const char *err = "sx_elliptic_solve: hipMalloc / copy of the factors failed";
        if (!st->d_F.upload(F, err) || !st->d_cls.upload(cls, 2, err)) return 1;
        st->alpha = alpha; st->bcl0 = dst->bcl0[vd]; st->bcl = dst->bcl[vd]; st->bcr = dst->bcr[vd];
    }
    flush_diag(src);
    if (dst != src) {
        flush_diag(dst);
        HIPCHK(hipStreamSynchronize(dst->stream));      // the destination's own work on its A is complete before another stream writes it
    }
    if (error_status()) return 1;

    EllArgs a;
    a.A = src->d_A; a.D = dst->d_A;
    a.P = two ? st->d_NM0 : st->d_M; a.Q = st->d_M0; a.F = st->d_F; a.cls = st->d_cls;
    a.Cs = src->C; a.Cd = dst->C;
    a.nb = nb; a.K2 = src->K2; a.ncol = src->Zb * src->K2; a.kind = rhs_kind;
    a.col_p = (int64_t)vp * a.ncol; a.col_q = (int64_t)vq * a.ncol; a.col_d = (int64_t)vd * a.ncol;
    // algorithmic bytes: the live source columns in (block 1 never; the partner block not for k = 0), the destination columns out, the factors
    const double live = (double)src->Zb * (src->has_l ? src->K2 - 1 : 1), partner = two ? (double)src->Zb * (src->K2 - 2) : 0.0;
    {
        TimedLaunch scope(src, "k_elliptic", 8.0 * nb * (live + partner + a.ncol) + 8.0 * 4.0 * nb * (src->kDim + 1));
        hipLaunchKernelGGL(k_elliptic, grid1(a.ncol, ELL_T), dim3(ELL_T), 0, src->stream, a);
    }
    HIPCHK(hipStreamSynchronize(src->stream));
    return error_status();
}

int sx_elliptic_check(const sx_grid_desc *grid, int32_t var_dst, int32_t k, double alpha, const double *g, double *a) {
    clear_error();
    const char *who = "sx_elliptic_check";
    if (!desc_ok(grid, who)) return 1;
    if (!g || !a) { set_error("sx_elliptic_check: null argument"); return 1; }
    if (var_dst < 1 || var_dst > grid->nvars) { set_error("sx_elliptic_check: variable index out of range"); return 1; }
    if (grid->tile_cell0 != 0 || grid->tile_num_cells != grid->num_cells) { set_error("sx_elliptic_check: the descriptor must be a one-tile patch"); return 1; }
    const EvalGeom eg = desc_geom(grid);
    if (k < 0 || k > eg.kDim) { set_error("sx_elliptic_check: wavenumber out of range"); return 1; }
    if (!ell_alpha_ok(alpha, who)) return 1;
    const int v = var_dst - 1;
    const int bcl = grid->bcl ? grid->bcl[v] : SX_BC_R0, bcr = grid->bcr ? grid->bcr[v] : SX_BC_R0;
    const int bcl0 = grid->bcl_k0 ? grid->bcl_k0[v] : bcl;
    EllBands eb;
    build_elliptic_bands(eg.has_l, eg.xmin, eg.xmax, eg.nc, eb);
    EllClass ec;
    std::string err;
    if (!build_elliptic_class(eb, eg.has_l, eg.xmin, k == 0 ? bcl0 : bcl, bcr, k, k, alpha, ec, err)) { set_error(std::string(who) + ": " + err); return 1; }
    std::vector<double> tmp(eb.nb);
    elliptic_apply_host(ec, k, eb.nb, g, tmp.data());
    std::copy(tmp.begin(), tmp.end(), a);
    return 0;
}

}  // extern "C"
