// sx_extrema / sx_extremum_refine / sx_newton_step: extrema of field programs with their locations, and the refinement of a gridpoint
// extremum to the stationary point of the continuous spectral function (include/scythe_hip.h).
//
// The scan, two stages.  k_extrema takes k_reduce's decomposition (sx_redprog.hpp): a workgroup takes one piece of one ring, a thread
// keeps ONE level and strides over the lambdas, reads every plane the program names once, evaluates all outputs in plain fp64 and keeps
// (min, its point, max, its point) per output in registers; the threads that share a level are combined through LDS.  Grids without an
// azimuth: thread = point.  k_extrema_rings folds the pieces of a ring (SX_EXT_AZIMUTH), k_extrema_domain folds pieces x levels with a
// fixed tree (SX_EXT_DOMAIN).  Candidates are ordered as (value, point index) with NaN before everything (ext_before): that order is
// total, so the fold is associative and commutative and the result does not depend on which lane folds what.  No atomics.
//
// The refinement.  k_refine is k_parcels with derivatives: one workgroup per start point, the same lane count, the same column a lane
// sums and the same order of the reduction, all stated once in sx_point.hpp; per iteration it forms the weights from the position,
// sums the 10 derivatives of order <= 2 in ONE pass over the 4 node rows, and lane 0 takes the step with newton_step - the function
// sx_newton_step runs on the host.
#include "sx_point.hpp"
#include "sx_redprog.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

constexpr int EXT_TF = 1024;              // threads per workgroup of k_extrema_domain
constexpr size_t REFINE_LDS_MAX = 64 * 1024;
constexpr int REFINE_ND = 10;             // u, u_r, u_l, u_z, u_rr, u_rl, u_rz, u_ll, u_lz, u_zz
constexpr int REFINE_BC = 8;              // doubles lane 0 hands to the workgroup: r, lambda, z, go-on flag

// ---- the order of the candidates -------------------------------------------------------------------------------------------------
// does candidate (w, j) come before (v, i)?  sign < 0: as a minimum, sign > 0: as a maximum.  An index < 0 is "no candidate".  A NaN
// comes before every number, the lower index first among NaNs and among equal values (-0.0 == +0.0).
__host__ __device__ inline bool ext_before(int sign, double w, int64_t j, double v, int64_t i) {
    if (j < 0) return false;
    if (i < 0) return true;
    const bool wn = w != w, vn = v != v;
    if (wn || vn) return wn && (!vn || j < i);
    if (w == v) return j < i;
    return sign < 0 ? w < v : w > v;
}
__host__ __device__ inline void ext_fold(int sign, double &v, int64_t &i, double w, int64_t j) {
    if (ext_before(sign, w, j, v, i)) { v = w; i = j; }
}

// the outputs of the program at one point, each the sum of its terms in term order (plain fp64)
template <class ST>
__device__ inline void ext_point(const Planes<ST> &P, int V, int64_t N, int64_t pt, double r, const RedProg &g, double (&q)[RED_OUT]) {
    double val[RED_PLANES];
    red_load_planes<ST>(P, V, N, pt, g, val);
    const RedPow pw = red_pow(r);
#pragma unroll
    for (int o = 0; o < RED_OUT; o++) q[o] = red_output(g, o, val, pw);
}

// RINGS: grid = pieces; a thread's level is tid % nz, its first lambda lam0 + tid / nz, its stride RED_T / nz lambdas.
// !RINGS (every ring has one lambda): grid = ceil(N / RED_T); thread = point; piece = ring.
// pv / pi [min, max][piece][output][level]
template <class ST, bool RINGS>
__global__ __launch_bounds__(RED_T) void k_extrema(Planes<ST> P, int V, int64_t N, int nz, const RedItem *__restrict__ items,
                                                   const int64_t *__restrict__ pstart, const double *__restrict__ rh, RedProg g, int n_items,
                                                   double *__restrict__ pv, long long *__restrict__ pi) {
    __shared__ double s_v[RED_T];
    __shared__ long long s_i[RED_T];
    const int tid = threadIdx.x;
    const int64_t half = (int64_t)n_items * g.n_out * nz;
    double q[RED_OUT];
    if (RINGS) {
        double mn[RED_OUT], mx[RED_OUT];
        int64_t in[RED_OUT], ix[RED_OUT];
#pragma unroll
        for (int o = 0; o < RED_OUT; o++) { mn[o] = mx[o] = 0.0; in[o] = ix[o] = -1; }
        const RedItem it = items[blockIdx.x];
        const int G = RED_T / nz, z = tid % nz, gl = tid / nz;
        const int64_t h0 = pstart[it.ring];
        const double r = rh[h0];
        if (gl < G)
            for (int l = it.lam0 + gl; l < it.lam0 + it.nlam; l += G) {
                const int64_t pt = (h0 + l) * nz + z;
                ext_point<ST>(P, V, N, pt, r, g, q);
#pragma unroll
                for (int o = 0; o < RED_OUT; o++) {
                    if (o >= g.n_out) continue;
                    ext_fold(-1, mn[o], in[o], q[o], pt);
                    ext_fold(+1, mx[o], ix[o], q[o], pt);
                }
            }
#pragma unroll
        for (int o = 0; o < RED_OUT; o++) {
            if (o >= g.n_out) continue;
#pragma unroll
            for (int w = 0; w < 2; w++) {
                s_v[tid] = w ? mx[o] : mn[o]; s_i[tid] = w ? ix[o] : in[o];
                __syncthreads();
                if (tid < nz) {
                    double a = s_v[tid];
                    int64_t b = s_i[tid];
                    for (int k = 1; k < G; k++) ext_fold(w ? +1 : -1, a, b, s_v[k * nz + tid], s_i[k * nz + tid]);
                    const int64_t e = w * half + ((int64_t)blockIdx.x * g.n_out + o) * nz + tid;
                    pv[e] = a; pi[e] = b;
                }
                __syncthreads();
            }
        }
    } else {
        const int64_t pt = (int64_t)blockIdx.x * RED_T + tid;
        if (pt >= N) return;
        const int64_t ring = pt / nz;
        const int z = (int)(pt - ring * nz);
        ext_point<ST>(P, V, N, pt, rh[ring], g, q);
#pragma unroll
        for (int o = 0; o < RED_OUT; o++) {
            if (o >= g.n_out) continue;
            const int64_t e = ((int64_t)ring * g.n_out + o) * nz + z;
            pv[e] = q[o]; pi[e] = pt;
            pv[half + e] = q[o]; pi[half + e] = pt;
        }
    }
}

// SX_EXT_AZIMUTH: thread = (min / max, ring, level, output), min / max fastest as in val; the ring's pieces folded
__global__ void k_extrema_rings(const double *__restrict__ pv, const long long *__restrict__ pi, const int *__restrict__ first, int n_items,
                                int nrings, int nz, int n_out, double *__restrict__ val, long long *__restrict__ idx) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)2 * nrings * nz * n_out) return;
    const int w = (int)(e & 1), ring = (int)(e / 2 % nrings), z = (int)(e / 2 / nrings % nz), o = (int)(e / 2 / nrings / nz);
    const int64_t half = (int64_t)n_items * n_out * nz;
    double a = 0.0;
    int64_t b = -1;
    for (int i = first[ring]; i < first[ring + 1]; i++) {
        const int64_t s = w * half + ((int64_t)i * n_out + o) * nz + z;
        ext_fold(w ? +1 : -1, a, b, pv[s], pi[s]);
    }
    val[e] = a; idx[e] = b;
}

// SX_EXT_DOMAIN: grid (n_out, 2); the (piece, level) entries of an output are dealt to the EXT_TF threads in order, then a fixed tree
__global__ __launch_bounds__(EXT_TF) void k_extrema_domain(const double *__restrict__ pv, const long long *__restrict__ pi, int n_items, int nz,
                                                           int n_out, double *__restrict__ val, long long *__restrict__ idx) {
    __shared__ double s_v[EXT_TF];
    __shared__ long long s_i[EXT_TF];
    const int tid = threadIdx.x, o = blockIdx.x, w = blockIdx.y, sign = w ? +1 : -1;
    const int64_t half = (int64_t)n_items * n_out * nz;
    double a = 0.0;
    int64_t b = -1;
    for (int64_t e = tid; e < (int64_t)n_items * nz; e += EXT_TF) {
        const int i = (int)(e / nz), z = (int)(e - (int64_t)i * nz);
        const int64_t s = w * half + ((int64_t)i * n_out + o) * nz + z;
        ext_fold(sign, a, b, pv[s], pi[s]);
    }
    s_v[tid] = a; s_i[tid] = b;
    __syncthreads();
    for (int s = EXT_TF / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            ext_fold(sign, a, b, s_v[tid + s], s_i[tid + s]);
            s_v[tid] = a; s_i[tid] = b;
        }
        __syncthreads();
    }
    if (tid == 0) { val[2 * o + w] = a; idx[2 * o + w] = b; }
}

// ---- the Newton step -------------------------------------------------------------------------------------------------------------
struct NewtonGeom {
    int pole;                              // pole: an RL / RLZ tile whose first cell starts at xmin == 0
    double DX, lo, hi, zmin, zmax;         // the tile's radial extent as eval_radius_ok reads it
};

// One safeguarded Newton step towards the stationary point of u from its derivatives d at pos = (r, lambda, z); what the header
// says of sx_newton_step.  Returns the status, -1 = took a step, go on.
__host__ __device__ inline int newton_step(const NewtonGeom &G, int want, int mask, double tol, const double (&pos)[3], const double (&d)[REFINE_ND],
                                           double (&np)[3]) {
    const double r = pos[0], lam = pos[1], z = pos[2];
    np[0] = r; np[1] = lam; np[2] = z;
    const bool fr = mask & 1, fl = mask & 2, fz = mask & 4, cart = fr && fl;
    if (mask == 0) return 0;
    if (cart && G.pole && r < 1e-6 * G.DX) return 3;
    const double ur = d[1], ul = d[2], uz = d[3], urr = d[4], url = d[5], urz = d[6], ull = d[7], ulz = d[8], uzz = d[9];
    // gradient and Hessian in the coordinates of the step: (X, Y, z) or (r, lambda, z)
    double g[3] = {ur, ul, uz};
    double H[3][3] = {{urr, url, urz}, {url, ull, ulz}, {urz, ulz, uzz}};
    double c = 1.0, s = 0.0;
    if (cart) {
        s = sin(lam); c = cos(lam);
        const double ri = 1.0 / r;
        const double a = (url * ri) - (ul * ri) * ri;              // (u_l / r)_r
        const double b = (ur * ri) + (ull * ri) * ri;              // u_r / r + u_ll / r^2
        g[0] = (ur * c) - ((ul * ri) * s);
        g[1] = (ur * s) + ((ul * ri) * c);
        H[0][0] = ((c * c) * urr - (2.0 * (s * c)) * a) + (s * s) * b;
        H[1][1] = ((s * s) * urr + (2.0 * (s * c)) * a) + (c * c) * b;
        H[0][1] = H[1][0] = (s * c) * (urr - b) + ((c * c) - (s * s)) * a;
        H[0][2] = H[2][0] = (urz * c) - ((ulz * ri) * s);
        H[1][2] = H[2][1] = (urz * s) + ((ulz * ri) * c);
    }
    // the free rows
    int act[3], n = 0;
    if (fr) act[n++] = 0;
    if (fl) act[n++] = 1;
    if (fz) act[n++] = 2;
    double M[3][3], b3[3];
    for (int i = 0; i < n; i++) {
        b3[i] = -g[act[i]];
        for (int j = 0; j < n; j++) M[i][j] = H[act[i]][act[j]];
    }
    // L D L^T without pivoting; definite in the sense `want` asks for: every pivot < 0 (MAX), > 0 (MIN), finite and != 0 (ANY)
    double D[3] = {0.0, 0.0, 0.0}, Lm[3][3] = {{0.0}};
    for (int j = 0; j < n; j++) {
        double dj = M[j][j];
        for (int k = 0; k < j; k++) dj -= (Lm[j][k] * Lm[j][k]) * D[k];
        D[j] = dj;
        const bool ok = want > 0 ? dj < 0.0 : want < 0 ? dj > 0.0 : (dj < 0.0 || dj > 0.0);
        if (!ok || !(fabs(dj) <= 1.79769313486231570815e308)) return 4;
        for (int i = j + 1; i < n; i++) {
            double x = M[i][j];
            for (int k = 0; k < j; k++) x -= (Lm[i][k] * Lm[j][k]) * D[k];
            Lm[i][j] = x / dj;
        }
    }
    double y[3], st[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < n; i++) {
        double x = b3[i];
        for (int k = 0; k < i; k++) x -= Lm[i][k] * y[k];
        y[i] = x;
    }
    for (int i = n - 1; i >= 0; i--) {
        double x = y[i] / D[i];
        for (int k = i + 1; k < n; k++) x -= Lm[k][i] * st[act[k]];
        st[act[i]] = x;
    }
    // one factor for the whole step: horizontal length <= DX, |dz| <= (zmax - zmin) / 8
    const double zlen = G.zmax - G.zmin;
    double hl = cart ? hypot(st[0], st[1]) : fr ? fabs(st[0]) : fl ? fabs(r * st[1]) : 0.0, vl = fz ? fabs(st[2]) : 0.0;
    double f = 1.0;
    if (hl > G.DX) f = G.DX / hl;
    if (fz && vl > zlen / 8.0) f = fmin(f, (zlen / 8.0) / vl);
    if (!(f >= 0.0 && f <= 1.0)) return 4;                         // a NaN step: nothing to follow
    if (f != 1.0) {
        for (int i = 0; i < 3; i++) st[i] *= f;
        hl *= f; vl *= f;
    }
    double rn = r, ln = lam, zn = z;
    if (cart) {
        const double X = (r * c) + st[0], Y = (r * s) + st[1];
        rn = hypot(X, Y);
        ln = rn == 0.0 ? 0.0 : atan2(Y, X);
        if (ln <= -M_PI) ln = M_PI;                                // (-pi, pi]
    } else if (fr) {
        rn = r + st[0];
    } else if (fl) {
        ln = lam + st[1];
        ln = ln - 6.283185307179586 * rint(ln / 6.283185307179586);
        if (ln <= -M_PI || ln > M_PI) ln = M_PI;                   // (-pi, pi]; a frozen lambda is never touched
    }
    if (fz) zn = z + st[2];
    if (!(rn >= G.lo && rn <= G.hi)) return 1;
    if (fz && !(zn >= G.zmin && zn <= G.zmax)) return 2;
    np[0] = rn; np[1] = ln; np[2] = zn;
    return (hl <= tol * G.DX && vl <= tol * zlen) ? 0 : -1;
}

// ---- k_refine --------------------------------------------------------------------------------------------------------------------
struct RefineArgs {
    const double *A;       // [b_rDim][C]
    const double *w3;      // [3][nz][Zb] CA, Dc CA, Dc Dc CA of the variable's vertical class (EvalClasses::d_w3)
    const double *start;   // [n_coord][n], |lambda| <= 2 pi
    double *pos, *grad;    // [n_coord][n]
    double *value;         // [n]
    int *status, *iters;   // [n]
    int64_t C, n;
    int var, cr, cl, cz, Zb, nz, K2, kDim, cell_lo, cell_hi, want, mask, max_iter;
    double xmin, tol;
    NewtonGeom G;
};

// LDS (doubles): cs [kDim + 1] double2 | t [nz] | wz [3][Zb] | red [waves][10] | bc [REFINE_BC]
__global__ __launch_bounds__(PARCEL_T) void k_refine(RefineArgs a) {
    extern __shared__ double lds[];
    double2 *cs = reinterpret_cast<double2 *>(lds);
    double *tz = lds + 2 * (size_t)(a.kDim + 1);
    double *wz = tz + a.nz;
    double *red = wz + 3 * (size_t)a.Zb;
    double *bc = red + REFINE_ND * (PARCEL_T / 64);
    const int tid = threadIdx.x, T = blockDim.x;
    const int64_t i = blockIdx.x;
    const int ncol = a.Zb * a.K2;

    double r = a.start[(int64_t)a.cr * a.n + i];
    double lam = a.cl >= 0 ? a.start[(int64_t)a.cl * a.n + i] : 0.0;
    double z = a.cz >= 0 ? a.start[(int64_t)a.cz * a.n + i] : 0.0;
    int steps = 0, status = 0;
    bool last = false;                      // the evaluation in progress is the one the outputs report

    for (;;) {
        // ---- weights (sx_point.hpp), with the derivative rows
        const int cell = point_cell(a.xmin, a.G.DX, a.cell_lo, a.cell_hi, r);
        double phi[3][4];
        point_basis<3>(a.xmin, a.G.DX, cell, r, phi);
        az_table(cs, a.kDim, lam, tid, T);
        if (a.cz >= 0) {
            const double th = cheb_theta(a.G.zmin, a.G.zmax, z);
            for (int n = tid; n < a.nz; n += T) tz[n] = cheb_entry(n, a.nz, th);
            __syncthreads();
            for (int q = tid; q < 3 * a.Zb; q += T) {
                const int m = q / a.Zb, zm = q - m * a.Zb;
                wz[q] = cheb_weight(tz, 1, a.w3 + (size_t)m * a.nz * a.Zb + zm, a.nz, a.Zb);
            }
        } else {
            if (tid < 3) wz[tid] = tid == 0 ? 1.0 : 0.0;          // Zb = 1 without a vertical
        }
        __syncthreads();

        // ---- one pass over the 4 node rows for the 10 derivatives
        double acc[REFINE_ND];
#pragma unroll
        for (int m = 0; m < REFINE_ND; m++) acc[m] = 0.0;
        const double *__restrict__ Ac = a.A + (int64_t)cell * a.C + (int64_t)a.var * ncol;
        for (int col = tid; col < ncol; col += T) {
            const int zm = col / a.K2, blk = col - zm * a.K2;
            if (az_padding(blk)) continue;
            double F0, F1, F2;
            az_factors(blk, cs, 1, F0, F1, F2);
            const double *__restrict__ p = Ac + col;
            const double a0 = p[0], a1 = p[a.C], a2 = p[2 * a.C], a3 = p[3 * a.C];
            const double s0 = fma(phi[0][3], a3, fma(phi[0][2], a2, fma(phi[0][1], a1, phi[0][0] * a0)));
            const double s1 = fma(phi[1][3], a3, fma(phi[1][2], a2, fma(phi[1][1], a1, phi[1][0] * a0)));
            const double s2 = fma(phi[2][3], a3, fma(phi[2][2], a2, fma(phi[2][1], a1, phi[2][0] * a0)));
            const double z0 = wz[zm], z1 = wz[a.Zb + zm], z2 = wz[2 * a.Zb + zm];
            acc[0] = fma(s0, F0 * z0, acc[0]);
            acc[1] = fma(s1, F0 * z0, acc[1]);
            acc[2] = fma(s0, F1 * z0, acc[2]);
            acc[3] = fma(s0, F0 * z1, acc[3]);
            acc[4] = fma(s2, F0 * z0, acc[4]);
            acc[5] = fma(s1, F1 * z0, acc[5]);
            acc[6] = fma(s1, F0 * z1, acc[6]);
            acc[7] = fma(s0, F2 * z0, acc[7]);
            acc[8] = fma(s0, F1 * z1, acc[8]);
            acc[9] = fma(s0, F0 * z2, acc[9]);
        }
        point_sum<REFINE_ND>(acc, red, tid, T);

        // ---- lane 0 decides
        if (tid == 0) {
            const double (&d)[REFINE_ND] = acc;
            bool go = false;
            if (!last) {
                const double pos[3] = {r, lam, z};
                double np[3];
                const int st = newton_step(a.G, a.want, a.mask, a.tol, pos, d, np);
                if (st == 0 && a.mask == 0) {
                    status = 0;
                } else if (st <= 0) {                              // moved: the outputs are those of one more evaluation there
                    r = np[0]; lam = np[1]; z = np[2];
                    steps++;
                    status = st == 0 ? 0 : 5;
                    last = st == 0 || steps >= a.max_iter;
                    go = true;
                } else {
                    status = st;
                }
            }
            if (!go) {
                a.pos[(int64_t)a.cr * a.n + i] = r; a.grad[(int64_t)a.cr * a.n + i] = d[1];
                if (a.cl >= 0) { a.pos[(int64_t)a.cl * a.n + i] = lam; a.grad[(int64_t)a.cl * a.n + i] = d[2]; }
                if (a.cz >= 0) { a.pos[(int64_t)a.cz * a.n + i] = z; a.grad[(int64_t)a.cz * a.n + i] = d[3]; }
                a.value[i] = d[0];
                a.status[i] = status;
                a.iters[i] = steps;
            }
            bc[0] = r; bc[1] = lam; bc[2] = z; bc[3] = go ? 1.0 : 0.0; bc[4] = last ? 1.0 : 0.0;
        }
        __syncthreads();
        const bool go = bc[3] != 0.0;
        r = bc[0]; lam = bc[1]; z = bc[2]; last = bc[4] != 0.0;
        __syncthreads();                                           // bc, cs, tz, wz and red are rewritten by the next iteration
        if (!go) return;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct ExtremaState : DiagState {      // The work list: the handle's scan table (sx_redprog.hpp)
    DevBuf<double> d_pv, d_val;     // [2][piece][output][level]; the results
    DevBuf<long long> d_pi, d_idx;
    // refinement
    DevBuf<double> d_f;             // start | pos | grad [n_coord][n] each, value [n]
    DevBuf<int> d_i;                // status | iters
};

static ExtremaState *extrema_state(sx_handle *h) {
    if (!h->diag[DIAG_EXTREMA]) h->diag[DIAG_EXTREMA].reset(new ExtremaState());
    return diag_state<ExtremaState>(h, DIAG_EXTREMA);
}

static size_t refine_lds(const sx_handle *h) {
    return sizeof(double) * (2 * (size_t)(h->kDim + 1) + (h->has_z ? h->nz : 1) + 3 * (size_t)(h->has_z ? h->Zb : 1) + REFINE_ND * (PARCEL_T / 64) + REFINE_BC);
}

static NewtonGeom newton_geom(const EvalGeom &g) {
    NewtonGeom G;
    G.pole = g.has_l && g.xmin == 0.0 && g.cell0 == 0;
    G.DX = g.DX; G.lo = g.tile_lo(); G.hi = g.tile_hi(); G.zmin = g.zmin; G.zmax = g.zmax;
    return G;
}

// what sx_extremum_refine and sx_newton_step refuse of (want, free_mask, tol)
static bool newton_args_ok(const EvalGeom &g, int want, int mask, double tol, const char *who) {
    if (want < -1 || want > 1) { set_error(std::string(who) + ": want must be SX_EXT_MIN, SX_EXT_ANY or SX_EXT_MAX"); return false; }
    if (mask & ~7) { set_error(std::string(who) + ": free_mask has bits other than SX_EXT_FREE_R | SX_EXT_FREE_L | SX_EXT_FREE_Z"); return false; }
    if ((mask & 2) && !g.has_l) { set_error(std::string(who) + ": SX_EXT_FREE_L on a geometry without an azimuth"); return false; }
    if ((mask & 4) && !g.has_z) { set_error(std::string(who) + ": SX_EXT_FREE_Z on a geometry without a vertical"); return false; }
    if (!std::isfinite(tol)) { set_error(std::string(who) + ": tol is NaN or Inf"); return false; }
    return true;
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_extrema(sx_handle *h, int32_t kind, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_out,
               double *val, int64_t *idx) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    if (kind != SX_EXT_DOMAIN && kind != SX_EXT_AZIMUTH) { set_error("sx_extrema: kind must be SX_EXT_DOMAIN or SX_EXT_AZIMUTH"); return 1; }
    const sx_grid_desc gd = desc_of(h);
    int32_t planes[RED_PLANES][2], n_planes = 0;
    RedProg prog;
    if (!red_program("sx_extrema", &gd, source, n_terms, coef, terms, n_out, planes, &n_planes, prog)) return 1;
    if (n_out > 0 && (!val || !idx)) { set_error("sx_extrema: null val or idx with n_out > 0"); return 1; }
    if (n_out == 0) return 0;
    ExtremaState *st = extrema_state(h);
    ScanGrid *sg = scan_grid(h, "sx_extrema", false);
    if (!sg) return 1;

    const size_t n_res = kind == SX_EXT_AZIMUTH ? (size_t)2 * h->nrings * h->nz * n_out : (size_t)2 * n_out;
    const size_t n_part = (size_t)2 * sg->n_items * n_out * h->nz;
    if (!st->d_pv.grow(n_part, "sx_extrema") || !st->d_pi.grow(n_part, "sx_extrema") || !st->d_val.grow(n_res, "sx_extrema") ||
        !st->d_idx.grow(n_res, "sx_extrema"))
        return 1;
    {
        TimedLaunch scope(h, "k_extrema", red_bytes(h, source, planes, n_planes));
        scan_dispatch(h, source, [&](auto st_t, auto rings, auto P) {
            constexpr bool RINGS = decltype(rings)::value;
            hipLaunchKernelGGL((k_extrema<decltype(st_t), RINGS>), dim3(RINGS ? (unsigned)sg->n_items : scan_flat_blocks(h)), dim3(RED_T), 0, h->stream, P,
                               h->V, h->N, h->nz, sg->d_items, h->d_pstart, h->d_r, prog, sg->n_items, st->d_pv, st->d_pi);
        });
    }
    {
        TimedLaunch scope(h, "k_extrema_final", 0.0);
        if (kind == SX_EXT_AZIMUTH)
            hipLaunchKernelGGL(k_extrema_rings, grid1((int64_t)n_res, 256), dim3(256), 0, h->stream, st->d_pv, st->d_pi, sg->d_first, sg->n_items,
                               h->nrings, h->nz, n_out, st->d_val, st->d_idx);
        else
            hipLaunchKernelGGL(k_extrema_domain, dim3((unsigned)n_out, 2), dim3(EXT_TF), 0, h->stream, st->d_pv, st->d_pi, sg->n_items, h->nz, n_out,
                               st->d_val, st->d_idx);
    }
    std::vector<double> rv(n_res);      // held back until the call has succeeded: a failed call writes nothing
    std::vector<long long> ri(n_res);
    HIPCHK(hipMemcpyAsync(rv.data(), st->d_val, sizeof(double) * n_res, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ri.data(), st->d_idx, sizeof(long long) * n_res, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (error_status()) return 1;
    std::memcpy(val, rv.data(), sizeof(double) * n_res);
    for (size_t q = 0; q < n_res; q++) idx[q] = (int64_t)ri[q];
    return 0;
}

int sx_extremum_refine(sx_handle *h, int32_t var, int32_t want, int32_t free_mask, double tol, int32_t max_iter, int64_t n, const double *start,
                       double *pos, double *value, double *grad, int32_t *status, int32_t *iters) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    const char *who = "sx_extremum_refine";
    if (n < 0) { set_error("sx_extremum_refine: n is negative"); return 1; }
    if (n > 0x7fffffff) { set_error("sx_extremum_refine: more than 2^31 - 1 points"); return 1; }
    if (n > 0 && (!start || !pos || !value || !grad || !status || !iters)) { set_error("sx_extremum_refine: null argument with n > 0"); return 1; }
    if (var < 1 || var > h->V) { set_error("sx_extremum_refine: var is 1-based and at most nvars"); return 1; }
    const EvalGeom g = eval_geom_of(h);
    if (!newton_args_ok(g, want, free_mask, tol, who)) return 1;
    if (h->ncells != h->nc) { set_error("sx_extremum_refine: one-tile patches only"); return 1; }
    if (refine_lds(h) > REFINE_LDS_MAX) {
        set_error("sx_extremum_refine: the weights of one point do not fit the LDS (need 2 (kDim + 1) + zDim + 3 b_zDim + 48 <= 8192 doubles)");
        return 1;
    }
    if (n == 0) return 0;
    if (!eval_points_ok(h, start, n, who, "start")) return 1;
    const EvalClasses *k = h->has_z ? eval_classes(h) : nullptr;
    if (h->has_z && !k) return 1;
    ExtremaState *st = extrema_state(h);
    const int nco = h->ncoord, Zb = h->has_z ? h->Zb : 1, nz = h->has_z ? h->nz : 1;
    const size_t per = (size_t)3 * nz * Zb;
    const size_t blk = (size_t)nco * n;
    if (!st->d_f.grow(3 * blk + n, who) || !st->d_i.grow(2 * (size_t)n, who)) return 1;
    std::vector<double> s0(start, start + blk);
    if (h->has_l)                                  // a lambda outside [-2 pi, 2 pi] into (-pi, pi]; a gridpoint's is used as given: frozen, it comes back bitwise
        for (int64_t i = 0; i < n; i++)
            if (std::fabs(start[n + i]) > 6.283185307179586) s0[n + i] = wrap_lambda(start[n + i]);
    flush_diag(h);                                 // as for every reader of A
    HIPCHK(hipMemcpyAsync(st->d_f, s0.data(), sizeof(double) * blk, hipMemcpyHostToDevice, h->stream));
    if (error_status()) return 1;

    RefineArgs a;
    a.A = h->d_A; a.w3 = k ? k->d_w3 + (size_t)k->vcls[var - 1] * per : nullptr;
    a.start = st->d_f; a.pos = st->d_f + blk; a.grad = st->d_f + 2 * blk; a.value = st->d_f + 3 * blk;
    a.status = st->d_i; a.iters = st->d_i + n;
    a.C = h->C; a.n = n; a.var = var - 1;
    a.cr = 0; a.cl = h->has_l ? 1 : -1; a.cz = h->has_z ? nco - 1 : -1;
    a.Zb = Zb; a.nz = nz; a.K2 = h->K2; a.kDim = h->kDim;
    a.cell_lo = h->cell0; a.cell_hi = h->cell0 + h->ncells - 1;
    a.want = want; a.mask = free_mask; a.max_iter = max_iter <= 0 ? 20 : max_iter;
    a.xmin = h->xmin; a.tol = tol <= 0.0 ? 1e-9 : tol;
    a.G = newton_geom(g);
    {
        TimedLaunch scope(h, "k_refine", 0.0);      // its bytes follow from the iteration counts: below
        hipLaunchKernelGGL(k_refine, dim3((unsigned)n), dim3(parcel_threads(h)), refine_lds(h), h->stream, a);
    }
    std::vector<double> rf(2 * blk + n);          // held back until the call has succeeded: a failed call writes nothing
    std::vector<int> ric(2 * (size_t)n);
    HIPCHK(hipMemcpyAsync(rf.data(), st->d_f + blk, sizeof(double) * rf.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ric.data(), st->d_i, sizeof(int) * ric.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (error_status()) return 1;
    std::memcpy(pos, rf.data(), sizeof(double) * blk);
    std::memcpy(grad, rf.data() + blk, sizeof(double) * blk);
    std::memcpy(value, rf.data() + 2 * blk, sizeof(double) * n);
    double evals = 0;
    for (int64_t i = 0; i < n; i++) { status[i] = ric[i]; iters[i] = ric[n + i]; evals += 1.0 + ric[n + i]; }
    // 4 node rows x every column of the variable but the padding block, once per evaluation (one more than the steps taken)
    set_kernel_bytes(h, "k_refine", 8.0 * 4.0 * (double)Zb * (h->has_l ? 2 * h->kDim + 1 : 1) * evals);
    return 0;
}

int sx_newton_step(const sx_grid_desc *gd, int32_t want, int32_t free_mask, double tol, const double *pos, const double *d, double *new_pos,
                   int32_t *status) {
    clear_error();
    if (!pos || !d || !new_pos || !status) { set_error("sx_newton_step: null argument"); return 1; }
    if (!desc_ok(gd, "sx_newton_step")) return 1;
    const EvalGeom g = desc_geom(gd);
    if (g.has_z && !(g.zmax > g.zmin)) { set_error("sx_newton_step: invalid vertical grid (need zmax > zmin)"); return 1; }
    if (!newton_args_ok(g, want, free_mask, tol, "sx_newton_step")) return 1;
    const double p3[3] = {pos[0], g.has_l ? pos[1] : 0.0, g.has_z ? pos[1 + g.has_l] : 0.0};
    std::string why;
    if (!std::isfinite(p3[0]) || !std::isfinite(p3[1]) || !std::isfinite(p3[2])) { set_error("sx_newton_step: a coordinate is NaN or Inf"); return 1; }
    if (!eval_radius_ok(g, p3[0], why) || !eval_height_ok(g, p3[2], why)) { set_error("sx_newton_step: " + why); return 1; }
    double dd[REFINE_ND], np[3];
    std::memcpy(dd, d, sizeof(dd));
    *status = newton_step(newton_geom(g), want, free_mask, tol <= 0.0 ? 1e-9 : tol, p3, dd, np);
    new_pos[0] = np[0];
    if (g.has_l) new_pos[1] = np[1];
    if (g.has_z) new_pos[1 + g.has_l] = np[2];
    return 0;
}

}  // extern "C"
