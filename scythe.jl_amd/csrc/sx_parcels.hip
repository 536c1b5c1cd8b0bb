// sx_parcels_*: Lagrangian parcels advected with the model on the device (include/scythe_hip.h).
//
// The parcel arrays live in HBM; one launch of k_parcels is one step of every active parcel: the kernel forms the parcel's weights
// from its position with the functions of sx_point.hpp (4 spline values, the Chebyshev row t(x) CA of each velocity variable, cos /
// sin k lambda), sums the two or three velocity variables from A in ONE pass over the 4 node rows (the weights and the sines are
// shared), and lane 0 moves the parcel with the model's Adams-Bashforth scheme (ab_value, sx_internal.hpp).  Nothing is made on the
// host per step and the launch is the only thing sx_parcels_advance enqueues.
//
// One workgroup per parcel, PARCEL_T_SMALL lanes (a wave) where a variable has at most PARCEL_WAVE_COLS columns and PARCEL_T
// lanes above: the choice, the column a lane sums (col = lane, lane + T, ...) and the order of the reduction (butterfly within a
// wave, waves in order) depend on the grid alone, so a parcel's path is bitwise independent of the other parcels of the set.
#include "sx_point.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

// PARCEL_T, PARCEL_T_SMALL, PARCEL_WAVE_COLS and parcel_threads: sx_point.hpp (k_refine of sx_extrema.hip takes the same lanes)
constexpr size_t PARCEL_LDS_MAX = 64 * 1024;
static const double PARCEL_MAGIC = 7.7012e7;
constexpr int PARCEL_HDR = 6;             // blob header: magic, n, n_coord, var_r, var_l, var_z

struct ParcelArgs {
    const double *A;       // [b_rDim][C]
    const double *w3;      // [ncls][3][nz][Zb] EvalClasses::d_w3; row 0 of a class, CA, is read (null without a vertical)
    double *pos, *vel, *h1, *h2;   // [n_coord][n]: position, last evaluated velocity, history levels n - 1 and n - 2
    int *cnt, *status;     // [n] steps taken; 0 active, 1 left radially, 2 left vertically
    int64_t C, n;
    int var[3], cls[3];    // coordinate slot (r, lambda, z) -> 0-based velocity variable or -1; its vertical class
    int cr, cl, cz;        // coordinate slot -> column of pos, -1 = the geometry has none
    int ncoord, Zb, nz, K2, kDim, cell_lo, cell_hi, wrap;
    double xmin, DX, lo, hi, wlo, wlen, zmin, zmax, dt;
};

// LDS (doubles): cs [kDim + 1] double2 | t [nz] | wz [3][Zb] | red [waves][3]
__global__ __launch_bounds__(PARCEL_T) void k_parcels(ParcelArgs a) {
    extern __shared__ double lds[];
    double2 *cs = reinterpret_cast<double2 *>(lds);
    double *tz = lds + 2 * (size_t)(a.kDim + 1);
    double *wz = tz + a.nz;
    double *red = wz + 3 * (size_t)a.Zb;
    const int tid = threadIdx.x, T = blockDim.x;
    const int64_t i = blockIdx.x;
    if (a.status[i] != 0) return;          // a frozen parcel is never evaluated again (uniform: the whole workgroup leaves)

    const double r = a.pos[(int64_t)a.cr * a.n + i];
    const double lam = a.cl >= 0 ? a.pos[(int64_t)a.cl * a.n + i] : 0.0;
    const double z = a.cz >= 0 ? a.pos[(int64_t)a.cz * a.n + i] : 0.0;

    // ---- weights
    const int cell = point_cell(a.xmin, a.DX, a.cell_lo, a.cell_hi, r);
    double phi[1][4];
    point_basis<1>(a.xmin, a.DX, cell, r, phi);
    az_table(cs, a.kDim, lam, tid, T);     // lambda is kept in (-pi, pi]
    if (a.cz >= 0) {
        const double th = cheb_theta(a.zmin, a.zmax, z);
        for (int n = tid; n < a.nz; n += T) tz[n] = cheb_entry(n, a.nz, th);
        __syncthreads();
        for (int q = tid; q < 3 * a.Zb; q += T) {
            const int m = q / a.Zb, zm = q - m * a.Zb;
            wz[q] = a.var[m] >= 0 ? cheb_weight(tz, 1, a.w3 + (size_t)a.cls[m] * 3 * a.nz * a.Zb + zm, a.nz, a.Zb) : 0.0;
        }
    } else {
        for (int q = tid; q < 3 * a.Zb; q += T) wz[q] = 1.0;      // Zb = 1 without a vertical
    }
    __syncthreads();

    // ---- one pass over A for every velocity variable
    double acc[3] = {0.0, 0.0, 0.0};
    const int ncol = a.Zb * a.K2;
    const double *__restrict__ Ac = a.A + (int64_t)cell * a.C;
    for (int col = tid; col < ncol; col += T) {
        const int zm = col / a.K2, blk = col - zm * a.K2;
        if (az_padding(blk)) continue;
        const double F = az_factor(blk, cs, 1);
#pragma unroll
        for (int m = 0; m < 3; m++) {
            if (a.var[m] < 0) continue;
            const double *__restrict__ p = Ac + (int64_t)a.var[m] * ncol + col;
            const double s = fma(phi[0][3], p[3 * a.C], fma(phi[0][2], p[2 * a.C], fma(phi[0][1], p[a.C], phi[0][0] * p[0])));
            acc[m] = fma(s, F * wz[m * a.Zb + zm], acc[m]);
        }
    }
    point_sum<3>(acc, red, tid, T);
    if (tid != 0) return;

    // ---- the parcel moves
    double u[3];
#pragma unroll
    for (int m = 0; m < 3; m++) u[m] = a.var[m] >= 0 ? acc[m] : 0.0;
    a.vel[(int64_t)a.cr * a.n + i] = u[0];
    if (a.cl >= 0) a.vel[(int64_t)a.cl * a.n + i] = u[1];
    if (a.cz >= 0) a.vel[(int64_t)a.cz * a.n + i] = u[2];
    const int t = min(a.cnt[i] + 1, 3);                            // Euler, AB2, then AB3
    double e[3] = {u[0], u[1], u[2]}, x0 = r, y0 = 0.0;
    if (a.cl >= 0) {                                               // Cartesian form: the centre is an ordinary point
        double s, c;
        sincos(lam, &s, &c);
        x0 = r * c; y0 = r * s;
        e[0] = (u[0] * c) - (u[1] * s);
        e[1] = (u[0] * s) + (u[1] * c);
    }
    const int col_of[3] = {a.cr, a.cl, a.cz};
    double nw3[3] = {0.0, 0.0, 0.0};
    const double old[3] = {x0, y0, z};
#pragma unroll
    for (int m = 0; m < 3; m++) {
        if (col_of[m] < 0) continue;
        const int64_t o = (int64_t)col_of[m] * a.n + i;
        nw3[m] = ab_value(t, a.dt, old[m], e[m], t >= 2 ? a.h1[o] : 0.0, t >= 3 ? a.h2[o] : 0.0);
    }
    double rn = nw3[0], ln = 0.0;
    if (a.cl >= 0) {
        rn = hypot(nw3[0], nw3[1]);
        ln = rn == 0.0 ? 0.0 : atan2(nw3[1], nw3[0]);
        if (ln <= -M_PI) ln = M_PI;                                // (-pi, pi]
    } else if (a.wrap) {
        rn = rn - floor((rn - a.wlo) / a.wlen) * a.wlen;           // into [xmin, xmax)
        if (rn >= a.wlo + a.wlen || rn < a.wlo) rn = a.wlo;
    }
    const double zn = nw3[2];
    int st = 0;
    if (!(rn >= a.lo && rn <= a.hi)) st = 1;
    else if (a.cz >= 0 && !(zn >= a.zmin && zn <= a.zmax)) st = 2;
    if (st) { a.status[i] = st; return; }                         // frozen at its last inside position
#pragma unroll
    for (int m = 0; m < 3; m++) {
        if (col_of[m] < 0) continue;
        const int64_t o = (int64_t)col_of[m] * a.n + i;
        a.h2[o] = a.h1[o];
        a.h1[o] = e[m];
    }
    a.pos[(int64_t)a.cr * a.n + i] = rn;
    if (a.cl >= 0) a.pos[(int64_t)a.cl * a.n + i] = ln;
    if (a.cz >= 0) a.pos[(int64_t)a.cz * a.n + i] = zn;
    a.cnt[i] = a.cnt[i] + 1;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct ParcelState : DiagState {
    int64_t n = 0;
    int var[3] = {0, 0, 0};              // 1-based (var_r, var_l, var_z), 0 = no motion
    DevBuf<double> d_f;                  // pos | vel | h1 | h2, [n_coord][n] each
    DevBuf<int> d_i;                     // cnt | status
    int cls[3] = {0, 0, 0};
    void drop_set() { d_f.release(); d_i.release(); n = 0; }      // the caller has synchronised the stream
};

static ParcelState *pstate(const sx_handle *h) { return diag_state<ParcelState>(h, DIAG_PARCELS); }

static size_t parcel_lds(const sx_handle *h) {
    return sizeof(double) * (2 * (size_t)(h->kDim + 1) + (h->has_z ? h->nz : 1) + 3 * (size_t)h->Zb + 3 * (PARCEL_T / 64));
}

// what sx_parcels_set and sx_parcels_set_state refuse of the variable indices
static bool parcel_vars_ok(const sx_handle *h, const int var[3], const char *who) {
    const char *nm[3] = {"var_r", "var_l", "var_z"};
    const int has[3] = {1, h->has_l, h->has_z};
    for (int m = 0; m < 3; m++) {
        if (var[m] < 0 || var[m] > h->V) {
            set_error(std::string(who) + ": " + nm[m] + " = " + std::to_string(var[m]) + " is not a 1-based variable index (at most " + std::to_string(h->V) + ") or 0");
            return false;
        }
        if (var[m] != 0 && !has[m]) { set_error(std::string(who) + ": " + nm[m] + " names a coordinate this geometry does not have"); return false; }
    }
    return true;
}

// the state of this handle; the classes of the set's variables
static ParcelState *parcel_prepare(sx_handle *h, const int var[3], int cls[3]) {
    ParcelState *st = pstate(h);
    if (parcel_lds(h) > PARCEL_LDS_MAX) { set_error("sx_parcels: the weights of one parcel do not fit the LDS (kDim or zDim too large)"); return nullptr; }
    const EvalClasses *k = h->has_z ? eval_classes(h) : nullptr;
    if (h->has_z && !k) return nullptr;
    if (!st) {
        h->diag[DIAG_PARCELS].reset(new ParcelState());
        st = pstate(h);
    }
    for (int m = 0; m < 3; m++) cls[m] = k && var[m] != 0 ? k->vcls[var[m] - 1] : 0;
    return st;
}

// replace the set's arrays by f [4][n_coord][n] and ic [2][n] (host), all or nothing
static bool parcel_install(sx_handle *h, ParcelState *st, int64_t n, const int var[3], const int cls[3], const double *f, const int *ic) {
    DevBuf<double> d_f;
    DevBuf<int> d_i;
    const char *err = "sx_parcels: hipMalloc of the parcel arrays failed";
    if (!d_f.upload(f, (size_t)4 * h->ncoord * n, err) || !d_i.upload(ic, (size_t)2 * n, err)) {
        (void)hipGetLastError();
        return false;
    }
    HIPCHK(hipStreamSynchronize(h->stream));      // a step of the set that goes may still be in flight
    st->d_f.swap(d_f); st->d_i.swap(d_i); st->n = n;      // the set that goes is freed on return
    for (int m = 0; m < 3; m++) { st->var[m] = var[m]; st->cls[m] = cls[m]; }
    set_kernel_bytes(h, "k_parcels", 0.0);      // the new set has not moved yet
    return true;
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_parcels_set(sx_handle *h, int64_t n, const double *positions, int32_t var_r, int32_t var_l, int32_t var_z) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    if (n < 0) { set_error("sx_parcels_set: n is negative"); return 1; }
    if (n == 0) {
        ParcelState *st = pstate(h);
        if (st && st->n) { HIPCHK(hipStreamSynchronize(h->stream)); st->drop_set(); }
        return error_status();
    }
    if (!positions) { set_error("sx_parcels_set: null argument"); return 1; }
    if (n > 0x7fffffff) { set_error("sx_parcels_set: more than 2^31 - 1 parcels"); return 1; }
    const int var[3] = {var_r, var_l, var_z};
    if (!parcel_vars_ok(h, var, "sx_parcels_set")) return 1;
    if (!eval_points_ok(h, positions, n, "sx_parcels_set", "parcel")) return 1;
    const int nco = h->ncoord;
    int cls[3];
    ParcelState *st = parcel_prepare(h, var, cls);
    if (!st) return 1;
    std::vector<double> f((size_t)4 * nco * n, 0.0);
    std::vector<int> ic((size_t)2 * n, 0);
    std::memcpy(f.data(), positions, sizeof(double) * nco * n);
    if (h->has_l)                                  // every lambda into (-pi, pi]
        for (int64_t i = 0; i < n; i++) f[n + i] = wrap_lambda(positions[n + i]);
    if (!parcel_install(h, st, n, var, cls, f.data(), ic.data())) return 1;
    return error_status();
}

int sx_parcels_count(const sx_handle *h, int64_t *n) {
    clear_error();
    if (!h || !n) { set_error("null argument"); return 1; }
    *n = pstate(h) ? pstate(h)->n : 0;
    return 0;
}

int sx_parcels_advance(sx_handle *h, double dt) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    if (!std::isfinite(dt)) { set_error("sx_parcels_advance: dt is NaN or Inf"); return 1; }
    ParcelState *st = pstate(h);
    if (!st || st->n == 0) return 0;
    if (h->diag_dirty && (st->var[0] == h->V || st->var[1] == h->V || st->var[2] == h->V)) flush_diag(h);   // as for every reader of A
    const int nco = h->ncoord;
    const size_t blk = (size_t)nco * st->n;
    ParcelArgs a;
    const EvalClasses *k = h->has_z ? eval_classes(h) : nullptr;      // made by parcel_prepare when the set was installed
    if (h->has_z && !k) return 1;
    a.A = h->d_A; a.w3 = k ? (const double *)k->d_w3 : nullptr;
    a.pos = st->d_f; a.vel = st->d_f + blk; a.h1 = st->d_f + 2 * blk; a.h2 = st->d_f + 3 * blk;
    a.cnt = st->d_i; a.status = st->d_i + st->n;
    a.C = h->C; a.n = st->n;
    int nv = 0;
    for (int m = 0; m < 3; m++) { a.var[m] = st->var[m] - 1; a.cls[m] = st->cls[m]; nv += st->var[m] != 0; }
    a.cr = 0; a.cl = h->has_l ? 1 : -1; a.cz = h->has_z ? nco - 1 : -1;
    a.ncoord = nco; a.Zb = h->has_z ? h->Zb : 1; a.nz = h->has_z ? h->nz : 1; a.K2 = h->K2; a.kDim = h->kDim;
    a.cell_lo = h->cell0; a.cell_hi = h->cell0 + h->ncells - 1;
    const EvalGeom g = eval_geom_of(h);
    a.xmin = h->xmin; a.DX = h->DX; a.lo = g.tile_lo(); a.hi = g.tile_hi(); a.zmin = h->zmin; a.zmax = h->zmax; a.dt = dt;
    a.wlo = h->xmin; a.wlen = h->xmax - h->xmin;
    a.wrap = !h->has_l && st->var[0] != 0 && h->bcl[st->var[0] - 1] == SX_BC_PERIODIC && h->bcr[st->var[0] - 1] == SX_BC_PERIODIC;
    // 4 node rows x every column but the padding block, once per velocity variable and parcel (frozen parcels read nothing: an upper bound)
    {
        TimedLaunch scope(h, "k_parcels", 8.0 * 4.0 * (double)a.Zb * (h->has_l ? 2 * h->kDim + 1 : 1) * nv * (double)st->n);
        hipLaunchKernelGGL(k_parcels, dim3((unsigned)st->n), dim3(parcel_threads(h)), parcel_lds(h), h->stream, a);
    }
    return error_status();
}

int sx_parcels_get(sx_handle *h, double *positions, double *velocity, int32_t *status) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    ParcelState *st = pstate(h);
    if (!st || st->n == 0) return 0;
    const size_t blk = (size_t)h->ncoord * st->n;
    if (positions) HIPCHK(hipMemcpyAsync(positions, st->d_f, sizeof(double) * blk, hipMemcpyDeviceToHost, h->stream));
    if (velocity) HIPCHK(hipMemcpyAsync(velocity, st->d_f + blk, sizeof(double) * blk, hipMemcpyDeviceToHost, h->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, st->d_i + st->n, sizeof(int) * st->n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return error_status();
}

// blob: [header: magic, n, n_coord, var_r, var_l, var_z][pos | vel | h1 | h2, [n_coord][n] each][cnt [n]][status [n]]
int sx_parcels_state_size(const sx_handle *h, int64_t *n_doubles) {
    clear_error();
    if (!h || !n_doubles) { set_error("null argument"); return 1; }
    const ParcelState *st = pstate(h);
    *n_doubles = st && st->n ? PARCEL_HDR + (int64_t)(4 * h->ncoord + 2) * st->n : 0;
    return 0;
}

int sx_parcels_get_state(sx_handle *h, double *out) {
    clear_error();
    if (!h || !out) { set_error("null argument"); return 1; }
    ParcelState *st = pstate(h);
    if (!st || st->n == 0) { set_error("sx_parcels_get_state: the handle has no parcel set"); return 1; }
    const size_t nf = (size_t)4 * h->ncoord * st->n, ni = (size_t)2 * st->n;
    std::vector<int> ic(ni);
    out[0] = PARCEL_MAGIC; out[1] = (double)st->n; out[2] = (double)h->ncoord;
    for (int m = 0; m < 3; m++) out[3 + m] = (double)st->var[m];
    HIPCHK(hipMemcpyAsync(out + PARCEL_HDR, st->d_f, sizeof(double) * nf, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ic.data(), st->d_i, sizeof(int) * ni, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t q = 0; q < ni; q++) out[PARCEL_HDR + nf + q] = (double)ic[q];
    return error_status();
}

int sx_parcels_set_state(sx_handle *h, const double *in, int64_t n_doubles) {
    clear_error();
    if (!h || !in) { set_error("null argument"); return 1; }
    const char *bad = "sx_parcels_set_state: the blob does not belong to a handle with these dimensions";
    if (n_doubles < PARCEL_HDR || in[0] != PARCEL_MAGIC || in[2] != (double)h->ncoord || !(in[1] >= 1.0 && in[1] <= 2147483647.0)) { set_error(bad); return 1; }
    const int64_t n = (int64_t)in[1];
    if ((double)n != in[1] || n_doubles != PARCEL_HDR + (int64_t)(4 * h->ncoord + 2) * n) { set_error(bad); return 1; }
    int var[3];
    for (int m = 0; m < 3; m++) {
        var[m] = (int)in[3 + m];
        if ((double)var[m] != in[3 + m]) { set_error(bad); return 1; }
    }
    if (!parcel_vars_ok(h, var, "sx_parcels_set_state")) return 1;
    const size_t nf = (size_t)4 * h->ncoord * n, ni = (size_t)2 * n;
    std::vector<int> ic(ni);
    for (size_t q = 0; q < ni; q++) {
        const double x = in[PARCEL_HDR + nf + q];
        if (!(x >= 0.0 && x <= 2147483647.0) || (q >= (size_t)n && x > 2.0)) { set_error(bad); return 1; }
        ic[q] = (int)x;
    }
    if (!eval_points_ok(h, in + PARCEL_HDR, n, "sx_parcels_set_state", "parcel")) return 1;      // the kernel indexes A by the position
    int cls[3];
    ParcelState *st = parcel_prepare(h, var, cls);
    if (!st) return 1;
    if (!parcel_install(h, st, n, var, cls, in + PARCEL_HDR, ic.data())) return 1;
    return error_status();
}

}  // extern "C"
