// sx_vortex_harmonics / sx_vortex_check: azimuthal harmonics of the state about a centre that is not the grid's (include/scythe_hip.h,
// DESIGN.md 17).  RL and RLZ grids, one-tile patches.
//
// Definition.  Centre (x0, y0) in the Cartesian frame x = r cos lambda, y = r sin lambda; radii rho_i from the centre; n_az samples per
// circle at phi_j = 2 pi j / n_az:  x_j = x0 + rho cos phi_j,  y_j = y0 + rho sin phi_j,  r_j = hypot(x_j, y_j),  lambda_j =
// atan2(y_j, x_j) in (-pi, pi], 0 at r == 0 (k_parcels' rules).  The state is summed with the SX_EVAL_ALL_K truncation, sx_evaluate's
// vertical series, boundary-condition classes and clamped radial cell, value slot only, and for a field f
//     c_k(rho_i, z_l) = (1 / n_az) sum_j f(x_j, y_j, z_l) e^{-i k phi_j},   k = 0 .. kmax,       f = Re sum eps_k c_k e^{i k phi}.
// SX_VORTEX_SCALAR: f = var_a.  SX_VORTEX_WIND: (var_a, var_b) = the grid's radial and tangential wind (u, v); two outputs, the radial
// and tangential wind about the centre, rad_j + i tan_j = (u_j + i v_j) w_j with w_j = e^{i (lambda_j - phi_j)}; a storm motion
// (cx, cy) is the field cx cos phi + cy sin phi (radial), -cx sin phi + cy cos phi (tangential): it is wave 1 alone and is subtracted
// in closed form, c_1 -= (cx - i cy) / 2 resp. (cy + i cx) / 2.
//
// The Fourier sum over phi commutes with the vertical product, so no sample at a height is ever formed.  With
//     g_v[j][zm] = sum_blk sum_node phi_node(r_j) F_blk(lambda_j) A_v[node][zm][blk]
// k_vortex_rings accumulates in mode space  H[acc][k][zm] = sum_j e^{-i k phi_j} q_j g_v[j][zm]  (a scalar field: one accumulator with
// q = 1; a wind field four: q = Re w, Im w for each of u and v, kept apart because u and v may belong to different vertical classes),
// and k_vortex_finish applies the vertical rows to (kmax + 1) x b_zDim numbers per accumulator.
//
// k_vortex_rings: grid (chunks of VORTEX_CHUNK sample points, live circles), VORTEX_T threads.  A workgroup walks its points in order.
// Per point every thread forms the position, the 4 spline weights and w; the cos / sin k lambda table goes to LDS (both with the
// functions of sx_point.hpp, as in k_parcels); then ONE pass over the 4 node rows of A serves all distinct source variables of the
// call: a wave owns whole (variable, zm) rows, its lanes stride over the contiguous blk axis (block 1, the padding, is skipped), a
// butterfly leaves g_v[zm] in LDS.  Then thread t adds the point's rank-1 update to the entries (acc, k, zm) = t, t + VORTEX_T, ...
// of H, which it alone touches (LDS), with
// e^{-i k phi_j} = conj(tab[(k j) mod n_az]) from the n_az-entry table the host forms in extended precision (the index is exact; no
// device sincos of k phi; cos / sin phi_j of the positions are tab[j]).  The chunk's H goes to scratch.  Every order of summation - the
// lane a column belongs to, the butterfly, the points of a chunk in order, the chunks in order - depends on the grid and on the call's
// (n_az, kmax, fields) alone, and an entry of H is summed by one thread whichever it is: a circle's result is bitwise independent of
// the other circles, and an output's of the other fields.
// k_vortex_finish: grid (live circles, outputs).  Adds the chunks' partials in chunk order, multiplies by the value row of the source
// variable's vertical class at every height (eval_vert_weights, rounded once: what sx_evaluate and sx_harmonics are handed; RL: b_zDim
// = 1 and a row of 1), forms rad = P(u Re w) - P(v Im w), tan = P(u Im w) + P(v Re w), divides by n_az, subtracts the motion, writes.
//
// Dynamic LDS, doubles: k_vortex_rings 2 (kDim + 1) + 2 n_acc (kmax + 1) b_zDim + n_src b_zDim; k_vortex_finish 4 (kmax + 1) b_zDim.
#include "sx_point.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

constexpr int VORTEX_T = 256;
constexpr int VORTEX_CHUNK = 16;                    // sample points per workgroup: a constant, so the chunking follows from n_az alone
constexpr int VORTEX_FIELDS = 8, VORTEX_SRC = 2 * VORTEX_FIELDS, VORTEX_ACC = 4 * VORTEX_FIELDS, VORTEX_OUT = 2 * VORTEX_FIELDS;
constexpr int VORTEX_NAZ_MAX = 4096, VORTEX_KMAX = 32;
constexpr size_t VORTEX_LDS_MAX = 64 * 1024;
constexpr size_t VORTEX_SCRATCH = (size_t)256 << 20;   // bytes of chunk partials per launch aimed at (one circle always fits)

struct VortexCircle {
    double rho;
    int orig, pad;         // index among the radii of the call
};

struct VortexRingArgs {
    const double *A;       // [b_rDim][C]
    const double2 *tab;    // [n_az] cos, sin of 2 pi m / n_az
    const VortexCircle *circ;
    double2 *part;         // [circle][chunk][acc][k][zm]
    int64_t C;
    double x0, y0, xmin, DX;
    int n_az, K, nsrc, nacc, Zb, K2, kDim, cell_lo, cell_hi, nchunks;
    int src[VORTEX_SRC];                                   // 0-based variable of each distinct source
    unsigned char acc_src[VORTEX_ACC], acc_q[VORTEX_ACC];  // accumulator -> source, q (0: 1, 1: Re w, 2: Im w)
};

// LDS: cs [kDim + 1] double2 | H [nacc][K][Zb] double2 | g [nsrc][Zb]
__global__ __launch_bounds__(VORTEX_T) void k_vortex_rings(VortexRingArgs a) {
    extern __shared__ double lds[];
    double2 *cs = reinterpret_cast<double2 *>(lds);
    double2 *H = cs + (a.kDim + 1);
    const int nent = a.nacc * a.K * a.Zb;
    double *g = reinterpret_cast<double *>(H + nent);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, ci = blockIdx.y;
    const double rho = a.circ[ci].rho;
    for (int e = tid; e < nent; e += VORTEX_T) H[e] = make_double2(0.0, 0.0);

    const int j0 = chunk * VORTEX_CHUNK, j1 = min(j0 + VORTEX_CHUNK, a.n_az);
    const int nrows = a.nsrc * a.Zb;
    for (int j = j0; j < j1; j++) {
        // ---- the point and its weights (every thread: uniform)
        const double2 t = a.tab[j];
        const double x = a.x0 + (rho * t.x), y = a.y0 + (rho * t.y);
        const double r = hypot(x, y);
        double lam = r == 0.0 ? 0.0 : atan2(y, x);
        if (lam <= -M_PI) lam = M_PI;                              // (-pi, pi]
        const int cell = point_cell(a.xmin, a.DX, a.cell_lo, a.cell_hi, r);
        double phi[1][4];
        point_basis<1>(a.xmin, a.DX, cell, r, phi);
        az_table(cs, a.kDim, lam, tid, VORTEX_T);
        double sl, cl;
        sincos(lam, &sl, &cl);
        const double wre = (cl * t.x) + (sl * t.y), wim = (sl * t.x) - (cl * t.y);      // w = e^{i lambda} e^{-i phi}
        __syncthreads();                                           // cs is complete; the update of the point before has read g

        // ---- one pass over the 4 node rows for every source variable: a wave owns whole (source, zm) rows
        const double *__restrict__ Ac = a.A + (int64_t)cell * a.C;
        for (int row = wave; row < nrows; row += VORTEX_T / 64) {
            const int s = row / a.Zb, zm = row - s * a.Zb;
            const double *__restrict__ p = Ac + ((int64_t)a.src[s] * a.Zb + zm) * a.K2;
            double acc = 0.0;
            for (int blk = lane; blk < a.K2; blk += 64) {
                if (az_padding(blk)) continue;
                const double F = az_factor(blk, cs, 1);
                const double sum = fma(phi[0][3], p[3 * a.C + blk], fma(phi[0][2], p[2 * a.C + blk], fma(phi[0][1], p[a.C + blk], phi[0][0] * p[blk])));
                acc = fma(sum, F, acc);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if (lane == 0) g[row] = acc;
        }
        __syncthreads();

        // ---- the rank-1 update of the entries this thread owns
        for (int e = tid; e < nent; e += VORTEX_T) {
            const int ak = e / a.Zb, zm = e - ak * a.Zb, ac = ak / a.K, k = ak - ac * a.K;
            const int q = a.acc_q[ac];
            const double v = g[a.acc_src[ac] * a.Zb + zm];
            const double qv = q == 0 ? v : (q == 1 ? wre : wim) * v;
            const double2 f = a.tab[(k * j) % a.n_az];             // e^{-i k phi_j} = (f.x, -f.y)
            double2 hh = H[e];
            hh.x = fma(f.x, qv, hh.x);
            hh.y = fma(-f.y, qv, hh.y);
            H[e] = hh;
        }
    }
    double2 *__restrict__ dst = a.part + ((int64_t)ci * a.nchunks + chunk) * nent;
    for (int e = tid; e < nent; e += VORTEX_T) dst[e] = H[e];
}

struct VortexOutput {
    int acc[2], cls[2];    // the accumulators combined (acc[1] = -1: a scalar field) and the vertical class of each one's source
    int sign, motion;      // out = P(acc[0]) + sign P(acc[1]);  motion 1: radial, 2: tangential, 0: none
};

struct VortexFinishArgs {
    const double2 *part;
    const double *wz;      // [cls][nz][Zb] value rows
    const VortexCircle *circ;
    double *res;           // [out][n_rho][nz][2 K]
    double cx, cy;
    int n_az, K, nacc, Zb, nchunks, nz, n_rho;
    VortexOutput out[VORTEX_OUT];
};

// LDS: Hs [2][K][Zb] double2
__global__ __launch_bounds__(VORTEX_T) void k_vortex_finish(VortexFinishArgs a) {
    extern __shared__ double lds[];
    double2 *Hs = reinterpret_cast<double2 *>(lds);
    const int tid = threadIdx.x, ci = blockIdx.x, o = blockIdx.y;
    const VortexOutput &q = a.out[o];
    const int per = a.K * a.Zb, nent = a.nacc * per;
    for (int e = tid; e < 2 * per; e += VORTEX_T) {
        const int s = e / per, i = e - s * per;
        double2 sum = make_double2(0.0, 0.0);
        if (q.acc[s] >= 0) {
            const double2 *__restrict__ p = a.part + (int64_t)ci * a.nchunks * nent + (int64_t)q.acc[s] * per + i;
            for (int c = 0; c < a.nchunks; c++) {                  // in chunk order
                const double2 v = p[(int64_t)c * nent];
                sum.x += v.x; sum.y += v.y;
            }
        }
        Hs[e] = sum;
    }
    __syncthreads();
    const int orig = a.circ[ci].orig;
    const double n = (double)a.n_az;
    for (int e = tid; e < a.K * a.nz; e += VORTEX_T) {
        const int k = e / a.nz, l = e - k * a.nz;
        double2 P[2] = {make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (q.acc[s] < 0) continue;
            const double *__restrict__ w = a.wz + ((int64_t)q.cls[s] * a.nz + l) * a.Zb;
            const double2 *__restrict__ hs = Hs + s * per + k * a.Zb;
            for (int zm = 0; zm < a.Zb; zm++) {
                P[s].x = fma(w[zm], hs[zm].x, P[s].x);
                P[s].y = fma(w[zm], hs[zm].y, P[s].y);
            }
        }
        double re = q.acc[1] < 0 ? P[0].x : (q.sign < 0 ? P[0].x - P[1].x : P[0].x + P[1].x);
        double im = q.acc[1] < 0 ? P[0].y : (q.sign < 0 ? P[0].y - P[1].y : P[0].y + P[1].y);
        re /= n; im /= n;
        if (k == 1 && q.motion == 1) { re -= 0.5 * a.cx; im -= -0.5 * a.cy; }       // eps_1 c_1 = cx - i cy
        if (k == 1 && q.motion == 2) { re -= 0.5 * a.cy; im -= 0.5 * a.cx; }        // eps_1 c_1 = cy + i cx
        double *__restrict__ dst = a.res + ((((int64_t)o * a.n_rho + orig) * a.nz + l) * a.K + k) * 2;
        dst[0] = re; dst[1] = im;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct VortexState : DiagState {
    DevBuf<double2> d_tab, d_part;
    DevBuf<VortexCircle> d_circ;
    DevBuf<double> d_wz, d_res;
    int tab_n = 0;
};

struct VortexPlan {        // what the fields of a call come to
    int nsrc = 0, nacc = 0, nout = 0;
    int src[VORTEX_SRC];
    unsigned char acc_src[VORTEX_ACC], acc_q[VORTEX_ACC];
    int out_acc[VORTEX_OUT][2], out_src[VORTEX_OUT][2], out_sign[VORTEX_OUT], out_motion[VORTEX_OUT];
};

static size_t vortex_rings_lds(int kDim, int Zb, int K, int nacc, int nsrc) {
    return sizeof(double) * (2 * (size_t)(kDim + 1) + 2 * (size_t)nacc * K * Zb + (size_t)nsrc * Zb);
}
static size_t vortex_finish_lds(int Zb, int K) { return sizeof(double) * 4 * (size_t)K * Zb; }

// 1: the circle of radius rho about a centre at distance d from the grid's leaves the tile's radial extent [lo, hi].  Closed form; the
// kernel's hypot, the sum d + rho and a rho the caller formed as hi - d are each off by an ulp, so a few ulp of what enters are absorbed:
// a circle tangent to the edge is inside, and its samples an ulp beyond the edge are evaluated in the clamped last cell
static int vortex_circle_status(double d, double rho, double lo, double hi) {
    const double tol = 8.0 * 2.220446049250313e-16 * (d + rho + hi);
    if (d + rho > hi + tol) return 1;
    if (lo > 0.0 && std::fabs(d - rho) < lo - tol) return 1;
    return 0;
}

// Everything both entry points refuse that a descriptor decides, and the circle rule.  g: desc_geom of the grid; V: its variables.
static bool vortex_validate(const char *who, int geometry, const EvalGeom &g, int V, const double *centre, const double *radii, int n_rho,
                            int n_az, int kmax, int n_fields, const int32_t *fields, VortexPlan &plan, int32_t *status) {
    const std::string w = std::string(who) + ": ";
    if (geometry != SX_GEOM_RL && geometry != SX_GEOM_RLZ) { set_error(w + "RL and RLZ grids only (the centre is a point of the horizontal plane)"); return false; }
    if (g.cell0 != 0 || g.ncells != g.nc) { set_error(w + "one-tile patches only"); return false; }
    if (n_rho < 0) { set_error(w + "n_rho is negative"); return false; }
    if (!centre || (n_rho > 0 && (!radii || !status))) { set_error(w + "null argument"); return false; }
    if (!std::isfinite(centre[0]) || !std::isfinite(centre[1])) { set_error(w + "the centre is NaN or Inf"); return false; }
    for (int i = 0; i < n_rho; i++) {
        if (!std::isfinite(radii[i])) { set_error(w + "radius " + std::to_string(i) + " is NaN or Inf"); return false; }
        if (radii[i] < 0.0) { set_error(w + "radius " + std::to_string(i) + " is negative"); return false; }
    }
    if (n_az < 4 || n_az % 4 != 0 || n_az > VORTEX_NAZ_MAX) { set_error(w + "n_az must be a multiple of 4 in 4 .. 4096"); return false; }
    if (kmax < 0 || 2 * kmax >= n_az || kmax > VORTEX_KMAX) { set_error(w + "kmax must be 0 .. 32 with 2 kmax < n_az"); return false; }
    if (n_fields < 1 || n_fields > VORTEX_FIELDS) { set_error(w + "n_fields must be 1 .. 8"); return false; }
    if (!fields) { set_error(w + "null fields"); return false; }
    plan = VortexPlan();
    auto source = [&](int var) {
        for (int s = 0; s < plan.nsrc; s++)
            if (plan.src[s] == var) return s;
        plan.src[plan.nsrc] = var;
        return plan.nsrc++;
    };
    auto accum = [&](int s, int q) {
        plan.acc_src[plan.nacc] = (unsigned char)s; plan.acc_q[plan.nacc] = (unsigned char)q;
        return plan.nacc++;
    };
    for (int f = 0; f < n_fields; f++) {
        const int32_t kind = fields[3 * f], va = fields[3 * f + 1], vb = fields[3 * f + 2];
        const std::string at = w + "field " + std::to_string(f) + ": ";
        if (kind != SX_VORTEX_SCALAR && kind != SX_VORTEX_WIND) { set_error(at + "kind must be SX_VORTEX_SCALAR or SX_VORTEX_WIND"); return false; }
        if (va < 1 || va > V) { set_error(at + "var_a = " + std::to_string(va) + " is 1-based and at most nvars"); return false; }
        if (kind == SX_VORTEX_WIND && (vb < 1 || vb > V)) { set_error(at + "var_b = " + std::to_string(vb) + " is 1-based and at most nvars"); return false; }
        if (kind == SX_VORTEX_SCALAR) {
            const int s = source(va - 1), o = plan.nout++;
            plan.out_acc[o][0] = accum(s, 0); plan.out_acc[o][1] = -1;
            plan.out_src[o][0] = s; plan.out_src[o][1] = s;
            plan.out_sign[o] = 1; plan.out_motion[o] = 0;
        } else {
            const int su = source(va - 1), sv = source(vb - 1);
            const int ure = accum(su, 1), uim = accum(su, 2), vre = accum(sv, 1), vim = accum(sv, 2);
            const int orad = plan.nout++, otan = plan.nout++;
            plan.out_acc[orad][0] = ure; plan.out_acc[orad][1] = vim; plan.out_sign[orad] = -1; plan.out_motion[orad] = 1;
            plan.out_acc[otan][0] = uim; plan.out_acc[otan][1] = vre; plan.out_sign[otan] = 1; plan.out_motion[otan] = 2;
            for (int o : {orad, otan}) { plan.out_src[o][0] = su; plan.out_src[o][1] = sv; }
        }
    }
    const int Zb = g.has_z ? g.Zb : 1, K = kmax + 1;
    const size_t need_r = vortex_rings_lds(g.kDim, Zb, K, plan.nacc, plan.nsrc), need_f = vortex_finish_lds(Zb, K);
    if (need_r > VORTEX_LDS_MAX || need_f > VORTEX_LDS_MAX) {
        set_error(w + "the accumulators of one circle do not fit the LDS: 2 (kDim + 1) + 2 n_acc (kmax + 1) b_zDim + n_src b_zDim = " +
                  std::to_string(need_r / 8) + " and 4 (kmax + 1) b_zDim = " + std::to_string(need_f / 8) + " doubles, at most 8192 each (kDim " +
                  std::to_string(g.kDim) + ", b_zDim " + std::to_string(Zb) + ", kmax " + std::to_string(kmax) + ", n_acc " + std::to_string(plan.nacc) +
                  ": 1 per scalar and 4 per wind field, n_src " + std::to_string(plan.nsrc) + ")");
        return false;
    }
    const double d = std::hypot(centre[0], centre[1]);
    for (int i = 0; i < n_rho; i++) status[i] = vortex_circle_status(d, radii[i], g.tile_lo(), g.tile_hi());
    return true;
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_vortex_check(const sx_grid_desc *gd, const double centre[2], const double *radii, int32_t n_rho, int32_t n_az, int32_t kmax,
                    int32_t n_fields, const int32_t *fields, int32_t *n_out, int32_t *status) {
    clear_error();
    if (!desc_ok(gd, "sx_vortex_check")) return 1;
    const EvalGeom g = desc_geom(gd);
    if (g.has_z && (g.nz < 4 || g.Zb > g.nz || !(g.zmax > g.zmin))) { set_error("invalid vertical grid (need zDim >= 4, b_zDim <= zDim, zmax > zmin)"); return 1; }
    VortexPlan plan;
    std::vector<int32_t> st(std::max<int32_t>(n_rho, 1));
    if (!vortex_validate("sx_vortex_check", gd->geometry, g, gd->nvars, centre, radii, n_rho, n_az, kmax, n_fields, fields, plan, n_rho > 0 && status ? st.data() : nullptr)) return 1;
    if (n_out) *n_out = plan.nout;
    if (n_rho > 0) std::memcpy(status, st.data(), sizeof(int32_t) * n_rho);
    return 0;
}

int sx_vortex_harmonics(sx_handle *h, const double centre[2], const double *motion, const double *radii, int32_t n_rho, const double *heights,
                        int32_t n_z, int32_t n_az, int32_t kmax, int32_t n_fields, const int32_t *fields, double *out, int32_t *status) {
    clear_error();
    if (!h) { set_error("null handle"); return 1; }
    const char *who = "sx_vortex_harmonics";
    const EvalGeom g = eval_geom_of(h);
    VortexPlan plan;
    std::vector<int32_t> stat(std::max<int32_t>(n_rho, 1));
    if (!vortex_validate(who, h->geom, g, h->V, centre, radii, n_rho, n_az, kmax, n_fields, fields, plan, n_rho > 0 && status ? stat.data() : nullptr)) return 1;
    if (motion && (!std::isfinite(motion[0]) || !std::isfinite(motion[1]))) { set_error("sx_vortex_harmonics: the motion is NaN or Inf"); return 1; }
    if (n_z < 0) { set_error("sx_vortex_harmonics: n_z is negative"); return 1; }
    if (!h->has_z && (heights || n_z != 0)) { set_error("sx_vortex_harmonics: the grid has no vertical: heights must be NULL and n_z 0"); return 1; }
    if (h->has_z && n_z > 0 && !heights) { set_error("sx_vortex_harmonics: null argument"); return 1; }
    std::string why;
    for (int i = 0; i < n_z; i++)
        if (!eval_height_ok(g, heights[i], why)) { set_error("sx_vortex_harmonics: height " + std::to_string(i) + ": " + why); return 1; }
    const int nz = h->has_z ? n_z : 1;
    if (n_rho == 0 || nz == 0) return 0;
    if (!out) { set_error("sx_vortex_harmonics: null argument"); return 1; }
    const EvalClasses *cls = eval_classes(h);
    if (!cls) return 1;
    if (!h->diag[DIAG_VORTEX]) h->diag[DIAG_VORTEX].reset(new VortexState());
    VortexState *st = diag_state<VortexState>(h, DIAG_VORTEX);
    flush_diag(h);                                 // as for every reader of A

    const int Zb = h->has_z ? h->Zb : 1, K = kmax + 1, ncls = std::max<int>(1, (int)cls->vert.size());
    const int nchunks = (n_az + VORTEX_CHUNK - 1) / VORTEX_CHUNK, nent = plan.nacc * K * Zb;
    // e^{i 2 pi m / n_az}, in extended precision and rounded once; kept while n_az stays
    if (st->tab_n != n_az) {
        const long double two_pi = 8.0L * atanl(1.0L);
        std::vector<double2> tab(n_az);
        for (int m = 0; m < n_az; m++) {
            // the octant symmetries exactly: multiples of a quarter turn are 0 and +-1
            const long double ang = two_pi * (long double)m / (long double)n_az;
            tab[m] = make_double2((double)cosl(ang), (double)sinl(ang));
            if ((4 * m) % n_az == 0) {
                const int qd = 4 * m / n_az;
                tab[m] = make_double2(qd == 0 ? 1.0 : qd == 2 ? -1.0 : 0.0, qd == 1 ? 1.0 : qd == 3 ? -1.0 : 0.0);
            }
        }
        HIPCHK(hipStreamSynchronize(h->stream));   // a launch that reads the table that goes may still be in flight
        if (!st->d_tab.upload(tab, "sx_vortex_harmonics: hipMalloc of the phase table failed")) { st->tab_n = 0; return 1; }
        st->tab_n = n_az;
    }
    // the value rows of every class at every height
    std::vector<double> wz((size_t)ncls * nz * Zb, 1.0), w3((size_t)3 * Zb);
    if (h->has_z)
        for (int c = 0; c < ncls; c++)
            for (int l = 0; l < nz; l++) {
                eval_vert_weights(cls->vert[c], h->zmin, h->zmax, h->nz, Zb, heights[l], w3.data());
                std::memcpy(&wz[((size_t)c * nz + l) * Zb], w3.data(), sizeof(double) * Zb);
            }
    std::vector<VortexCircle> live;
    for (int i = 0; i < n_rho; i++)
        if (stat[i] == 0) live.push_back(VortexCircle{radii[i], i, 0});
    const size_t n_res = (size_t)plan.nout * n_rho * nz * 2 * K;
    std::vector<double> res(n_res, std::nan(""));      // held back until the call has succeeded: a failed call writes nothing to out
    // every live circle of the call: n_az points x distinct source variables x 4 rows x b_zDim x (2 kDim + 1) of A
    const double rings_bytes = 8.0 * 4.0 * (double)Zb * (2 * h->kDim + 1) * plan.nsrc * (double)n_az * (double)live.size();
    if (live.empty()) set_kernel_bytes(h, "k_vortex_rings", 0.0);
    if (!live.empty()) {
        const size_t per_circle = (size_t)nchunks * nent;
        const int batch = (int)std::max<size_t>(1, std::min<size_t>({live.size(), VORTEX_SCRATCH / (per_circle * sizeof(double2)), (size_t)32768}));
        if (!st->d_circ.grow(live.size(), who) || !st->d_part.grow(per_circle * batch, who) || !st->d_wz.grow(wz.size(), who) || !st->d_res.grow(n_res, who)) return 1;
        HIPCHK(hipMemcpyAsync(st->d_circ, live.data(), sizeof(VortexCircle) * live.size(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(st->d_wz, wz.data(), sizeof(double) * wz.size(), hipMemcpyHostToDevice, h->stream));
        if (error_status()) return 1;

        VortexRingArgs ra;
        std::memset(&ra, 0, sizeof(ra));
        ra.A = h->d_A; ra.tab = st->d_tab; ra.part = st->d_part; ra.C = h->C;
        ra.x0 = centre[0]; ra.y0 = centre[1]; ra.xmin = h->xmin; ra.DX = h->DX;
        ra.n_az = n_az; ra.K = K; ra.nsrc = plan.nsrc; ra.nacc = plan.nacc; ra.Zb = Zb; ra.K2 = h->K2; ra.kDim = h->kDim;
        ra.cell_lo = h->cell0; ra.cell_hi = h->cell0 + h->ncells - 1; ra.nchunks = nchunks;
        std::memcpy(ra.src, plan.src, sizeof(ra.src));
        std::memcpy(ra.acc_src, plan.acc_src, sizeof(ra.acc_src));
        std::memcpy(ra.acc_q, plan.acc_q, sizeof(ra.acc_q));
        VortexFinishArgs fa;
        std::memset(&fa, 0, sizeof(fa));
        fa.part = st->d_part; fa.wz = st->d_wz; fa.res = st->d_res;
        fa.cx = motion ? motion[0] : 0.0; fa.cy = motion ? motion[1] : 0.0;
        fa.n_az = n_az; fa.K = K; fa.nacc = plan.nacc; fa.Zb = Zb; fa.nchunks = nchunks; fa.nz = nz; fa.n_rho = n_rho;
        for (int o = 0; o < plan.nout; o++) {
            VortexOutput &q = fa.out[o];
            for (int s = 0; s < 2; s++) {
                q.acc[s] = plan.out_acc[o][s];
                q.cls[s] = h->has_z ? cls->vcls[plan.src[plan.out_src[o][s]]] : 0;
            }
            q.sign = plan.out_sign[o];
            q.motion = motion ? plan.out_motion[o] : 0;
        }
        const size_t lds_r = vortex_rings_lds(h->kDim, Zb, K, plan.nacc, plan.nsrc), lds_f = vortex_finish_lds(Zb, K);
        for (size_t c0 = 0; c0 < live.size(); c0 += batch) {
            const unsigned nb = (unsigned)std::min<size_t>(batch, live.size() - c0);
            ra.circ = fa.circ = st->d_circ + c0;
            {
                TimedLaunch scope(h, "k_vortex_rings", rings_bytes);
                hipLaunchKernelGGL(k_vortex_rings, dim3((unsigned)nchunks, nb), dim3(VORTEX_T), lds_r, h->stream, ra);
            }
            {
                TimedLaunch scope(h, "k_vortex_finish", 0.0);
                hipLaunchKernelGGL(k_vortex_finish, dim3(nb, (unsigned)plan.nout), dim3(VORTEX_T), lds_f, h->stream, fa);
            }
        }
        std::vector<double> dev(n_res);
        HIPCHK(hipMemcpyAsync(dev.data(), st->d_res, sizeof(double) * n_res, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (error_status()) return 1;
        const size_t per = (size_t)nz * 2 * K;
        for (int o = 0; o < plan.nout; o++)
            for (const VortexCircle &c : live)
                std::memcpy(&res[((size_t)o * n_rho + c.orig) * per], &dev[((size_t)o * n_rho + c.orig) * per], sizeof(double) * per);
    }
    std::memcpy(out, res.data(), sizeof(double) * n_res);
    std::memcpy(status, stat.data(), sizeof(int32_t) * n_rho);
    return 0;
}

}  // extern "C"
