// sx_derive: function programs - nonlinear derived fields (a speed, a potential vorticity, temperature, pressure, theta_e) as the
// variables of a companion handle (include/scythe_hip.h).
//
// k_derive is a streaming, pointwise kernel after k_project (sx_project.hip): a lane takes one point of the flat [N] array, loads every
// plane the mids name there once (stat_load_planes), forms the mids with red_output, interprets the operation list and stores the
// registers the destination asks for into its var_np1 planes.  The register file - up to 16 mids + 32 results per point, indexed by
// run-time operands - is a column of LDS per lane, reg[k][lane]: stride-1 8-byte accesses, no bank conflicts, (n_mid + n_ops) x 2 KB
// per workgroup (dynamic, so a short program keeps the occupancy of k_project), and nothing in scratch.  The operation list and the
// constants are kernel arguments: uniform across the wave, so the dispatch on fn is a scalar branch.  A lane reads and writes its own
// column only: no barrier, no atomics, nothing across lanes.  One point per lane: two would double the LDS column for the sake of
// 16-byte accesses in a kernel that fp64 pow / exp bound wherever the program has them.
// fn_eval is the one statement of an operation, for the kernel and for sx_derive_point on the host.
#include "sx_redprog.hpp"
#include "sx_thermo.hpp"
#include <cmath>

namespace sx {

constexpr int FN_OPS = 32, FN_CONSTS = 16, FN_REGS = RED_OUT + FN_OPS;

struct FnProg {
    double c[FN_CONSTS];
    int16_t op[FN_OPS][4];      // fn, a, b, c
    uint8_t reg_dst[FN_REGS];   // register of destination variable v
    int n_mid, n_ops, n_dst;
};

// register operands each fn takes (R, Z: none; REF: none, its a and b are literal)
__host__ __device__ inline int fn_arity(int fn) {
    switch (fn) {
        case SX_FN_R: case SX_FN_Z: case SX_FN_REF: return 0;
        case SX_FN_NEG: case SX_FN_ABS: case SX_FN_SQRT: case SX_FN_EXP: case SX_FN_LOG: case SX_FN_AHYP: case SX_FN_DRY_DENSITY: case SX_FN_L_V: return 1;
        case SX_FN_SELECT: case SX_FN_TEMPERATURE: case SX_FN_PRESSURE: return 3;
        default: return 2;
    }
}

// operation fn on the operand values a, b, c (those beyond its arity are not read); ia, ib: REF's literal profile and slot; ref:
// the reference state [3][3][nz] with lev the point's level (only REF reads it: ref is null on a source that has none)
__host__ __device__ inline double fn_eval(int fn, double a, double b, double c, int ia, int ib, double r, double z, const double *ref, int nz, int lev) {
    switch (fn) {
        case SX_FN_ADD: return a + b;
        case SX_FN_SUB: return a - b;
        case SX_FN_MUL: return a * b;
        case SX_FN_DIV: return a / b;
        case SX_FN_NEG: return -a;
        case SX_FN_ABS: return fabs(a);
        case SX_FN_MIN: return a != a ? a : b != b ? b : b < a ? b : a;
        case SX_FN_MAX: return a != a ? a : b != b ? b : b > a ? b : a;
        case SX_FN_SQRT: return sqrt(a);
        case SX_FN_SELECT: return a >= 0.0 ? b : c;
        case SX_FN_EXP: return exp(a);
        case SX_FN_LOG: return log(a);
        case SX_FN_POW: return pow(a, b);
        case SX_FN_ATAN2: return atan2(a, b);
        case SX_FN_R: return r;
        case SX_FN_Z: return z;
        case SX_FN_REF: return ref[(ia * 3 + ib) * nz + lev];
        case SX_FN_AHYP: return thermo::ahyp(a);
        case SX_FN_TEMPERATURE: return thermo::temperature(a, b, c);
        case SX_FN_ESAT_BUCK: return thermo::sat_pressure_liquid_buck(a, b);
        case SX_FN_DRY_DENSITY: return thermo::dry_density(a);
        case SX_FN_PRESSURE: return thermo::pressure(a, b, c);
        case SX_FN_VAPOR_PRESSURE: return thermo::vapor_pressure(a, b);
        case SX_FN_L_V: return thermo::L_v(a);
    }
    return 0.0;      // not reached: fn_check has passed the list
}

template <class ST>
__global__ __launch_bounds__(RED_T) void k_derive(Planes<ST> P, int V, int64_t N, int nz, const double *__restrict__ rh, const double *__restrict__ zh,
                                                  const double *__restrict__ ref, RedProg g, FnProg f, double *__restrict__ out) {
    extern __shared__ double reg[];                       // [n_mid + n_ops][RED_T]: this lane's registers at reg[k * RED_T + lane]
    const int lane = threadIdx.x;
    const int64_t pt = (int64_t)blockIdx.x * RED_T + lane;
    if (pt >= N) return;
    double val0[RED_PLANES], val1[RED_PLANES];            // val1 is not used (W = 1)
    stat_load_planes<ST, 1>(P, V, N, pt, g, val0, val1);
    const int64_t col = pt / nz;
    const int lev = (int)(pt - col * nz);
    const double r = rh[col], z = zh[lev];
    const RedPow pw = red_pow(r);
#pragma unroll
    for (int o = 0; o < RED_OUT; o++) {
        if (o >= f.n_mid) continue;
        reg[o * RED_T + lane] = red_output(g, o, val0, pw);
    }
    for (int i = 0; i < f.n_ops; i++) {                   // f is uniform: scalar loads and scalar branches
        const int fn = f.op[i][0], ia = f.op[i][1], ib = f.op[i][2], ic = f.op[i][3], na = fn_arity(fn);
        const double a = na < 1 ? 0.0 : ia >= 0 ? reg[ia * RED_T + lane] : f.c[-1 - ia];
        const double b = na < 2 ? 0.0 : ib >= 0 ? reg[ib * RED_T + lane] : f.c[-1 - ib];
        const double c = na < 3 ? 0.0 : ic >= 0 ? reg[ic * RED_T + lane] : f.c[-1 - ic];
        reg[(f.n_mid + i) * RED_T + lane] = fn_eval(fn, a, b, c, ia, ib, r, z, ref, nz, lev);
    }
    for (int v = 0; v < f.n_dst; v++) out[(int64_t)v * N + pt] = reg[f.reg_dst[v] * RED_T + lane];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// what sx_derive, sx_derive_check and sx_derive_point refuse of the operation list
static bool fn_check(const char *who, bool has_z, bool has_ref, int n_mid, int n_ops, const int32_t *ops, int n_consts) {
    if (n_mid < 0 || n_mid > RED_OUT) { set_error(std::string(who) + ": n_mid = " + std::to_string(n_mid) + " is outside 0 .. 16"); return false; }
    if (n_ops < 0 || n_ops > FN_OPS) { set_error(std::string(who) + ": n_ops = " + std::to_string(n_ops) + " is outside 0 .. 32"); return false; }
    if (n_consts < 0 || n_consts > FN_CONSTS) { set_error(std::string(who) + ": n_consts = " + std::to_string(n_consts) + " is outside 0 .. 16"); return false; }
    if (n_ops > 0 && !ops) { set_error(std::string(who) + ": null ops with n_ops > 0"); return false; }
    for (int i = 0; i < n_ops; i++) {
        const int32_t *q = ops + (size_t)i * 4;
        const std::string at = std::string(who) + ": operation " + std::to_string(i);
        if (q[0] < 0 || q[0] >= SX_FN_COUNT) { set_error(at + ": unknown fn " + std::to_string(q[0])); return false; }
        if (q[0] == SX_FN_Z && !has_z) { set_error(at + ": Z on a grid without a vertical"); return false; }
        if (q[0] == SX_FN_REF) {
            if (!has_ref) { set_error(at + ": REF, and the source has no reference state"); return false; }
            if (q[1] < 0 || q[1] > 2 || q[2] < 0 || q[2] > 2) { set_error(at + ": REF of profile " + std::to_string(q[1]) + ", slot " + std::to_string(q[2]) + " (both 0 .. 2)"); return false; }
        }
        for (int k = 0; k < fn_arity(q[0]); k++) {
            const int x = q[1 + k];
            if (x >= n_mid + i) { set_error(at + ": operand " + std::to_string(x) + " names its own or a later register (its own is " + std::to_string(n_mid + i) + ")"); return false; }
            if (x < -n_consts) { set_error(at + ": operand " + std::to_string(x) + " names constant " + std::to_string(-1 - x) + " of " + std::to_string(n_consts)); return false; }
        }
    }
    return true;
}

static void fn_pack(FnProg &f, int n_mid, int n_ops, const int32_t *ops, int n_consts, const double *consts, int n_dst, const int32_t *reg_dst) {
    std::memset(&f, 0, sizeof(f));
    f.n_mid = n_mid; f.n_ops = n_ops; f.n_dst = n_dst;
    for (int k = 0; k < n_consts; k++) f.c[k] = consts[k];
    for (int i = 0; i < n_ops; i++)
        for (int k = 0; k < 4; k++) f.op[i][k] = (int16_t)ops[(size_t)i * 4 + k];
    for (int v = 0; v < n_dst; v++) f.reg_dst[v] = (uint8_t)reg_dst[v];
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_derive_check(const sx_grid_desc *src, int32_t has_ref_state, const sx_grid_desc *dst, int32_t source, int32_t n_terms, const int32_t *terms,
                    int32_t n_mid, int32_t n_ops, const int32_t *ops, int32_t n_consts, int32_t n_reg_dst, const int32_t *reg_dst) {
    clear_error();
    const char *who = "sx_derive";
    if (!desc_ok(src, "sx_derive_check") || !desc_ok(dst, "sx_derive_check")) return 1;
    if (n_terms > 0 && !terms) { set_error("sx_derive: null terms with n_terms > 0"); return 1; }
    if (n_reg_dst > 0 && !reg_dst) { set_error("sx_derive: null reg_dst with a destination variable to write"); return 1; }
    if (!companion_pair_ok(who, src, dst)) return 1;
    if (sx_reduce_planes(src, source, n_terms, terms, n_mid, nullptr, nullptr)) return 1;      // n_mid <= 16 from here on
    bool fed[RED_OUT] = {};
    for (int t = 0; t < n_terms; t++) fed[terms[(size_t)t * RED_TERM_W]] = true;
    for (int o = 0; o < n_mid; o++)
        if (!fed[o]) { set_error("sx_derive: mid " + std::to_string(o) + " has no term"); return 1; }
    if (!fn_check(who, desc_geom(src).has_z, has_ref_state != 0, n_mid, n_ops, ops, n_consts)) return 1;
    if (n_reg_dst != dst->nvars || n_reg_dst > FN_REGS) {
        set_error("sx_derive: " + std::to_string(n_reg_dst) + " entries of reg_dst for the destination's " + std::to_string(dst->nvars) + " variables (at most 48): every variable of the destination is written");
        return 1;
    }
    for (int v = 0; v < n_reg_dst; v++)
        if (reg_dst[v] < 0 || reg_dst[v] >= n_mid + n_ops) {
            set_error("sx_derive: reg_dst[" + std::to_string(v) + "] = " + std::to_string(reg_dst[v]) + " is outside the registers 0 .. " + std::to_string(n_mid + n_ops - 1));
            return 1;
        }
    return 0;
}

int sx_derive_point(int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_mid, int32_t n_ops, const int32_t *ops, int32_t n_consts,
                    const double *consts, int32_t n_planes, const int32_t *planes, const double *val, double r, double z, const double *ref, double *regs) {
    clear_error();
    const char *who = "sx_derive_point";
    if (!fn_check(who, true, ref != nullptr, n_mid, n_ops, ops, n_consts)) return 1;
    if ((n_consts > 0 && !consts) || (n_mid + n_ops > 0 && !regs)) { set_error("sx_derive_point: null pointer with a non-zero count"); return 1; }
    if (sx_project_point(n_terms, coef, terms, n_mid, n_planes, planes, val, r, regs)) return 1;      // the mids, by k_project's arithmetic
    FnProg f;
    fn_pack(f, n_mid, n_ops, ops, n_consts, consts, 0, nullptr);
    for (int i = 0; i < n_ops; i++) {
        const int fn = f.op[i][0], na = fn_arity(fn);
        double x[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < na; k++) x[k] = f.op[i][1 + k] >= 0 ? regs[f.op[i][1 + k]] : f.c[-1 - f.op[i][1 + k]];
        regs[n_mid + i] = fn_eval(fn, x[0], x[1], x[2], f.op[i][1], f.op[i][2], r, z, ref, 1, 0);
    }
    return 0;
}

int sx_derive(sx_handle *src, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_mid, int32_t n_ops,
              const int32_t *ops, int32_t n_consts, const double *consts, sx_handle *dst, const int32_t *reg_dst) {
    clear_error();
    const char *who = "sx_derive";
    if (!src || !dst) { set_error("null handle"); return 1; }
    if (!red_coef_ok(who, n_terms, coef)) return 1;
    if (n_consts > 0 && !consts) { set_error("sx_derive: null consts with n_consts > 0"); return 1; }
    if (dst == src) { set_error("sx_derive: the destination is the source (the forward transform reads var_np1, which is the model's state): derive into a companion handle"); return 1; }
    if (dst->eq != SX_EQ_NONE) { set_error("sx_derive: the destination handle has an equation set (only SX_EQ_NONE handles are overwritten)"); return 1; }
    const sx_grid_desc gs = companion_desc(src), gd = companion_desc(dst);
    if (sx_derive_check(&gs, src->d_ref != nullptr, &gd, source, n_terms, terms, n_mid, n_ops, ops, n_consts, dst->V, reg_dst)) return 1;
    int32_t planes[RED_PLANES][2] = {}, n_planes = 0;
    RedProg prog;
    if (!red_program(who, &gs, source, n_terms, coef, terms, n_mid, planes, &n_planes, prog)) return 1;
    FnProg f;
    fn_pack(f, n_mid, n_ops, ops, n_consts, consts, dst->V, reg_dst);
    CompanionWrite *st = companion_write_state(src, DIAG_DERIVE);
    if (!st) return 1;

    if (source == SX_REDUCE_PHYSICAL) flush_diag(src);
    HIPCHK(hipStreamSynchronize(dst->stream));      // the destination's own work on var_np1, B and A is complete before another stream writes them
    if (error_status()) return 1;
    const size_t lds = (size_t)std::max(n_mid + n_ops, 1) * RED_T * sizeof(double);      // <= 96 KB of the 160 KB
    {
        TimedLaunch scope(src, "k_derive", red_bytes(src, source, planes, n_planes) + 8.0 * dst->V * (double)src->N);
        scan_dispatch(src, source, [&](auto st_t, auto, auto P) {      // flat, no RINGS form
            auto kernel = k_derive<decltype(st_t)>;
            if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(FN_REGS * RED_T * sizeof(double))));
            hipLaunchKernelGGL(kernel, dim3(scan_flat_blocks(src)), dim3(RED_T), lds, src->stream, P, src->V, src->N, src->nz, src->d_r, src->d_z,
                               src->d_ref, prog, f, dst->d_np1);
        });
    }
    return companion_transform(src, dst, st);
}

}  // extern "C"
