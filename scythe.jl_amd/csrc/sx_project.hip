// sx_project: field programs projected onto the spectral basis - derived fields as the variables of a companion handle
// (include/scythe_hip.h).
//
// k_project is a streaming, pointwise kernel in the manner of k_stats (sx_stats.hip): a lane takes W consecutive points of the flat
// [N] array, loads every plane the program names there once, forms the n_out outputs with red_output and stores each into its var_np1
// plane of the destination.  W = 2 where N is even - every plane of the source and of the destination then starts on a 16-byte
// boundary, and every access is 16 bytes per lane (8 for an fp32-stored plane) - else 1, the 8-byte form for every point (an odd N
// puts every other plane off the boundary, so there is no vector body for a scalar tail to follow).  r is the ring table's entry of
// the point's column (d_r [N / zDim], what the flat forms of k_reduce / k_stats read); the two points of a lane share it unless they
// straddle a column (odd zDim).  No LDS, no atomics, nothing across lanes: a point's outputs depend on that point's planes alone.
// The transform that follows is the destination's own forward chain (launch_fl_forward, launch_sb, launch_solve).
#include "sx_redprog.hpp"
#include <cstring>

namespace sx {

struct ProjDst { uint8_t var[RED_OUT]; };     // 0-based destination variable of output o

template <class ST, int W>
__global__ __launch_bounds__(RED_T) void k_project(Planes<ST> P, int V, int64_t N, int nz, const double *__restrict__ rh, RedProg g, ProjDst d,
                                                   double *__restrict__ out) {
    using VD = typename StatVec<W>::d;
    const int64_t pt = ((int64_t)blockIdx.x * RED_T + threadIdx.x) * W;
    if (pt >= N) return;                                  // W divides N: pt + W - 1 < N
    double val0[RED_PLANES], val1[RED_PLANES];            // one array per point: each stays in registers (val1 is not used when W = 1)
    stat_load_planes<ST, W>(P, V, N, pt, g, val0, val1);
    const int64_t col = pt / nz;
    const RedPow pw0 = red_pow(rh[col]);
    RedPow pw1 = pw0;
    if (W == 2 && pt + 1 - col * nz == nz) pw1 = red_pow(rh[col + 1]);
#pragma unroll
    for (int o = 0; o < RED_OUT; o++) {
        if (o >= g.n_out) continue;
        double q[W];
        red_output<W>(g, o, val0, val1, pw0, pw1, q);
        VD y;
        stat_pack(y, q);
        *reinterpret_cast<VD *>(out + (int64_t)d.var[o] * N + pt) = y;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
using ProjectState = CompanionWrite;

// what sx_project and sx_project_check refuse of the pointers
static bool proj_pointers_ok(const char *who, int n_terms, const double *coef, bool need_coef, const int32_t *terms, int n_out, const int32_t *var_dst) {
    if (need_coef && !red_coef_ok(who, n_terms, coef)) return false;
    if (n_terms > 0 && !terms) { set_error(std::string(who) + ": null terms with n_terms > 0"); return false; }
    if (n_out > 0 && !var_dst) { set_error(std::string(who) + ": null var_dst with n_out > 0"); return false; }
    return true;
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_project_check(const sx_grid_desc *src, const sx_grid_desc *dst, int32_t source, int32_t n_terms, const int32_t *terms, int32_t n_out,
                     const int32_t *var_dst) {
    clear_error();
    const char *who = "sx_project";
    if (!desc_ok(src, "sx_project_check") || !desc_ok(dst, "sx_project_check")) return 1;
    if (!proj_pointers_ok(who, n_terms, nullptr, false, terms, n_out, var_dst)) return 1;
    if (!companion_pair_ok(who, src, dst)) return 1;
    if (n_out != dst->nvars) {
        set_error("sx_project: n_out = " + std::to_string(n_out) + " is not the destination's number of variables (" + std::to_string(dst->nvars) + "): every variable of the destination is written");
        return 1;
    }
    if (sx_reduce_planes(src, source, n_terms, terms, n_out, nullptr, nullptr)) return 1;      // n_out <= 16 from here on
    bool seen[RED_OUT] = {};
    for (int o = 0; o < n_out; o++) {
        if (var_dst[o] < 1 || var_dst[o] > n_out || seen[var_dst[o] - 1]) {
            set_error("sx_project: var_dst is not a permutation of 1 .. " + std::to_string(n_out) + " (var_dst[" + std::to_string(o) + "] = " + std::to_string(var_dst[o]) + ")");
            return 1;
        }
        seen[var_dst[o] - 1] = true;
    }
    bool fed[RED_OUT] = {};
    for (int t = 0; t < n_terms; t++) fed[terms[(size_t)t * RED_TERM_W]] = true;
    for (int o = 0; o < n_out; o++)
        if (!fed[o]) { set_error("sx_project: output " + std::to_string(o) + " has no term"); return 1; }
    return 0;
}

int sx_project_point(int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_out, int32_t n_planes, const int32_t *planes,
                     const double *val, double r, double *out) {
    clear_error();
    const char *who = "sx_project_point";
    if (n_terms < 0 || n_terms > RED_TERMS || n_out < 0 || n_out > RED_OUT || n_planes < 0 || n_planes > RED_PLANES) {
        set_error("sx_project_point: n_terms must be 0 .. 64, n_out 0 .. 16, n_planes 0 .. 16");
        return 1;
    }
    if ((n_terms > 0 && (!coef || !terms)) || (n_planes > 0 && (!planes || !val)) || (n_out > 0 && !out)) { set_error(std::string(who) + ": null pointer with a non-zero count"); return 1; }
    int32_t pl[RED_PLANES][2] = {};
    for (int j = 0; j < n_planes; j++) {
        pl[j][0] = planes[2 * j]; pl[j][1] = planes[2 * j + 1];
        if (pl[j][0] < 1 || pl[j][0] > 256 || pl[j][1] < 0 || pl[j][1] > 6) { set_error(std::string(who) + ": plane " + std::to_string(j) + " is no (1-based variable, slot)"); return 1; }
    }
    for (int t = 0; t < n_terms; t++) {
        const int32_t *q = terms + (size_t)t * RED_TERM_W;
        if (q[0] < 0 || q[0] >= n_out || q[1] < -2 || q[1] > 2 || q[2] < 0 || q[2] > RED_FACTORS) {
            set_error(std::string(who) + ": term " + std::to_string(t) + ": out, r_power or n_factors out of range");
            return 1;
        }
        for (int f = 0; f < q[2]; f++) {
            int j = 0;
            while (j < n_planes && (pl[j][0] != q[3 + f] || pl[j][1] != q[3 + RED_FACTORS + f])) j++;
            if (j == n_planes) { set_error(std::string(who) + ": term " + std::to_string(t) + " names a plane that `planes` does not list"); return 1; }
        }
    }
    RedProg prog;
    red_pack(prog, pl, n_planes, n_terms, coef, terms, n_out);
    double v[RED_PLANES] = {};
    for (int j = 0; j < n_planes; j++) v[j] = val[j];
    const RedPow pw = red_pow(r);
    for (int o = 0; o < n_out; o++) out[o] = red_output(prog, o, v, pw);
    return 0;
}

int sx_project(sx_handle *src, int32_t source, int32_t n_terms, const double *coef, const int32_t *terms, int32_t n_out, sx_handle *dst,
               const int32_t *var_dst) {
    clear_error();
    const char *who = "sx_project";
    if (!src || !dst) { set_error("null handle"); return 1; }
    if (!proj_pointers_ok(who, n_terms, coef, true, terms, n_out, var_dst)) return 1;
    if (dst == src) { set_error("sx_project: the destination is the source (the forward transform reads var_np1, which is the model's state): project into a companion handle"); return 1; }
    if (dst->eq != SX_EQ_NONE) { set_error("sx_project: the destination handle has an equation set (only SX_EQ_NONE handles are overwritten)"); return 1; }
    const sx_grid_desc gs = companion_desc(src), gd = companion_desc(dst);
    if (sx_project_check(&gs, &gd, source, n_terms, terms, n_out, var_dst)) return 1;
    int32_t planes[RED_PLANES][2] = {}, n_planes = 0;
    RedProg prog;
    if (!red_program(who, &gs, source, n_terms, coef, terms, n_out, planes, &n_planes, prog)) return 1;
    ProjectState *st = companion_write_state(src, DIAG_PROJECT);
    if (!st) return 1;

    ProjDst pd = {};
    for (int o = 0; o < n_out; o++) pd.var[o] = (uint8_t)(var_dst[o] - 1);

    if (source == SX_REDUCE_PHYSICAL) flush_diag(src);
    HIPCHK(hipStreamSynchronize(dst->stream));      // the destination's own work on var_np1, B and A is complete before another stream writes them
    if (error_status()) return 1;
    {
        TimedLaunch scope(src, "k_project", red_bytes(src, source, planes, n_planes) + 8.0 * n_out * (double)src->N);
        scan_dispatch(src, source, [&](auto st_t, auto, auto P) {      // W = 2 where N is even (above); no RINGS form
            auto launch = [&](auto width) {
                constexpr int W = decltype(width)::value;
                hipLaunchKernelGGL((k_project<decltype(st_t), W>), dim3(scan_flat_blocks(src, W)), dim3(RED_T), 0, src->stream, P, src->V, src->N, src->nz,
                                   src->d_r, prog, pd, dst->d_np1);
            };
            if (src->N % 2 == 0) launch(std::integral_constant<int, 2>());
            else launch(std::integral_constant<int, 1>());
        });
    }
    return companion_transform(src, dst, st);
}

}  // extern "C"
