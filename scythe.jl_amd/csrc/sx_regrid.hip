// sx_regrid / sx_regrid_check / sx_regrid_columns: the state of one grid laid down on another - resized, re-levelled, re-centred
// (include/scythe_hip.h, "onto another grid").
//
// Every gridpoint of the destination receives the continuous function of the source there (sx_evaluate with SX_EVAL_ALL_K), as the
// destination's var_np1; the destination's own forward chain then makes its B and A.  In a column (r, lambda) the radial and azimuthal
// sums do not depend on z, so the work splits as sx_isosurface's does:
//   stage 1  the profiles C[zm] of kind (0, 0) of every source variable named, in the destination's columns mapped into the source
//            (regrid_map): k_column_profiles / k_column_profiles_rz of sx_isosurface.hip through launch_column_profiles, the columns
//            sorted by source cell and batched by colprof_batches (sx_colprof.hpp).  Only the columns inside the source are sent.
//   stage 2  k_regrid_levels: var_np1_dst[z, column, v] = sum_zm E_v[z][zm] C_v[zm][column], E_v the rows of sx_evaluate's vertical
//            operator (eval_vert_weights, row 0) of the source variable's class at the destination's levels: extended precision,
//            rounded once, cached per destination level set.  On grids without a vertical b_zDim = 1, E = (1) and the stage is a
//            copy into var_np1 order (fma(1, C, +0) = C).
// k_regrid_levels (RLZ): one wave per (16 destination columns in gridpoint order, destination variable) on the f64 matrix cores.  The
// 16 profiles are staged in LDS once (coalesced along zm, stride 17 so that the operand reads spread over the banks), then for every
// tile of 16 levels the product runs over K = zm in ascending steps of 4 - one chain, whatever the launch - with the A operand the
// profiles (row = column) and the B operand E^T (column = level), so that a register of the result is 16 consecutive levels of one
// column: 128 contiguous bytes of var_np1, z fastest.  The columns are un-sorted on the way in (pidx: destination column -> profile,
// -1 = outside the source), and an outside column is written with the variable's fill value.  Columns of the product do not mix and a
// short tile is padded with zeros: a column's values do not depend on the other columns, nor one variable's on the others.
// k_regrid_levels_lane (R, RL, RZ): one lane per output, the same sum as an fma chain over zm from +0.0.  The path follows from the
// geometry alone - never from the number of columns - so that a column's bits do not depend on how many columns the call has.
// No atomics, nothing summed across columns: two calls agree bitwise.
#include "sx_colprof.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

constexpr int64_t REGRID_COLS_MAX = (int64_t)1 << 20;
constexpr int RG_CS = 17;                 // row stride of the staged profiles in doubles

typedef double rg_d4 __attribute__((ext_vector_type(4)));

// ---- the column map: stated once, for host and device -------------------------------------------------------------------------------
// The destination's column (r, lambda) about its axis at (x0, y0) of the source's Cartesian frame, in the source's polar coordinates.
// Plain fp64, every product and sum rounded on its own; with the axes together the map is the identity, bit for bit.
__host__ __device__ inline void regrid_map(double x0, double y0, double r, double lam, double &r_s, double &lam_s) {
    if (x0 == 0.0 && y0 == 0.0) { r_s = r; lam_s = lam; return; }
    const double x = x0 + r * cos(lam), y = y0 + r * sin(lam);
    r_s = hypot(x, y);
    lam_s = atan2(y, x);
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------------------
struct RegridVar {
    int var, prof, cls, pad;              // 0-based destination variable; its profile; vertical class of the source variable
    double fill;
};
struct RegridArgs {
    const double *P;                      // [n_in][nprof][Zb] profiles of the inside columns
    const double *ET;                     // [ncls][Kp][Mp] E^T, zero-padded
    const int *pidx;                      // [n_cols] destination column -> its row of P, -1 = outside the source
    const RegridVar *rv;                  // the destination variables of the launch
    double *out;                          // the destination's var_np1 [V][N]
    int64_t N;
    int n_cols, nprof, Zb, Kp, Mp, nz, nrv;
};

// grid (ceil(n_cols / 16), variables of the launch)
__global__ __launch_bounds__(64) void k_regrid_levels(const RegridArgs a) {
    extern __shared__ double sC[];        // [Kp][RG_CS]: profile entry zm of the tile's column q at zm * RG_CS + q
    const int lane = threadIdx.x, j = lane & 15, kk = lane >> 4;
    const int c0 = blockIdx.x * 16;
    const RegridVar rv = a.rv[blockIdx.y];
    for (int e = lane; e < 16 * a.Kp; e += 64) {
        const int zm = e % a.Kp, q = e / a.Kp, c = c0 + q;
        const int pi = c < a.n_cols ? a.pidx[c] : -1;
        sC[zm * RG_CS + q] = pi >= 0 && zm < a.Zb ? a.P[((int64_t)pi * a.nprof + rv.prof) * a.Zb + zm] : 0.0;
    }
    const int pj = c0 + j < a.n_cols ? a.pidx[c0 + j] : -1;
    const unsigned inside = (unsigned)(__ballot(pj >= 0) & 0xffffull);       // bit q: column q of the tile lies inside the source
    __syncthreads();
    const double *__restrict__ ET = a.ET + (int64_t)rv.cls * a.Kp * a.Mp;
    double *__restrict__ out = a.out + (int64_t)rv.var * a.N;
    const int nks = a.Kp >> 2;
    for (int t = 0; t < (a.Mp >> 4); t++) {
        rg_d4 acc = rg_d4{0.0, 0.0, 0.0, 0.0};
        for (int ks = 0; ks < nks; ks++) {
            const int zm = 4 * ks + kk;
            // A operand: row (column of the tile) lane & 15, K lane >> 4;  B operand: K lane >> 4, column (level) lane & 15
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sC[zm * RG_CS + j], ET[(int64_t)zm * a.Mp + t * 16 + j], acc, 0, 0, 0);
        }
        // C / D layout of v_mfma_f64_16x16x4: column (level) lane & 15, row (column of the tile) (lane >> 4) + 4 reg
        const int lev = t * 16 + j;
        if (lev >= a.nz) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int q = kk + 4 * r, c = c0 + q;
            if (c < a.n_cols) out[(int64_t)c * a.nz + lev] = (inside >> q & 1u) ? acc[r] : rv.fill;
        }
    }
}

// grids without an azimuth or without a vertical: one lane per output (level, column, variable of the launch)
__global__ __launch_bounds__(256) void k_regrid_levels_lane(const RegridArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, per = (int64_t)a.n_cols * a.nz;
    if (e >= per * a.nrv) return;
    const RegridVar rv = a.rv[e / per];
    const int64_t pt = e % per;
    const int lev = (int)(pt % a.nz), pi = a.pidx[pt / a.nz];
    double acc = rv.fill;
    if (pi >= 0) {
        const double *__restrict__ Cp = a.P + ((int64_t)pi * a.nprof + rv.prof) * a.Zb;
        const double *__restrict__ ET = a.ET + (int64_t)rv.cls * a.Kp * a.Mp + lev;
        acc = 0.0;
        for (int zm = 0; zm < a.Zb; zm++) acc = fma(ET[(int64_t)zm * a.Mp], Cp[zm], acc);
    }
    a.out[(int64_t)rv.var * a.N + pt] = acc;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct RegridTable {                      // E^T of every class of the source at one destination level set
    double zmin = 0, zmax = 0;
    int nz = 0, Kp = 0, Mp = 0;
    DevBuf<double> d_ET;
};
struct RegridState : DiagState {          // kept with the SOURCE handle
    hipEvent_t done = nullptr;            // recorded on the source's stream behind stage 2; the destination's stream waits on it
    std::vector<std::unique_ptr<RegridTable>> tables;
    DevBuf<double> d_cols, d_P;
    DevBuf<int> d_idx, d_pidx;            // order | batches;  destination column -> profile row
    DevBuf<RegridVar> d_rv;
    ~RegridState() override { if (done) hipEventDestroy(done); }
};

// the handle's grid with what the checks read beyond desc_of
static sx_grid_desc regrid_desc(const sx_handle *h) {
    sx_grid_desc gd = desc_of(h);
    gd.ring_uniform_L = h->uniform_L; gd.zmin = h->zmin; gd.zmax = h->zmax;
    return gd;
}

static int64_t regrid_count(const EvalGeom &g) {
    int64_t n = 0;
    for (int i = 0; i < MUBAR * g.nc; i++) {
        int L, km;
        double off;
        ring_table(g.has_l, g.uniform_L, i + 1, L, km, off);
        n += L;
    }
    return n;
}

// the source coordinates of every destination column, in the destination's gridpoint order (sx_get_gridpoints' r and lambda, formed
// as it forms them), and whether the column lies inside the source; returns the number outside
static int64_t regrid_map_columns(const EvalGeom &gs, const EvalGeom &gd, const double *centre, int64_t n_cols, double *cols, int32_t *inside,
                                  int64_t *first_out) {
    const double x0 = centre ? centre[0] : 0.0, y0 = centre ? centre[1] : 0.0;
    int64_t c = 0, n_out = 0;
    for (int i = 0; i < MUBAR * gd.nc; i++) {
        int L, km;
        double off;
        ring_table(gd.has_l, gd.uniform_L, i + 1, L, km, off);
        const double r = ring_radius(gd.xmin, gd.DX, 0, i);
        for (int l = 0; l < L; l++, c++) {
            double r_s = r, lam_s = 0.0;
            if (gd.has_l) regrid_map(x0, y0, r, off + 2.0 * M_PI * l / L, r_s, lam_s);
            const bool in = r_s >= gs.xmin && r_s <= gs.xmax;
            if (!in && n_out++ == 0 && first_out) *first_out = c;
            if (cols) {
                cols[c] = r_s;
                if (gd.has_l) cols[n_cols + c] = lam_s;
            }
            if (inside) inside[c] = in ? 1 : 0;
        }
    }
    return n_out;
}

static bool regrid_vertical_ok(const EvalGeom &g) { return g.nz >= 4 && g.nz <= 256 && g.Zb >= 1 && g.Zb <= g.nz && g.zmax > g.zmin; }

// everything two descriptors, the centre, var_src and `outside` decide, in the header's order; n_cols: the destination's columns
static int regrid_check(const sx_grid_desc *src, const sx_grid_desc *dst, const double *centre, const int32_t *var_src, int32_t outside,
                        EvalGeom &gs, EvalGeom &gd, int64_t &n_cols) {
    if (!desc_ok(src, "sx_regrid") || !desc_ok(dst, "sx_regrid")) return 1;
    if (src->tile_cell0 != 0 || src->tile_num_cells != src->num_cells || dst->tile_cell0 != 0 || dst->tile_num_cells != dst->num_cells) {
        set_error("sx_regrid: source and destination must be one-tile patches");
        return 1;
    }
    if (src->geometry != dst->geometry) { set_error("sx_regrid: the geometries differ (R -> R, RZ -> RZ, RL -> RL and RLZ -> RLZ only)"); return 1; }
    gs = desc_geom(src); gd = desc_geom(dst);
    if (centre && !gs.has_l) { set_error("sx_regrid: a centre is allowed on RL / RLZ grids only (pass NULL)"); return 1; }
    if (centre && (!std::isfinite(centre[0]) || !std::isfinite(centre[1]))) { set_error("sx_regrid: the centre is NaN or Inf"); return 1; }
    if (!var_src) { set_error("sx_regrid: null var_src"); return 1; }
    for (int v = 0; v < dst->nvars; v++)
        if (var_src[v] < 1 || var_src[v] > src->nvars) {
            set_error("sx_regrid: var_src[" + std::to_string(v) + "] = " + std::to_string(var_src[v]) + " is not a variable of the source (1 .. " + std::to_string(src->nvars) + ")");
            return 1;
        }
    if (outside != SX_REGRID_REFUSE && outside != SX_REGRID_FILL) { set_error("sx_regrid: outside must be SX_REGRID_REFUSE or SX_REGRID_FILL"); return 1; }
    n_cols = regrid_count(gd);
    if (n_cols > REGRID_COLS_MAX) { set_error("sx_regrid: the destination has " + std::to_string(n_cols) + " columns (at most 1048576)"); return 1; }
    if (gs.has_z) {
        if (!regrid_vertical_ok(gs) || !regrid_vertical_ok(gd)) { set_error("sx_regrid: invalid vertical grid (need 4 <= zDim <= 256, b_zDim <= zDim, zmax > zmin)"); return 1; }
        if (!(gd.zmin >= gs.zmin && gd.zmax <= gs.zmax)) {
            set_error("sx_regrid: the destination's [zmin, zmax] = [" + std::to_string(gd.zmin) + ", " + std::to_string(gd.zmax) + "] does not lie within the source's [" + std::to_string(gs.zmin) + ", " + std::to_string(gs.zmax) + "]");
            return 1;
        }
    }
    if (gs.has_l && colprof_lds(gs.kDim) > ISO_LDS_MAX) {
        set_error("sx_regrid: the tables of one column batch do not fit the LDS (need 32 (kDim + 1) + 2304 <= 8192 doubles)");
        return 1;
    }
    return 0;
}

static void regrid_refused_outside(int64_t n_out, int64_t first) {
    set_error("sx_regrid: " + std::to_string(n_out) + " column(s) of the destination lie outside the source's [xmin, xmax] (the first: column " + std::to_string(first) + ") and outside = SX_REGRID_REFUSE");
}

// E^T of the source's classes at the destination's levels, made on first use of a level set and kept
static const RegridTable *regrid_table(RegridState *st, const sx_handle *src, const EvalClasses *k, const sx_handle *dst) {
    for (const auto &t : st->tables)
        if (t->zmin == dst->zmin && t->zmax == dst->zmax && t->nz == dst->nz) return t.get();
    std::unique_ptr<RegridTable> t(new RegridTable());
    t->zmin = dst->zmin; t->zmax = dst->zmax; t->nz = dst->nz;
    const int Zb = src->Zb, nz = dst->nz, ncls = std::max<int>(1, (int)k->vert.size());
    t->Kp = (Zb + 3) & ~3; t->Mp = (nz + 15) & ~15;
    std::vector<double> ET((size_t)ncls * t->Kp * t->Mp, 0.0), w3((size_t)3 * Zb, 0.0);
    if (!src->has_z) ET[0] = 1.0;
    else
        for (int c = 0; c < ncls; c++)
            for (int n = 0; n < nz; n++) {
                eval_vert_weights(k->vert[c], src->zmin, src->zmax, src->nz, Zb, level_height(dst->zmin, dst->zmax, nz, n), w3.data());
                for (int zm = 0; zm < Zb; zm++) ET[((size_t)c * t->Kp + zm) * t->Mp + n] = w3[zm];
            }
    if (!t->d_ET.upload(ET, "sx_regrid: hipMalloc of the vertical operator failed")) return nullptr;
    st->tables.push_back(std::move(t));
    return st->tables.back().get();
}

}  // namespace sx

using namespace sx;

extern "C" {

int sx_regrid_check(const sx_grid_desc *src, const sx_grid_desc *dst, const double *centre, const int32_t *var_src, int32_t outside) {
    clear_error();
    EvalGeom gs, gd;
    int64_t n_cols = 0, first = 0;
    if (regrid_check(src, dst, centre, var_src, outside, gs, gd, n_cols)) return 1;
    if (outside == SX_REGRID_REFUSE) {
        const int64_t n_out = regrid_map_columns(gs, gd, centre, n_cols, nullptr, nullptr, &first);
        if (n_out > 0) { regrid_refused_outside(n_out, first); return 1; }
    }
    return 0;
}

int sx_regrid_columns(const sx_grid_desc *src, const sx_grid_desc *dst, const double *centre, double *columns, int32_t *inside, int64_t *n_cols) {
    clear_error();
    EvalGeom gs, gd;
    int64_t n = 0;
    std::vector<int32_t> vs(dst ? std::max(dst->nvars, 0) : 0, 1);      // the columns do not depend on the variables
    if (regrid_check(src, dst, centre, vs.data(), SX_REGRID_FILL, gs, gd, n)) return 1;
    if (n_cols) *n_cols = n;
    if (columns || inside) regrid_map_columns(gs, gd, centre, n, columns, inside, nullptr);
    return 0;
}

int sx_regrid(sx_handle *src, sx_handle *dst, const double *centre, const int32_t *var_src, int32_t outside, const double *fill, int64_t *n_outside) {
    clear_error();
    const char *who = "sx_regrid";
    if (!src || !dst) { set_error("sx_regrid: null handle"); return 1; }
    if (dst == src) { set_error("sx_regrid: the destination is the source (the forward transform overwrites the A that is read): regrid into another handle"); return 1; }
    const sx_grid_desc ds = regrid_desc(src), dd = regrid_desc(dst);
    EvalGeom gs, gd;
    int64_t n_cols = 0, first = 0;
    if (regrid_check(&ds, &dd, centre, var_src, outside, gs, gd, n_cols)) return 1;
    const int Vd = dst->V, ncc = src->has_l ? 2 : 1;
    if (outside == SX_REGRID_FILL) {
        if (!fill) { set_error("sx_regrid: null fill with outside = SX_REGRID_FILL"); return 1; }
        for (int v = 0; v < Vd; v++)
            if (!std::isfinite(fill[v])) { set_error("sx_regrid: fill[" + std::to_string(v) + "] is NaN or Inf"); return 1; }
    }
    if (n_cols * dst->nz != dst->N) { set_error("sx_regrid: internal: the destination's column count does not match its gridpoints"); return 1; }
    std::vector<double> cols((size_t)ncc * n_cols);
    std::vector<int32_t> inside(n_cols);
    const int64_t n_out = regrid_map_columns(gs, gd, centre, n_cols, cols.data(), inside.data(), &first);
    if (n_out > 0 && outside == SX_REGRID_REFUSE) { regrid_refused_outside(n_out, first); return 1; }

    // the inside columns, compacted in the destination's order: what stage 1 is sent.  A lambda outside [-2 pi, 2 pi] (a native ring's
    // last points) goes into (-pi, pi] as sx_isosurface sends it
    const int64_t n_in = n_cols - n_out;
    std::vector<double> cin((size_t)ncc * std::max<int64_t>(n_in, 1));
    std::vector<int> pidx(n_cols);
    for (int64_t c = 0, q = 0; c < n_cols; c++) {
        pidx[c] = inside[c] ? (int)q : -1;
        if (!inside[c]) continue;
        cin[q] = cols[c];
        if (src->has_l) { const double lam = cols[n_cols + c]; cin[n_in + q] = std::fabs(lam) > 6.283185307179586 ? wrap_lambda(lam) : lam; }
        q++;
    }
    std::vector<int> idx;
    std::vector<IsoBatch> batches;
    colprof_batches(src, cin.data(), n_in, idx, batches);

    const EvalClasses *k = eval_classes(src);
    if (!k) return 1;
    if (!src->diag[DIAG_REGRID]) src->diag[DIAG_REGRID].reset(new RegridState());
    RegridState *st = diag_state<RegridState>(src, DIAG_REGRID);
    if (!st->done) HIPCHK(hipEventCreateWithFlags(&st->done, hipEventDisableTiming));
    if (error_status()) return 1;
    const RegridTable *tab = regrid_table(st, src, k, dst);
    if (!tab) return 1;

    // the distinct source variables in groups of at most RED_PLANES: one stage-1 launch and one stage-2 launch per group
    std::vector<int> distinct;
    for (int v = 0; v < Vd; v++)
        if (std::find(distinct.begin(), distinct.end(), var_src[v] - 1) == distinct.end()) distinct.push_back(var_src[v] - 1);
    const int Zb = src->Zb, ngroups = ((int)distinct.size() + RED_PLANES - 1) / RED_PLANES;
    const int gmax = std::min<int>((int)distinct.size(), RED_PLANES);
    const size_t n_idx = (size_t)n_in + 4 * batches.size();
    if (!st->d_cols.grow(cin.size(), who) || !st->d_P.grow((size_t)std::max<int64_t>(n_in, 1) * gmax * Zb, who) || !st->d_idx.grow(std::max<size_t>(n_idx, 1), who) ||
        !st->d_pidx.grow(n_cols, who) || !st->d_rv.grow(Vd, who))
        return 1;

    flush_diag(src);                                 // as for every reader of A
    HIPCHK(hipStreamSynchronize(dst->stream));       // the destination's own work on var_np1, B and A is complete before another stream writes them
    HIPCHK(hipMemcpyAsync(st->d_cols, cin.data(), sizeof(double) * cin.size(), hipMemcpyHostToDevice, src->stream));
    if (n_in > 0) HIPCHK(hipMemcpyAsync(st->d_idx, idx.data(), sizeof(int) * n_in, hipMemcpyHostToDevice, src->stream));
    if (!batches.empty()) HIPCHK(hipMemcpyAsync(st->d_idx + n_in, batches.data(), sizeof(IsoBatch) * batches.size(), hipMemcpyHostToDevice, src->stream));
    HIPCHK(hipMemcpyAsync(st->d_pidx, pidx.data(), sizeof(int) * n_cols, hipMemcpyHostToDevice, src->stream));
    // the variables of every group, group after group
    std::vector<RegridVar> rv;
    std::vector<int> g_first(ngroups + 1, 0);
    for (int g = 0; g < ngroups; g++) {
        for (int v = 0; v < Vd; v++) {
            const int p = (int)(std::find(distinct.begin(), distinct.end(), var_src[v] - 1) - distinct.begin());
            if (p / RED_PLANES == g) rv.push_back(RegridVar{v, p % RED_PLANES, src->has_z ? k->vcls[var_src[v] - 1] : 0, 0, fill ? fill[v] : 0.0});
        }
        g_first[g + 1] = (int)rv.size();
    }
    HIPCHK(hipMemcpyAsync(st->d_rv, rv.data(), sizeof(RegridVar) * rv.size(), hipMemcpyHostToDevice, src->stream));
    if (error_status()) return 1;

    const int ncls_used = src->has_z ? (int)k->vert.size() : 1;
    // the profiles in (once per destination variable), E of the classes, the column table, the var_np1 planes out
    const double levels_bytes = 8.0 * ((double)Vd * Zb * n_in + (double)ncls_used * Zb * dst->nz + (double)Vd * dst->N) + 4.0 * n_cols;
    const bool mfma = dst->has_l && dst->has_z;
    for (int g = 0; g < ngroups; g++) {
        const int p0 = g * RED_PLANES, np = std::min<int>((int)distinct.size() - p0, RED_PLANES);
        if (n_in > 0) {
            ColProfArgs pa;
            std::memset(&pa, 0, sizeof(pa));
            colprof_grid_args(src, pa);
            pa.cols = st->d_cols; pa.order = st->d_idx; pa.batch = reinterpret_cast<const IsoBatch *>(st->d_idx + n_in); pa.P = st->d_P;
            pa.n_cols = (int)n_in; pa.nprof = np;
            for (int p = 0; p < np; p++) {
                pa.v[p].var = distinct[p0 + p];
                for (int kd = 0; kd < ISO_KINDS; kd++) pa.v[p].prof[kd] = kd == 0 ? p : -1;
                pa.pvar[p] = (uint8_t)distinct[p0 + p]; pa.psr[p] = 0;
            }
            launch_column_profiles(src, pa, (int)batches.size(), np, 0.0);
        }
        RegridArgs ra;
        std::memset(&ra, 0, sizeof(ra));
        ra.P = st->d_P; ra.ET = tab->d_ET; ra.pidx = st->d_pidx; ra.rv = st->d_rv + g_first[g]; ra.out = dst->d_np1;
        ra.N = dst->N; ra.n_cols = (int)n_cols; ra.nprof = np; ra.Zb = Zb; ra.Kp = tab->Kp; ra.Mp = tab->Mp; ra.nz = dst->nz;
        ra.nrv = g_first[g + 1] - g_first[g];
        {
            TimedLaunch scope(src, "k_regrid_levels", levels_bytes);
            if (mfma)
                hipLaunchKernelGGL(k_regrid_levels, dim3((unsigned)((n_cols + 15) / 16), (unsigned)ra.nrv), dim3(64), sizeof(double) * tab->Kp * RG_CS, src->stream, ra);
            else
                hipLaunchKernelGGL(k_regrid_levels_lane, grid1(n_cols * dst->nz * ra.nrv, 256), dim3(256), 0, src->stream, ra);
        }
    }
    HIPCHK(hipEventRecord(st->done, src->stream));
    HIPCHK(hipStreamWaitEvent(dst->stream, st->done, 0));
    if (error_status()) return 1;
    // the destination's own forward chain, every variable: what sx_spectral_transform + sx_spline_transform launch
    dst->diag_dirty = false;
    launch_fl_forward(dst);
    launch_sb(dst);
    launch_solve(dst);
    HIPCHK(hipStreamSynchronize(dst->stream));
    HIPCHK(hipStreamSynchronize(src->stream));
    if (error_status()) return 1;
    if (n_outside) *n_outside = n_out;
    return 0;
}

}  // extern "C"
