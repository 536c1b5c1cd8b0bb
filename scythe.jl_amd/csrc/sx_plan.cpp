// Launch plans: which kernel instantiation and which grid a launcher takes, as pure functions of plain integers and the
// switches.  No handle, no device: the launchers (sx_kernels.hip, sx_pcr.hip, sx_rz.hip) dispatch on these, and sx_launch_plan returns
// them to a caller without a GPU, so the tests name the launch shapes from the same arithmetic that launches them.
#include "sx_internal.hpp"
#include <algorithm>

namespace sx {

static bool fused_rz(int geometry, int sp32, const Switches &sw) { return sw.rz_fused && geometry == SX_GEOM_RZ && !sp32; }   // = rz_fused(h)

// spectralTransform!'s radial inner products B = sum over cells (fused with the vertical forward transform where there is one)
SbPlan plan_sb(int geometry, int nz, int Zb, int K2, int v_cnt, int ncells, int sp32, const Switches &sw) {
    SbPlan p;
    if (fused_rz(geometry, sp32, sw)) { p.kernel = SbKernel::rz_forward; return p; }
    if (geometry != SX_GEOM_RZ && geometry != SX_GEOM_RLZ) { p.kernel = SbKernel::sb; p.threads = 256; return p; }
    if (nz != 32 && nz != 64 && nz != 128) { p.kernel = SbKernel::sbz; p.threads = 256; p.bw = 64; return p; }
    const bool mf = sw.sbw_mfma && (nz <= 64 ? Zb <= 64 : Zb <= 96);      // matrix-core contraction + prefetch (k_sbw_mfma)
    if (sp32 && !mf) return p;                                            // refused
    const bool t256 = sw.sbw_t256 && mf && nz == 64;
    const bool narrow = (mf && nz == 128) || t256;
    const bool pf = (sw.sbw_prefetch && nz <= 64) || mf;
    // cells per workgroup (+3 warm-up cells).  With the prefetch (zDim <= 64: 177 VGPRs, one 512-thread workgroup per
    // CU) the grid is ONE round of at most 256 workgroups; without it (zDim 128: 16 values per thread and ring leave no
    // registers for a second set; or SX_SBW_PF=0) about 1.5 workgroups per CU as before.  On large tiles never fewer
    // than 6 cells so that the warm-up stays below half of the reads
    p.threads = t256 ? 256 : 512;
    p.bw = narrow ? 32 : 64;
    p.groups = ((K2 + p.bw - 1) / p.bw) * v_cnt;
    p.nseg = sw.sbw_seg > 0 ? sw.sbw_seg : std::max(1, (narrow ? 512 : pf || nz == 128 ? 256 : 384) / p.groups);
    // small tiles (multi-GPU strong scaling): the kernel is then one workgroup's latency chain, which is proportional
    // to the cells it walks, so short segments (down to 2 cells + 3 warm-up) beat the saved re-reads
    p.cps = std::max(ncells <= 64 ? 2 : 6, (ncells + p.nseg - 1) / p.nseg);
    p.segs = (ncells + p.cps - 1) / p.cps;
    using K = SbKernel;
    if (sp32) p.kernel = t256 ? K::mfma_64_t256_f32 : nz == 64 ? K::mfma_64_f32 : nz == 32 ? K::mfma_32_f32 : K::mfma_128_f32;
    else if (t256) p.kernel = K::mfma_64_t256;
    else if (mf) p.kernel = nz == 64 ? K::mfma_64 : nz == 32 ? K::mfma_32 : K::mfma_128;
    else p.kernel = nz == 64 ? (pf ? K::sbw_64_pf : K::sbw_64) : nz == 32 ? (pf ? K::sbw_32_pf : K::sbw_32) : K::sbw_128;
    return p;
}

// spectralTransform! as k_fl_forward_cells + k_nodes_z: wherever the forward FFT kernel and the fp64 matrix-core sliding-window kernel
// are both taken today, on rings of at most 256 points (at 512 a lane carries four wavenumbers: 64 doubles of open node sums, which
// leave the transform no registers).  Everything else - native rings, RL, RZ, fp32 spectra, SX_SBW_MFMA=2 - keeps its kernels.
// By default only launches of the measured kind take it: segments of at least 9 cells that fill three quarters of a round of CUs
// (the bench grid).  On small tiles - an 8-way split's 21 cells: S = 3, 168 workgroups, each a serial chain of 9 rings at ~7,000
// cycles a ring - the one-workgroup-per-CU kernel is a latency chain: forced there, k_fl_forward doubles, k_sbz gains less, and the
// slowest tile of the 8-tile step gets 1.2 % slower (profiles/r05/ab_forward_cells.txt); SX_SBW_MFMA=3 takes the pair wherever its kernels apply (tests, A/B at other shapes).
CellsPlan plan_fwd_cells(int geometry, int nz, int Zb, int K2, int nvars, int v_cnt, int ncells, int sp32, int uniform_L, const Switches &sw) {
    CellsPlan p;
    const int L = uniform_L;
    if (sw.sbw_mfma == 2 || geometry != SX_GEOM_RLZ || sp32 || L < 16 || L > 256 || (L & (L - 1)) || nz % 16) return p;
    const SbPlan sb = plan_sb(geometry, nz, Zb, K2, v_cnt, ncells, sp32, sw);
    using K = SbKernel;
    if (sb.kernel != K::mfma_32 && sb.kernel != K::mfma_64 && sb.kernel != K::mfma_64_t256 && sb.kernel != K::mfma_128) return p;
    p.on = true;
    while ((1 << p.logL) < L) p.logL++;
    p.threads = std::max(64, 8 * std::min(L / 4, 64));
    // Segment length: a workgroup's time is proportional to the cells it walks, every workgroup of the launch walks the same number,
    // and a CU holds one 512-thread workgroup (its registers: sx_fft.hip), so the launch takes ceil(workgroups / 256) rounds of S
    // cells: the S with the smallest rounds x (S + 1), see below.  At least 3 cells: a node then
    // lies in at most two segments.  Bench grid (171 cells, 4 chunks, 6 variables): S = 18, 10 segments, 240 workgroups in one round
    // (measured on one MI355X with the segment length forced, steps/s of the bench step: S = 3 990, 5 999, 6 1013, 9 1026, 12 979, 18 1036).
    // Each segment also stores three edge rows on top of its S node rows and starts with a tile load nothing hides: one cell's worth
    // per round, which orders the measured lengths as measured (cost 24, 24, 21, 20, 26, 19 for S = 3, 5, 6, 9, 12, 18).
    const int wg_per_seg = (nz / 16) * nvars, slots = 256;
    int64_t best = 0;
    for (int s = 3; s <= 24; s++) {
        const int segs = (ncells + s - 1) / s;
        const int64_t cost = (int64_t)((wg_per_seg * segs + slots - 1) / slots) * (std::min(s, ncells) + 1);
        if (p.S == 0 || cost < best) { best = cost; p.S = s; }
    }
    p.segs = (ncells + p.S - 1) / p.S;
    if (sw.sbw_mfma != 3 && (p.S < 9 || 4 * wg_per_seg * p.segs < 3 * slots)) return CellsPlan();
    // k_nodes_z: the sliding-window kernel's workgroup shape over runs of whole nodes, about one round of workgroups (the operator
    // fragments are fetched into LDS once per workgroup)
    p.zk = sb.kernel;
    p.zthreads = sb.threads;
    p.bw = sb.bw;
    const int nbt = ncells + 3, runs = std::max(1, (p.bw == 32 ? 512 : 256) / std::max(1, sb.groups));
    p.nps = std::max(1, (nbt + runs - 1) / runs);
    p.zsegs = (nbt + p.nps - 1) / p.nps;
    return p;
}

// the vertical inverse into Az (k_zinv)
ZinvPlan plan_zinv(int geometry, int nz, int K2, int sp32, const Switches &sw) {
    ZinvPlan p;
    if ((geometry != SX_GEOM_RZ && geometry != SX_GEOM_RLZ) || fused_rz(geometry, sp32, sw)) return p;   // RZ: part of k_rz_inverse (sx_rz.hip)
    // only CT = 1, 2, 4 are instantiated at 128 levels (1, 2 at 64): any other request takes the default, never a grid sized for a kernel that is not launched
    const int ct = sw.zinv_ct;
    p.CT = nz == 128 ? ((ct == 1 || ct == 4) ? ct : 2) : (nz == 64 && ct == 2 ? 2 : 1);
    p.grid_x = (K2 + 64 * p.CT - 1) / (64 * p.CT);
    p.f32 = sp32 != 0;
    using K = ZinvKernel;
    p.kernel = nz == 32 ? K::mfma_2_1 : nz == 64 ? (p.CT == 2 ? K::mfma_4_2 : K::mfma_4_1)
               : nz == 128 ? (p.CT == 1 ? K::mfma_8_1 : p.CT == 4 ? K::mfma_8_4 : K::mfma_8_2) : K::colmat;
    return p;
}

// k_solve_pcr over `ngroups` (variable, z-mode) groups: R columns per workgroup, by the launch's column count unless SX_PCR_R names
// it; a power of two, and small enough that one thread per (block row, column) fits a workgroup (nblk_max R <= 1024)
PcrPlan plan_pcr(int nblk_max, int b_rDim, int K2, int ngroups, const Switches &sw) {
    PcrPlan p;
    const int64_t total = (int64_t)ngroups * (K2 > 1 ? K2 - 1 : 1);
    int R = sw.pcr_r > 0 ? sw.pcr_r : total <= 4096 ? 4 : total <= 16384 ? 8 : 16;
    while (R > 1 && (int64_t)nblk_max * R > 1024) R >>= 1;
    while ((1 << (p.logR + 1)) <= R) p.logR++;
    p.R = 1 << p.logR;
    p.threads = std::min(1024, ((std::max(nblk_max * p.R, (b_rDim * p.R + PCR_IPT - 1) / PCR_IPT) + 63) / 64) * 64);
    return p;
}

// k_solve_part over `ncols` right-hand sides of the contiguous one-tile solve: the number of partitions, 0 where the launch keeps
// k_solve / k_solve_pcr.  The interface form needs 9 cells per partition (a partition of a rank-3 class then owns 6 unknowns
// or more), the register array holds PART_NR unknowns per partition (176 patch rows at most; the bench grid has 174), PERIODIC classes have
// their corner blocks and keep k_solve.  By default only launches that PCR does not take and that give every SIMD of the chip
// a wave (1024 waves of 64 columns, PART_P waves per workgroup); SX_SOLVE_PCR=2: wherever the tables exist.
int plan_solve_part(int b_rDim, int periodic, int contiguous, int64_t ncols, const Switches &sw) {
    const int P = PART_P, NR = PART_NR;
    if (sw.solve_pcr == 0 || sw.solve_pcr == 1 || periodic || !contiguous) return 0;
    if (b_rDim - 3 < 9 * P || b_rDim > P * NR) return 0;
    if (sw.solve_pcr == 2) return P;
    return sw.solve_pcr < 0 && ncols > sw.pcr_maxcols && ncols >= (int64_t)1024 * 64 / PART_P ? P : 0;
}

// tileTransform! on a fused RZ grid.  Nodes form (default): workgroup = 13 cells (the 16 nodes they touch) x variable x 4 level tiles;
// LDS = the A rows [Zp][16] (Zp = b_zDim rounded up to chunks of 32 rows), the Az tile [3][16][65] and the weights [3][39][4].  It is
// taken while that fits the default dynamic-LDS limit; else, and with SX_RZ_INV=0, the ring-tile form: 16 rings per workgroup,
// LDS = [3][Zp][16] with chunks of 64 rows, above 64 KB (b_zDim >= 129) with the kernel's limit raised first.
RzInvPlan plan_rz_inverse(int nz, int Zb, int ncells, int V, int f32, const Switches &sw) {
    RzInvPlan p;
    p.f32 = f32 != 0;
    p.gy = V;
    p.gz = ((nz + 15) / 16 + 3) / 4;
    constexpr int CHN = 4 * RZ_NODES_KC, CH = 4 * RZ_KC;
    const int Zpn = (Zb + CHN - 1) / CHN * CHN;
    const size_t ldsn = sizeof(double) * ((size_t)Zpn * RZ_T + 3 * RZ_T * RZ_NODES_ZS + 3 * RZ_CT * MUBAR * 4);
    if (sw.rz_inv && ldsn <= (size_t)LDS_DEFAULT_MAX) {
        p.gx = (ncells + RZ_CT - 1) / RZ_CT;
        p.lds = (int)ldsn;
        p.chunks = Zpn / CHN;
        return p;
    }
    const int Zp = (Zb + CH - 1) / CH * CH;
    p.nodes = false;
    p.gx = (ncells * MUBAR + RZ_T - 1) / RZ_T;
    p.lds = (int)(sizeof(double) * 3 * Zp * RZ_T);
    p.chunks = Zp / CH;
    p.attr = p.lds > LDS_DEFAULT_MAX;
    return p;
}

// spectralTransform! on a fused RZ grid: workgroup = 16 nodes x variable x group of mt_per_wg tiles of 16 modes (one tile per wave:
// more workgroups beat fewer restagings at this size); LDS = the radial inner products [Np][16] (Np = zDim rounded up to chunks of
// 64 levels) and the weights of the 19 cells around the node tile [57][4]
RzFwdPlan plan_rz_forward(int nz, int Zb, int ncells, int v_cnt) {
    RzFwdPlan p;
    constexpr int CH = 4 * RZ_KC;
    const int Np = (nz + CH - 1) / CH * CH, nmt = (Zb + 15) / 16;
    p.mt_per_wg = std::min(nmt, 4);
    p.gx = (ncells + 3 + RZ_T - 1) / RZ_T;
    p.gy = v_cnt;
    p.gz = (nmt + p.mt_per_wg - 1) / p.mt_per_wg;
    p.chunks = Np / CH;
    p.lds = (int)(sizeof(double) * ((size_t)Np * RZ_T + 19 * MUBAR * 4));
    return p;
}

// semiimplicit_adjustment over ncol columns.  k_semi_mfma: 16 columns per workgroup, one wave per tile of 16 levels up to 8 waves (above
// 128 levels a wave takes a second tile), LDS = four [Kp][16] column tiles (Kp = zDim rounded up to chunks of 64 levels), above 64 KB
// (zDim > 128) with the kernel's limit raised first.  SX_SEMI_MFMA=0: k_semiimplicit, 256 / zDim whole columns per workgroup (at
// least one), a thread per level, LDS = three columns each.
SemiPlan plan_semi(int nz, int64_t ncol, const Switches &sw) {
    SemiPlan p;
    p.mfma = sw.semi_mfma != 0;
    if (!p.mfma) {
        p.cpb = nz >= 256 ? 1 : 256 / nz;
        p.wgs = (int)((ncol + p.cpb - 1) / p.cpb);
        p.threads = p.cpb * nz;
        p.lds = (int)(sizeof(double) * 3 * p.cpb * nz);
        return p;
    }
    constexpr int CH = 4 * RZ_KC;
    const int Kp = (nz + CH - 1) / CH * CH, nzt = (nz + 15) / 16;
    p.wgs = (int)((ncol + RZ_T - 1) / RZ_T);
    p.tiles_per_trip = std::min(8, nzt);
    p.threads = 64 * p.tiles_per_trip;
    p.chunks = Kp / CH;
    p.lds = (int)(sizeof(double) * 4 * Kp * RZ_T);
    p.attr = p.lds > LDS_DEFAULT_MAX;
    return p;
}

std::string kernel_name(const RzInvPlan &p) {
    return std::string(p.nodes ? "k_rz_inverse_nodes<" : "k_rz_inverse<") + (p.f32 ? "float" : "double") + ">";
}

std::string kernel_name(SbKernel k) {
    static const char *const NAMES[] = {
        "", "k_sb", "k_sbz", "k_rz_forward", "k_sbw<32, false>", "k_sbw<32, true>", "k_sbw<64, false>", "k_sbw<64, true>", "k_sbw<128, false>",
        "k_sbw_mfma<32>", "k_sbw_mfma<64>", "k_sbw_mfma<64, 32, 256>", "k_sbw_mfma<128, 32>", "k_sbw_mfma<32, 64, 512, float>",
        "k_sbw_mfma<64, 64, 512, float>", "k_sbw_mfma<64, 32, 256, float>", "k_sbw_mfma<128, 32, 512, float>"};
    static_assert(sizeof(NAMES) / sizeof(NAMES[0]) == (size_t)SbKernel::mfma_128_f32 + 1, "one name per SbKernel");
    return NAMES[(int)k];
}

std::string kernel_name(const ZinvPlan &p) {
    if (p.kernel == ZinvKernel::none) return "";
    if (p.kernel == ZinvKernel::colmat) return "k_colmat";
    static const int MT[] = {2, 4, 4, 8, 8, 8};      // mfma_<MT>_<CT> in enum order; CT is the plan's
    return "k_colmat_mfma<" + std::to_string(MT[(int)p.kernel - (int)ZinvKernel::mfma_2_1]) + ", " + (p.f32 ? "float" : "double") + ", " +
           std::to_string(p.CT) + ">";
}

}  // namespace sx
