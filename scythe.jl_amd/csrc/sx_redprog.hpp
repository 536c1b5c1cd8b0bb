// What sx_reduce (sx_reduce.hip), sx_extrema (sx_extrema.hip) and sx_distribution (sx_distribution.hip) share: the integrand program as the kernels read it, the ring pieces
// a workgroup takes, and the loads of the planes a program names at one point.  Stated once so that the two entry points accept, pack
// and read a program identically.
#pragma once
#include "sx_internal.hpp"
#include <cstring>
#include <type_traits>

namespace sx {

constexpr int RED_T = 256;          // threads per workgroup of k_reduce / k_extrema
constexpr int RED_ITERS = 32;       // strides of a workgroup over its piece of a ring: pieces per ring = ceil(strides / RED_ITERS)
constexpr int RED_TERMS = 64, RED_OUT = 16, RED_PLANES = 16, RED_FACTORS = 4, RED_TERM_W = 11;

struct RedProg {
    double coef[RED_TERMS];
    int8_t p[RED_TERMS], nf[RED_TERMS];
    uint8_t f[RED_TERMS][RED_FACTORS];      // plane of each factor
    uint8_t start[RED_OUT + 1];             // terms of output o: [start[o], start[o + 1])
    uint8_t pvar[RED_PLANES], pslot[RED_PLANES];   // 0-based variable, slot
    int n_planes, n_out;
};

struct RedItem { int ring, lam0, nlam, pad; };

// the planes of the program at one point, widened to fp64 (a derivative slot is read in the type it is stored in)
template <class ST>
__device__ inline void red_load_planes(const Planes<ST> &P, int V, int64_t N, int64_t pt, const RedProg &g, double (&val)[RED_PLANES]) {
#pragma unroll
    for (int j = 0; j < RED_PLANES; j++) {
        val[j] = 0.0;
        if (j < g.n_planes) {
            const int v = g.pvar[j], s = g.pslot[j];
            val[j] = s == 0 ? P.val[(int64_t)v * N + pt] : (double)P.der[((int64_t)(s - 1) * V + v) * N + pt];
        }
    }
}

// W consecutive points per lane: one 16-byte access of an fp64 plane (8 of an fp32-stored one) where W = 2
template <int W> struct StatVec;
template <> struct StatVec<1> { using d = double; using f = float; };
template <> struct StatVec<2> { using d = double2; using f = float2; };
__device__ inline double stat_lane(double v, int) { return v; }
__device__ inline double stat_lane(float v, int) { return (double)v; }
__device__ inline double stat_lane(const double2 &v, int k) { return k ? v.y : v.x; }
__device__ inline double stat_lane(const float2 &v, int k) { return (double)(k ? v.y : v.x); }
__device__ inline void stat_pack(double &o, const double (&a)[1]) { o = a[0]; }
__device__ inline void stat_pack(double2 &o, const double (&a)[2]) { o = make_double2(a[0], a[1]); }

// red_load_planes W points wide (k_stats, k_project): the planes of the program at W consecutive points from pt (a multiple of W), one access per plane
template <class ST, int W>
__device__ inline void stat_load_planes(const Planes<ST> &P, int V, int64_t N, int64_t pt, const RedProg &g, double (&val0)[RED_PLANES],
                                        double (&val1)[RED_PLANES]) {
    using VD = typename StatVec<W>::d;
    using VS = typename std::conditional<std::is_same<ST, float>::value, typename StatVec<W>::f, VD>::type;
#pragma unroll
    for (int j = 0; j < RED_PLANES; j++) {
        val0[j] = val1[j] = 0.0;
        if (j < g.n_planes) {
            const int v = g.pvar[j], s = g.pslot[j];
            if (s == 0) {
                const VD x = *reinterpret_cast<const VD *>(P.val + (int64_t)v * N + pt);
                val0[j] = stat_lane(x, 0);
                if (W == 2) val1[j] = stat_lane(x, 1);
            } else {
                const VS x = *reinterpret_cast<const VS *>(P.der + ((int64_t)(s - 1) * V + v) * N + pt);
                val0[j] = stat_lane(x, 0);
                if (W == 2) val1[j] = stat_lane(x, 1);
            }
        }
    }
}

// term t at a point: coef r^p prod field, the factors in the program's order (also on the host: sx_project_point)
__host__ __device__ inline double red_term(const RedProg &g, int t, const double (&val)[RED_PLANES], double r, double rr, double ri, double rri) {
    const int p = g.p[t], nf = g.nf[t];
    double x = g.coef[t];
    if (p != 0) x *= p == 1 ? r : p == 2 ? rr : p == -1 ? ri : rri;
#pragma unroll
    for (int f = 0; f < RED_FACTORS; f++)
        if (f < nf) x *= val[g.f[t][f]];
    return x;
}

// the double-double sums of sx_reduce and sx_distribution: (hi, lo) += x, the rounding error of the sum kept in lo (Knuth's two-sum: no ordering of |hi|, |x| assumed)
__device__ inline void dd_add(double &hi, double &lo, double x) {
    const double s = hi + x, b = s - hi;
    lo += (hi - (s - b)) + (x - b);
    hi = s;
}
__device__ inline void dd_add(double &hi, double &lo, double xh, double xl) {
    dd_add(hi, lo, xh);
    lo += xl;
}

// the work list: ring pieces (grids with an azimuth) or whole rings; first [nrings + 1] = first piece of each ring.  A function of the
// grid alone.
inline void red_items(const sx_handle *h, std::vector<RedItem> &items, std::vector<int> &first) {
    items.clear();
    first.assign(h->nrings + 1, 0);
    const int G = RED_T / h->nz;         // lambdas per stride (nz <= 256: sx_create)
    for (int i = 0; i < h->nrings; i++) {
        first[i] = (int)items.size();
        const int L = h->hL[i];
        const int strides = (L + G - 1) / G, pieces = h->has_l ? (strides + RED_ITERS - 1) / RED_ITERS : 1;
        for (int c = 0; c < pieces; c++) {
            const int l0 = (int)((int64_t)L * c / pieces), l1 = (int)((int64_t)L * (c + 1) / pieces);
            items.push_back(RedItem{i, l0, l1 - l0, 0});
        }
    }
    first[h->nrings] = (int)items.size();
}

// the program as the kernels read it, from one that sx_reduce_planes has passed: terms by output (their order within an output
// kept), factors as plane numbers
inline void red_pack(RedProg &prog, const int32_t (*planes)[2], int n_planes, int n_terms, const double *coef, const int32_t *terms, int n_out) {
    std::memset(&prog, 0, sizeof(prog));
    prog.n_planes = n_planes; prog.n_out = n_out;
    for (int j = 0; j < n_planes; j++) { prog.pvar[j] = (uint8_t)(planes[j][0] - 1); prog.pslot[j] = (uint8_t)planes[j][1]; }
    int k = 0;
    for (int o = 0; o < n_out; o++) {
        prog.start[o] = (uint8_t)k;
        for (int t = 0; t < n_terms; t++) {
            const int32_t *q = terms + (size_t)t * RED_TERM_W;
            if (q[0] != o) continue;
            prog.coef[k] = coef[t]; prog.p[k] = (int8_t)q[1]; prog.nf[k] = (int8_t)q[2];
            for (int f = 0; f < q[2]; f++) {
                int j = 0;
                while (planes[j][0] != q[3 + f] || planes[j][1] != q[3 + RED_FACTORS + f]) j++;
                prog.f[k][f] = (uint8_t)j;
            }
            k++;
        }
    }
    for (int o = n_out; o <= RED_OUT; o++) prog.start[o] = (uint8_t)k;
}

// bytes k_reduce / k_extrema read: the planes named x N x their element size
inline double red_bytes(const sx_handle *h, int source, const int32_t (*planes)[2], int n_planes) {
    double b = 0;
    for (int j = 0; j < n_planes; j++) b += (double)h->N * (source == SX_REDUCE_PHYSICAL && h->f32 && planes[j][1] > 0 ? 4.0 : 8.0);
    return b;
}

}  // namespace sx
