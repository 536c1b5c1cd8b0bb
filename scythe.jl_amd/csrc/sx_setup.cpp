// Host-side operator construction for libscythe_hip.so.
//
// Everything here restates arithmetic the reference obtains from the external Springsteel.jl package
// (Project.toml:20) - cubic B-spline basis, quadrature, P + eps_q Q assembly, boundary-condition projection,
// Cholesky factorisation, Chebyshev collocation / derivative / integral operators - following SURVEY.md 8(c).
// The quadrature-weight ratio 8:5:8 is the one the reference's notebook known-answer pins.
#include "sx_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sx {

static const double SQRT35 = std::sqrt(3.0 / 5.0);
static const double GAUSS_OFF[MUBAR] = {-SQRT35 / 2.0, 0.0, SQRT35 / 2.0};
static const double QUAD_W[MUBAR] = {8.0 / 21.0, 5.0 / 21.0, 8.0 / 21.0};

// d-th derivative of the cardinal cubic B-spline with respect to its argument
template <class T>
static T bspl(T delta, int d) {
    T z = std::fabs(delta);
    if (z >= T(2.0)) return T(0.0);
    T s = delta > 0 ? T(1.0) : T(-1.0);
    T p = T(2.0) - z, q = z < T(1.0) ? T(1.0) - z : T(0.0);
    switch (d) {
        case 0: return p * p * p / T(6.0) - T(4.0) * q * q * q / T(6.0);
        case 1: return -s * (p * p / T(2.0) - T(2.0) * q * q);
        case 2: return p - T(4.0) * q;
        default: return s * (z < T(1.0) ? T(3.0) : T(-1.0));
    }
}

// phi[d][mu][j]: d-th x-derivative of basis function of node (cell - 1 + j) at mish point mu of that cell
void basis_tables(double DX, double phi[4][MUBAR][4]) {
    for (int d = 0; d < 4; d++) {
        double sc = 1.0 / std::pow(DX, d);
        for (int mu = 0; mu < MUBAR; mu++)
            for (int j = 0; j < 4; j++) phi[d][mu][j] = bspl<double>(1.5 + GAUSS_OFF[mu] - j, d) * sc;
    }
}

void quad_weights(double DX, double w[MUBAR]) {
    for (int mu = 0; mu < MUBAR; mu++) w[mu] = DX * QUAD_W[mu];
}

int bc_rank(int bc) {
    switch (bc) {
        case SX_BC_R0: return 0;
        case SX_BC_R1T0: case SX_BC_R1T1: case SX_BC_R1T2: return 1;
        case SX_BC_R2T10: case SX_BC_R2T20: return 2;
        case SX_BC_R3: return 3;
        default: return -1;
    }
}

// rows of dependent boundary coefficients: a_dep[i] = g[i][0] * free_first + g[i][1] * free_second
static bool boundary_rows(int bc, double g[3][2]) {
    std::memset(g, 0, sizeof(double) * 6);
    switch (bc) {
        case SX_BC_R0: case SX_BC_R3: return true;
        case SX_BC_R1T0: g[0][0] = -4.0; g[0][1] = -1.0; return true;
        case SX_BC_R1T1: g[0][0] = 0.0; g[0][1] = 1.0; return true;
        case SX_BC_R1T2: g[0][0] = 2.0; g[0][1] = -1.0; return true;
        case SX_BC_R2T10: g[0][0] = 1.0; g[1][0] = -0.5; return true;
        case SX_BC_R2T20: g[0][0] = -1.0; g[1][0] = 0.0; return true;
        default: return false;
    }
}

// Gamma as sparse rows: free j -> list of (patch row, weight), from the class's rank and boundary rows
static std::vector<std::vector<std::pair<int, double>>> gamma_rows(const SplineClass &sc, int nb) {
    const int n = sc.nfree;
    std::vector<std::vector<std::pair<int, double>>> G(n);
    if (sc.periodic) {
        for (int m = 0; m < nb; m++) G[(m - 1 + n) % n].push_back({m, 1.0});
    } else {
        for (int j = 0; j < n; j++) G[j].push_back({sc.rl + j, 1.0});
        for (int i = 0; i < sc.rl; i++) {
            if (sc.gl[i][0] != 0.0) G[0].push_back({i, sc.gl[i][0]});
            if (sc.gl[i][1] != 0.0) G[1].push_back({i, sc.gl[i][1]});
        }
        for (int i = 0; i < sc.rr; i++) {
            if (sc.gr[i][0] != 0.0) G[n - 1].push_back({nb - 1 - i, sc.gr[i][0]});
            if (sc.gr[i][1] != 0.0) G[n - 2].push_back({nb - 1 - i, sc.gr[i][1]});
        }
    }
    return G;
}

bool build_spline_class(int nc, double DX, double l_q, int bcl, int bcr, SplineClass &out, std::string &err) {
    const int nb = nc + 3;
    out.bcl = bcl;
    out.bcr = bcr;
    out.periodic = (bcl == SX_BC_PERIODIC || bcr == SX_BC_PERIODIC);
    if (out.periodic && bcl != bcr) { err = "PERIODIC must be set on both sides"; return false; }
    if (!out.periodic) {
        out.rl = bc_rank(bcl);
        out.rr = bc_rank(bcr);
        if (out.rl < 0 || out.rr < 0 || !boundary_rows(bcl, out.gl) || !boundary_rows(bcr, out.gr)) {
            err = "unknown radial boundary condition code";
            return false;
        }
        out.nfree = nb - out.rl - out.rr;
    } else {
        out.rl = out.rr = 0;
        out.nfree = nc;
    }
    const int n = out.nfree;
    if (n < (out.periodic ? 7 : 4)) { err = "too few cells for the requested boundary conditions"; return false; }

    // P + eps_q Q, 7-diagonal: Pb[mi][mj - mi + 3]
    double phi[4][MUBAR][4], w[MUBAR];
    basis_tables(DX, phi);
    quad_weights(DX, w);
    const double eps_q = std::pow(l_q * DX / (2.0 * M_PI), 6);
    std::vector<double> Pb((size_t)nb * 7, 0.0);
    for (int c = 0; c < nc; c++)
        for (int mu = 0; mu < MUBAR; mu++)
            for (int j = 0; j < 4; j++)
                for (int k = 0; k < 4; k++)
                    Pb[(size_t)(c + j) * 7 + (k - j + 3)] +=
                        w[mu] * (phi[0][mu][j] * phi[0][mu][k] + eps_q * phi[3][mu][j] * phi[3][mu][k]);
    auto P = [&](int i, int j) -> double {
        int dj = j - i + 3;
        return (dj < 0 || dj > 6) ? 0.0 : Pb[(size_t)i * 7 + dj];
    };
    const std::vector<std::vector<std::pair<int, double>>> G = gamma_rows(out, nb);
    // PQ = Gamma P Gamma^T (dense, symmetric)
    std::vector<double> A((size_t)n * n, 0.0);
    for (int a = 0; a < n; a++)
        for (int b = 0; b <= a; b++) {
            double s = 0.0;
            for (auto &ia : G[a])
                for (auto &jb : G[b]) s += ia.second * P(ia.first, jb.first) * jb.second;
            A[(size_t)a * n + b] = s;
            A[(size_t)b * n + a] = s;
        }
    out.Mdense = A;
    out.Gam = G;
    // dense Cholesky A = L L^T (lower)
    for (int j = 0; j < n; j++) {
        double d = A[(size_t)j * n + j];
        for (int k = 0; k < j; k++) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
        if (!(d > 0.0)) { err = "spline matrix is not positive definite"; return false; }
        d = std::sqrt(d);
        A[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; i++) {
            // skip structural zeros cheaply: only band rows and (periodic) the last three rows are non-zero
            if (i - j > 3 && !(out.periodic && i >= n - 3)) { A[(size_t)i * n + j] = 0.0; continue; }
            double s = A[(size_t)i * n + j];
            for (int k = 0; k < j; k++) s -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
            A[(size_t)i * n + j] = s / d;
        }
    }
    out.Lband.assign((size_t)nb * 4, 0.0);
    out.Larrow.assign((size_t)3 * nb, 0.0);
    for (int i = 0; i < n; i++)
        for (int q = 0; q < 4; q++)
            if (i - q >= 0) out.Lband[(size_t)i * 4 + (3 - q)] = A[(size_t)i * n + (i - q)];
    if (out.periodic)
        for (int r = 0; r < 3; r++)
            for (int k = 0; k <= n - 3 + r; k++) out.Larrow[(size_t)r * nb + k] = A[(size_t)(n - 3 + r) * n + k];
    return true;
}

// ---------------------------------------------------------------------------------------------- parallel cyclic reduction tables
typedef long double pxr;
struct B3 { pxr a[9]; };
static B3 b3_zero() { B3 z; for (int i = 0; i < 9; i++) z.a[i] = 0.0L; return z; }
static B3 b3_mul(const B3 &x, const B3 &y) {
    B3 r = b3_zero();
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++)
            for (int j = 0; j < 3; j++) r.a[i * 3 + j] += x.a[i * 3 + k] * y.a[k * 3 + j];
    return r;
}
static B3 b3_sub(const B3 &x, const B3 &y) { B3 r; for (int i = 0; i < 9; i++) r.a[i] = x.a[i] - y.a[i]; return r; }
static bool b3_inv(const B3 &m, B3 &out) {
    const pxr *a = m.a;
    const pxr c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
    const pxr det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    if (det == 0.0L) return false;
    const pxr id = 1.0L / det;
    out.a[0] = c00 * id; out.a[1] = (a[2] * a[7] - a[1] * a[8]) * id; out.a[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    out.a[3] = c01 * id; out.a[4] = (a[0] * a[8] - a[2] * a[6]) * id; out.a[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    out.a[6] = c02 * id; out.a[7] = (a[1] * a[6] - a[0] * a[7]) * id; out.a[8] = (a[0] * a[4] - a[1] * a[3]) * id;
    return true;
}
static pxr b3_norm(const B3 &m) { pxr s = 0.0L; for (int i = 0; i < 9; i++) s = std::max(s, fabsl(m.a[i])); return s; }

bool build_pcr_tables(const SplineClass &sc, int nb, PcrTables &t, std::string &err) {
    const int n = sc.nfree;
    t.n = n; t.periodic = sc.periodic;
    t.nblk = (n + 2) / 3;
    const int np = 3 * t.nblk;
    if ((int)sc.Mdense.size() != n * n) { err = "build_pcr_tables: the class has no dense matrix"; return false; }
    auto Mc = [&](int i, int j) -> pxr { return (pxr)sc.Mdense[(size_t)i * n + j]; };
    // band part (PERIODIC: the corner blocks leave through the rank-6 correction below); padding unknowns are identity rows
    auto Mb = [&](int i, int j) -> pxr {
        if (i >= n || j >= n) return i == j ? 1.0L : 0.0L;
        return std::abs(i - j) <= 3 ? Mc(i, j) : 0.0L;
    };
    std::vector<B3> Lb(t.nblk), Db(t.nblk), Ub(t.nblk);
    for (int i = 0; i < t.nblk; i++) {
        Lb[i] = Db[i] = Ub[i] = b3_zero();
        for (int p = 0; p < 3; p++)
            for (int q = 0; q < 3; q++) {
                Db[i].a[p * 3 + q] = Mb(3 * i + p, 3 * i + q);
                if (i > 0) Lb[i].a[p * 3 + q] = Mb(3 * i + p, 3 * (i - 1) + q);
                if (i + 1 < t.nblk) Ub[i].a[p * 3 + q] = Mb(3 * i + p, 3 * (i + 1) + q);
            }
    }
    t.coef.clear();
    t.levels = 0;
    for (int s = 1; s < 2 * t.nblk; s <<= 1) {
        pxr off = 0.0L, dia = 0.0L;
        for (int i = 0; i < t.nblk; i++) { off = std::max(off, std::max(b3_norm(Lb[i]), b3_norm(Ub[i]))); dia = std::max(dia, b3_norm(Db[i])); }
        // block diagonal already - exactly (s >= nblk) or far below anything a double-precision right-hand side can see
        if (off == 0.0L || off < dia * 1e-34L) break;
        std::vector<B3> Di(t.nblk), Ln(t.nblk), Dn(t.nblk), Un(t.nblk);
        for (int i = 0; i < t.nblk; i++)
            if (!b3_inv(Db[i], Di[i])) { err = "build_pcr_tables: singular diagonal block"; return false; }
        const size_t base = t.coef.size();
        t.coef.resize(base + (size_t)t.nblk * 18, 0.0);
        for (int i = 0; i < t.nblk; i++) {
            B3 al = b3_zero(), ga = b3_zero();
            Dn[i] = Db[i]; Ln[i] = b3_zero(); Un[i] = b3_zero();
            if (i - s >= 0) {
                al = b3_mul(Lb[i], Di[i - s]);
                Dn[i] = b3_sub(Dn[i], b3_mul(al, Ub[i - s]));
                Ln[i] = b3_sub(b3_zero(), b3_mul(al, Lb[i - s]));
            }
            if (i + s < t.nblk) {
                ga = b3_mul(Ub[i], Di[i + s]);
                Dn[i] = b3_sub(Dn[i], b3_mul(ga, Lb[i + s]));
                Un[i] = b3_sub(b3_zero(), b3_mul(ga, Ub[i + s]));
            }
            for (int q = 0; q < 9; q++) {
                t.coef[base + (size_t)i * 18 + q] = (double)al.a[q];
                t.coef[base + (size_t)i * 18 + 9 + q] = (double)ga.a[q];
            }
        }
        Lb.swap(Ln); Db.swap(Dn); Ub.swap(Un);
        t.levels++;
    }
    t.dinv.assign((size_t)t.nblk * 9, 0.0);
    for (int i = 0; i < t.nblk; i++) {
        B3 di;
        if (!b3_inv(Db[i], di)) { err = "build_pcr_tables: singular reduced block"; return false; }
        for (int q = 0; q < 9; q++) t.dinv[(size_t)i * 9 + q] = (double)di.a[q];
    }
    // Gamma b and Gamma^T x as gather tables
    t.gin_row.assign((size_t)np * 4, -1); t.gin_w.assign((size_t)np * 4, 0.0);
    t.gout_j.assign((size_t)nb * 2, -1); t.gout_w.assign((size_t)nb * 2, 0.0);
    std::vector<int> cnt_out(nb, 0);
    for (int j = 0; j < n; j++) {
        if (sc.Gam[j].size() > 4) { err = "build_pcr_tables: more than 4 patch rows per free unknown"; return false; }
        int q = 0;
        for (auto &e : sc.Gam[j]) {
            t.gin_row[(size_t)j * 4 + q] = e.first; t.gin_w[(size_t)j * 4 + q] = e.second; q++;
            if (cnt_out[e.first] >= 2) { err = "build_pcr_tables: more than 2 free unknowns per patch row"; return false; }
            t.gout_j[(size_t)e.first * 2 + cnt_out[e.first]] = j; t.gout_w[(size_t)e.first * 2 + cnt_out[e.first]] = e.second;
            cnt_out[e.first]++;
        }
    }
    t.G.clear();
    if (sc.periodic) {
        // M_c = M_b + E C E^T over the edge unknowns e = {0, 1, 2, n-3, n-2, n-1};  x = y - W (I + C E^T W)^-1 C E^T y,  W = M_b^-1 E
        if (n < 7) { err = "build_pcr_tables: periodic class with fewer than 7 unknowns"; return false; }
        const int e[6] = {0, 1, 2, n - 3, n - 2, n - 1};
        // W by banded Gaussian elimination (no pivoting: M_b is symmetric positive definite) in extended precision
        std::vector<pxr> band((size_t)n * 7), W((size_t)n * 6, 0.0L);
        for (int i = 0; i < n; i++)
            for (int d = -3; d <= 3; d++) band[(size_t)i * 7 + d + 3] = (i + d >= 0 && i + d < n) ? Mb(i, i + d) : 0.0L;
        for (int q = 0; q < 6; q++) W[(size_t)e[q] * 6 + q] = 1.0L;
        for (int k = 0; k < n; k++) {
            const pxr piv = band[(size_t)k * 7 + 3];
            if (!(piv > 0.0L)) { err = "build_pcr_tables: band part of the periodic matrix is not positive definite"; return false; }
            for (int i = k + 1; i <= std::min(n - 1, k + 3); i++) {
                const pxr f = band[(size_t)i * 7 + (k - i) + 3] / piv;
                if (f == 0.0L) continue;
                for (int j = k; j <= std::min(n - 1, k + 3); j++) band[(size_t)i * 7 + (j - i) + 3] -= f * band[(size_t)k * 7 + (j - k) + 3];
                for (int q = 0; q < 6; q++) W[(size_t)i * 6 + q] -= f * W[(size_t)k * 6 + q];
            }
        }
        for (int k = n - 1; k >= 0; k--)
            for (int q = 0; q < 6; q++) {
                pxr s = W[(size_t)k * 6 + q];
                for (int j = k + 1; j <= std::min(n - 1, k + 3); j++) s -= band[(size_t)k * 7 + (j - k) + 3] * W[(size_t)j * 6 + q];
                W[(size_t)k * 6 + q] = s / band[(size_t)k * 7 + 3];
            }
        pxr C[6][6], S[6][6], Si[6][6];
        for (int p = 0; p < 6; p++)
            for (int q = 0; q < 6; q++) C[p][q] = std::abs(e[p] - e[q]) > 3 ? Mc(e[p], e[q]) : 0.0L;
        for (int p = 0; p < 6; p++)
            for (int q = 0; q < 6; q++) {
                pxr s = p == q ? 1.0L : 0.0L;
                for (int k = 0; k < 6; k++) s += C[p][k] * W[(size_t)e[k] * 6 + q];
                S[p][q] = s;
                Si[p][q] = p == q ? 1.0L : 0.0L;
            }
        for (int c = 0; c < 6; c++) {            // Gauss-Jordan with partial pivoting, 6 x 6
            int piv = c;
            for (int r = c + 1; r < 6; r++) if (fabsl(S[r][c]) > fabsl(S[piv][c])) piv = r;
            if (S[piv][c] == 0.0L) { err = "build_pcr_tables: singular periodic correction"; return false; }
            for (int j = 0; j < 6; j++) { std::swap(S[piv][j], S[c][j]); std::swap(Si[piv][j], Si[c][j]); }
            const pxr d = 1.0L / S[c][c];
            for (int j = 0; j < 6; j++) { S[c][j] *= d; Si[c][j] *= d; }
            for (int r = 0; r < 6; r++) {
                if (r == c) continue;
                const pxr f = S[r][c];
                for (int j = 0; j < 6; j++) { S[r][j] -= f * S[c][j]; Si[r][j] -= f * Si[c][j]; }
            }
        }
        pxr SC[6][6];
        for (int p = 0; p < 6; p++)
            for (int q = 0; q < 6; q++) { pxr s = 0.0L; for (int k = 0; k < 6; k++) s += Si[p][k] * C[k][q]; SC[p][q] = s; }
        t.G.assign((size_t)np * 6, 0.0);
        for (int i = 0; i < n; i++)
            for (int q = 0; q < 6; q++) { pxr s = 0.0L; for (int k = 0; k < 6; k++) s += W[(size_t)i * 6 + k] * SC[k][q]; t.G[(size_t)i * 6 + q] = (double)s; }
    }
    return true;
}

void pcr_apply_host(const PcrTables &t, int nb, const double *b, double *a) {
    const int np = 3 * t.nblk;
    std::vector<double> r(np, 0.0), rn(np, 0.0);
    for (int j = 0; j < t.n; j++) {
        double s = 0.0;
        for (int q = 0; q < 4; q++) if (t.gin_row[(size_t)j * 4 + q] >= 0) s += t.gin_w[(size_t)j * 4 + q] * b[t.gin_row[(size_t)j * 4 + q]];
        r[j] = s;
    }
    for (int l = 0; l < t.levels; l++) {
        const int s = 1 << l;
        for (int i = 0; i < t.nblk; i++) {
            const double *c = t.coef.data() + ((size_t)l * t.nblk + i) * 18;
            for (int p = 0; p < 3; p++) {
                double v = r[3 * i + p];
                for (int q = 0; q < 3; q++) {
                    if (i - s >= 0) v -= c[p * 3 + q] * r[3 * (i - s) + q];
                    if (i + s < t.nblk) v -= c[9 + p * 3 + q] * r[3 * (i + s) + q];
                }
                rn[3 * i + p] = v;
            }
        }
        r.swap(rn);
    }
    std::vector<double> x(np, 0.0);
    for (int i = 0; i < t.nblk; i++)
        for (int p = 0; p < 3; p++) {
            double v = 0.0;
            for (int q = 0; q < 3; q++) v += t.dinv[(size_t)i * 9 + p * 3 + q] * r[3 * i + q];
            x[3 * i + p] = v;
        }
    if (t.periodic) {
        const int e[6] = {0, 1, 2, t.n - 3, t.n - 2, t.n - 1};
        double ye[6];
        for (int q = 0; q < 6; q++) ye[q] = x[e[q]];
        for (int i = 0; i < t.n; i++) {
            double v = x[i];
            for (int q = 0; q < 6; q++) v -= t.G[(size_t)i * 6 + q] * ye[q];
            x[i] = v;
        }
    }
    for (int m = 0; m < nb; m++) {
        double s = 0.0;
        for (int q = 0; q < 2; q++) if (t.gout_j[(size_t)m * 2 + q] >= 0) s += t.gout_w[(size_t)m * 2 + q] * x[t.gout_j[(size_t)m * 2 + q]];
        a[m] = s;
    }
}

void cholesky_apply_host(const SplineClass &sc, int nb, const double *b, double *a) {
    // dense statement of what k_solve computes: rhs = Gamma b, L L^T x = rhs with the class's factor rows, a = Gamma^T x
    const int n = sc.nfree;
    std::vector<long double> rhs(n, 0.0L), y(n), x(n);
    for (int j = 0; j < n; j++)
        for (auto &e : sc.Gam[j]) rhs[j] += (long double)e.second * b[e.first];
    auto Lf = [&](int i, int j) -> long double {          // factor entry (i >= j)
        if (i - j <= 3) return sc.Lband[(size_t)i * 4 + (3 - (i - j))];
        if (sc.periodic && i >= n - 3) return sc.Larrow[(size_t)(i - (n - 3)) * nb + j];
        return 0.0L;
    };
    for (int i = 0; i < n; i++) {
        long double s = rhs[i];
        for (int j = (sc.periodic && i >= n - 3) ? 0 : std::max(0, i - 3); j < i; j++) s -= Lf(i, j) * y[j];
        y[i] = s / Lf(i, i);
    }
    for (int i = n - 1; i >= 0; i--) {
        long double s = y[i];
        for (int j = i + 1; j < n; j++) {
            const long double l = Lf(j, i);
            if (l != 0.0L) s -= l * x[j];
        }
        x[i] = s / Lf(i, i);
    }
    for (int m = 0; m < nb; m++) a[m] = 0.0;
    for (int j = 0; j < n; j++)
        for (auto &e : sc.Gam[j]) a[e.first] += (double)((long double)e.second * x[j]);
}

// ---------------------------------------------------------------------------------------------- elliptic inversion
// The operators of sx_elliptic_solve (include/scythe_hip.h, "elliptic inversion"): the five 7-diagonal matrices of
// the patch's spline basis by Gauss-Legendre quadrature with 8 points per cell in extended precision (exact for S, M, N, M0; for
// T = int phi phi / r the rule is the definition), and per boundary-condition class and wavenumber the banded Cholesky factor of
// K_k = Gamma (S + k^2 T + alpha M) Gamma^T, worked out in extended precision and rounded once.

// nodes (on [-1, 1]) and weights of the 8-point Gauss-Legendre rule: Newton's iteration on P_8 in extended precision
static void gauss_legendre8(pxr x[8], pxr w[8]) {
    const int n = 8;
    const pxr PI = acosl(-1.0L);
    for (int i = 0; i < n; i++) {
        pxr z = cosl(PI * ((pxr)i + 0.75L) / ((pxr)n + 0.5L)), dp = 1.0L;
        for (int it = 0; it < 100; it++) {
            pxr p0 = 1.0L, p1 = z;
            for (int j = 2; j <= n; j++) { const pxr p2 = ((2 * j - 1) * z * p1 - (j - 1) * p0) / j; p0 = p1; p1 = p2; }
            dp = n * (z * p1 - p0) / (z * z - 1.0L);
            const pxr dz = p1 / dp;
            z -= dz;
            if (fabsl(dz) < 1e-19L) break;
        }
        pxr p0 = 1.0L, p1 = z;
        for (int j = 2; j <= n; j++) { const pxr p2 = ((2 * j - 1) * z * p1 - (j - 1) * p0) / j; p0 = p1; p1 = p2; }
        dp = n * (z * p1 - p0) / (z * z - 1.0L);
        x[i] = z;
        w[i] = 2.0L / ((1.0L - z * z) * dp * dp);
    }
}

void build_elliptic_bands(int has_l, double xmin, double xmax, int nc, EllBands &eb) {
    const int nb = nc + 3;
    eb.nb = nb;
    std::vector<pxr> *all[5] = {&eb.S, &eb.T, &eb.M, &eb.N, &eb.M0};
    for (auto *m : all) m->assign((size_t)nb * 7, 0.0L);
    pxr gx[8], gw[8];
    gauss_legendre8(gx, gw);
    const pxr DX = ((pxr)xmax - (pxr)xmin) / (pxr)nc;
    for (int c = 0; c < nc; c++)
        for (int q = 0; q < 8; q++) {
            const pxr t = 0.5L * (1.0L + gx[q]), r = (pxr)xmin + ((pxr)c + t) * DX, w = 0.5L * DX * gw[q];   // t: position in the cell
            const pxr J = has_l ? r : 1.0L;
            pxr ph[4], dph[4];
            for (int j = 0; j < 4; j++) { ph[j] = bspl<pxr>(t + 1.0L - j, 0); dph[j] = bspl<pxr>(t + 1.0L - j, 1) / DX; }   // node c + j
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) {
                    const size_t e = (size_t)(c + i) * 7 + (j - i + 3);
                    eb.S[e] += w * J * dph[i] * dph[j];
                    eb.M[e] += w * J * ph[i] * ph[j];
                    eb.M0[e] += w * ph[i] * ph[j];
                    eb.N[e] += w * r * ph[i] * dph[j];
                    if (has_l) eb.T[e] += w * ph[i] * ph[j] / r;
                }
        }
}

// the value of every constrained basis function (row of Gamma) at the left / right end of the patch is zero
static bool ell_vanishes(const std::vector<std::vector<std::pair<int, double>>> &G, int nb, bool right) {
    for (const auto &row : G) {
        pxr s = 0.0L;
        for (const auto &e : row) {
            const int d = right ? e.first - (nb - 2) : e.first - 1;     // node offset from the end node, in cells
            s += (pxr)e.second * bspl<pxr>((pxr)-d, 0);
        }
        if (fabsl(s) > 1e-12L) return false;
    }
    return true;
}

bool build_elliptic_class(const EllBands &eb, int has_l, double xmin, int bcl, int bcr, int k_lo, int k_hi, double alpha, EllClass &out,
                          std::string &err) {
    const int nb = eb.nb;
    if (bcl == SX_BC_PERIODIC || bcr == SX_BC_PERIODIC) { err = "PERIODIC radial boundary conditions on the solution variable are not supported"; return false; }
    SplineClass sc;
    sc.bcl = bcl; sc.bcr = bcr;
    sc.rl = bc_rank(bcl); sc.rr = bc_rank(bcr);
    if (sc.rl < 0 || sc.rr < 0 || !boundary_rows(bcl, sc.gl) || !boundary_rows(bcr, sc.gr)) { err = "unknown radial boundary condition code"; return false; }
    sc.nfree = nb - sc.rl - sc.rr;
    const int n = sc.nfree;
    if (n < 4) { err = "too few cells for the requested boundary conditions"; return false; }
    const auto G = gamma_rows(sc, nb);
    const bool zero_l = ell_vanishes(G, nb, false), zero_r = ell_vanishes(G, nb, true);
    if (k_lo == 0 && alpha == 0.0 && !zero_l && !zero_r) {
        err = "alpha = 0 with wavenumber-0 boundary conditions that fix the value on neither side: the problem is singular";
        return false;
    }
    if (has_l && xmin == 0.0 && k_hi >= 1 && !zero_l) {
        err = "the boundary conditions of wavenumbers k >= 1 do not make the solution vanish at r = 0: int phi phi / r has no meaning";
        return false;
    }
    out.bcl = bcl; out.bcr = bcr; out.n = n; out.rl = sc.rl; out.rr = sc.rr; out.k_lo = k_lo; out.k_hi = k_hi;
    std::memcpy(out.gl, sc.gl, sizeof(sc.gl));
    std::memcpy(out.gr, sc.gr, sizeof(sc.gr));
    out.Gam = G;
    out.L.assign((size_t)(k_hi - k_lo + 1) * nb * 4, 0.0);
    std::vector<pxr> Kb((size_t)n * 4), Lx((size_t)n * 4);       // [a][q]: entry (a, a - q), q = 0 .. 3
    for (int k = k_lo; k <= k_hi; k++) {
        const pxr k2 = (pxr)k * (pxr)k, al = (pxr)alpha;
        auto B = [&](int i, int j) -> pxr {
            const int d = j - i + 3;
            if (d < 0 || d > 6) return 0.0L;
            const size_t e = (size_t)i * 7 + d;
            return eb.S[e] + k2 * eb.T[e] + al * eb.M[e];
        };
        for (int a = 0; a < n; a++)
            for (int q = 0; q < 4; q++) {
                pxr s = 0.0L;
                if (a - q >= 0)
                    for (const auto &ia : G[a])
                        for (const auto &jb : G[a - q]) s += (pxr)ia.second * B(ia.first, jb.first) * (pxr)jb.second;
                Kb[(size_t)a * 4 + q] = s;
            }
        for (int j = 0; j < n; j++)
            for (int i = j; i <= std::min(j + 3, n - 1); i++) {
                pxr s = Kb[(size_t)i * 4 + (i - j)];
                for (int c = std::max(0, i - 3); c < j; c++) s -= Lx[(size_t)i * 4 + (i - c)] * Lx[(size_t)j * 4 + (j - c)];
                if (i == j) {
                    if (!(s > 0.0L)) { err = "the elliptic operator of wavenumber " + std::to_string(k) + " is not positive definite"; return false; }
                    Lx[(size_t)j * 4] = sqrtl(s);
                } else {
                    Lx[(size_t)i * 4 + (i - j)] = s / Lx[(size_t)j * 4];
                }
            }
        double *Lk = out.L.data() + (size_t)(k - k_lo) * nb * 4;
        for (int i = 0; i < n; i++) {
            for (int q = 1; q < 4; q++)
                if (i - q >= 0) Lk[(size_t)i * 4 + (3 - q)] = (double)Lx[(size_t)i * 4 + q];
            Lk[(size_t)i * 4 + 3] = (double)(1.0L / Lx[(size_t)i * 4]);
        }
    }
    return true;
}

// the arithmetic of k_elliptic from the right-hand side on (fold, the two sweeps, expand), operation by operation, on the host
void elliptic_apply_host(const EllClass &c, int k, int nb, const double *g, double *a) {
    const int n = c.n, rl = c.rl, rr = c.rr;
    const double *F = c.L.data() + (size_t)(k - c.k_lo) * nb * 4;
    double br0 = 0.0, br1 = 0.0, bl0 = 0.0, bl1 = 0.0;
    for (int q = 0; q < rr; q++) { br0 = std::fma(c.gr[q][0], g[nb - 1 - q], br0); br1 = std::fma(c.gr[q][1], g[nb - 1 - q], br1); }
    for (int q = 0; q < rl; q++) { bl0 = std::fma(c.gl[q][0], g[q], bl0); bl1 = std::fma(c.gl[q][1], g[q], bl1); }
    double y1 = 0.0, y2 = 0.0, y3 = 0.0;
    for (int i = 0; i < n; i++) {
        double s = g[rl + i];
        if (i == 0) s += bl0;
        if (i == 1) s += bl1;
        if (i == n - 1) s += br0;
        if (i == n - 2) s += br1;
        const double *l = F + (size_t)i * 4;
        double t = std::fma(-l[2], y1, -s);
        t = std::fma(-l[1], y2, t);
        t = std::fma(-l[0], y3, t);
        const double y = t * l[3];
        y3 = y2; y2 = y1; y1 = y;
        a[rl + i] = y;
    }
    double x1 = 0.0, x2 = 0.0, x3 = 0.0, xl0 = 0.0, xl1 = 0.0, xr0 = 0.0, xr1 = 0.0;
    const double zero[4] = {0.0, 0.0, 0.0, 0.0};
    const double *f1 = zero, *f2 = zero, *f3 = zero;
    for (int i = n - 1; i >= 0; i--) {
        const double *l = F + (size_t)i * 4;
        double t = std::fma(-f1[2], x1, a[rl + i]);
        t = std::fma(-f2[1], x2, t);
        t = std::fma(-f3[0], x3, t);
        const double x = t * l[3];
        x3 = x2; x2 = x1; x1 = x;
        f3 = f2; f2 = f1; f1 = l;
        a[rl + i] = x;
        if (i == 0) xl0 = x;
        if (i == 1) xl1 = x;
        if (i == n - 1) xr0 = x;
        if (i == n - 2) xr1 = x;
    }
    for (int q = 0; q < rl; q++) a[q] = std::fma(c.gl[q][1], xl1, c.gl[q][0] * xl0);
    for (int q = 0; q < rr; q++) a[nb - 1 - q] = std::fma(c.gr[q][1], xr1, c.gr[q][0] * xr0);
}

// ---------------------------------------------------------------------------------------------- antiderivatives
// The tables of sx_antiderivative along r (include/scythe_hip.h, "antiderivatives").  With Phi_j(r) = int_{xmin}^{r} w phi_j,
// c_j = int w phi_j and m_i = int phi_i over the patch,  b_i = int phi_i F dr = sum_j a_j int phi_i Phi_j.  phi_j lives on the four cells
// below node j + 2, so on the support of phi_i:  Phi_j = c_j for j <= i - 4 (phi_j ends before phi_i begins), Phi_j = 0 for j >= i + 4, and
// only |j - i| <= 3 needs the integral itself: a 7-diagonal band plus m_i times a running sum.  FROM_HIGH: Psi_j = c_j - Phi_j, the constant
// on the other side.
// Degrees: on a cell phi is a cubic and w phi of degree 3 (w = 1) or 4 (w = r), so Phi_j is of degree 4 or 5 there and phi_i Phi_j of
// degree 7 or 8.  The 8-point rule is exact up to degree 15: 8 points per cell for the outer integral, and the same rule on [cell start, r]
// for Phi_j at each of them (degree 4) - nothing is approximated; the entries carry the rounding of extended precision and are rounded
// to double once.
void build_antiderivative_tables(double xmin, double xmax, int nc, int origin, int weight, AntiTables &out) {
    const int nb = nc + 3;
    pxr gx[8], gw[8];
    gauss_legendre8(gx, gw);
    const pxr DX = ((pxr)xmax - (pxr)xmin) / (pxr)nc;
    auto phi = [](pxr t, int j) { return bspl<pxr>(t + 1.0L - j, 0); };       // node c + j at position t of cell c
    // int_0^t w phi_{c + j} over the first t of cell c (in r: the factor DX included)
    auto part = [&](int c, int j, pxr t) {
        pxr s = 0.0L;
        for (int q = 0; q < 8; q++) {
            const pxr u = 0.5L * t * (1.0L + gx[q]);
            const pxr r = (pxr)xmin + ((pxr)c + u) * DX;
            s += 0.5L * t * gw[q] * (weight == SX_INT_W_R ? r : 1.0L) * phi(u, j);
        }
        return s * DX;
    };
    std::vector<pxr> ctot(nb, 0.0L), mtot(nb, 0.0L), band((size_t)nb * 7, 0.0L);
    for (int c = 0; c < nc; c++)
        for (int j = 0; j < 4; j++) {
            ctot[c + j] += part(c, j, 1.0L);
            for (int q = 0; q < 8; q++) mtot[c + j] += 0.5L * DX * gw[q] * phi(0.5L * (1.0L + gx[q]), j);
        }
    std::vector<pxr> below(nb, 0.0L);           // int w phi_j over the cells below the current one
    for (int c = 0; c < nc; c++) {
        for (int q = 0; q < 8; q++) {
            const pxr t = 0.5L * (1.0L + gx[q]), wq = 0.5L * DX * gw[q];
            pxr here[4];
            for (int j = 0; j < 4; j++) here[j] = part(c, j, t);
            for (int il = 0; il < 4; il++) {
                const int i = c + il;
                const pxr pi = wq * phi(t, il);
                for (int j = std::max(0, i - 3); j <= std::min(nb - 1, i + 3); j++) {
                    pxr Phi = below[j] + ((j >= c && j <= c + 3) ? here[j - c] : 0.0L);
                    if (origin == SX_INT_FROM_HIGH) Phi = ctot[j] - Phi;
                    band[(size_t)i * 7 + (j - i + 3)] += pi * Phi;
                }
            }
        }
        for (int j = 0; j < 4; j++) below[c + j] += part(c, j, 1.0L);
    }
    out.nb = nb; out.origin = origin; out.weight = weight;
    out.P.assign((size_t)nb * 7, 0.0); out.c.assign(nb, 0.0); out.m.assign(nb, 0.0);
    for (int s = 0; s < nb; s++) {
        const int i = origin == SX_INT_FROM_HIGH ? nb - 1 - s : s;
        out.c[s] = (double)ctot[i];
        out.m[s] = (double)mtot[i];
        for (int d = 0; d < 7; d++) out.P[(size_t)s * 7 + d] = (double)band[(size_t)i * 7 + (origin == SX_INT_FROM_HIGH ? 6 - d : d)];
    }
}

// The projection that goes with the exact right-hand side: Gamma (P + eps_q Q) Gamma^T with P[i][j] = int phi_i phi_j the exact Gram matrix
// (build_elliptic_bands' M0) - NOT build_spline_class's P, whose 3-point weights 8 : 5 : 8 define the model's discrete inner product and
// pair only with right-hand sides formed by the same rule (its diagonal is 0.355 DX where int phi phi is 0.336 DX) - and Q[i][j] =
// int phi_i''' phi_j''' (phi''' is constant on a cell: any rule is exact) with the class's own eps_q = (l_q DX / 2 pi)^6, Gamma and ranks.
// Banded Cholesky in extended precision, rounded once: F [nb][4] = L[i][i - 3], L[i][i - 2], L[i][i - 1], 1 / L[i][i].
bool build_antiderivative_class(double xmin, double xmax, int nc, double l_q, int bcl, int bcr, SplineClass &sc, std::vector<double> &F,
                                std::string &err) {
    const int nb = nc + 3;
    if (bcl == SX_BC_PERIODIC || bcr == SX_BC_PERIODIC) { err = "PERIODIC radial boundary conditions on the destination variable are not supported"; return false; }
    sc = SplineClass();
    sc.bcl = bcl; sc.bcr = bcr;
    sc.rl = bc_rank(bcl); sc.rr = bc_rank(bcr);
    if (sc.rl < 0 || sc.rr < 0 || !boundary_rows(bcl, sc.gl) || !boundary_rows(bcr, sc.gr)) { err = "unknown radial boundary condition code"; return false; }
    sc.nfree = nb - sc.rl - sc.rr;
    const int n = sc.nfree;
    if (n < 4) { err = "too few cells for the requested boundary conditions"; return false; }
    sc.Gam = gamma_rows(sc, nb);
    EllBands eb;
    build_elliptic_bands(0, xmin, xmax, nc, eb);
    const pxr DX = ((pxr)xmax - (pxr)xmin) / (pxr)nc, PI = acosl(-1.0L);
    pxr eps_q = (pxr)l_q * DX / (2.0L * PI);
    eps_q = eps_q * eps_q * eps_q; eps_q = eps_q * eps_q;
    std::vector<pxr> B((size_t)nb * 7, 0.0L);
    for (int c = 0; c < nc; c++)
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++)
                B[(size_t)(c + i) * 7 + (j - i + 3)] += DX * bspl<pxr>(1.5L - i, 3) * bspl<pxr>(1.5L - j, 3) / (DX * DX * DX * DX * DX * DX);
    for (size_t e = 0; e < B.size(); e++) B[e] = eb.M0[e] + eps_q * B[e];
    auto Bm = [&](int i, int j) -> pxr { const int d = j - i + 3; return (d < 0 || d > 6) ? 0.0L : B[(size_t)i * 7 + d]; };
    std::vector<pxr> Kb((size_t)n * 4), Lx((size_t)n * 4, 0.0L);       // [a][q]: entry (a, a - q), q = 0 .. 3
    for (int a = 0; a < n; a++)
        for (int q = 0; q < 4; q++) {
            pxr s = 0.0L;
            if (a - q >= 0)
                for (const auto &ia : sc.Gam[a])
                    for (const auto &jb : sc.Gam[a - q]) s += (pxr)ia.second * Bm(ia.first, jb.first) * (pxr)jb.second;
            Kb[(size_t)a * 4 + q] = s;
        }
    for (int j = 0; j < n; j++)
        for (int i = j; i <= std::min(j + 3, n - 1); i++) {
            pxr s = Kb[(size_t)i * 4 + (i - j)];
            for (int c = std::max(0, i - 3); c < j; c++) s -= Lx[(size_t)i * 4 + (i - c)] * Lx[(size_t)j * 4 + (j - c)];
            if (i == j) {
                if (!(s > 0.0L)) { err = "the projection matrix of the destination variable is not positive definite"; return false; }
                Lx[(size_t)j * 4] = sqrtl(s);
            } else {
                Lx[(size_t)i * 4 + (i - j)] = s / Lx[(size_t)j * 4];
            }
        }
    F.assign((size_t)nb * 4, 0.0);
    for (int i = 0; i < n; i++) {
        for (int q = 1; q < 4; q++)
            if (i - q >= 0) F[(size_t)i * 4 + (3 - q)] = (double)Lx[(size_t)i * 4 + q];
        F[(size_t)i * 4 + 3] = (double)(1.0L / Lx[(size_t)i * 4]);
    }
    return true;
}

void antiderivative_r_host(const AntiTables &t, const SplineClass &sc, const double *F, const double *a_src, double *a) {
    const int nb = t.nb, n = sc.nfree, rl = sc.rl, rr = sc.rr;
    const bool high = t.origin == SX_INT_FROM_HIGH;
    auto row = [&](int s) { return high ? nb - 1 - s : s; };
    auto ld = [&](int s) { return s >= 0 && s < nb ? a_src[row(s)] : 0.0; };
    // the right-hand side in walk order: band product of the 7-row window, plus m times the sum of what has left the window
    double w[7], S = 0.0;
    for (int d = 0; d < 7; d++) w[d] = ld(d - 3);
    for (int s = 0; s < nb; s++) {
        double acc = 0.0;
        for (int d = 0; d < 7; d++) acc = std::fma(t.P[(size_t)s * 7 + d], w[d], acc);
        a[row(s)] = std::fma(t.m[s], S, acc);
        S = std::fma(s >= 3 ? t.c[s - 3] : 0.0, w[0], S);
        for (int d = 0; d < 6; d++) w[d] = w[d + 1];
        w[6] = ld(s + 4);
    }
    // fold with Gamma, L y = Gamma b, L^T x = y, a = Gamma^T x
    double br0 = 0.0, br1 = 0.0, bl0 = 0.0, bl1 = 0.0;
    for (int q = 0; q < rr; q++) { br0 = std::fma(sc.gr[q][0], a[nb - 1 - q], br0); br1 = std::fma(sc.gr[q][1], a[nb - 1 - q], br1); }
    for (int q = 0; q < rl; q++) { bl0 = std::fma(sc.gl[q][0], a[q], bl0); bl1 = std::fma(sc.gl[q][1], a[q], bl1); }
    double y1 = 0.0, y2 = 0.0, y3 = 0.0;
    for (int i = 0; i < n; i++) {
        double s = a[rl + i];
        if (i == 0) s += bl0;
        if (i == 1) s += bl1;
        if (i == n - 1) s += br0;
        if (i == n - 2) s += br1;
        const double *l = F + (size_t)i * 4;
        double v = std::fma(-l[2], y1, s);
        v = std::fma(-l[1], y2, v);
        v = std::fma(-l[0], y3, v);
        const double y = v * l[3];
        y3 = y2; y2 = y1; y1 = y;
        a[rl + i] = y;
    }
    double x1 = 0.0, x2 = 0.0, x3 = 0.0, xl0 = 0.0, xl1 = 0.0, xr0 = 0.0, xr1 = 0.0;
    const double zero[4] = {0.0, 0.0, 0.0, 0.0};
    const double *f1 = zero, *f2 = zero, *f3 = zero;
    for (int i = n - 1; i >= 0; i--) {
        const double *l = F + (size_t)i * 4;
        double v = std::fma(-f1[2], x1, a[rl + i]);
        v = std::fma(-f2[1], x2, v);
        v = std::fma(-f3[0], x3, v);
        const double x = v * l[3];
        x3 = x2; x2 = x1; x1 = x;
        f3 = f2; f2 = f1; f1 = l;
        a[rl + i] = x;
        if (i == 0) xl0 = x;
        if (i == 1) xl1 = x;
        if (i == n - 1) xr0 = x;
        if (i == n - 2) xr1 = x;
    }
    for (int q = 0; q < rl; q++) a[q] = std::fma(sc.gl[q][1], xl1, sc.gl[q][0] * xl0);
    for (int q = 0; q < rr; q++) a[nb - 1 - q] = std::fma(sc.gr[q][1], xr1, sc.gr[q][0] * xr0);
}

// ---------------------------------------------------------------------------------------------- Chebyshev
// The collocation operators are assembled in extended precision and rounded to double once at the end: the
// second-derivative matrix has entries O(N^4 / Lz^2), and products of double-rounded factors would carry a relative
// error of cond * eps into every step (visible as ~1e-9 field differences at zDim = 128).
typedef long double xreal;
typedef std::vector<xreal> xmat;

static void matmul(const xmat &A, const xmat &B, xmat &Cm, int n, int k, int m) {
    Cm.assign((size_t)n * m, 0.0L);
    for (int i = 0; i < n; i++)
        for (int p = 0; p < k; p++) {
            xreal a = A[(size_t)i * k + p];
            if (a == 0.0L) continue;
            for (int j = 0; j < m; j++) Cm[(size_t)i * m + j] += a * B[(size_t)p * m + j];
        }
}

static std::vector<double> to_double(const xmat &A) { return std::vector<double>(A.begin(), A.end()); }

struct ChebX {       // extended-precision factors shared by build_cheb_ops and build_helmholtz
    xmat T, Dc, TD, TDD;
};

static void cheb_factors(double zmin, double zmax, int N, ChebX &x) {
    const xreal PI = 4.0L * atanl(1.0L);
    const xreal Lz = (xreal)zmax - (xreal)zmin;
    x.T.assign((size_t)N * N, 0.0L);
    for (int n = 0; n < N; n++)
        for (int k = 0; k < N; k++)
            x.T[(size_t)n * N + k] = ((k == 0 || k == N - 1) ? 1.0L : 2.0L) * cosl((xreal)((long)n * k) * PI / (xreal)(N - 1));
    // coefficient-space derivative: ax_{k-1} = ax_{k+1} + k c_k with c_k = 2 a_k (interior), a_{N-1} (last)
    x.Dc.assign((size_t)N * N, 0.0L);
    std::vector<xreal> ax(N + 2);
    for (int j = 0; j < N; j++) {
        std::fill(ax.begin(), ax.end(), 0.0L);
        for (int k = N - 1; k >= 1; k--) {
            xreal ck = (k == j) ? ((k == N - 1) ? 1.0L : 2.0L) : 0.0L;
            ax[k - 1] = ax[k + 1] + k * ck;
        }
        for (int i = 0; i < N; i++) x.Dc[(size_t)i * N + j] = ax[i] * (-2.0L / Lz);
    }
    matmul(x.T, x.Dc, x.TD, N, N, N);
    matmul(x.TD, x.Dc, x.TDD, N, N, N);
}

// b -> a: padding to N coefficients and the projection onto the boundary conditions (bcb, bct), [N][Zb]
static bool cheb_ca(const ChebX &x, int N, int Zb, int bcb, int bct, xmat &CA, std::string &err) {
    // BC projection (orthogonal projection onto the null space of the constraint rows)
    std::vector<std::vector<xreal>> rows;
    const int bcs[2] = {bcb, bct}, rix[2] = {0, N - 1};
    for (int s = 0; s < 2; s++) {
        const xmat *src = nullptr;
        switch (bcs[s]) {
            case SX_BC_R0: continue;
            case SX_BC_R1T0: src = &x.T; break;
            case SX_BC_R1T1: src = &x.TD; break;
            case SX_BC_R1T2: src = &x.TDD; break;
            default: err = "unsupported vertical boundary condition"; return false;
        }
        rows.emplace_back(src->begin() + (size_t)rix[s] * N, src->begin() + (size_t)(rix[s] + 1) * N);
    }
    xmat proj((size_t)N * N, 0.0L);
    for (int i = 0; i < N; i++) proj[(size_t)i * N + i] = 1.0L;
    if (!rows.empty()) {
        const int m = (int)rows.size();
        xreal G[2][2] = {{0, 0}, {0, 0}}, Gi[2][2] = {{0, 0}, {0, 0}};
        for (int a = 0; a < m; a++)
            for (int b = 0; b < m; b++)
                for (int k = 0; k < N; k++) G[a][b] += rows[a][k] * rows[b][k];
        if (m == 1) {
            Gi[0][0] = 1.0L / G[0][0];
        } else {
            xreal det = G[0][0] * G[1][1] - G[0][1] * G[1][0];
            Gi[0][0] = G[1][1] / det; Gi[0][1] = -G[0][1] / det; Gi[1][0] = -G[1][0] / det; Gi[1][1] = G[0][0] / det;
        }
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) {
                xreal s = 0.0L;
                for (int a = 0; a < m; a++)
                    for (int b = 0; b < m; b++) s += rows[a][i] * Gi[a][b] * rows[b][j];
                proj[(size_t)i * N + j] -= s;
            }
    }
    CA.assign((size_t)N * Zb, 0.0L);
    for (int i = 0; i < N; i++)
        for (int k = 0; k < Zb; k++) CA[(size_t)i * Zb + k] = proj[(size_t)i * N + k];
    return true;
}

static void cheb_integral(int N, xreal Lz, xmat &Ic);

bool build_cheb_ops(double zmin, double zmax, int nz, int Zb, int bcb, int bct, ChebOps &o, std::string &err) {
    if (nz < 4) { err = "zDim must be >= 4"; return false; }
    o.bcb = bcb;
    o.bct = bct;
    const int N = nz;
    const xreal PI = 4.0L * atanl(1.0L);
    const xreal Lz = (xreal)zmax - (xreal)zmin;
    o.z.resize(N);
    for (int n = 0; n < N; n++) o.z[n] = std::cos(n * M_PI / (N - 1)) * (-0.5 * (zmax - zmin)) + 0.5 * (zmin + zmax);
    (void)PI;
    ChebX x;
    cheb_factors(zmin, zmax, N, x);
    xmat CB((size_t)Zb * N);
    for (int k = 0; k < Zb; k++)
        for (int n = 0; n < N; n++) CB[(size_t)k * N + n] = x.T[(size_t)k * N + n] / (2.0L * (N - 1));
    xmat Ic;
    cheb_integral(N, Lz, Ic);
    xmat CA;
    if (!cheb_ca(x, N, Zb, bcb, bct, CA, err)) return false;
    xmat M0, M1, M2, TI, TICA, Mint, Mdz, Mrec, Mdzz;
    matmul(x.T, CA, M0, N, N, Zb);
    matmul(x.TD, CA, M1, N, N, Zb);
    matmul(x.TDD, CA, M2, N, N, Zb);
    matmul(x.T, Ic, TI, N, N, N);
    matmul(TI, CA, TICA, N, N, Zb);
    matmul(TICA, CB, Mint, N, Zb, N);
    matmul(M1, CB, Mdz, N, Zb, N);
    matmul(M0, CB, Mrec, N, Zb, N);
    matmul(M2, CB, Mdzz, N, Zb, N);
    o.T = to_double(x.T); o.Dc = to_double(x.Dc); o.CB = to_double(CB); o.CA = to_double(CA);
    o.M[0] = to_double(M0); o.M[1] = to_double(M1); o.M[2] = to_double(M2);
    o.Mint = to_double(Mint); o.Mdz = to_double(Mdz); o.Mrec = to_double(Mrec); o.Mdzz = to_double(Mdzz);
    o.zmin = zmin; o.zmax = zmax;
    return true;
}

// coefficient-space integral [N][N], zero at the bottom (x = +1 where every T_k = 1)
static void cheb_integral(int N, xreal Lz, xmat &Ic) {
    Ic.assign((size_t)N * N, 0.0L);
    std::vector<xreal> ai(N);
    for (int j = 0; j < N; j++) {
        std::fill(ai.begin(), ai.end(), 0.0L);
        auto a = [&](int k) { return k == j ? 1.0L : 0.0L; };
        for (int k = 1; k < N - 1; k++) {
            xreal up = (k + 1 < N - 1) ? a(k + 1) : 0.5L * a(k + 1);
            ai[k] = (a(k - 1) - up) / (2.0L * k);
        }
        ai[N - 1] = a(N - 2) / (xreal)(N - 1);
        xreal s = 0.0L;
        for (int k = 1; k < N; k++) {
            ai[k] *= (-0.5L * Lz);
            s += (k == N - 1 ? 1.0L : 2.0L) * ai[k];
        }
        ai[0] = -s;
        for (int i = 0; i < N; i++) Ic[(size_t)i * N + j] = ai[i];
    }
}

// The operator of sx_antiderivative along z in coefficient space (include/scythe_hip.h, "antiderivatives"): the truncated b
// coefficients of the source -> those of F.  V = T Ic CA [N][Zb] holds F(z_n) = int_{zmin}^{z_n} per unit source coefficient (ChebOps::Mint
// before its CB); FROM_HIGH takes F(zmax) - F(z_n), the top level being row N - 1; Z = CB V.  Returned transposed and zero-padded, as
// k_antiderivative_z reads its operator fragments.
bool build_antiderivative_z(double zmin, double zmax, int nz, int Zb, int bcb, int bct, int origin, std::vector<double> &ZT, int &Kp, int &Mp,
                            std::string &err) {
    if (nz < 4) { err = "zDim must be >= 4"; return false; }
    const int N = nz;
    ChebX x;
    cheb_factors(zmin, zmax, N, x);
    xmat Ic, CA, TI, V, Z, CB((size_t)Zb * N);
    cheb_integral(N, (xreal)zmax - (xreal)zmin, Ic);
    if (!cheb_ca(x, N, Zb, bcb, bct, CA, err)) return false;
    for (int k = 0; k < Zb; k++)
        for (int n = 0; n < N; n++) CB[(size_t)k * N + n] = x.T[(size_t)k * N + n] / (2.0L * (N - 1));
    matmul(x.T, Ic, TI, N, N, N);
    matmul(TI, CA, V, N, N, Zb);
    if (origin == SX_INT_FROM_HIGH)
        for (int n = 0; n < N; n++)         // the top row last: it becomes zero
            for (int k = 0; k < Zb; k++) V[(size_t)n * Zb + k] = V[(size_t)(N - 1) * Zb + k] - V[(size_t)n * Zb + k];
    matmul(CB, V, Z, Zb, N, Zb);
    Kp = (Zb + 3) & ~3; Mp = (Zb + 15) & ~15;
    ZT.assign((size_t)Kp * Mp, 0.0);
    for (int i = 0; i < Zb; i++)
        for (int k = 0; k < Zb; k++) ZT[(size_t)k * Mp + i] = (double)Z[(size_t)i * Zb + k];
    return true;
}

bool build_helmholtz(const ChebOps &w, double pxi_bar, double tau, std::vector<double> &Wmat, std::vector<double> &Xmat,
                     std::string &err) {
    const int N = (int)w.z.size();
    const xreal c = (xreal)tau * (xreal)tau * (xreal)pxi_bar;
    ChebX x;
    cheb_factors(w.zmin, w.zmax, N, x);
    // H = [c T[0,:]; c T[N-1,:]; (c TDD - T)[1..N-2, :]]   (src/semiimplicit.jl:776-779)
    xmat H((size_t)N * N), Inv((size_t)N * N, 0.0L);
    for (int j = 0; j < N; j++) {
        H[j] = c * x.T[j];
        H[(size_t)N + j] = c * x.T[(size_t)(N - 1) * N + j];
        for (int i = 1; i < N - 1; i++) H[(size_t)(i + 1) * N + j] = c * x.TDD[(size_t)i * N + j] - x.T[(size_t)i * N + j];
    }
    for (int i = 0; i < N; i++) Inv[(size_t)i * N + i] = 1.0L;
    // Gauss-Jordan with partial pivoting in extended precision (the reference factorises in double, :780)
    for (int col = 0; col < N; col++) {
        int piv = col;
        for (int r = col + 1; r < N; r++)
            if (fabsl(H[(size_t)r * N + col]) > fabsl(H[(size_t)piv * N + col])) piv = r;
        if (H[(size_t)piv * N + col] == 0.0L) { err = "singular Helmholtz matrix"; return false; }
        if (piv != col)
            for (int j = 0; j < N; j++) {
                std::swap(H[(size_t)piv * N + j], H[(size_t)col * N + j]);
                std::swap(Inv[(size_t)piv * N + j], Inv[(size_t)col * N + j]);
            }
        xreal d = 1.0L / H[(size_t)col * N + col];
        for (int j = 0; j < N; j++) { H[(size_t)col * N + j] *= d; Inv[(size_t)col * N + j] *= d; }
        for (int r = 0; r < N; r++) {
            if (r == col) continue;
            xreal f = H[(size_t)r * N + col];
            if (f == 0.0L) continue;
            for (int j = 0; j < N; j++) {
                H[(size_t)r * N + j] -= f * H[(size_t)col * N + j];
                Inv[(size_t)r * N + j] -= f * Inv[(size_t)col * N + j];
            }
        }
    }
    xmat W, X;
    matmul(x.T, Inv, W, N, N, N);
    matmul(x.TD, Inv, X, N, N, N);
    Wmat = to_double(W);
    Xmat = to_double(X);
    return true;
}

// ---------------------------------------------------------------------------------------------- evaluation at arbitrary points
// The weights sx_evaluate's kernel applies and sx_eval_basis returns (sx_eval.hip), formed in extended precision from the Float64
// coordinate and rounded once.

// what every pure host helper refuses of a descriptor
bool desc_ok(const sx_grid_desc *gd, const char *who) {
    if (!gd) { set_error(std::string(who) + ": null argument"); return false; }
    if (gd->abi_version != SX_ABI_VERSION) { set_error("sx_grid_desc.abi_version mismatch"); return false; }
    if (gd->geometry < SX_GEOM_R || gd->geometry > SX_GEOM_RLZ) { set_error("Unknown geometry"); return false; }
    if (gd->num_cells < 3 || gd->nvars < 1 || !(gd->xmax > gd->xmin)) { set_error("invalid grid parameters"); return false; }
    if (gd->tile_cell0 < 0 || gd->tile_num_cells < 1 || gd->tile_cell0 + gd->tile_num_cells > gd->num_cells) { set_error("tile range outside the patch"); return false; }
    return true;
}

EvalGeom desc_geom(const sx_grid_desc *gd) {
    EvalGeom g;
    g.has_l = gd->geometry == SX_GEOM_RL || gd->geometry == SX_GEOM_RLZ;
    g.has_z = gd->geometry == SX_GEOM_RZ || gd->geometry == SX_GEOM_RLZ;
    g.nc = gd->num_cells; g.cell0 = gd->tile_cell0; g.ncells = gd->tile_num_cells;
    g.uniform_L = g.has_l ? gd->ring_uniform_L : 0;
    g.xmin = gd->xmin; g.xmax = gd->xmax; g.DX = (gd->xmax - gd->xmin) / gd->num_cells;
    for (int r = 0; r < MUBAR * g.nc; r++) {
        int L, km;
        double off;
        ring_table(g.has_l, g.uniform_L, r + 1, L, km, off);
        g.kDim = std::max(g.kDim, km);
    }
    if (g.has_z) {
        g.nz = gd->zDim;
        g.Zb = gd->b_zDim > 0 ? gd->b_zDim : default_bzdim(gd->zDim);
        g.zmin = gd->zmin; g.zmax = gd->zmax;
    }
    return g;
}

EvalGeom eval_geom_of(const sx_handle *h) {
    EvalGeom g;
    g.has_l = h->has_l; g.has_z = h->has_z; g.nc = h->nc; g.cell0 = h->cell0; g.ncells = h->ncells; g.uniform_L = h->uniform_L;
    g.kDim = h->kDim; g.nz = h->nz; g.Zb = h->Zb; g.xmin = h->xmin; g.xmax = h->xmax; g.DX = h->DX; g.zmin = h->zmin; g.zmax = h->zmax;
    return g;
}

sx_grid_desc desc_of(const sx_handle *h) {
    sx_grid_desc gd = {};
    gd.abi_version = SX_ABI_VERSION; gd.geometry = h->geom; gd.xmin = h->xmin; gd.xmax = h->xmax; gd.num_cells = h->nc; gd.nvars = h->V;
    gd.tile_cell0 = h->cell0; gd.tile_num_cells = h->ncells; gd.zDim = h->nz; gd.b_zDim = h->Zb;
    return gd;
}

// SX_EVAL_RING_K: kmax of the last patch ring at or below r (ring 1 below the first); SX_EVAL_ALL_K: the patch's kDim
static int eval_kcap(const EvalGeom &g, double r, int flags) {
    if (!g.has_l) return 0;
    if (flags == SX_EVAL_ALL_K) return g.kDim;
    const double t = (r - g.xmin) / g.DX;
    const int c = std::min(std::max((int)std::floor(t), 0), g.nc - 1);
    // a ring radius is printed as xmin + DX (c + 0.5 + offset): a few ulp of what went into t absorb its rounding on the way back
    const double tol = 4.0 * 2.220446049250313e-16 * (std::fabs(t) + 1.0 + std::max(std::fabs(g.xmin), std::fabs(g.xmax)) / g.DX);
    int cnt = 0;
    for (int mu = 0; mu < MUBAR; mu++)
        if (0.5 + gauss_offset(mu) <= t - c + tol) cnt++;
    const int ring = std::max(MUBAR * c + cnt - 1, 0);
    int L, kmax;
    double off;
    ring_table(1, g.uniform_L, ring + 1, L, kmax, off);
    return kmax;
}

// One radius as the kernels' point records hold it.  wr [3][4]: phi, phi', phi'' of the 4 nodes that overlap the cell of r (tile
// cells only: the tile's A rows are the ones the handle holds); cell = the patch row of the first node; kcap = eval_kcap
void eval_radial_pt(const EvalGeom &g, double r, int flags, double (&wr)[12], int &cell, int &kcap) {
    int c = (int)std::floor((r - g.xmin) / g.DX);
    c = std::min(std::max(c, g.cell0), g.cell0 + g.ncells - 1);
    cell = c;
    const xreal DX = (xreal)g.DX;
    for (int j = 0; j < 4; j++) {
        const xreal delta = ((xreal)r - ((xreal)g.xmin + (xreal)(c - 1 + j) * DX)) / DX;
        xreal sc = 1.0L;
        for (int d = 0; d < 3; d++, sc *= DX) wr[4 * d + j] = (double)(bspl<xreal>(delta, d) / sc);
    }
    kcap = eval_kcap(g, r, flags);
}

std::vector<double> cheb_dc(double zmin, double zmax, int nz) {
    ChebX x;
    cheb_factors(zmin, zmax, nz, x);
    return to_double(x.Dc);
}

// CA, Dc CA, Dc Dc CA of a vertical boundary-condition class, [nz][Zb] each, kept in extended precision
bool build_eval_vert(double zmin, double zmax, int nz, int Zb, int bcb, int bct, EvalVert &o, std::string &err) {
    if (nz < 4) { err = "zDim must be >= 4"; return false; }
    ChebX x;
    cheb_factors(zmin, zmax, nz, x);
    xmat CA, DCA, DDCA;
    if (!cheb_ca(x, nz, Zb, bcb, bct, CA, err)) return false;
    matmul(x.Dc, CA, DCA, nz, nz, Zb);
    matmul(x.Dc, DCA, DDCA, nz, nz, Zb);
    o.bcb = bcb; o.bct = bct;
    o.W[0] = CA; o.W[1] = DCA; o.W[2] = DDCA;
    return true;
}

// rows of the b -> (value, d/dz, d2/dz2) operator at z: the DCT-I series a0 + 2 sum a_k T_k(x) + a_{N-1} T_{N-1}(x) at
// x = (z - mid) / (-Lz / 2) applied to a = CA b and to its coefficient-space derivatives; w [3][Zb]
void eval_vert_weights(const EvalVert &ev, double zmin, double zmax, int nz, int Zb, double z, double *w) {
    const xreal mid = ((xreal)zmin + (xreal)zmax) / 2.0L, half = ((xreal)zmax - (xreal)zmin) / 2.0L;
    xreal x = ((xreal)z - mid) / (-half);
    x = std::min(std::max(x, (xreal)-1.0L), (xreal)1.0L);
    const xreal th = acosl(x);
    std::vector<xreal> t(nz);
    for (int n = 0; n < nz; n++) t[n] = ((n == 0 || n == nz - 1) ? 1.0L : 2.0L) * cosl((xreal)n * th);
    for (int s = 0; s < 3; s++)
        for (int k = 0; k < Zb; k++) {
            xreal acc = 0.0L;
            for (int n = 0; n < nz; n++) acc += t[n] * ev.W[s][(size_t)n * Zb + k];
            w[(size_t)s * Zb + k] = (double)acc;
        }
}

std::vector<double> height_tiles(const std::vector<EvalVert> &vert, const double *heights, int n, double zmin, double zmax, int nz, int Zb) {
    const bool has_z = !vert.empty();
    if (!has_z) { n = 1; Zb = 1; }
    const int ncls = has_z ? (int)vert.size() : 1, nht = (n + 15) / 16, Zp = (Zb + 3) & ~3;
    std::vector<double> wz((size_t)ncls * nht * 3 * Zp * 16, 0.0), w3((size_t)3 * Zb, 0.0);
    w3[0] = 1.0;
    for (int c = 0; c < ncls; c++)
        for (int zj = 0; zj < n; zj++) {
            if (has_z) eval_vert_weights(vert[c], zmin, zmax, nz, Zb, heights[zj], w3.data());
            for (int row = 0; row < 3; row++)
                for (int zm = 0; zm < Zb; zm++)
                    wz[((((size_t)c * nht + zj / 16) * 3 + row) * Zp + zm) * 16 + zj % 16] = w3[(size_t)row * Zb + zm];
        }
    return wz;
}

// ---------------------------------------------------------------------------------------------- quadrature weights of sx_reduce
// The weights of the domain integral (include/scythe_hip.h, "integrals and azimuthal means"), formed in extended precision and
// rounded once; any output pointer may be null.  w_r[ring] = DX (5, 8, 5) / 18 J(r): 3-point Gauss-Legendre on the cell, whose nodes
// the tile's radial gridpoints are (NOT quad_weights' 8:5:8 projection weights, which do not integrate x^2), J = r - the double
// sx_get_gridpoints returns - with an azimuth and 1 without.  w_l[ring] = 2 pi / L, 1 without an azimuth.  w_z[level] =
// Clenshaw-Curtis weights of the nz Chebyshev-Gauss-Lobatto levels times (zmax - zmin) / 2 (symmetric: bottom-first and top-first agree).
void reduce_weights(const EvalGeom &g, double *w_r, double *w_l, double *w_z) {
    const xreal DX = ((xreal)g.xmax - (xreal)g.xmin) / (xreal)g.nc, PI = acosl(-1.0L);
    for (int i = 0; i < MUBAR * g.ncells; i++) {
        const int mu = i % MUBAR, c = g.cell0 + i / MUBAR;
        const double r = g.xmin + g.DX * (c + 0.5 + gauss_offset(mu));
        int L, km;
        double off;
        ring_table(g.has_l, g.uniform_L, MUBAR * g.cell0 + i + 1, L, km, off);
        if (w_r) w_r[i] = (double)(DX * (xreal)(mu == 1 ? 8 : 5) / 18.0L * (g.has_l ? (xreal)r : 1.0L));
        if (w_l) w_l[i] = g.has_l ? (double)(2.0L * PI / (xreal)L) : 1.0;
    }
    if (w_z && g.has_z) {
        const int n = g.nz - 1;
        const xreal half = ((xreal)g.zmax - (xreal)g.zmin) / 2.0L;
        for (int j = 0; j <= n; j++) {
            xreal s = 1.0L;
            for (int k = 1; 2 * k <= n; k++)
                s -= (2 * k == n ? 1.0L : 2.0L) / (xreal)(4 * k * k - 1) * cosl(2.0L * (xreal)k * (xreal)j * PI / (xreal)n);
            w_z[j] = (double)(((j == 0 || j == n) ? 1.0L : 2.0L) / (xreal)n * s * half);
        }
    }
}

void ring_table(int has_l, int uniform_L, int ri, int &L, int &kmax, double &off) {
    if (!has_l) { L = 1; kmax = 0; off = 0.0; return; }
    if (uniform_L > 0) {
        L = uniform_L;
        kmax = ri < uniform_L / 2 - 1 ? ri : uniform_L / 2 - 1;
        off = 0.0;
    } else {
        L = 4 + 4 * ri;
        kmax = ri;
        off = 0.5 * (2.0 * M_PI / L) * (ri - 1);
    }
}

}  // namespace sx
