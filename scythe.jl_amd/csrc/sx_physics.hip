// Equation sets (gfx950): the tendencies of every model, explicit_timestep, semiimplicit_adjustment and condensation_adjustment,
// and their launchers.  Each formula that more than one kernel needs is stated once, as a __forceinline__ function in the
// grouping of the reference; the library is built with -ffp-contract=off, so a call rounds exactly as the inline text would.
// Data layout: sx_kernels.hip.
#include "sx_internal.hpp"
#include "sx_thermo.hpp"

namespace sx {

template <class ST>
struct PhysArgsT {
    Planes<ST> P;         // physical
    double *En;           // expdot_n  [V][N]
    double *E1, *E2;      // expdot_nm1 / nm2 (read)
    double *In;           // impdot_n
    double *np1;          // var_np1
    const double *r, *cosl, *sinl, *z;
    const double *MintT, *MdzT;
    int64_t N;
    int V, nz, t, eq;
    int s_u, s_r, s_rr, s_l, s_ll, s_z, s_zz;
    double ts;
    double par[SX_NPARAMS];
    // column range of this launch and, for the node-space variant, the node transforms G [slot][v][NG] + basis weights
    int64_t col0, col1;
    Planes<ST> G;
    const double *phi;
    const double *ref;    // ReferenceState [3][3][nz] (Euler_test)
    int write_w;          // store the diagnostic w into physical[:, 6, 1] (src/shallowWaterModels.jl:66-67, 426-429): only the
                          // stand-alone sx_physics needs it there; inside sx_advance nothing reads that plane again
    int64_t NG;
    int L, nrings;
    CellConsts cc;        // cell-independent constants of the cell-wise kernel (sx_internal.hpp)
    long long *dbg;       // phase stamps [workgroup][8] of the diagnostic build (-DSX_PHASES, profiles/phases.sh); otherwise null
};

// A diagnostic variable has expdot == 0 for ever (src/shallowWaterModels.jl:69, 185, 430): explicit_timestep reduces to
// var_np1 = value, and its (all-zero) tendency history is neither read nor written.
template <class A>
__device__ __forceinline__ void diag_step(const A &a, int v, int64_t p, double u) { a.np1[(int64_t)v * a.N + p] = u; }

// explicit_timestep: ab_value (sx_internal.hpp, shared with the parcel kernel) with its loads and stores; history arrays are rotated by the host instead of copied
template <class A>
__device__ __forceinline__ double ab_step(const A &a, int v, int64_t p, double u, double en) {
    const int64_t o = (int64_t)v * a.N + p;
    a.En[o] = en;
    // each order reads the history it uses and no more (before step 3 the older buffers hold none)
    const double un = a.t == 1 ? ab_value(1, a.ts, u, en, 0.0, 0.0)
                    : a.t == 2 ? ab_value(2, a.ts, u, en, a.E1[o], 0.0)
                               : ab_value(3, a.ts, u, en, a.E1[o], a.E2[o]);
    a.np1[o] = un;
    return un;
}

// ---- formulas of the shallow-water sets, each stated once.  Radius policy: the reference divides by r and r^2, and so do
// k_phys_hrbl and the slab sets; 22 divisions per point would make the matrix-core kernels VALU-bound (an f64 division is ~25
// instructions), so they multiply by a reciprocal formed once per thread (differs from the reference's a / r by <= 1.5 ulp).
struct DivR {
    double r;
    __device__ __forceinline__ double over_r(double x) const { return x / r; }
    __device__ __forceinline__ double over_r2(double x) const { return x / (r * r); }
};
struct MulRinv {
    double ri, ri2;
    __device__ __forceinline__ static MulRinv of(double ri) { return MulRinv{ri, ri * ri}; }
    __device__ __forceinline__ double over_r(double x) const { return x * ri; }
    __device__ __forceinline__ double over_r2(double x) const { return x * ri2; }
};

// free-layer tendencies of h, ug, vg (src/shallowWaterModels.jl:60-108, 176-228, 346-511); the Twoway set adds its S1 term to e0
template <class R>
__device__ __forceinline__ void sw_free_layer(const R &q, double g, double Hfree, double f, double h, double hr, double hl, double ug,
                                              double ugr, double ugl, double vg, double vgr, double vgl, double &e0, double &e1,
                                              double &e2) {
    e0 = (q.over_r(-vg * hl) + (-ug * hr)) + (-(Hfree + h) * (q.over_r(ug) + ugr + q.over_r(vgl)));
    e1 = (q.over_r(-vg * ugl) + (-ug * ugr)) + (-g * hr) + (vg * (f + q.over_r(vg)));
    e2 = (q.over_r(-vg * vgl) + (-ug * vgr)) + (-g * q.over_r(hl)) + (-ug * (f + q.over_r(vg)));
}

// boundary-layer tendencies of ub, vb of the height-resolved set: wb, vdu, vdv are the results of the three column operators
template <class R>
__device__ __forceinline__ void hrbl_boundary_layer(const R &q, double g, double Kh, double f, double hr, double hl, double ub, double ubr,
                                                    double ubrr, double ubl, double ubll, double ubz, double vb, double vbr, double vbrr,
                                                    double vbl, double vbll, double vbz, double wb, double vdu, double vdv, double &e3,
                                                    double &e4) {
    e3 = (q.over_r(-vb * ubl) + (-ub * ubr) + (-wb * ubz)) + (-g * hr) + (vb * (f + q.over_r(vb))) + vdu +
         (Kh * (q.over_r(ubr) + ubrr - q.over_r2(ub) + q.over_r2(ubll) - q.over_r2(2.0 * vbl)));
    e4 = (q.over_r(-vb * vbl) + (-ub * vbr) + (-wb * vbz)) + (-g * q.over_r(hl)) + (-ub * (f + q.over_r(vb))) + vdv +
         (Kh * (q.over_r(vbr) + vbrr - q.over_r2(vb) + q.over_r2(vbll) + q.over_r2(2.0 * ubl)));
}

// inputs of the column operators: the divergence (integrated to wb) and the fluxes Kv du/dz with Kv = l^2 S
__device__ __forceinline__ double mixing_length(double z) { return 1.0 / ((1.0 / (0.4 * z)) + (1.0 / 80.0)); }
template <class R>
__device__ __forceinline__ void hrbl_column_inputs(const R &q, double l, double ub, double ubr, double vbl, double ubz, double vbz,
                                                   double &div, double &fu, double &fv) {
    const double S = sqrt((ubz * ubz) + (vbz * vbz));
    const double Kv = (l * l) * S;
    div = -(q.over_r(ub) + ubr + q.over_r(vbl));
    fu = Kv * ubz;
    fv = Kv * vbz;
}

// surface drag replaces the level-0 fluxes (src/shallowWaterModels.jl:463-482): ub1, vb1 are the winds at level 1 ("10 m")
__device__ __forceinline__ void surface_drag(const double *par, double cs, double sn, double ub1, double vb1, double &fu, double &fv) {
    const double Um = par[SX_P_UM], Vm = par[SX_P_VM];
    const double sfcu = (Um * cs) + (Vm * sn), sfcv = (Vm * cs) - (Um * sn);
    const double u10 = ub1 + sfcu, v10 = vb1 + sfcv;
    const double U10 = sqrt(u10 * u10 + v10 * v10);
    double Cd = par[SX_P_CD];
    if (U10 < 5.2) Cd = 1.0e-3;
    else if (U10 < 33.6) Cd = 4.4e-4 * sqrt(U10);
    fu = Cd * U10 * u10;
    fv = Cd * U10 * v10;
}

// value of variable v / derivative slot s (>= 1) of variable v at point p
#define PSV(v) a.P.val[(int64_t)(v) * a.N + p]

// What Euler_test and rainfall_test share: the six ReferenceState rows they read (of sbar, sbar_z, sbar_zz, xibar, xibar_z,
// xibar_zz, mubar, mubar_z, mubar_zz) at level k, and the moist state both derive from them and from s, xi, mu.  rho_t differs
// between the two sets (1 + q_v against 1 + q_t) and stays with them.
struct MoistState {
    double sbar, sbar_z, xibar, xibar_z, mubar, mubar_z;
    double q_v, rho_d, Tk, dmudq, qvp_x, qvp_z, rhobar;
    __device__ __forceinline__ MoistState(const double *ref, int nz, int k, double s, double xi, double mu, double mu_x, double mu_z)
        : sbar(ref[k]), sbar_z(ref[nz + k]), xibar(ref[3 * nz + k]), xibar_z(ref[4 * nz + k]), mubar(ref[6 * nz + k]),
          mubar_z(ref[7 * nz + k]) {
        q_v = thermo::ahyp(mu + mubar);
        rho_d = thermo::dry_density(xi + xibar);
        Tk = thermo::temperature(s + sbar, rho_d, q_v);
        dmudq = thermo::dmudq(mu + mubar, q_v);
        qvp_x = mu_x / dmudq;
        qvp_z = mu_z / dmudq;
        rhobar = thermo::dry_density(xibar) * (1.0 + thermo::ahyp(mubar));
    }
};

#define PS(v, s) ((double)a.P.der[((int64_t)((s) - 1) * a.V + (v)) * a.N + p])

template <class ST>
__global__ void k_phys_pointwise(PhysArgsT<ST> a) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.N) return;
    const double *par = a.par;
    const double r = a.r[p / a.nz];
    switch (a.eq) {
        case SX_EQ_NONE:
            for (int v = 0; v < a.V; v++) a.np1[(int64_t)v * a.N + p] = PSV(v);
            return;
        case SX_EQ_LINEAR_ADVECTION_1D: {      // src/testModels.jl:15
            const double e = -(par[SX_P_C0] * PS(0, a.s_r)) + (par[SX_P_K] * PS(0, a.s_rr));
            ab_step(a, 0, p, PSV(0), e);
            for (int v = 1; v < a.V; v++) ab_step(a, v, p, PSV(v), 0.0);
        } break;
        case SX_EQ_LINEAR_ADVECTION_RZ: {      // src/testModels.jl:40
            const double hr = PS(0, a.s_r);
            const double e = (-PSV(1) * hr) + (-PSV(3) * PS(0, a.s_z)) +
                             (par[SX_P_K] * ((hr / r) + PS(0, a.s_rr) + PS(0, a.s_zz)));
            ab_step(a, 0, p, PSV(0), e);
            for (int v = 1; v < a.V; v++) ab_step(a, v, p, PSV(v), 0.0);
        } break;
        case SX_EQ_LINEAR_ADVECTION_RL:        // src/testModels.jl:62-68
        case SX_EQ_LINEAR_ADVECTION_RLZ: {     // src/testModels.jl:93
            const double hr = PS(0, a.s_r), hl = PS(0, a.s_l);
            double e = (-PSV(1) * hr) - (PSV(2) * (hl / r));
            if (a.eq == SX_EQ_LINEAR_ADVECTION_RLZ || par[SX_P_K] > 0.0)
                e += par[SX_P_K] * ((hr / r) + PS(0, a.s_rr) + (PS(0, a.s_ll) / (r * r)));
            ab_step(a, 0, p, PSV(0), e);
            for (int v = 1; v < a.V; v++) ab_step(a, v, p, PSV(v), 0.0);
        } break;
        case SX_EQ_ONEWAY_SW_SLAB:             // src/shallowWaterModels.jl:60-108
        case SX_EQ_TWOWAY_SW_SLAB: {           // src/shallowWaterModels.jl:176-228
            const double g = par[SX_P_G], K = par[SX_P_K], Cd = par[SX_P_CD], Hfree = par[SX_P_HFREE],
                         Hb = par[SX_P_HB], f = par[SX_P_F];
            const double h = PSV(0), hr = PS(0, a.s_r), hl = PS(0, a.s_l);
            const double ug = PSV(1), ugr = PS(1, a.s_r), ugl = PS(1, a.s_l);
            const double vg = PSV(2), vgr = PS(2, a.s_r), vgl = PS(2, a.s_l);
            const double ub = PSV(3), ubr = PS(3, a.s_r), ubrr = PS(3, a.s_rr), ubl = PS(3, a.s_l), ubll = PS(3, a.s_ll);
            const double vb = PSV(4), vbr = PS(4, a.s_r), vbrr = PS(4, a.s_rr), vbl = PS(4, a.s_l), vbll = PS(4, a.s_ll);
            const double U = 0.78 * sqrt((ub * ub) + (vb * vb));
            const double w = -Hb * ((ub / r) + ubr + (vbl / r));
            if (a.write_w) a.P.val[(int64_t)5 * a.N + p] = w;
            const double w_ = 0.5 * fabs(w) - w;
            double e0, e1, e2;
            sw_free_layer(DivR{r}, g, Hfree, f, h, hr, hl, ug, ugr, ugl, vg, vgr, vgl, e0, e1, e2);
            if (a.eq == SX_EQ_TWOWAY_SW_SLAB) e0 += -(Hfree + h) * w * par[SX_P_S1];
            const double e3 = ((-vb * ubl / r) + (-ub * ubr)) + (-g * hr) + (vb * (f + (vb / r))) + (-(Cd * U * ub / Hb)) +
                              (w_ * (ug - ub) / Hb) +
                              (K * ((ubr / r) + ubrr - (ub / (r * r)) + (ubll / (r * r)) - (2.0 * vbl / (r * r))));
            const double e4 = ((-vb * vbl / r) + (-ub * vbr)) + (-g * (hl / r)) + (-ub * (f + (vb / r))) + (-(Cd * U * vb / Hb)) +
                              (w_ * (vg - vb) / Hb) +
                              (K * ((vbr / r) + vbrr - (vb / (r * r)) + (vbll / (r * r)) + (2.0 * ubl / (r * r))));
            ab_step(a, 0, p, h, e0);
            ab_step(a, 1, p, ug, e1);
            ab_step(a, 2, p, vg, e2);
            ab_step(a, 3, p, ub, e3);
            ab_step(a, 4, p, vb, e4);
            diag_step(a, 5, p, w);
            for (int v = 6; v < a.V; v++) ab_step(a, v, p, PSV(v), 0.0);
        } break;
        case SX_EQ_LINEAR_ACOUSTIC_RZ: {
            const double K = par[SX_P_K], pxi = par[SX_P_PXI_BAR];
            const double u = PSV(3), w = PSV(4);
            double e[5];
            for (int v = 0; v < 5; v++) e[v] = (-u * PS(v, a.s_r)) + (-w * PS(v, a.s_z));
            const double d0 = K * (PS(0, a.s_rr) + PS(0, a.s_zz)), d2 = K * (PS(2, a.s_rr) + PS(2, a.s_zz));
            const double d3 = K * (PS(3, a.s_rr) + PS(3, a.s_zz)), d4 = K * (PS(4, a.s_rr) + PS(4, a.s_zz));
            const double xir = PS(1, a.s_r), xiz = PS(1, a.s_z), wz = PS(4, a.s_z);
            e[0] = e[0] + d0;
            e[1] = e[1] - PS(3, a.s_r) - wz;
            e[2] = e[2] + d2;
            e[3] = e[3] + (-(pxi * xir)) + d3;
            e[4] = e[4] + (-(pxi * xiz)) + d4;
            for (int v = 0; v < 5; v++) {
                ab_step(a, v, p, PSV(v), e[v]);
                if (a.In) a.In[(int64_t)v * a.N + p] = (v == 1) ? -wz : (v == 4) ? -(pxi * xiz) : 0.0;
            }
        } break;
        case SX_EQ_EULER_TEST: {               // src/testModels.jl:100-215
            const double K = par[SX_P_K], pxi = par[SX_P_PXI_BAR];
            const double s_x = PS(0, a.s_r), s_z = PS(0, a.s_z), xi_x = PS(1, a.s_r), xi_z = PS(1, a.s_z);
            const double mu = PSV(2), mu_x = PS(2, a.s_r), mu_z = PS(2, a.s_z);
            const double u = PSV(3), u_x = PS(3, a.s_r), u_z = PS(3, a.s_z), w = PSV(4), w_x = PS(4, a.s_r), w_z = PS(4, a.s_z);
            const MoistState m(a.ref, a.nz, (int)(p % a.nz), PSV(0), PSV(1), mu, mu_x, mu_z);
            const double q_v = m.q_v, rho_d = m.rho_d, Tk = m.Tk, qvp_x = m.qvp_x, qvp_z = m.qvp_z;
            const double rho_t = rho_d * (1.0 + q_v);
            const double rho_p = rho_t - m.rhobar;
            double e[5];
            e[0] = ((-u * s_x) + (-w * (s_z + m.sbar_z))) + (K * (PS(0, a.s_rr) + PS(0, a.s_zz)));
            e[1] = ((-u * xi_x) + (-w * (xi_z + m.xibar_z))) - u_x - w_z;
            e[2] = ((-u * mu_x) + (-w * (mu_z + m.mubar_z))) + (K * (PS(2, a.s_rr) + PS(2, a.s_zz)));
            e[3] = ((-u * u_x) + (-w * u_z)) + (-(thermo::pressure_gradient(Tk, rho_d, q_v, s_x, xi_x, qvp_x) / rho_t)) +
                   (K * (PS(3, a.s_rr) + PS(3, a.s_zz)));
            e[4] = ((-u * w_x) + (-w * w_z)) +
                   (-(thermo::gravity * rho_p / rho_t) - (thermo::pressure_gradient(Tk, rho_d, q_v, s_z, xi_z, qvp_z) / rho_t)) +
                   (K * (PS(4, a.s_rr) + PS(4, a.s_zz)));
            for (int v = 0; v < 5; v++) {
                ab_step(a, v, p, PSV(v), e[v]);
                if (a.In) a.In[(int64_t)v * a.N + p] = (v == 1) ? -w_z : (v == 4) ? -(pxi * xi_z) : 0.0;      // impdot: only kept when semi-implicit
            }
            for (int v = 5; v < a.V; v++) ab_step(a, v, p, PSV(v), 0.0);
        } break;
        case SX_EQ_LINEAR_SW_1D: {             // src/shallowWaterModels.jl:235-259
            const double g = par[SX_P_G], K = par[SX_P_K], H = par[SX_P_H];
            const double e0 = -H * PS(1, a.s_r);
            const double e1 = (-g * PS(0, a.s_r)) + (K * PS(1, a.s_rr));
            ab_step(a, 0, p, PSV(0), e0);
            ab_step(a, 1, p, PSV(1), e1);
            for (int v = 2; v < a.V; v++) ab_step(a, v, p, PSV(v), 0.0);
        } break;
        case SX_EQ_LINEAR_SW_RL: {             // src/shallowWaterModels.jl:261-298 (no -u / r^2 term, unlike the slab sets)
            const double g = par[SX_P_G], K = par[SX_P_K], H = par[SX_P_H];
            const double u = PSV(1), ur = PS(1, a.s_r), urr = PS(1, a.s_rr), ull = PS(1, a.s_ll);
            const double vr = PS(2, a.s_r), vrr = PS(2, a.s_rr), vl = PS(2, a.s_l), vll = PS(2, a.s_ll);
            const double e0 = -H * ((u / r) + ur + (vl / r));
            const double e1 = (-g * PS(0, a.s_r)) + (K * ((ur / r) + urr + (ull / (r * r))));
            const double e2 = (-g * (PS(0, a.s_l) / r)) + (K * ((vr / r) + vrr + (vll / (r * r))));
            ab_step(a, 0, p, PSV(0), e0);
            ab_step(a, 1, p, u, e1);
            ab_step(a, 2, p, PSV(2), e2);
            for (int v = 3; v < a.V; v++) ab_step(a, v, p, PSV(v), 0.0);
        } break;
        default: break;
    }
}

// rainfall_test (src/testModels.jl:387-585): Euler_test with Ooyama (2001) warm rain; variables s, xi, mu, u, w, mu_c, mu_r, qss by
// position.  A kernel of its own so that this exp / log / pow chain leaves the register allocation of k_phys_pointwise alone.
// condensation_adjustment follows in k_condensation, after the semi-implicit step.
template <class ST>
__global__ void __launch_bounds__(256) k_phys_rain(PhysArgsT<ST> a) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.N) return;
    const double *par = a.par;
    const double K = par[SX_P_K], Pxi_bar = par[SX_P_PXI_BAR];
    const double N_c = 100.0, r_c = 10.0;                  // :500-501
    const double s = PSV(0), s_x = PS(0, a.s_r), s_z = PS(0, a.s_z);
    const double xi = PSV(1), xi_x = PS(1, a.s_r), xi_z = PS(1, a.s_z);
    const double mu = PSV(2), mu_x = PS(2, a.s_r), mu_z = PS(2, a.s_z);
    const double u = PSV(3), u_x = PS(3, a.s_r), u_z = PS(3, a.s_z);
    const double w = PSV(4), w_x = PS(4, a.s_r), w_z = PS(4, a.s_z);
    const double mu_c = PSV(5), mu_r = PSV(6), qss = PSV(7);

    const MoistState m(a.ref, a.nz, (int)(p % a.nz), s, xi, mu, mu_x, mu_z);
    const double q_v = m.q_v, rho_d = m.rho_d, Tk = m.Tk, mu_factor = m.dmudq, qvp_x = m.qvp_x, qvp_z = m.qvp_z, rhobar = m.rhobar;
    const double pr = thermo::pressure(Tk, rho_d, q_v);
    const double q_c = thermo::ahyp(mu_c), q_r = thermo::ahyp(mu_r);
    const double q_l = q_c + q_r, q_t = q_v + q_l;
    const double rho_t = rho_d * (1.0 + q_t);
    const double rho_p = rho_t - rhobar;
    const double dpdx = thermo::pressure_gradient(Tk, rho_d, q_v, s_x, xi_x, qvp_x);
    const double dpdz = thermo::pressure_gradient(Tk, rho_d, q_v, s_z, xi_z, qvp_z);

    const double Cm = (q_l * thermo::Cl) / (thermo::Cvd + (q_v * thermo::Cvv) + (q_l * thermo::Cl));
    const double s_div = Cm * (thermo::Rd + q_v * thermo::Rv) * (u_x + w_z);
    const double q_cond = thermo::q_condensation(qss, Tk, pr, q_v, q_l, N_c, r_c);
    const double s_cond = thermo::s_condensation(q_cond, Tk, rho_d, q_v, q_l, pr);
    const double cloudtau = thermo::invtau_condensation(Tk, pr, N_c, r_c);
    const double raintau = thermo::rain_evaporation(q_r, rho_d, Tk, pr);
    const double q_evap = -qss * raintau;
    const double qss_cond = thermo::dqsdp(Tk, pr, rho_d, q_v, q_l) * ((u * dpdx) + (w * (dpdz - rhobar * thermo::gravity))) -
                            qss * (cloudtau + raintau);
    const double q_auto = thermo::autoconversion(q_c, rho_d);
    const double q_coll = thermo::collection(q_c, q_r, rho_d, Tk);
    // No sedimentation term: Vt_flux = CIx(q_r .* Vt) ./ rho_d (:524-528) is identically zero because sedimentation clamps its
    // Vt = -14.164 rho_r^0.1364 (rho_d0 / rho_d)^0.5 f_ice(Tk) <= 0 at 0 from below (src/microphysics.jl:252-261), so no column
    // operator is built for it

    double e[8];
    e[0] = (((-u * s_x) + (-w * (s_z + m.sbar_z))) + (s_cond + s_div)) + (K * (PS(0, a.s_rr) + PS(0, a.s_zz)));
    e[1] = ((-u * xi_x) + (-w * (xi_z + m.xibar_z))) + (-u_x - w_z);
    e[2] = (((-u * mu_x) + (-w * (mu_z + m.mubar_z))) + (mu_factor * (q_evap - q_cond))) + (K * (PS(2, a.s_rr) + PS(2, a.s_zz)));
    e[3] = (((-u * u_x) + (-w * u_z)) + (-dpdx / rho_t)) + (K * (PS(3, a.s_rr) + PS(3, a.s_zz)));
    e[4] = (((-u * w_x) + (-w * w_z)) + (((-thermo::gravity * rho_p) - dpdz) / rho_t)) + (K * (PS(4, a.s_rr) + PS(4, a.s_zz)));
    e[5] = (((-u * PS(5, a.s_r)) + (-w * PS(5, a.s_z))) + (thermo::dmudq(mu_c, q_c) * (q_cond - q_auto - q_coll))) +
           (K * (PS(5, a.s_rr) + PS(5, a.s_zz)));
    e[6] = (((-u * PS(6, a.s_r)) + (-w * PS(6, a.s_z))) + (thermo::dmudq(mu_r, q_r) * (q_auto + q_coll - q_evap))) +
           (K * (PS(6, a.s_rr) + PS(6, a.s_zz)));
    e[7] = ((-u * PS(7, a.s_r)) + (-w * PS(7, a.s_z))) + qss_cond;
    const double vals[8] = {s, xi, mu, u, w, mu_c, mu_r, qss};
    for (int v = 0; v < 8; v++) ab_step(a, v, p, vals[v], e[v]);
    for (int v = 8; v < a.V; v++) ab_step(a, v, p, PSV(v), 0.0);
    if (a.In) {            // impdot: only kept when semi-implicit; mu and qss hold q_v and qss for the reference's (unused) history
        for (int v = 0; v < a.V; v++)
            a.In[(int64_t)v * a.N + p] = (v == 1) ? -w_z : (v == 2) ? q_v : (v == 4) ? -(Pxi_bar * xi_z) : (v == 7) ? qss : 0.0;
    }
}

// Oneway_ShallowWater_HeightResolvedBL (src/shallowWaterModels.jl:346-511). One workgroup handles `cpb` columns;
// thread (c, k) owns level k of column c. The three per-column Chebyshev operators (integral of the divergence,
// derivative of the two vertical fluxes) are dense nz x nz mat-vecs with the operands staged in LDS.
template <class ST>
__global__ void __launch_bounds__(256) k_phys_hrbl(PhysArgsT<ST> a, int cpb) {
    extern __shared__ double sm[];
    const int nz = a.nz;
    const int k = threadIdx.x % nz, cl = threadIdx.x / nz;
    const int64_t col = (int64_t)blockIdx.x * cpb + cl;
    const int64_t ncol = a.N / nz;
    const bool live = (cl < cpb) && (col < ncol);
    double *sdiv = sm, *sfu = sm + (size_t)cpb * nz, *sfv = sm + (size_t)2 * cpb * nz;
    double *sub = sm + (size_t)3 * cpb * nz, *svb = sm + (size_t)4 * cpb * nz;
    const double *par = a.par;
    const double g = par[SX_P_G], Kh = par[SX_P_KH], Hfree = par[SX_P_HFREE], f = par[SX_P_F];
    const int64_t p = live ? col * nz + k : 0;
    double r = 1.0, h = 0, hr = 0, hl = 0, ug = 0, ugr = 0, ugl = 0, vg = 0, vgr = 0, vgl = 0;
    double ub = 0, ubr = 0, ubrr = 0, ubl = 0, ubll = 0, ubz = 0, vb = 0, vbr = 0, vbrr = 0, vbl = 0, vbll = 0, vbz = 0;
    if (live) {
        r = a.r[col];
        h = PSV(0); hr = PS(0, a.s_r); hl = PS(0, a.s_l);
        ug = PSV(1); ugr = PS(1, a.s_r); ugl = PS(1, a.s_l);
        vg = PSV(2); vgr = PS(2, a.s_r); vgl = PS(2, a.s_l);
        ub = PSV(3); ubr = PS(3, a.s_r); ubrr = PS(3, a.s_rr); ubl = PS(3, a.s_l); ubll = PS(3, a.s_ll); ubz = PS(3, a.s_z);
        vb = PSV(4); vbr = PS(4, a.s_r); vbrr = PS(4, a.s_rr); vbl = PS(4, a.s_l); vbll = PS(4, a.s_ll); vbz = PS(4, a.s_z);
        hrbl_column_inputs(DivR{r}, mixing_length(a.z[k]), ub, ubr, vbl, ubz, vbz, sdiv[cl * nz + k], sfu[cl * nz + k], sfv[cl * nz + k]);
        sub[cl * nz + k] = ub;
        svb[cl * nz + k] = vb;
    }
    __syncthreads();
    if (live && k == 0) surface_drag(par, a.cosl[col], a.sinl[col], sub[cl * nz + 1], svb[cl * nz + 1], sfu[cl * nz], sfv[cl * nz]);
    __syncthreads();
    if (!live) return;
    double wb = 0.0, vdu = 0.0, vdv = 0.0;
    const double *xd = sdiv + cl * nz, *xu = sfu + cl * nz, *xv = sfv + cl * nz;
    for (int j = 0; j < nz; j++) {
        const double mi = a.MintT[(int64_t)j * nz + k], md = a.MdzT[(int64_t)j * nz + k];
        wb += mi * xd[j];
        vdu += md * xu[j];
        vdv += md * xv[j];
    }
    if (a.write_w) a.P.val[(int64_t)5 * a.N + p] = wb;
    double e0, e1, e2, e3, e4;
    sw_free_layer(DivR{r}, g, Hfree, f, h, hr, hl, ug, ugr, ugl, vg, vgr, vgl, e0, e1, e2);
    hrbl_boundary_layer(DivR{r}, g, Kh, f, hr, hl, ub, ubr, ubrr, ubl, ubll, ubz, vb, vbr, vbrr, vbl, vbll, vbz, wb, vdu, vdv, e3, e4);
    ab_step(a, 0, p, h, e0);
    ab_step(a, 1, p, ug, e1);
    ab_step(a, 2, p, vg, e2);
    ab_step(a, 3, p, ub, e3);
    ab_step(a, 4, p, vb, e4);
    diag_step(a, 5, p, wb);
    for (int v = 6; v < a.V; v++) ab_step(a, v, p, PSV(v), 0.0);
}

// MFMA variant of the same equation set for zDim = NZ (multiple of 16): 16 columns per workgroup. The three column
// operators are genuine contractions  Y[NZ x 16] = M[NZ x NZ] * X[NZ x 16]  and run on the f64 matrix cores
// (v_mfma_f64_16x16x4_f64): wave w < 12 owns (operand w / 4, row tile w % 4); A comes straight from the
// (L2-resident) operator, B and the result tiles live in LDS, column-major with a 2-double pad (bank-conflict free).
typedef double mfma_d4 __attribute__((ext_vector_type(4)));

// 16 bytes per lane for streams that are 8 bytes per point.  A wave owns 64 consecutive doubles of every stream; lanes
// 0-31 fetch TWO consecutive elements of stream a, lanes 32-63 of stream b (one global_load_dwordx4 instead of two
// dwordx2), and one v_permlane32_swap per dword leaves (a[e], b[e]) in every lane with e = 2 (lane & 31) + (lane >> 5) -
// which is therefore the element (level) a lane works on.  Stores run the same exchange backwards.  The load and the
// exchange are SEPARATE steps (RawPair): an exchange right behind its load makes the wave wait for that load alone, and a
// handful of such round trips in a row was most of this kernel's time (phase stamps, profiles/r02/phases_*.txt).
typedef double dbl2v __attribute__((ext_vector_type(2)));
typedef float flt2v __attribute__((ext_vector_type(2)));
template <class T> struct Vec2;
template <> struct Vec2<double> { typedef dbl2v type; };
template <> struct Vec2<float> { typedef flt2v type; };
__device__ __forceinline__ int wide_elem(int lane) { return 2 * (lane & 31) + (lane >> 5); }

// pa / pb point at the lane's pair of stream a / b
template <bool NT, class T>
__device__ __forceinline__ typename Vec2<T>::type issue_pair(const T *pa, const T *pb, int lane) {
    typedef typename Vec2<T>::type V;
    const V *p = reinterpret_cast<const V *>(lane < 32 ? pa : pb);
    return NT ? __builtin_nontemporal_load(p) : *p;
}
__device__ __forceinline__ void take_pair(dbl2v t, double &xa, double &xb) {
    const auto r0 = __builtin_amdgcn_permlane32_swap(__double2loint(t.x), __double2loint(t.y), false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(__double2hiint(t.x), __double2hiint(t.y), false, false);
    xa = __hiloint2double(r1[0], r0[0]);
    xb = __hiloint2double(r1[1], r0[1]);
}
__device__ __forceinline__ void take_pair(flt2v t, double &xa, double &xb) {
    const auto r0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(t.x), __float_as_uint(t.y), false, false);
    xa = (double)__uint_as_float(r0[0]);
    xb = (double)__uint_as_float(r0[1]);
}
// every lane hands over its element of streams a and b; lanes 0-31 then store two consecutive elements of a, lanes 32-63 of b
__device__ __forceinline__ void store_pair_nt(double *pa, double *pb, int lane, double xa, double xb) {
    const auto r0 = __builtin_amdgcn_permlane32_swap(__double2loint(xa), __double2loint(xb), false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(__double2hiint(xa), __double2hiint(xb), false, false);
    dbl2v t;
    t.x = __hiloint2double(r1[0], r0[0]);
    t.y = __hiloint2double(r1[1], r0[1]);
    __builtin_nontemporal_store(t, reinterpret_cast<dbl2v *>(lane < 32 ? pa : pb));
}

// In-kernel phase stamps (s_memtime) of the diagnostic build only; the stamps go to a buffer nothing else reads.
#ifdef SX_PHASES
#define SX_STAMP(i) do { if (threadIdx.x == 0 && a.dbg) a.dbg[(int64_t)blockIdx.x * 8 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define SX_STAMP(i) do { } while (0)
#endif
// keeps the loads in front of it in front of the loads behind it (the memory counter retires in issue order: what is
// needed first must be issued first)
#define SX_LOAD_FENCE() asm volatile("" ::: "memory")

// CPB columns per workgroup (<= 16, the MFMA tile width).  Used for the rings on the ring-wise path (all of them without
// the node-space inverse, the inner ones with it; k_phys_hrbl_cell takes the rest).
// Load discipline as in k_phys_hrbl_cell: one burst at entry, oldest = needed first (the memory counter retires in issue
// order); the tendency history and the second half of the planes are consumed only after the column operators; all operator
// fragments of a wave's jobs are requested before its first MFMA.  WIDE: 16-byte-per-lane pairs (issue_pair / take_pair).
template <int NZ, int CPB, class ST, bool WIDE>
__global__ void __launch_bounds__(CPB * NZ, 4) k_phys_hrbl_mfma(PhysArgsT<ST> a) {      // 4 waves per SIMD: <= 128 VGPRs, two 512-thread workgroups per CU
    constexpr int CS = NZ + 2;                     // column stride in LDS
    __shared__ double X[3][16 * CS];               // div, Kv*ubz, Kv*vbz   -> inputs (columns >= CPB unused)
    // wb, d/dz(...), d/dz(...) -> outputs.  At zDim = 128 the two tile sets would exceed the 64 KB of static LDS: the results
    // then wait in the accumulators until every wave has finished reading X and are written over it.
    constexpr bool ALIAS = (NZ > 64);
    __shared__ double Ysep[ALIAS ? 1 : 3][ALIAS ? 1 : 16 * CS];
    double (*Y)[16 * CS] = ALIAS ? X : reinterpret_cast<double (*)[16 * CS]>(&Ysep[0][0]);
    __shared__ double s1[2][16];                   // ub, vb at level 1 ("10 m")
    const int lane = threadIdx.x & 63, wbase = threadIdx.x & ~63;
    const int elem = WIDE ? wbase + wide_elem(lane) : (int)threadIdx.x;      // element of the workgroup's CPB x NZ block
    const int k = elem % NZ, cl = elem / NZ;
    const int64_t col = a.col0 + (int64_t)blockIdx.x * CPB + cl;
    const bool live = col < a.col1;
    const double *par = a.par;
    const double g = par[SX_P_G], Kh = par[SX_P_KH], Hfree = par[SX_P_HFREE], f = par[SX_P_F];
    const int64_t p = live ? col * NZ + k : 0;
    // this lane's PAIR (elements 2i, 2i + 1 of the wave's 64: same column as its own element since NZ is even)
    const int64_t pw = live ? (a.col0 + (int64_t)blockIdx.x * CPB) * NZ + wbase + 2 * (lane & 31) : 0;
    typedef typename Vec2<ST>::type SV;
    double xd = 0.0, xu = 0.0, xv = 0.0;
    // ---- the burst.  Small per-column values first (they come back first), then the planes the column operators need,
    // then the rest.
    double r = 1.0, zk = 1.0, cs_d = 0.0, sn_d = 0.0;
    if (live) { r = a.r[col]; zk = a.z[k]; }
    if (live && k == 0) { cs_d = a.cosl[col]; sn_d = a.sinl[col]; }
    // planes as (value-type) v0: ub | v1: vb | v2: h | v3: ug | v4: vg and (derivative-type) pairs
    double ub = 0, vb = 0, h = 0, ug = 0, vg = 0;
    double ubr = 0, vbl = 0, ubz = 0, vbz = 0, hr = 0, hl = 0, ugr = 0, ugl = 0, vgr = 0, vgl = 0, ubrr = 0, ubl = 0, ubll = 0, vbr = 0, vbrr = 0, vbll = 0;
    dbl2v rv0, rv1;              // (ub, vb), (h, ug); vg travels alone
    SV rd[8];                    // (ubr, vbl) (ubz, vbz) | (hr, hl) (ugr, ugl) (vgr, vgl) (ubrr, ubl) (ubll, vbr) (vbrr, vbll)
#define PV(v) (a.P.val + (int64_t)(v) * a.N)
#define PD(v, s) (a.P.der + ((int64_t)((s) - 1) * a.V + (v)) * a.N)
#define LD2V(raw, x, y, va, vb_) { if (WIDE) raw = issue_pair<false>(PV(va) + pw, PV(vb_) + pw, lane); else { x = PV(va)[p]; y = PV(vb_)[p]; } }
#define LD2D(raw, x, y, va, sa, vb_, sb) { if (WIDE) raw = issue_pair<false>(PD(va, sa) + pw, PD(vb_, sb) + pw, lane); else { x = (double)PD(va, sa)[p]; y = (double)PD(vb_, sb)[p]; } }
    if (live) {
        LD2V(rv0, ub, vb, 3, 4)
        LD2D(rd[0], ubr, vbl, 3, a.s_r, 4, a.s_l)
        LD2D(rd[1], ubz, vbz, 3, a.s_z, 4, a.s_z)
        SX_LOAD_FENCE();
        LD2V(rv1, h, ug, 0, 1)
        vg = PV(2)[p];
        LD2D(rd[2], hr, hl, 0, a.s_r, 0, a.s_l)
        LD2D(rd[3], ugr, ugl, 1, a.s_r, 1, a.s_l)
        LD2D(rd[4], vgr, vgl, 2, a.s_r, 2, a.s_l)
        LD2D(rd[5], ubrr, ubl, 3, a.s_rr, 3, a.s_l)
        LD2D(rd[6], ubll, vbr, 3, a.s_ll, 4, a.s_r)
        LD2D(rd[7], vbrr, vbll, 4, a.s_rr, 4, a.s_ll)
        SX_LOAD_FENCE();
    }
    // tendency history of the five prognostic variables: requested behind the operator fragments (below)
    double e1h[5] = {0, 0, 0, 0, 0}, e2h[5] = {0, 0, 0, 0, 0};
    dbl2v rh[5];
    MulRinv q = MulRinv::of(1.0);
    if (live) {
        if (WIDE) { take_pair(rv0, ub, vb); take_pair(rd[0], ubr, vbl); take_pair(rd[1], ubz, vbz); }
        q = MulRinv::of(1.0 / r);
        hrbl_column_inputs(q, mixing_length(zk), ub, ubr, vbl, ubz, vbz, xd, xu, xv);
        if (k == 1) { s1[0][cl] = ub; s1[1][cl] = vb; }
    }
    __syncthreads();
    if (live && k == 0) surface_drag(par, cs_d, sn_d, s1[0][cl], s1[1][cl], xu, xv);
    X[0][cl * CS + k] = xd;
    X[1][cl * CS + k] = xu;
    X[2][cl * CS + k] = xv;
    __syncthreads();
    {
        const int wave = threadIdx.x >> 6;
        constexpr int RT = NZ / 16;                 // row tiles per operand
        constexpr int NW = CPB * NZ / 64;           // waves in the workgroup
        constexpr int JPW = (3 * RT + NW - 1) / NW;  // jobs per wave
        constexpr int KS = NZ / 4;                  // MFMA steps per job
        constexpr int KC = 8;                       // operator fragments requested at a time (register budget: 128 VGPRs)
        mfma_d4 acc[JPW];
#pragma unroll
        for (int jj = 0; jj < JPW; jj++) {
            const int job = wave + jj * NW;
            acc[jj] = mfma_d4{0.0, 0.0, 0.0, 0.0};
            const bool has = job < 3 * RT;
            const int op = has ? job / RT : 0, rt = has ? job % RT : 0;
            const double *MT = (op == 0) ? a.MintT : a.MdzT;      // MT[j][k] = M[k][j]
            const double *xb = X[op] + (lane & 15) * CS + (lane >> 4);
            const double *ma = MT + (int64_t)(lane >> 4) * NZ + rt * 16 + (lane & 15);
            for (int kc = 0; kc < KS; kc += KC) {
                double af[KC];
#pragma unroll
                for (int ks = 0; ks < KC; ks++) af[ks] = has ? ma[(int64_t)(kc + ks) * 4 * NZ] : 0.0;
                if (jj == 0 && kc == 0) {
                    // the history goes out BEHIND the first operator fragments: fragments issued after it would wait for its
                    // HBM latency before the first MFMA
                    SX_LOAD_FENCE();
                    if (live) {
#pragma unroll
                        for (int v = 0; v < 5; v++) {
                            if (WIDE) {
                                if (a.t >= 2) rh[v] = issue_pair<true>(a.E1 + (int64_t)v * a.N + pw, a.E2 + (int64_t)v * a.N + pw, lane);
                            } else {
                                if (a.t >= 2) e1h[v] = __builtin_nontemporal_load(a.E1 + (int64_t)v * a.N + p);
                                if (a.t >= 3) e2h[v] = __builtin_nontemporal_load(a.E2 + (int64_t)v * a.N + p);
                            }
                        }
                    }
                    SX_LOAD_FENCE();
                }
                if (has) {
#pragma unroll
                    for (int ks = 0; ks < KC; ks++)
                        acc[jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ks], xb[(kc + ks) * 4], acc[jj], 0, 0, 0);
                }
            }
        }
        if (ALIAS) __syncthreads();
#pragma unroll
        for (int jj = 0; jj < JPW; jj++) {
            const int job = wave + jj * NW;
            if (job < 3 * RT) {
                const int op = job / RT, rt = job % RT;
                double *yo = Y[op] + (lane & 15) * CS + rt * 16 + (lane >> 4);
                yo[0] = acc[jj][0]; yo[4] = acc[jj][1]; yo[8] = acc[jj][2]; yo[12] = acc[jj][3];
            }
        }
    }
    __syncthreads();
    if (!live) return;
    if (WIDE) {
        take_pair(rv1, h, ug);
        take_pair(rd[2], hr, hl); take_pair(rd[3], ugr, ugl); take_pair(rd[4], vgr, vgl);
        take_pair(rd[5], ubrr, ubl); take_pair(rd[6], ubll, vbr); take_pair(rd[7], vbrr, vbll);
#pragma unroll
        for (int v = 0; v < 5; v++)
            if (a.t >= 2) { take_pair(rh[v], e1h[v], e2h[v]); if (a.t < 3) e2h[v] = 0.0; }
    }
    const double wb = Y[0][cl * CS + k], vdu = Y[1][cl * CS + k], vdv = Y[2][cl * CS + k];
    if (a.write_w) a.P.val[(int64_t)5 * a.N + p] = wb;
    double ee[5];
    sw_free_layer(q, g, Hfree, f, h, hr, hl, ug, ugr, ugl, vg, vgr, vgl, ee[0], ee[1], ee[2]);
    hrbl_boundary_layer(q, g, Kh, f, hr, hl, ub, ubr, ubrr, ubl, ubll, ubz, vb, vbr, vbrr, vbl, vbll, vbz, wb, vdu, vdv, ee[3], ee[4]);
    const double uu[5] = {h, ug, vg, ub, vb};
#pragma unroll
    for (int v = 0; v < 5; v++) {          // explicit_timestep with the prefetched history
        const int64_t o = (int64_t)v * a.N + p;
        const double un = ab_value(a.t, a.ts, uu[v], ee[v], e1h[v], e2h[v]);
        if (WIDE) {
            store_pair_nt(a.En + (int64_t)v * a.N + pw, a.np1 + (int64_t)v * a.N + pw, lane, ee[v], un);
        } else {
            __builtin_nontemporal_store(ee[v], a.En + o);
            __builtin_nontemporal_store(un, a.np1 + o);
        }
    }
    __builtin_nontemporal_store(wb, a.np1 + (int64_t)5 * a.N + p);
    for (int v = 6; v < a.V; v++) ab_step(a, v, p, PSV(v), 0.0);
#undef PV
#undef PD
#undef LD2V
#undef LD2D
}

// Cell-wise node-space variant ("radial last", uniform rings): one workgroup = LAM azimuths x NZ levels of ONE radial
// cell, i.e. the 3 rings that share the same 4 spline nodes.  Each thread loads the 14 node transforms of its
// (lambda, z) at the 4 nodes once (56 values, kept in registers) and evaluates all 3 rings from them, so a node value
// enters the CU once instead of three times (the ring-wise grouping was bound by L1 fill rate, not by HBM).
// The column operators of the 3 x LAM columns run as one f64-MFMA batch; the fields are re-formed from the registers
// after it, ring by ring, for the tendencies.
// Load schedule (what the phase stamps asked for): every load a workgroup needs is issued in ONE burst at entry, oldest =
// needed first; nothing small is fetched on its own later.  The per-ring constants come without memory traffic: the
// basis weights phi / phi' / phi'' at a cell's three Gauss points are the same for every cell (kernel arguments, scalar
// registers) and r is recomputed from the cell index exactly as sx_create tabulates it.
// WIDE: 16-byte-per-lane loads / stores with the lane <-> level map of issue_pair (needs 64 | LAM * NZ, always true here).
template <int NZ, int LAM, class ST, bool WIDE>
__global__ void __launch_bounds__(LAM * NZ, 2) k_phys_hrbl_cell(PhysArgsT<ST> a, int cell0) {
    constexpr int CS = NZ + 2;
    constexpr int NCOL = 3 * LAM, NT = (NCOL + 15) / 16;
    __shared__ double X[3][NT * 16 * CS];
    // results of the column operators; at zDim = 128 they wait in the accumulators and are written over X (64 KB of static LDS)
    constexpr bool ALIAS = (NZ > 64);
    __shared__ double Ysep[ALIAS ? 1 : 3][ALIAS ? 1 : NT * 16 * CS];
    double (*Y)[NT * 16 * CS] = ALIAS ? X : reinterpret_cast<double (*)[NT * 16 * CS]>(&Ysep[0][0]);
    __shared__ double s1[2][NCOL];
    SX_STAMP(0);
    const int lane = threadIdx.x & 63, wbase = threadIdx.x & ~63;
    const int elem = WIDE ? wbase + wide_elem(lane) : (int)threadIdx.x;      // element of the workgroup's LAM x NZ block
    const int k = elem % NZ, ll = elem / NZ;
    const int nlb = a.L / LAM;
    const int cell = cell0 + blockIdx.x / nlb;
    const int lam = (blockIdx.x % nlb) * LAM + ll;
    // offset of this lane's PAIR inside a stream of the workgroup's block (WIDE)
    const int64_t pairo = (int64_t)(blockIdx.x % nlb) * LAM * NZ + wbase + 2 * (lane & 31);
    const double *par = a.par;
    const double g = par[SX_P_G], Kh = par[SX_P_KH], Hfree = par[SX_P_HFREE], f = par[SX_P_F];
    const int64_t gp = ((int64_t)cell * a.L + lam) * NZ + k;
    const int64_t gs = (int64_t)a.L * NZ;
    const int64_t gw = (int64_t)cell * a.L * NZ + pairo;                      // this lane's pair at node 0 of the cell
    const int64_t pc = ((int64_t)(cell * MUBAR) * a.L + lam) * NZ + k;        // this lane's point on ring mu = 0; + mu * gs
    const int64_t pw = (int64_t)(cell * MUBAR) * a.L * NZ + pairo;            // this lane's pair on ring mu = 0

    // ---- the one burst of loads, oldest first: level height and surface-drag angles (one small load each, L2-resident)
    const double zk = a.z[k];
    double cs_d = 0.0, sn_d = 0.0;
    if (k < MUBAR) {       // the surface-drag lanes (k < 3: one ring each)
        const int64_t col = (int64_t)(cell * MUBAR + k) * a.L + lam;
        cs_d = a.cosl[col]; sn_d = a.sinl[col];
    }
    // node transforms [transform][node].  WIDE keeps the raw 16-byte pairs (nodes 0|1 and 2|3) until they are needed.
    typedef typename Vec2<ST>::type SV;
    double qh[4], qhl[4], qug[4], qugl[4], qvg[4], qvgl[4];
    double qub[4], qubl[4], qubll[4], qubz[4], qvb[4], qvbl[4], qvbll[4], qvbz[4];
    dbl2v rv[5][2];         // value planes: ub, vb | h, ug, vg
    SV rd[9][2];            // derivative planes: ubz, vbz, vbl | hl, ugl, vgl, ubl, ubll, vbll
#define NODE_V(dst, raw, v)                                                                        \
    {                                                                                              \
        const double *gq = a.G.val + (int64_t)(v) * a.NG;                                          \
        if (WIDE) { raw[0] = issue_pair<false>(gq + gw, gq + gw + gs, lane); raw[1] = issue_pair<false>(gq + gw + 2 * gs, gq + gw + 3 * gs, lane); } \
        else { dst[0] = gq[gp]; dst[1] = gq[gp + gs]; dst[2] = gq[gp + 2 * gs]; dst[3] = gq[gp + 3 * gs]; } \
    }
#define NODE_D(dst, raw, v, s)                                                                     \
    {                                                                                              \
        const ST *gq = a.G.der + ((int64_t)((s) - 1) * a.V + (v)) * a.NG;                          \
        if (WIDE) { raw[0] = issue_pair<false>(gq + gw, gq + gw + gs, lane); raw[1] = issue_pair<false>(gq + gw + 2 * gs, gq + gw + 3 * gs, lane); } \
        else { dst[0] = gq[gp]; dst[1] = gq[gp + gs]; dst[2] = gq[gp + 2 * gs]; dst[3] = gq[gp + 3 * gs]; } \
    }
#define NODE_TAKE(dst, raw) { if (WIDE) { take_pair(raw[0], dst[0], dst[1]); take_pair(raw[1], dst[2], dst[3]); } }
    // what the column operators' inputs need ...
    NODE_V(qub, rv[0], 3) NODE_D(qubz, rd[0], 3, a.s_z) NODE_D(qvbz, rd[1], 4, a.s_z) NODE_D(qvbl, rd[2], 4, a.s_l) NODE_V(qvb, rv[1], 4)
    SX_LOAD_FENCE();
    // ... then everything else, needed only after the column operators
    NODE_V(qh, rv[2], 0) NODE_D(qhl, rd[3], 0, a.s_l) NODE_V(qug, rv[3], 1) NODE_D(qugl, rd[4], 1, a.s_l) NODE_V(qvg, rv[4], 2) NODE_D(qvgl, rd[5], 2, a.s_l)
    NODE_D(qubl, rd[6], 3, a.s_l) NODE_D(qubll, rd[7], 3, a.s_ll) NODE_D(qvbll, rd[8], 4, a.s_ll)
    // tendency history: ring 0 with the entry burst, ring 1 behind the first operator fragments (in flight during the MFMA
    // phase and ring 0), ring 2 at the start of the final phase; the fragments come in two chunks of 8 so that all of
    // this fits the 256 registers of a two-waves-per-SIMD kernel.  WIDE:
    // expdot_nm1 / nm2 of a variable travel as one pair; before step 3 the buffers exist but hold no history yet.
    double e1h[MUBAR][5], e2h[MUBAR][5];
    dbl2v rh[MUBAR][5];
#define HIST(mu)                                                                                   \
    _Pragma("unroll") for (int v = 0; v < 5; v++) {                                                \
        if (WIDE) {                                                                                \
            if (a.t >= 2) rh[mu][v] = issue_pair<true>(a.E1 + (int64_t)v * a.N + pw + (mu) * gs, a.E2 + (int64_t)v * a.N + pw + (mu) * gs, lane);   \
        } else {                                                                                   \
            e1h[mu][v] = (a.t >= 2) ? __builtin_nontemporal_load(a.E1 + (int64_t)v * a.N + pc + (mu) * gs) : 0.0;   \
            e2h[mu][v] = (a.t >= 3) ? __builtin_nontemporal_load(a.E2 + (int64_t)v * a.N + pc + (mu) * gs) : 0.0;   \
        }                                                                                          \
    }
#define HIST_TAKE(mu)                                                                              \
    _Pragma("unroll") for (int v = 0; v < 5; v++) {                                                \
        if (WIDE) {                                                                                \
            if (a.t >= 2) { take_pair(rh[mu][v], e1h[mu][v], e2h[mu][v]); if (a.t < 3) e2h[mu][v] = 0.0; }   \
            else { e1h[mu][v] = 0.0; e2h[mu][v] = 0.0; }                                           \
        }                                                                                          \
    }
    HIST(0)
    SX_LOAD_FENCE();

    // ---- inputs of the column operators
    NODE_TAKE(qub, rv[0]) NODE_TAKE(qubz, rd[0]) NODE_TAKE(qvbz, rd[1]) NODE_TAKE(qvbl, rd[2]) NODE_TAKE(qvb, rv[1])
#define DOT(w, q) ((w)[0] * q[0] + (w)[1] * q[1] + (w)[2] * q[2] + (w)[3] * q[3])
    const double lmix = mixing_length(zk);
    double rinv[MUBAR];
#pragma unroll
    for (int mu = 0; mu < MUBAR; mu++) {
        // r of the ring, as sx_create tabulates it (xmin + DX (c + 0.5 + offset of the Gauss point))
        rinv[mu] = 1.0 / (a.cc.xmin + a.cc.DX * ((a.cc.gcell0 + cell) + 0.5 + a.cc.goff[mu]));
        const double *w0 = a.cc.phiw[0][mu], *w1 = a.cc.phiw[1][mu];
        const double ub = DOT(w0, qub), ubr = DOT(w1, qub), vbl = DOT(w0, qvbl), ubz = DOT(w0, qubz), vbz = DOT(w0, qvbz);
        const int c = mu * LAM + ll;
        hrbl_column_inputs(MulRinv::of(rinv[mu]), lmix, ub, ubr, vbl, ubz, vbz, X[0][c * CS + k], X[1][c * CS + k], X[2][c * CS + k]);
        if (k == 1) { s1[0][c] = ub; s1[1][c] = DOT(w0, qvb); }
    }
    SX_STAMP(1);
    __syncthreads();
    if (k < MUBAR) {       // lane k takes ring k
        const int c = k * LAM + ll;
        surface_drag(par, cs_d, sn_d, s1[0][c], s1[1][c], X[1][c * CS], X[2][c * CS]);
    }
    __syncthreads();
    SX_STAMP(2);
    {
        const int wave = threadIdx.x >> 6;
        constexpr int RT = NZ / 16, NW = LAM * NZ / 64;
        constexpr int UPW = (RT * NT + NW - 1) / NW;         // (row tile, column tile) units per wave
        constexpr int KC = 8;                                // operator fragments fetched per chunk (register budget)
        mfma_d4 c0[UPW], c1[UPW], c2[UPW];
#pragma unroll
        for (int uu = 0; uu < UPW; uu++) {
            const int unit = wave + uu * NW;
            c0[uu] = mfma_d4{0.0, 0.0, 0.0, 0.0}; c1[uu] = c0[uu]; c2[uu] = c0[uu];
            if (unit < RT * NT) {
                const int rt = unit % RT, nt = unit / RT;
                const int64_t ao = (int64_t)(lane >> 4) * NZ + rt * 16 + (lane & 15);      // MT[j][k] = M[k][j]
                const int xo = (nt * 16 + (lane & 15)) * CS + (lane >> 4);
                for (int kc = 0; kc < NZ / 4; kc += KC) {
                    double ai[KC], ad[KC];
#pragma unroll
                    for (int ks = 0; ks < KC; ks++) {
                        ai[ks] = a.MintT[ao + (int64_t)(kc + ks) * 4 * NZ];
                        ad[ks] = a.MdzT[ao + (int64_t)(kc + ks) * 4 * NZ];
                    }
                    if (uu == 0 && kc == 0) {
                        // ring 1's history goes out BEHIND the first operator fragments: the memory counter retires in issue
                        // order, so fragments issued after it would wait for its HBM latency before the first MFMA
                        SX_LOAD_FENCE();
                        HIST(1)
                        SX_LOAD_FENCE();
                    }
#pragma unroll
                    for (int ks = 0; ks < KC; ks++) {
                        c0[uu] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[ks], X[0][xo + (kc + ks) * 4], c0[uu], 0, 0, 0);
                        c1[uu] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[ks], X[1][xo + (kc + ks) * 4], c1[uu], 0, 0, 0);
                        c2[uu] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[ks], X[2][xo + (kc + ks) * 4], c2[uu], 0, 0, 0);
                    }
                }
            }
        }
        if (RT * NT < NW && wave >= RT * NT) { HIST(1) }      // waves without a unit (never at the shipped shapes)
        SX_STAMP(3);
        if (ALIAS) __syncthreads();
#pragma unroll
        for (int uu = 0; uu < UPW; uu++) {
            const int unit = wave + uu * NW;
            if (unit < RT * NT) {
                const int rt = unit % RT, nt = unit / RT;
                const int yo = (nt * 16 + (lane & 15)) * CS + rt * 16 + (lane >> 4);
                Y[0][yo] = c0[uu][0]; Y[0][yo + 4] = c0[uu][1]; Y[0][yo + 8] = c0[uu][2]; Y[0][yo + 12] = c0[uu][3];
                Y[1][yo] = c1[uu][0]; Y[1][yo + 4] = c1[uu][1]; Y[1][yo + 8] = c1[uu][2]; Y[1][yo + 12] = c1[uu][3];
                Y[2][yo] = c2[uu][0]; Y[2][yo + 4] = c2[uu][1]; Y[2][yo + 8] = c2[uu][2]; Y[2][yo + 12] = c2[uu][3];
            }
        }
    }
    __syncthreads();
    SX_STAMP(4);
    HIST(2)
    SX_LOAD_FENCE();
    NODE_TAKE(qh, rv[2]) NODE_TAKE(qhl, rd[3]) NODE_TAKE(qug, rv[3]) NODE_TAKE(qugl, rd[4]) NODE_TAKE(qvg, rv[4]) NODE_TAKE(qvgl, rd[5])
    NODE_TAKE(qubl, rd[6]) NODE_TAKE(qubll, rd[7]) NODE_TAKE(qvbll, rd[8])
    double wb_keep = 0.0;
#pragma unroll
    for (int mu = 0; mu < MUBAR; mu++) {
        const int64_t p = pc + mu * gs;
        HIST_TAKE(mu)
        const double *w0 = a.cc.phiw[0][mu], *w1 = a.cc.phiw[1][mu], *w2 = a.cc.phiw[2][mu];
        const MulRinv q = MulRinv::of(rinv[mu]);
        const double h = DOT(w0, qh), hr = DOT(w1, qh), hl = DOT(w0, qhl);
        const double ug = DOT(w0, qug), ugr = DOT(w1, qug), ugl = DOT(w0, qugl);
        const double vg = DOT(w0, qvg), vgr = DOT(w1, qvg), vgl = DOT(w0, qvgl);
        const double ub = DOT(w0, qub), ubr = DOT(w1, qub), ubrr = DOT(w2, qub);
        const double ubl = DOT(w0, qubl), ubll = DOT(w0, qubll), ubz = DOT(w0, qubz);
        const double vb = DOT(w0, qvb), vbr = DOT(w1, qvb), vbrr = DOT(w2, qvb);
        const double vbl = DOT(w0, qvbl), vbll = DOT(w0, qvbll), vbz = DOT(w0, qvbz);
        const int c = mu * LAM + ll;
        const double wb = Y[0][c * CS + k], vdu = Y[1][c * CS + k], vdv = Y[2][c * CS + k];
        if (a.write_w) a.P.val[(int64_t)5 * a.N + p] = wb;
        double ee[5];
        sw_free_layer(q, g, Hfree, f, h, hr, hl, ug, ugr, ugl, vg, vgr, vgl, ee[0], ee[1], ee[2]);
        hrbl_boundary_layer(q, g, Kh, f, hr, hl, ub, ubr, ubrr, ubl, ubll, ubz, vb, vbr, vbrr, vbl, vbll, vbz, wb, vdu, vdv, ee[3], ee[4]);
        const double uu[5] = {h, ug, vg, ub, vb};
#pragma unroll
        for (int v = 0; v < 5; v++) {          // explicit_timestep with the prefetched history
            const int64_t o = (int64_t)v * a.N + p;
            const double un = ab_value(a.t, a.ts, uu[v], ee[v], e1h[mu][v], e2h[mu][v]);
            // expdot_n is read again only by the next step; var_np1 (0.4 GB per step) next by the forward transform, after
            // everything else of this kernel has gone through the caches: both non-temporal
            if (WIDE) {
                const int64_t ow = (int64_t)v * a.N + pw + mu * gs;
                store_pair_nt(a.En + ow, a.np1 + ow, lane, ee[v], un);
            } else {
                __builtin_nontemporal_store(ee[v], a.En + o);
                __builtin_nontemporal_store(un, a.np1 + o);
            }
        }
        if (WIDE) {        // the diagnostic w of rings 0 and 1 leaves as one pair, ring 2's on its own
            if (mu == 0) wb_keep = wb;
            else if (mu == 1) store_pair_nt(a.np1 + (int64_t)5 * a.N + pw, a.np1 + (int64_t)5 * a.N + pw + gs, lane, wb_keep, wb);
            else __builtin_nontemporal_store(wb, a.np1 + (int64_t)5 * a.N + p);
        } else {
            __builtin_nontemporal_store(wb, a.np1 + (int64_t)5 * a.N + p);
        }
        SX_STAMP(5 + mu);
    }
#undef DOT
#undef HIST
#undef HIST_TAKE
#undef NODE_V
#undef NODE_D
#undef NODE_TAKE
}

// semiimplicit_adjustment (src/semiimplicit.jl:521-597), one workgroup per group of columns
__global__ void __launch_bounds__(256) k_semiimplicit(SemiArgs a, int cpb) {
    extern __shared__ double sm[];
    const int nz = a.nz;
    const int k = threadIdx.x % nz, cl = threadIdx.x / nz;
    const int64_t col = (int64_t)blockIdx.x * cpb + cl;
    const bool live = (cl < cpb) && (col < a.N / nz);
    double *sw = sm, *sx_ = sm + (size_t)cpb * nz, *sg = sm + (size_t)2 * cpb * nz;
    const int64_t p = live ? col * nz + k : 0;
    const double ts = a.ts;
    if (live) {
        const int vv[2] = {a.wi, a.xi};
        double out[2];
        for (int q = 0; q < 2; q++) {
            const int64_t o = (int64_t)vv[q] * a.N + p;
            double x = a.np1[o];
            const double In = a.In[o];
            if (a.t == 1) x = x - (ts * In) + (ts * 0.5 * In);
            else if (a.t == 2) x = x - (0.5 * ts) * ((3.0 * In) - a.I1[o]) - (ts * In) + (ts * 0.75 * a.I1[o]);
            else x = x - ((ts / 12.0) * ((23.0 * In) - (16.0 * a.I1[o]) + (5.0 * a.I2[o]))) - (ts * In) + (ts * 0.75 * a.I1[o]);
            out[q] = x;
        }
        sw[cl * nz + k] = out[0];
        sx_[cl * nz + k] = out[1];
    }
    __syncthreads();
    double xrec = 0.0, xz = 0.0;
    if (live) {
        const double *x = sx_ + cl * nz;
        for (int j = 0; j < nz; j++) {
            xrec += a.MrecT[(int64_t)j * nz + k] * x[j];
            xz += a.MdzT[(int64_t)j * nz + k] * x[j];
        }
        // g = [0; 0; (tau Pxi xi*_z - w*)[2 : nz-1]]
        if (k >= 1 && k < nz - 1) sg[cl * nz + k + 1] = (a.tau * a.pxi * xz) - sw[cl * nz + k];
        if (k < 2) sg[cl * nz + k] = 0.0;
    }
    __syncthreads();
    if (!live) return;
    double wn = 0.0, wz = 0.0;
    const double *gv = sg + cl * nz;
    for (int j = 0; j < nz; j++) {
        wn += a.WT[(int64_t)j * nz + k] * gv[j];
        wz += a.XT[(int64_t)j * nz + k] * gv[j];
    }
    a.np1[(int64_t)a.wi * a.N + p] = wn;
    a.np1[(int64_t)a.xi * a.N + p] = xrec - (a.tau * wz);
}

// condensation_adjustment (src/microphysics.jl:139-195) of rainfall_test on var_np1, one workgroup per group of columns: thread (c, k)
// owns level k of column c.  The reference hands it one RZ column at a time (src/semiimplicit.jl:334-349) and clamps with
//     q_cond = min(q_v, q_cond);  q_cond = max(-q_c, q_cond)          (:185-187, vectors, not broadcast)
// Julia's min / max of two vectors compare them with isless, which is lexicographic (cmp walks to the first level where
// !isequal(a, b) and compares with isless there), so each clamp keeps ONE of its two arguments for the whole column.  Kept for
// parity: an LDS minimum finds that first level, and every thread of the column reads the isless result stored at it.  No level
// differs: the first argument stays.
__global__ void __launch_bounds__(256) k_condensation(double *__restrict__ np1, const double *__restrict__ ref, int64_t N, int nz,
                                                       int cpb) {
    extern __shared__ int smi[];
    int *first = smi;                        // [2][cpb]: first differing level of the min step, of the max step
    int *lt = smi + 2 * cpb;                 // [2][cpb][nz]: isless at each level, for the min step and the max step
    const int k = threadIdx.x % nz, cl = threadIdx.x / nz;
    const int64_t col = (int64_t)blockIdx.x * cpb + cl;
    const bool live = (cl < cpb) && (col < N / nz);
    const int64_t p = live ? col * nz + k : 0;
    if (cl < cpb && k == 0) { first[cl] = nz; first[cpb + cl] = nz; }
    double s = 0.0, mu = 0.0, mu_c = 0.0, mu_total = 0.0, q_v = 0.0, rho_d = 0.0, Tk = 0.0, pr = 0.0, q_c = 0.0, q_l = 0.0;
    double q_cond = 0.0;
    __syncthreads();
    if (live) {
        s = np1[p];
        const double xi = np1[N + p];
        mu = np1[2 * N + p];
        mu_c = np1[5 * N + p];
        const double mu_r = np1[6 * N + p], qss = np1[7 * N + p];
        // ReferenceState rows 0, 3, 6: sbar, xibar, mubar
        mu_total = mu + ref[6 * nz + k];
        q_v = thermo::ahyp(mu_total);
        rho_d = thermo::dry_density(xi + ref[3 * nz + k]);
        Tk = thermo::temperature(s + ref[k], rho_d, q_v);
        pr = thermo::pressure(Tk, rho_d, q_v);
        q_c = thermo::ahyp(mu_c);
        const double q_r = thermo::ahyp(mu_r);
        q_l = q_c + q_r;
        const double q_sat = thermo::q_sat_liquid(Tk, pr);
        const double Q_s = thermo::Q_s_factor(Tk, pr, q_v, q_l);
        q_cond = (q_v - q_sat - qss) / (1.0 + Q_s);
        // min(q_v, q_cond) = isless(q_cond, q_v) ? q_cond : q_v
        if (!thermo::jl_isequal(q_cond, q_v)) atomicMin(&first[cl], k);
        lt[cl * nz + k] = thermo::jl_isless(q_cond, q_v) ? 1 : 0;
    }
    __syncthreads();
    if (live) {
        const int f = first[cl];
        if (!(f < nz && lt[cl * nz + f])) q_cond = q_v;
        // max(-q_c, q_cond) = isless(q_cond, -q_c) ? -q_c : q_cond
        if (!thermo::jl_isequal(q_cond, -q_c)) atomicMin(&first[cpb + cl], k);
        lt[(cpb + cl) * nz + k] = thermo::jl_isless(q_cond, -q_c) ? 1 : 0;
    }
    __syncthreads();
    if (!live) return;
    const int f = first[cpb + cl];
    if (f < nz && lt[(cpb + cl) * nz + f]) q_cond = -q_c;
    // explicit Euler increment with tau_r = 0.25, elementwise (:188-190); q_l is the liquid before the increment
    const double tau_r = 0.25;
    np1[2 * N + p] = mu - tau_r * thermo::dmudq(mu_total, q_v) * q_cond;
    np1[5 * N + p] = mu_c + tau_r * thermo::dmudq(mu_c, q_c) * q_cond;
    np1[p] = s + tau_r * thermo::s_condensation(q_cond, Tk, rho_d, q_v, q_l, pr);
}

// ------------------------------------------------------------------------------------------------ launchers
#ifdef SX_PHASES
// diagnostic build: stamps of the LAST cell-kernel launch, written to $SX_PHASES_OUT (binary int64 [nwg][8]) by sx_destroy
static long long *g_ph_buf = nullptr;
static int64_t g_ph_n = 0;
void phases_dump() {
    const char *path = getenv("SX_PHASES_OUT");
    if (!path || !g_ph_buf) return;
    std::vector<long long> hst((size_t)g_ph_n * 8);
    hipDeviceSynchronize();
    hipMemcpy(hst.data(), g_ph_buf, sizeof(long long) * hst.size(), hipMemcpyDeviceToHost);
    FILE *f = fopen(path, "wb");
    if (f) { fwrite(hst.data(), sizeof(long long), hst.size(), f); fclose(f); }
}
static long long *phases_buffer(int64_t nwg) {
    if (!g_ph_buf) {
        hipMalloc(&g_ph_buf, sizeof(long long) * nwg * 8);
        hipMemset(g_ph_buf, 0, sizeof(long long) * nwg * 8);
        g_ph_n = nwg;
    }
    return nwg <= g_ph_n ? g_ph_buf : nullptr;
}
#endif

template <class ST>
static PhysArgsT<ST> phys_args(sx_handle *h, int t) {
    PhysArgsT<ST> a;
    a.P = planes_of<ST>(h->d_phys, h->V, h->N);
    a.En = h->d_E[h->rot % 3];
    a.E1 = h->d_E[(h->rot + 1) % 3];
    a.E2 = h->d_E[(h->rot + 2) % 3];
    a.In = h->d_I[0] ? h->d_I[h->rot % 3] : nullptr;
    a.np1 = h->d_np1;
    a.r = h->d_r; a.cosl = h->d_cosl; a.sinl = h->d_sinl; a.z = h->d_z;
    a.MintT = h->d_MintT; a.MdzT = h->d_MdzT; a.ref = h->d_ref; a.write_w = h->in_advance ? 0 : 1;
    a.N = h->N; a.V = h->V; a.nz = h->nz; a.t = t; a.eq = h->eq;
    a.s_u = h->slot[0]; a.s_r = h->slot[1]; a.s_rr = h->slot[2]; a.s_l = h->slot[3]; a.s_ll = h->slot[4];
    a.s_z = h->slot[5]; a.s_zz = h->slot[6];
    a.ts = h->ts;
    for (int i = 0; i < SX_NPARAMS; i++) a.par[i] = h->par[i];
    a.col0 = 0; a.col1 = h->Nh; a.G = Planes<ST>{nullptr, nullptr}; a.phi = nullptr; a.NG = 0; a.L = 1; a.nrings = h->nrings;
    a.cc = h->cell_consts;
    a.dbg = nullptr;
    return a;
}

// History rotation replaces the copies of explicit_timestep: after step t the buffer written as expdot_n becomes
// expdot_nm1 and the previous nm1 becomes nm2. rot decreases by one (mod 3) per step.
constexpr int PCPB = 8;       // columns per workgroup of the ring-wise MFMA HRBL kernel: two resident 512-thread workgroups per CU
                              // (A/B on one box: 0.146 ms vs 0.154 ms with 16 columns / one workgroup per CU)

template <class ST>
static void launch_physics_t(sx_handle *h, int t, int part) {
    // part: 0 = everything; 1 = only the rings on the ring-wise path, 2 = only the node-space rings (the two halves of
    // launch_inverse_and_physics; the history rotation happens once, in part 1 before and in part 2 after)
    if (h->eq != SX_EQ_NONE && t == 1 && part != 2) h->rot = 0;
    PhysArgsT<ST> a = phys_args<ST>(h, t);
    // Algorithmic bytes: read the requested slots, E_nm1, E_nm2; write E_n, var_np1.  The shallow-water sets keep no tendency history
    // for their diagnostic w (-3 planes; inside sx_advance its plane is not stored either)
    const double N = (double)h->N, V = h->V, eq_planes = plane_bytes(h, h->mask_eq_bits, h->mask_eq_val);
    const bool diag_w = h->eq == SX_EQ_ONEWAY_SW_SLAB || h->eq == SX_EQ_TWOWAY_SW_SLAB || h->eq == SX_EQ_ONEWAY_SW_HRBL;
    const double pointwise_bytes = N * (eq_planes + 8.0 * (4.0 * V + (diag_w ? -3.0 : 0.0)));
    if (h->eq == SX_EQ_ONEWAY_SW_HRBL && mfma_levels(h->nz)) {      // any ring table: the ring-wise kernel reads physical slots
        // rings [0, R_in): ring-wise physical slots; rings [R_in, nrings): node-space transforms (node_mode only)
        const int64_t split = (h->node_mode && h->node_active) ? (int64_t)h->R_in * h->uniform_L : h->Nh;
        if (h->d_G) a.G = planes_of<ST>(h->d_G, h->V, h->NG);
        a.phi = h->d_phi; a.NG = h->NG; a.L = h->uniform_L; a.nrings = h->nrings;
        const double fin = (double)h->R_in / h->nrings;        // split < Nh: the fraction of rings on the ring-wise path
        if (split > 0 && part != 2) {
            TimedLaunch scope(h, split < h->Nh ? "k_phys_hrbl_inner" : "k_phys_hrbl",
                              split < h->Nh ? N * fin * (eq_planes + 8.0 * (4.0 * V - 3.0)) : pointwise_bytes);
            a.col0 = 0; a.col1 = split;
#define RING_LAUNCH(NZ_, CPB_)                                                                                                     \
            do {                                                                                                                      \
                if (h->sw.wide) hipLaunchKernelGGL((k_phys_hrbl_mfma<NZ_, CPB_, ST, true>), grid1(split, CPB_), dim3(CPB_ * NZ_), 0, h->stream, a);   \
                else hipLaunchKernelGGL((k_phys_hrbl_mfma<NZ_, CPB_, ST, false>), grid1(split, CPB_), dim3(CPB_ * NZ_), 0, h->stream, a);          \
            } while (0)
            if (h->nz == 64) RING_LAUNCH(64, PCPB);
            else if (h->nz == 32) RING_LAUNCH(32, PCPB);
            else RING_LAUNCH(128, 8);
#undef RING_LAUNCH
        }
        if (split < h->Nh && part != 1) {
            // node transforms (read once) + history + outputs
            TimedLaunch scope(h, "k_phys_hrbl", node_points(h) * plane_bytes(h, h->mask_node_bits, h->mask_node_val) + N * (1.0 - fin) * 8.0 * (4.0 * V - 3.0));
            a.col0 = split; a.col1 = h->Nh;
            const int ncell = (h->nrings - h->R_in) / MUBAR;         // R_in is a multiple of 3 (sx_create)
#ifdef SX_PHASES
            a.dbg = phases_buffer((int64_t)ncell * (h->uniform_L / (h->nz == 32 ? 8 : 4)));
#endif
#define CELL_LAUNCH(NZ_, LAM_)                                                                                                     \
            do {                                                                                                                      \
                if (h->sw.wide) hipLaunchKernelGGL((k_phys_hrbl_cell<NZ_, LAM_, ST, true>), dim3(ncell * (h->uniform_L / LAM_)), dim3(LAM_ * NZ_), 0, h->stream, a, h->R_in / MUBAR);   \
                else hipLaunchKernelGGL((k_phys_hrbl_cell<NZ_, LAM_, ST, false>), dim3(ncell * (h->uniform_L / LAM_)), dim3(LAM_ * NZ_), 0, h->stream, a, h->R_in / MUBAR);          \
            } while (0)
            if (h->nz == 64) CELL_LAUNCH(64, 4);      // LAM 2: 0.55 ms (6 of 16 MFMA columns, 1 KB chunks); 4: 0.41 ms
            else if (h->nz == 32) CELL_LAUNCH(32, 8);
            else CELL_LAUNCH(128, 4);   // 512 threads, one workgroup per CU: 12 of 16 MFMA columns (LAM 2: 6 of 16, 3.23 vs 2.58 ms at config 5)
#undef CELL_LAUNCH
        }
    } else if (h->eq == SX_EQ_ONEWAY_SW_HRBL) {
        TimedLaunch scope(h, "k_phys_hrbl", pointwise_bytes);
        const int cpb = h->nz >= 256 ? 1 : 256 / h->nz;
        const int bs = cpb * h->nz;
        const size_t lds = sizeof(double) * 5 * cpb * h->nz;
        hipLaunchKernelGGL(k_phys_hrbl<ST>, grid1(h->Nh, cpb), dim3(bs), lds, h->stream, a, cpb);
    } else if (h->eq == SX_EQ_RAINFALL_TEST) {
        TimedLaunch scope(h, "k_phys_rain", N * (eq_planes + 8.0 * (4.0 * V + (h->semi ? V : 0.0))));      // as k_phys_pointwise, + impdot
        hipLaunchKernelGGL(k_phys_rain<ST>, grid1(h->N, 256), dim3(256), 0, h->stream, a);
    } else {
        TimedLaunch scope(h, "k_phys_pointwise", pointwise_bytes);
        hipLaunchKernelGGL(k_phys_pointwise<ST>, grid1(h->N, 256), dim3(256), 0, h->stream, a);
    }
    if (h->semi && h->eq != SX_EQ_NONE) {
        TimedLaunch scope(h, "k_semiimplicit", 8.0 * N * 2.0 * 5.0);
        SemiArgs s;
        s.np1 = h->d_np1;
        s.In = h->d_I[h->rot % 3]; s.I1 = h->d_I[(h->rot + 1) % 3]; s.I2 = h->d_I[(h->rot + 2) % 3];
        const int which = (t == 1) ? 0 : 1;
        s.MrecT = h->d_MrecT; s.MdzT = h->d_MdzT; s.WT = h->d_WT[which]; s.XT = h->d_XT[which];
        s.N = h->N; s.nz = h->nz; s.t = t; s.wi = h->w_index - 1; s.xi = h->xi_index - 1;
        s.ts = h->ts; s.tau = h->tau[which]; s.pxi = h->par[SX_P_PXI_BAR];
        const SemiPlan sp = plan_semi(h->nz, h->Nh, h->sw);
        if (sp.mfma) launch_semi_mfma(h, s);               // the four column operators on the matrix cores (sx_rz.hip)
        else hipLaunchKernelGGL(k_semiimplicit, dim3((unsigned)sp.wgs), dim3(sp.threads), (size_t)sp.lds, h->stream, s, sp.cpb);
    }
    if (h->eq == SX_EQ_RAINFALL_TEST) {        // after the explicit and the semi-implicit step (src/testModels.jl:572-580)
        TimedLaunch scope(h, "k_condensation", 8.0 * N * (6.0 + 3.0));      // read s, xi, mu, mu_c, mu_r, qss of var_np1; write s, mu, mu_c
        const int cpb = h->nz >= 256 ? 1 : 256 / h->nz;
        const size_t lds = sizeof(int) * 2 * cpb * (1 + h->nz);
        hipLaunchKernelGGL(k_condensation, grid1(h->Nh, cpb), dim3(cpb * h->nz), lds, h->stream, h->d_np1, h->d_ref, h->N, h->nz, cpb);
    }
    if (h->eq != SX_EQ_NONE && part != 1) h->rot = (h->rot + 2) % 3;
}

static void launch_physics_part(sx_handle *h, int t, int part) {
    if (h->f32) launch_physics_t<float>(h, t, part);
    else launch_physics_t<double>(h, t, part);
}

void launch_physics(sx_handle *h, int t) { launch_physics_part(h, t, 0); }

// sx_advance's inverse transform + equation set.  With the node-space inverse the tile has two independent chains -
// inner rings: ring-wise FFT -> ring-wise HRBL kernel; outer rings: node FFT -> cell-wise HRBL kernel - that touch
// disjoint points.  With SX_OVERLAP=1 the inner chain runs on a second (non-blocking) stream, forked after the vertical
// inverse and joined before the forward transform (measured gain 2.6 %: off by default, see sx_internal.hpp).
void launch_inverse_and_physics(sx_handle *h, int t) {
    struct Scope { sx_handle *h; Scope(sx_handle *x) : h(x) { h->in_advance = true; } ~Scope() { h->in_advance = false; } } scope(h);
    const bool two = h->node_mode && h->R_in > 0 && h->sw.overlap && h->eq == SX_EQ_ONEWAY_SW_HRBL && !h->semi;
    if (!two) {
        launch_rl_inverse(h, false);
        launch_physics(h, t);
        return;
    }
    h->node_active = 1;
    if (!h->stream2) {
        HIPCHK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    }
    hipStream_t s0 = h->stream;
    HIPCHK(hipEventRecord(h->ev_fork, s0));
    HIPCHK(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
    h->stream = h->stream2;                                  // launchers and timers follow h->stream
    launch_rl_inverse_fft(h, h->d_mask_eq, h->R_in);
    launch_physics_part(h, t, 1);
    HIPCHK(hipEventRecord(h->ev_join, h->stream2));
    h->stream = s0;
    launch_node_fft(h);
    // overlap = 2: only the node FFT shares the chip with the inner chain; the cell-wise equation-set kernel (the dominant
    // one, whose event-timed duration is the roofline measurement) starts after the join and runs alone
    if (h->sw.overlap == 2) HIPCHK(hipStreamWaitEvent(s0, h->ev_join, 0));
    launch_physics_part(h, t, 2);
    if (h->sw.overlap != 2) HIPCHK(hipStreamWaitEvent(s0, h->ev_join, 0));
}

}  // namespace sx
