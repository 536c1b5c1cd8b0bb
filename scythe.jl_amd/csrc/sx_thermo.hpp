// The moist thermodynamics of Euler_test and rainfall_test, stated once for the equation-set kernels (sx_physics.hip) and for the
// function programs of sx_derive (sx_derive.hip): a diagnosed temperature is formed by the very code the model steps with.  The
// functions are host and device so that sx_derive_point can state a composite on the host.
#pragma once
#include "sx_internal.hpp"

namespace sx {
// Moist thermodynamics of Euler_test and rainfall_test (src/thermodynamics.jl; constants :2-17, :31-32)
namespace thermo {
constexpr double Rd = 287.04, Rv = 461.50, Cvd = 716.96, Cvv = 1410.0, gravity = 9.81, L_v0 = 2.501e6, T_0 = 273.16, p_0 = 1000.0,
                 q0 = 1.0e-7;
constexpr double rho_d0 = 100.0 * p_0 / (T_0 * Rd);
// rho_v0 = 100 sat_pressure_liquid(T_0) / (T_0 Rv), sat_pressure_liquid(T) = 6.112 exp(17.67 Tc / (Tc + 243.5)) (:19-23, :32)
__host__ __device__ __forceinline__ double rho_v0() { const double Tc = T_0 - 273.15; return 100.0 * (6.112 * exp(17.67 * Tc / (Tc + 243.5))) / (T_0 * Rv); }
__host__ __device__ __forceinline__ double ahyp(double mu) { return mu < 0.0 ? 0.0 : sqrt(mu * mu + q0 * q0) + mu - q0; }            // :190-198
__host__ __device__ __forceinline__ double dmudq(double mu, double q_v) { return ((q_v + q0) - mu) / (q_v + q0); }                    // :200-203
__host__ __device__ __forceinline__ double dry_density(double xi) { return rho_d0 * exp(xi); }                                        // :205-208
__host__ __device__ __forceinline__ double temperature(double s, double rho_d, double q_v) {                                          // :67-80
    const double Cf = Cvd + (q_v * Cvv);
    double qf = 1.0;
    if (q_v != 0.0) qf = pow(rho_d * q_v / rho_v0(), (q_v * Rv) / Cf);
    const double rf = pow(rho_d / rho_d0, Rd / Cf);
    const double Tf = exp((s - (q_v * L_v0 / T_0)) / Cf);
    return T_0 * Tf * rf * qf;
}
__host__ __device__ __forceinline__ double P_s(double Tk, double rho_d, double q_v) {                                                 // :215-219
    return Tk * ((rho_d * Rd) + (q_v * rho_d * Rv)) / (Cvd + (q_v * Cvv));
}
__host__ __device__ __forceinline__ double P_xi(double Tk, double rho_d, double q_v) {                                                // :221-224
    return (Rd + (q_v * rho_d * Rv)) * ((rho_d * Tk) + P_s(Tk, rho_d, q_v));
}
__host__ __device__ __forceinline__ double P_qv(double Tk, double rho_d, double q_v) {                                                // :232-242
    if (q_v == 0.0) return 0.0;
    const double rho_v = q_v * rho_d;
    double qf = Rv * (1 + log(rho_v / rho_v0())) - (Cvv * log(Tk / T_0)) - L_v0 / T_0;
    qf *= P_s(Tk, rho_d, q_v);
    return (rho_d * Rv * Tk) + qf;
}
__host__ __device__ __forceinline__ double pressure_gradient(double Tk, double rho_d, double q_v, double s_x, double xi_x, double qv_x) {   // :250-258
    return (P_s(Tk, rho_d, q_v) * s_x) + (P_xi(Tk, rho_d, q_v) * xi_x) + (P_qv(Tk, rho_d, q_v) * qv_x);
}
// rainfall_test's additions: the constants Cl, Cpd, Cpv, Eps (:2-17), the saturation functions (:82-186) and Ooyama's (2001) warm
// rain (src/microphysics.jl:84-137, 197-261), each written expression by expression as in the reference (Julia's x^2 is x * x)
constexpr double Cl = 4186.0, Cpd = Cvd + Rd, Cpv = Cvv + Rv, Eps = Rd / Rv;
__host__ __device__ __forceinline__ double L_v(double Tk) { return L_v0 + ((Cpv - Cl) * (Tk - T_0)); }                             // :41-44
// p of thermodynamic_tuple (:260-269), total pressure in hPa
__host__ __device__ __forceinline__ double pressure(double Tk, double rho_d, double q_v) {
    return (0.01 * Rd * Tk * rho_d) + (0.01 * Rv * Tk * rho_d * q_v);
}
__host__ __device__ __forceinline__ double vapor_pressure(double p, double q_v) { return (p * q_v) / (Eps + q_v); }                  // :89-94
__host__ __device__ __forceinline__ double sat_pressure_liquid_buck(double Tk, double phPa) {                                        // :101-118
    const double Tc = Tk - 273.15;
    const double A = 7.2e-4, B = 3.20e-6, C = 5.9e-10;
    const double fw4 = 1.0 + A + (phPa * (B + (C * (Tc * Tc))));
    const double a = 6.1121, b = 18.729, c = 257.87, d = 227.3;
    const double ew4 = a * exp((b - (Tc / d)) * Tc / (Tc + c));
    return fw4 * ew4;
}
__host__ __device__ __forceinline__ double sat_pressure_liquid_buck_dT(double Tk, double phPa) {                                     // :120-142
    const double Tc = Tk - 273.15;
    const double A = 7.2e-4, B = 3.20e-6, C = 5.9e-10;
    const double fw4 = 1.0 + A + (phPa * (B + (C * (Tc * Tc))));
    const double d_fw4 = 2.0 * phPa * C * Tc;
    const double a = 6.1121, b = 18.729, c = 257.87, d = 227.3;
    const double ew4 = a * exp((b - (Tc / d)) * Tc / (Tc + c));
    const double T1 = (d * b - (2.0 * Tc)) * (d * (Tc + c)) - d * ((d * b * Tc) - (Tc * Tc));
    const double dTc = d * (Tc + c);
    const double T2 = dTc * dTc;
    const double d_ew4 = ew4 * T1 / T2;
    return ew4 * d_fw4 + fw4 * d_ew4;
}
__host__ __device__ __forceinline__ double q_sat_liquid(double Tk, double phPa) {                                                    // :163-170
    const double ew = sat_pressure_liquid_buck(Tk, phPa);
    return Eps * ew / (phPa - ew);
}
__host__ __device__ __forceinline__ double cp_moist(double q_v, double q_l) { return Cpd + (q_v * Cpv) + (q_l * Cl); }
// dq_sat/dT of Q_s_factor and dqsdp (src/microphysics.jl:107-124)
__host__ __device__ __forceinline__ double dqsdT(double Tk, double p, double e_s) {
    const double pe = p - e_s;
    return sat_pressure_liquid_buck_dT(Tk, p) * Eps * p / (pe * pe);
}
__host__ __device__ __forceinline__ double Q_s_factor(double Tk, double p, double q_v, double q_l) {                                 // microphysics.jl:107-114
    const double e_s = sat_pressure_liquid_buck(Tk, p);
    return L_v(Tk) * dqsdT(Tk, p, e_s) / cp_moist(q_v, q_l);
}
__host__ __device__ __forceinline__ double dqsdp(double Tk, double p, double rho_d, double q_v, double q_l) {                        // :116-124
    const double q_sat = q_sat_liquid(Tk, p);
    const double e_s = sat_pressure_liquid_buck(Tk, p);
    return (q_sat / (100.0 * (p - e_s)) - (dqsdT(Tk, p, e_s) / (rho_d * cp_moist(q_v, q_l))));
}
__host__ __device__ __forceinline__ double vapor_diffusity(double Tk, double p) { return 0.211 * pow(Tk / 273.15, 1.94) * (1013.25 / p); }   // :134-140
__host__ __device__ __forceinline__ double invtau_condensation(double Tk, double p, double N_c, double r_c) {                         // :126-132
    return 4.0 * M_PI * vapor_diffusity(Tk, p) * N_c * (r_c * 1.0e-4);
}
// Julia's scalar min / max on Float64: NaN propagates and -0.0 < 0.0
__host__ __device__ __forceinline__ double jl_min(double x, double y) {
    return ((y < x) || (signbit(y) > signbit(x))) ? (isnan(x) ? x : y) : (isnan(y) ? y : x);
}
__host__ __device__ __forceinline__ double jl_max(double x, double y) {
    return ((y > x) || (signbit(y) < signbit(x))) ? (isnan(x) ? x : y) : (isnan(y) ? y : x);
}
// Julia's isequal / isless on Float64 (the element comparisons of cmp on vectors): NaN equals NaN and is above every number,
// -0.0 is below 0.0
__host__ __device__ __forceinline__ bool jl_isequal(double x, double y) {
    return (isnan(x) && isnan(y)) || ((signbit(x) == signbit(y)) && (x == y));
}
__host__ __device__ __forceinline__ bool jl_isless(double x, double y) {
    return (!isnan(x) && (isnan(y) || (signbit(x) && !signbit(y)))) || (x < y);
}
__host__ __device__ __forceinline__ double q_condensation(double qss, double Tk, double p, double q_v, double q_l, double N_c,       // :84-93
                                                 double r_c) {
    const double Q_s = Q_s_factor(Tk, p, q_v, q_l);
    double q_cond = qss / (1.0 + Q_s);
    q_cond = jl_min(q_v, q_cond);              // broadcast in the reference: elementwise
    q_cond = jl_max(-q_l, q_cond);
    return q_cond * invtau_condensation(Tk, p, N_c, r_c);
}
__host__ __device__ __forceinline__ double s_condensation(double q_cond, double Tk, double rho_d, double q_v, double q_l, double p) {   // :96-105
    const double Cm = (q_l * Cl) / (Cvd + (q_v * Cvv) + (q_l * Cl));
    const double e = vapor_pressure(p, q_v);
    const double sat_e = sat_pressure_liquid_buck(Tk, p);
    return q_cond * (((-L_v(Tk) * Cm) / Tk) - (Cl * log(Tk / T_0)) + (Rv * log(e / sat_e)));
}
__host__ __device__ __forceinline__ double autoconversion(double q_c, double rho_d) {                                                              // :197-206
    double q_auto = 0.001 * (q_c - 0.001);
    if (q_auto < 0.0) q_auto = 0.0;
    return q_auto;
}
__host__ __device__ __forceinline__ double f_ice(double Tk) {                                                                         // :219-227
    if (Tk < 273.15) return 0.2 + 0.8 * (1.0 / cosh((273.15 - Tk) / 5.0));
    return 1.0;
}
__host__ __device__ __forceinline__ double collection(double q_c, double q_r, double rho_d, double Tk) {                                           // :208-217
    double q_coll = 2.20 * q_c * pow(q_r, 0.875) * f_ice(Tk);
    if (q_coll < 0.0) q_coll = 0.0;
    return q_coll;
}
__host__ __device__ __forceinline__ double f_ventilation(double q_r, double rho_d, double Tk) {                                      // :243-250
    const double rho_r = q_r * rho_d;
    double f_vent = 1.6 + 30.39 * pow(rho_r, 0.2046) * pow(f_ice(Tk), 1.5);
    if (f_vent < 0.0) f_vent = 0.0;
    return f_vent;
}
__host__ __device__ __forceinline__ double rain_evaporation(double q_r, double rho_d, double Tk, double p) {                         // :229-241
    const double e_s = sat_pressure_liquid_buck(Tk, p);
    const double rho_vs = e_s / (Rv * Tk);
    const double rho_r = q_r * rho_d;
    double q_evap = (f_ventilation(q_r, rho_d, Tk) * pow(rho_r, 0.525)) / (1.0e4 * ((2.03 * rho_vs) + (3.337 / Tk)));
    if (q_evap < 0.0) q_evap = 0.0;
    return q_evap;
}
// :252-261.  Vt is -14.164 times a non-negative number and then clamped at 0 from below, so it is 0.0 or -0.0 for every finite
// state: k_phys_rain drops the flux divergence it feeds (src/testModels.jl:524-528) and never calls this
__host__ __device__ __forceinline__ double sedimentation(double q_r, double rho_d, double Tk) {
    const double rho_r = q_r * rho_d;
    double Vt = -14.164 * pow(rho_r, 0.1364) * pow(rho_d0 / rho_d, 0.5) * f_ice(Tk);
    if (Vt < 0.0) Vt = 0.0;
    return Vt;
}
}  // namespace thermo

}  // namespace sx
