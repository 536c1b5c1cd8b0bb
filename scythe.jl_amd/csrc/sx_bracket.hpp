// The bracket iteration that refines one crossing of sx_crossings (a radius along a ray) and sx_isosurface (a height in a column) -
// the function sx_bracket_step runs on the host.  scan_crossings of sx_point.hpp drives it on the device for both, so that a radius
// and a height are refined by the same steps.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace sx {

// The bracket of one crossing: d = g - c changes sign between a (inner) and b (outer); fa, fb are d there, ga, gb the values the false
// position is drawn through (an end kept twice in a row has its value halved: Illinois), x the trial point whose d the next step takes
struct Bracket {
    double a, fa, b, fb, ga, gb, x;
    int side, bis;                        // the end the last step replaced (-1 inner, +1 outer, 0 none yet); next trial by bisection
};
__host__ __device__ inline bool bracket_done(const Bracket &B, double wtol) { return B.fa == 0.0 || B.fb == 0.0 || !(B.b - B.a > wtol); }
__host__ __device__ inline void bracket_trial(Bracket &B) {
    double x = B.b - (B.gb * (B.b - B.a)) / (B.gb - B.ga);
    if (B.bis || !(x > B.a && x < B.b)) x = B.a + 0.5 * (B.b - B.a);
    B.x = x;
}
// 0: finished, -1: evaluate d at x and step
__host__ __device__ inline int bracket_start(Bracket &B, double wtol) {
    B.ga = B.fa; B.gb = B.fb; B.side = 0; B.bis = 0; B.x = B.a;
    if (bracket_done(B, wtol)) return 0;
    bracket_trial(B);
    return -1;
}
// One step with fx = d(x): 0 finished, -1 go on, 2 fx is NaN (the bracket stays).  The bracket always holds the sign change; a step
// that does not halve it is followed by a bisection.
__host__ __device__ inline int bracket_step(Bracket &B, double fx, double wtol) {
    if (fx != fx) return 2;
    const double w0 = B.b - B.a;
    if (fx == 0.0) { B.a = B.b = B.x; B.fa = B.fb = B.ga = B.gb = 0.0; return 0; }
    if ((fx < 0.0) == (B.fa < 0.0)) {
        B.a = B.x; B.fa = B.ga = fx;
        if (B.side < 0) B.gb *= 0.5;
        B.side = -1;
    } else {
        B.b = B.x; B.fb = B.gb = fx;
        if (B.side > 0) B.ga *= 0.5;
        B.side = 1;
    }
    B.bis = B.b - B.a > 0.5 * w0;
    if (bracket_done(B, wtol)) return 0;
    bracket_trial(B);
    return -1;
}
// the end with the smaller |d|, the inner one on a tie
__host__ __device__ inline double bracket_root(const Bracket &B) { return fabs(B.fa) <= fabs(B.fb) ? B.a : B.b; }

}  // namespace sx
