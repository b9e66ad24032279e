// Exact circle / pixel overlap as a signed sum of quarter-box areas (oracle/photometry.py), shared by the units
// that sum over an aperture: photometry.hip (k_aperture) and detect.hip (k_candidate_cuts).
#pragma once
#include "zm_internal.h"

__device__ inline double ap_P(double u, double r) {
    double v = fmax(r * r - u * u, 0.0);
    double t = fmin(fmax(u / r, -1.0), 1.0);
    return 0.5 * (u * sqrt(v) + r * r * asin(t));
}

__device__ inline double ap_quarter(double x, double y, double r) {
    x = fmin(x, r);
    y = fmin(y, r);
    if (x * x + y * y <= r * r) return x * y;
    double xc = sqrt(fmax(r * r - y * y, 0.0));
    double xm = fmin(x, xc);
    return y * xm + ap_P(x, r) - ap_P(xm, r);
}

__device__ inline double ap_signed(double x, double y, double r) {
    double s = ((x > 0) - (x < 0)) * ((y > 0) - (y < 0));
    return s * ap_quarter(fabs(x), fabs(y), r);
}
