// Exact circle / pixel overlap as a signed sum of quarter-box areas (oracle/photometry.py), shared by the units
// that sum over an aperture: photometry.hip (k_aperture), lightcurve.hip (k_lc_batch) and detect.hip (k_candidate_cuts).
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

// One wave, one aperture: the body of k_aperture, shared with k_lc_batch (lightcurve.hip) so that the two cannot drift
// apart.  (xc, yc) is the 0-based centre; every lane of the wave calls it with its lane number and gets the same three
// results back: flux = sum(img frac), err = sqrt(sum(rms^2 frac)), flags = OR of mask over the clipped bounding box.
__device__ __forceinline__ void ap_wave_sum(const float* __restrict__ img, const float* __restrict__ rms,
                                            const int32_t* __restrict__ mask, int nx, int ny, double xc, double yc, double r,
                                            int lane, double* flux, double* err, int32_t* flags) {
    int ixmin = 0, ixmax = 0, iymin = 0, iymax = 0;
    if (isfinite(xc) && isfinite(yc)) {
        // photutils BoundingBox.from_float(x - r, x + r, y - r, y + r), clipped to the frame.  The bounds are
        // clamped to [-1, n + 1] while still double: a double outside int's range has no defined conversion
        ixmin = max((int)fmin(fmax(floor(xc - r + 0.5), -1.0), nx + 1.0), 0);
        ixmax = min((int)fmin(fmax(ceil(xc + r + 0.5), -1.0), nx + 1.0), nx);
        iymin = max((int)fmin(fmax(floor(yc - r + 0.5), -1.0), ny + 1.0), 0);
        iymax = min((int)fmin(fmax(ceil(yc + r + 0.5), -1.0), ny + 1.0), ny);
    }
    const int bw = ixmax - ixmin, bh = iymax - iymin;
    double f = 0.0, v = 0.0;
    int fl = 0;
    if (bw > 0 && bh > 0) {
        for (int e = lane; e < bw * bh; e += 64) {
            const int j = iymin + e / bw, i = ixmin + e % bw;
            const double x0 = i - 0.5 - xc, x1 = i + 0.5 - xc, y0 = j - 0.5 - yc, y1 = j + 0.5 - yc;
            const double frac = ap_signed(x1, y1, r) - ap_signed(x0, y1, r) - ap_signed(x1, y0, r) +
                                ap_signed(x0, y0, r);
            const size_t idx = (size_t)j * nx + i;
            f += (double)img[idx] * frac;
            if (rms) { double s = rms[idx]; v += s * s * frac; }
            if (mask) fl |= mask[idx];
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        f += __shfl_xor(f, o);
        v += __shfl_xor(v, o);
        fl |= __shfl_xor(fl, o);
    }
    *flux = f;
    // a finite sum that rounds below 0 is 0; one that is not finite stays so (fmax alone would turn a NaN
    // variance into an error of 0)
    *err = sqrt(isfinite(v) ? fmax(v, 0.0) : v);
    *flags = fl;
}
