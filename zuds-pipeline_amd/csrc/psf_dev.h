// PSF photometry (DESIGN.md "PSF photometry"): the Lanczos-3 taps and the body of one fit, shared by k_psf_fit and
// k_psf_batch (psf.hip) the way ap_wave_sum serves k_aperture and k_lc_batch, so that the two cannot drift apart.
#pragma once
#include "zm_internal.h"

// comparisons against radii are meant as the plain IEEE operations a float64 restatement performs; this also keeps the
// fit the same instruction sequence in both kernels that inline it
#pragma clang fp contract(off)

#define PSF_PI 3.14159265358979323846
#define PSF_BOX_MAX 27           // pixels across the box of a fit: 2 (ceil(R) + 1) + 1 with R <= ZM_PSF_HALF_MAX - 3.5

// sinc(u) sinc(u / 3)
__device__ __forceinline__ double psf_lanczos3(double u) {
    if (u == 0.0) return 1.0;
    const double a = PSF_PI * u;
    return (sinpi(u) / a) * (sinpi(u / 3.0) / (a / 3.0));
}

// The six taps at offsets -2 .. 3 from the floor sample for the fractional part d, scaled to unit sum.  d == 0: a delta
// (the caller then takes the single sample as the footprint on that axis).
__device__ __forceinline__ void psf_taps(double d, double t[6]) {
    if (d == 0.0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) t[k] = k == 2 ? 1.0 : 0.0;
        return;
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        t[k] = psf_lanczos3(d - (double)(k - 2));
        s += t[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] /= s;
}

__device__ __forceinline__ double psf_wave_add(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int psf_wave_or(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

struct psf_fit_out {
    double flux, err, chi2, sky, cover;
    int32_t npix, flags;
};

// One wave, one fit.  sm: the model in LDS, (2 half + 1)^2 doubles, already visible to every lane; sP: PSF_BOX_MAX^2
// doubles of LDS owned by this wave (each lane reads back only what it wrote).  (x, y) is the 0-based position.  Every
// lane calls it with its lane number and gets the same results.  The walk over the box is made three times: the
// weights and the weighted mean of the profile, the normal sums about that mean (the 2 x 2 system of {flux, sky} without
// the cancellation of its determinant), the residuals.
__device__ __forceinline__ void psf_wave_fit(const double* sm, int half, double* sP, const float* __restrict__ img,
                                             const float* __restrict__ rms, const int32_t* __restrict__ mask,
                                             int32_t bad_bits, int nx, int ny, double x, double y, double R, int fit_sky,
                                             int lane, psf_fit_out* o) {
    const double qnan = __builtin_nan("");
    o->flux = o->err = o->chi2 = o->sky = o->cover = qnan;
    o->npix = 0;
    if (!(isfinite(x) && isfinite(y))) {
        o->flags = ZM_PSF_BADPOS;
        return;
    }
    const double ixd = floor(x + 0.5), iyd = floor(y + 0.5);
    const double fx = x - ixd, fy = y - iyd;
    const int m = min((int)ceil(R) + 1, (PSF_BOX_MAX - 1) / 2), bw = 2 * m + 1, mw = 2 * half + 1;
    // the model at (i - fx, j - fy): floor sample i + ox, fractional part dx, the same for every pixel of the fit
    const double dx = fx > 0.0 ? 1.0 - fx : -fx, dy = fy > 0.0 ? 1.0 - fy : -fy;
    const int ox = (fx > 0.0 ? -1 : 0) + half - 2, oy = (fy > 0.0 ? -1 : 0) + half - 2;
    double tx[6], ty[6];
    psf_taps(dx, tx);
    psf_taps(dy, ty);
    const double R2 = R * R;

    double Sw = 0.0, SwP = 0.0, Pall = 0.0, Pused = 0.0;
    int n = 0, fl = 0;
    unsigned used = 0;
    {
        int it = 0;
        for (int e = lane; e < bw * bw; e += 64, ++it) {
            const int j = e / bw - m, i = e % bw - m;
            const double ddx = (double)i - fx, ddy = (double)j - fy;
            if (!(ddx * ddx + ddy * ddy <= R2)) continue;
            const double px = ixd + (double)i, py = iyd + (double)j;
            if (px < 0.0 || py < 0.0 || px >= (double)nx || py >= (double)ny) {
                fl |= ZM_PSF_CLIPPED;
                continue;
            }
            double P = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const int r = j + oy + a;
                double acc = 0.0;
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    const int c = i + ox + b;
                    const double mv = ((unsigned)r < (unsigned)mw && (unsigned)c < (unsigned)mw) ? sm[r * mw + c] : 0.0;
                    acc += tx[b] * mv;
                }
                P += ty[a] * acc;
            }
            sP[e] = P;
            Pall += P;
            const size_t idx = (size_t)(int)py * nx + (int)px;
            bool ok = true;
            if (!isfinite(img[idx])) {
                fl |= ZM_PSF_NONFINITE;
                ok = false;
            }
            if (mask && (mask[idx] & bad_bits)) {
                fl |= ZM_PSF_BAD;
                ok = false;
            }
            double w = 1.0;
            if (rms) {
                const double s = rms[idx];
                if (isfinite(s) && s > 0.0) {
                    w = 1.0 / (s * s);
                } else {
                    fl |= ZM_PSF_BADRMS;
                    ok = false;
                }
            }
            if (ok) {
                used |= 1u << it;
                Sw += w;
                SwP += w * P;
                Pused += P;
                ++n;
            }
        }
    }
    Sw = psf_wave_add(Sw);
    SwP = psf_wave_add(SwP);
    Pall = psf_wave_add(Pall);
    Pused = psf_wave_add(Pused);
    n = (int)psf_wave_add((double)n);
    fl = psf_wave_or(fl);

    const double pbar = fit_sky ? SwP / Sw : 0.0;
    double Sxx = 0.0, Sxd = 0.0, Swd = 0.0;
    {
        int it = 0;
        for (int e = lane; e < bw * bw; e += 64, ++it) {
            if (!((used >> it) & 1u)) continue;
            const int j = e / bw - m, i = e % bw - m;
            const size_t idx = (size_t)((int)iyd + j) * nx + ((int)ixd + i);
            double w = 1.0;
            if (rms) {
                const double s = rms[idx];
                w = 1.0 / (s * s);
            }
            const double d = img[idx], q = sP[e] - pbar;
            Sxx += w * (q * q);
            Sxd += w * (q * d);
            Swd += w * d;
        }
    }
    Sxx = psf_wave_add(Sxx);
    Sxd = psf_wave_add(Sxd);
    Swd = psf_wave_add(Swd);
    const int nparam = fit_sky ? 2 : 1;
    const bool singular = n < nparam || !(Sxx > 0.0);
    const double flux = Sxd / Sxx;
    const double sky = fit_sky ? (Swd - flux * SwP) / Sw : 0.0;
    double chi2 = 0.0;
    {
        int it = 0;
        for (int e = lane; e < bw * bw; e += 64, ++it) {
            if (!((used >> it) & 1u)) continue;
            const int j = e / bw - m, i = e % bw - m;
            const size_t idx = (size_t)((int)iyd + j) * nx + ((int)ixd + i);
            double w = 1.0;
            if (rms) {
                const double s = rms[idx];
                w = 1.0 / (s * s);
            }
            const double r = ((double)img[idx] - flux * sP[e]) - sky;
            chi2 += w * (r * r);
        }
    }
    chi2 = psf_wave_add(chi2);
    double err = 1.0 / sqrt(Sxx);
    if (!rms) err = n > nparam ? err * sqrt(chi2 / (double)(n - nparam)) : qnan;
    const double cover = Pused / Pall;
    if (cover < 0.5) fl |= ZM_PSF_LOWCOVER;
    o->npix = n;
    if (singular) {
        o->flags = fl | ZM_PSF_SINGULAR;
        return;
    }
    o->flux = flux;
    o->err = err;
    o->chi2 = chi2;
    o->sky = sky;
    o->cover = cover;
    o->flags = fl;
}
