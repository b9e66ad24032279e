// PSF-fit forced photometry on resident planes (DESIGN.md "PSF photometry"): the star model and the batched fits.  This
// operator is the project's own; the reference has no PSF photometry.
//
//   k_psf_cutouts   one wave per star: the (2h + 1)^2 Lanczos-3 samples of (img - sky) / norm about its centroid, the 12
//                   taps made once per star; NaN where a tap of the footprint is off the frame, not finite or masked
//   (zm_clipped_median_dev, photcal.hip: the clipped median over the stars of every entry)
//   k_psf_finish    one wave: support (NORM_RADIUS), the floor on n_used, unit sum
//   k_psf_fit       one wave per position: the model into LDS, then psf_wave_fit (psf_dev.h)
//   k_psf_batch     one wave per (image, source) pair of a footprint join: the image by the binary search of k_lc_batch,
//                   sky -> pixel with the image's WCS (zm_plane2pix), the image's model into LDS, then psf_wave_fit
//
// Every sum is fp64 in a fixed order (lane-strided walk, xor-shuffle tree): no float atomics, the same bits on every run.
#include <algorithm>
#include <cmath>

#include "wcs_math.h"
#include "psf_dev.h"

#define PSF_MODEL_MAX ((2 * ZM_PSF_HALF_MAX + 1) * (2 * ZM_PSF_HALF_MAX + 1))
#define PSF_MAX_GRID (1 << 24)
#define PSF_D2R 0.017453292519943295

struct psf_rec {                      // one image of the batch, uniform across a wave
    const float* img;
    const float* rms;                 // or NULL
    const int32_t* mask;              // or NULL
    const double* model;
    int32_t nx, ny, half, pad_;
    double fr[9];                     // zm_wcs_frame of wcs
    zm_wcs wcs;                       // private copy, TPV order marked
};

__global__ __launch_bounds__(64) void k_psf_cutouts(const float* __restrict__ img, const int32_t* __restrict__ mask,
                                                    int32_t bad_bits, int nx, int ny, int nstar,
                                                    const double* __restrict__ xs, const double* __restrict__ ys,
                                                    const double* __restrict__ skys, const double* __restrict__ norms,
                                                    int half, double* __restrict__ out, long long stride) {
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= nstar) return;
    const int w = 2 * half + 1, ne = w * w;
    double* __restrict__ row = out + (size_t)s * stride;
    const double xc = xs[s], yc = ys[s], sky = skys[s], norm = norms[s];
    if (!(isfinite(xc) && isfinite(yc) && isfinite(sky) && isfinite(norm) && norm > 0.0)) {
        for (int e = lane; e < ne; e += 64) row[e] = __builtin_nan("");
        return;
    }
    const double x0 = floor(xc), y0 = floor(yc);
    const double dx = xc - x0, dy = yc - y0;
    double tx[6], ty[6];
    psf_taps(dx, tx);
    psf_taps(dy, ty);
    const bool onex = dx == 0.0, oney = dy == 0.0;      // a delta: the footprint on that axis is the single sample
    for (int e = lane; e < ne; e += 64) {
        const int j = e / w - half, i = e % w - half;
        double acc = 0.0;
        bool bad = false;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            if (oney && a != 2) continue;
            const double py = y0 + (double)(j + a - 2);
            double racc = 0.0;
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                if (onex && b != 2) continue;
                const double px = x0 + (double)(i + b - 2);
                if (px < 0.0 || py < 0.0 || px >= (double)nx || py >= (double)ny) {
                    bad = true;
                    continue;
                }
                const size_t idx = (size_t)(int)py * nx + (int)px;
                const float v = img[idx];
                if (!isfinite(v) || (mask && (mask[idx] & bad_bits))) {
                    bad = true;
                    continue;
                }
                racc += tx[b] * ((double)v - sky);
            }
            acc += ty[a] * racc;
        }
        row[e] = bad ? __builtin_nan("") : acc / norm;
    }
}

// o4: {median, sigma, n_used, n_valid} per entry, as zm_clipped_median_dev leaves them
__global__ __launch_bounds__(64) void k_psf_finish(const double* __restrict__ o4, int half, double norm_radius,
                                                   int min_stars_pixel, double* __restrict__ model,
                                                   int32_t* __restrict__ n_used) {
    const int lane = threadIdx.x, w = 2 * half + 1, ne = w * w;
    const double r2 = norm_radius * norm_radius;
    double sum = 0.0;
    for (int e = lane; e < ne; e += 64) {
        const int j = e / w - half, i = e % w - half;
        const double med = o4[4 * (size_t)e];
        const int nu = (int)o4[4 * (size_t)e + 2];
        const bool keep = (double)(i * i + j * j) <= r2 && nu >= min_stars_pixel && isfinite(med);
        const double v = keep ? med : 0.0;
        model[e] = v;
        n_used[e] = nu;
        sum += v;
    }
    sum = psf_wave_add(sum);
    const bool good = isfinite(sum) && sum > 0.0;       // a model without a positive sum has no scale: every entry NaN
    for (int e = lane; e < ne; e += 64) model[e] = good ? model[e] / sum : __builtin_nan("");
}

__device__ __forceinline__ void psf_stage_model(const double* __restrict__ model, int half, double* sm, int lane) {
    const int ne = (2 * half + 1) * (2 * half + 1);
    for (int e = lane; e < ne; e += 64) sm[e] = model[e];
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_psf_fit(const float* __restrict__ img, const float* __restrict__ rms,
                                                const int32_t* __restrict__ mask, int32_t bad_bits, int nx, int ny,
                                                int npos, const double* __restrict__ xs, const double* __restrict__ ys,
                                                const double* __restrict__ model, int half, double R, int fit_sky,
                                                double* __restrict__ flux, double* __restrict__ err,
                                                double* __restrict__ chi2, double* __restrict__ sky,
                                                double* __restrict__ cover, int32_t* __restrict__ npix,
                                                int32_t* __restrict__ flags) {
    __shared__ double sm[PSF_MODEL_MAX];
    __shared__ double sP[PSF_BOX_MAX * PSF_BOX_MAX];
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= npos) return;
    psf_stage_model(model, half, sm, lane);
    psf_fit_out o;
    psf_wave_fit(sm, half, sP, img, rms, mask, bad_bits, nx, ny, xs[k], ys[k], R, fit_sky, lane, &o);
    if (lane == 0) {
        flux[k] = o.flux;
        err[k] = o.err;
        chi2[k] = o.chi2;
        sky[k] = o.sky;
        cover[k] = o.cover;
        npix[k] = o.npix;
        flags[k] = o.flags;
    }
}

// One wave per pair (grid = npairs, strided beyond PSF_MAX_GRID); the pair index comes from blockIdx.x, so the search
// and every field of the image's record are uniform.
__global__ __launch_bounds__(64) void k_psf_batch(const psf_rec* __restrict__ recs, int nimg,
                                                  const long long* __restrict__ offsets,
                                                  const int32_t* __restrict__ src_idx, long long npairs, int nsrc,
                                                  const double* __restrict__ ra, const double* __restrict__ dec,
                                                  int32_t bad_bits, double R, int fit_sky, double* __restrict__ xo,
                                                  double* __restrict__ yo, double* __restrict__ flux,
                                                  double* __restrict__ err, double* __restrict__ chi2,
                                                  double* __restrict__ sky, double* __restrict__ cover,
                                                  int32_t* __restrict__ npix, int32_t* __restrict__ flags) {
    __shared__ double sm[PSF_MODEL_MAX];
    __shared__ double sP[PSF_BOX_MAX * PSF_BOX_MAX];
    const int lane = threadIdx.x;
    for (long long p = blockIdx.x; p < npairs; p += gridDim.x) {
        int lo = 0, hi = nimg;                           // offsets[lo] <= p < offsets[hi], whatever lies between
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= p) lo = mid; else hi = mid;
        }
        const psf_rec* __restrict__ Q = recs + lo;
        const int s = src_idx[p];
        double x = __builtin_nan(""), y = x;
        if (s >= 0 && s < nsrc) {
            // zm_wcs_sky2pix, step by step (as k_lc_batch)
            const double a = ra[s] * PSF_D2R, d = dec[s] * PSF_D2R;
            const double v[3] = {cos(d) * cos(a), cos(d) * sin(a), sin(d)};
            double ta = 0, tb = 0, tc = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ta += v[k] * Q->fr[k];
                tb += v[k] * Q->fr[3 + k];
                tc += v[k] * Q->fr[6 + k];
            }
            zm_plane2pix(&Q->wcs, ta / tc / PSF_D2R, tb / tc / PSF_D2R, &x, &y);
            x -= 1.0;                                    // FITS 1-based -> 0-based
            y -= 1.0;
        }
        __syncthreads();                                 // the model of the pair before is no longer read
        psf_stage_model(Q->model, Q->half, sm, lane);
        psf_fit_out o;
        psf_wave_fit(sm, Q->half, sP, Q->img, Q->rms, Q->mask, bad_bits, Q->nx, Q->ny, x, y, R, fit_sky, lane, &o);
        if (lane == 0) {
            xo[p] = x;
            yo[p] = y;
            flux[p] = o.flux;
            err[p] = o.err;
            chi2[p] = o.chi2;
            sky[p] = o.sky;
            cover[p] = o.cover;
            npix[p] = o.npix;
            flags[p] = o.flags;
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
static int psf_check_half(const char* who, int half) {
    ZM_CHECK(half >= 1 && half <= ZM_PSF_HALF_MAX, "%s: half %d outside 1 .. %d", who, half, ZM_PSF_HALF_MAX);
    return 0;
}

static int psf_check_radius(const char* who, double R, int half) {
    ZM_CHECK(R > 0 && std::isfinite(R), "%s: fit radius %g must be positive", who, R);
    ZM_CHECK(R + 3.5 <= (double)half, "%s: fit radius %g needs a model of half width >= %g, this one has %d", who, R, R + 3.5,
             half);
    return 0;
}

static int psf_build_check(const char* who, zm_ctx* ctx, const float* img, int nx, int ny, int nstar, const double* x,
                           const double* y, const double* sky, const double* norm, int half, double norm_radius,
                           double kappa, int maxiter, int min_stars_pixel, const double* model, const int32_t* n_used,
                           const double* cutouts, int64_t stride) {
    ZM_CHECK(ctx && img && model && n_used, "%s: null argument", who);
    ZM_CHECK(nx > 0 && ny > 0 && nstar >= 0, "%s: bad sizes", who);
    ZM_TRY(psf_check_half(who, half));
    ZM_CHECK(nstar == 0 || (x && y && sky && norm), "%s: null star arrays", who);
    ZM_CHECK(nstar <= ZM_CLIPMED_NMAX, "%s: %d stars, the clipped median holds at most %d", who, nstar, ZM_CLIPMED_NMAX);
    ZM_CHECK(norm_radius > 0 && std::isfinite(norm_radius), "%s: norm radius %g must be positive", who, norm_radius);
    ZM_CHECK(kappa > 0 && kappa < 1e30 && maxiter >= 0, "%s: bad kappa %g or maxiter %d", who, kappa, maxiter);
    ZM_CHECK(min_stars_pixel >= 0, "%s: min_stars_pixel %d is negative", who, min_stars_pixel);
    ZM_CHECK(!cutouts || stride >= (int64_t)(2 * half + 1) * (2 * half + 1), "%s: cutout stride %lld below %d", who,
             (long long)stride, (2 * half + 1) * (2 * half + 1));
    return 0;
}

extern "C" int zm_psf_build_dev(zm_ctx* ctx, const float* img, const int32_t* mask, int32_t bad_bits, int nx, int ny,
                                int nstar, const double* x, const double* y, const double* sky, const double* norm,
                                int half, double norm_radius, double kappa, int maxiter, int min_stars_pixel,
                                double* out_model, int32_t* out_n_used, double* out_cutouts, int64_t cutout_stride) {
    ZM_TRY(psf_build_check("zm_psf_build_dev", ctx, img, nx, ny, nstar, x, y, sky, norm, half, norm_radius, kappa, maxiter,
                           min_stars_pixel, out_model, out_n_used, out_cutouts, cutout_stride));
    if (nstar == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t ne = (size_t)(2 * half + 1) * (2 * half + 1);
    double* wsp = nullptr;
    ZM_TRY(ctx->get("psf_build", sizeof(double) * (4 * ne + (out_cutouts ? 0 : ne * (size_t)nstar)), (void**)&wsp));
    double* o4 = wsp;
    double* cut = out_cutouts ? out_cutouts : wsp + 4 * ne;
    const int64_t stride = out_cutouts ? cutout_stride : (int64_t)ne;
    {
        zm_scope_timer t(ctx, "psf_cutouts");
        hipLaunchKernelGGL(k_psf_cutouts, dim3(nstar), dim3(64), 0, ctx->stream, img, mask, bad_bits, nx, ny, nstar, x, y,
                           sky, norm, half, cut, (long long)stride);
        ZM_HIP(hipGetLastError());
    }
    ZM_TRY(zm_clipped_median_dev(ctx, cut, nstar, (int)ne, stride, kappa, maxiter, o4));
    zm_scope_timer t(ctx, "psf_finish");
    hipLaunchKernelGGL(k_psf_finish, dim3(1), dim3(64), 0, ctx->stream, o4, half, norm_radius, min_stars_pixel, out_model,
                       out_n_used);
    ZM_HIP(hipGetLastError());
    return 0;
}

static int psf_stage_planes(zm_ctx* ctx, const float* img, const float* rms, const int32_t* mask, int nx, int ny,
                            float** d_img, float** d_rms, int32_t** d_mask) {
    const size_t np = (size_t)nx * ny;
    ZM_TRY(ctx->get("h_img", np * 4, (void**)d_img));
    ZM_HIP(hipMemcpyAsync(*d_img, img, np * 4, hipMemcpyHostToDevice, ctx->stream));
    if (rms) {
        ZM_TRY(ctx->get("h_wgt", np * 4, (void**)d_rms));
        ZM_HIP(hipMemcpyAsync(*d_rms, rms, np * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (mask) {
        ZM_TRY(ctx->get("h_mask", np * 4, (void**)d_mask));
        ZM_HIP(hipMemcpyAsync(*d_mask, mask, np * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    return 0;
}

extern "C" int zm_psf_build(zm_ctx* ctx, const float* img, const int32_t* mask, int32_t bad_bits, int nx, int ny,
                            int nstar, const double* x, const double* y, const double* sky, const double* norm, int half,
                            double norm_radius, double kappa, int maxiter, int min_stars_pixel, double* out_model,
                            int32_t* out_n_used, double* out_cutouts, int64_t cutout_stride) {
    ZM_TRY(psf_build_check("zm_psf_build", ctx, img, nx, ny, nstar, x, y, sky, norm, half, norm_radius, kappa, maxiter,
                           min_stars_pixel, out_model, out_n_used, out_cutouts, cutout_stride));
    if (nstar == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    float *d_img = nullptr, *d_rms = nullptr;
    int32_t* d_mask = nullptr;
    ZM_TRY(psf_stage_planes(ctx, img, nullptr, mask, nx, ny, &d_img, &d_rms, &d_mask));
    const size_t ne = (size_t)(2 * half + 1) * (2 * half + 1), ns = (size_t)nstar;
    // x, y, sky, norm, the model, the cutouts (rows ne apart) as doubles, then n_used
    double* d = nullptr;
    ZM_TRY(ctx->get("h_psf_io", sizeof(double) * (4 * ns + ne + ne * ns) + sizeof(int32_t) * ne, (void**)&d));
    double *d_x = d, *d_y = d + ns, *d_sky = d + 2 * ns, *d_norm = d + 3 * ns, *d_model = d + 4 * ns, *d_cut = d_model + ne;
    int32_t* d_nu = reinterpret_cast<int32_t*>(d_cut + ne * ns);
    ZM_HIP(hipMemcpyAsync(d_x, x, sizeof(double) * ns, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_y, y, sizeof(double) * ns, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_sky, sky, sizeof(double) * ns, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_norm, norm, sizeof(double) * ns, hipMemcpyHostToDevice, ctx->stream));
    ZM_TRY(zm_psf_build_dev(ctx, d_img, d_mask, bad_bits, nx, ny, nstar, d_x, d_y, d_sky, d_norm, half, norm_radius, kappa,
                            maxiter, min_stars_pixel, d_model, d_nu, d_cut, (int64_t)ne));
    ZM_HIP(hipMemcpyAsync(out_model, d_model, sizeof(double) * ne, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_n_used, d_nu, sizeof(int32_t) * ne, hipMemcpyDeviceToHost, ctx->stream));
    if (out_cutouts)
        ZM_HIP(hipMemcpy2DAsync(out_cutouts, sizeof(double) * (size_t)cutout_stride, d_cut, sizeof(double) * ne,
                                sizeof(double) * ne, ns, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

static int psf_fit_check(const char* who, zm_ctx* ctx, const float* img, int nx, int ny, int npos, const double* x,
                         const double* y, const double* model, int half, double R, const void* o1, const void* o2,
                         const void* o3, const void* o4, const void* o5, const void* o6, const void* o7) {
    ZM_CHECK(ctx && img && model && o1 && o2 && o3 && o4 && o5 && o6 && o7, "%s: null argument", who);
    ZM_CHECK(nx > 0 && ny > 0 && npos >= 0, "%s: bad sizes", who);
    ZM_CHECK(npos == 0 || (x && y), "%s: null positions", who);
    ZM_TRY(psf_check_half(who, half));
    ZM_TRY(psf_check_radius(who, R, half));
    return 0;
}

extern "C" int zm_psf_photometry_dev(zm_ctx* ctx, const float* img, const float* rms, const int32_t* mask,
                                     int32_t bad_bits, int nx, int ny, int npos, const double* x, const double* y,
                                     const double* model, int half, double fit_radius, int fit_sky, double* out_flux,
                                     double* out_err, double* out_chi2, double* out_sky, double* out_cover,
                                     int32_t* out_npix, int32_t* out_flags) {
    ZM_TRY(psf_fit_check("zm_psf_photometry_dev", ctx, img, nx, ny, npos, x, y, model, half, fit_radius, out_flux, out_err,
                         out_chi2, out_sky, out_cover, out_npix, out_flags));
    if (npos == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    zm_scope_timer t(ctx, "psf_fit");
    hipLaunchKernelGGL(k_psf_fit, dim3(npos), dim3(64), 0, ctx->stream, img, rms, mask, bad_bits, nx, ny, npos, x, y, model,
                       half, fit_radius, fit_sky ? 1 : 0, out_flux, out_err, out_chi2, out_sky, out_cover, out_npix,
                       out_flags);
    ZM_HIP(hipGetLastError());
    return 0;
}

extern "C" int zm_psf_photometry(zm_ctx* ctx, const float* img, const float* rms, const int32_t* mask, int32_t bad_bits,
                                 int nx, int ny, int npos, const double* x, const double* y, const double* model, int half,
                                 double fit_radius, int fit_sky, double* out_flux, double* out_err, double* out_chi2,
                                 double* out_sky, double* out_cover, int32_t* out_npix, int32_t* out_flags) {
    ZM_TRY(psf_fit_check("zm_psf_photometry", ctx, img, nx, ny, npos, x, y, model, half, fit_radius, out_flux, out_err,
                         out_chi2, out_sky, out_cover, out_npix, out_flags));
    if (npos == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    float *d_img = nullptr, *d_rms = nullptr;
    int32_t* d_mask = nullptr;
    ZM_TRY(psf_stage_planes(ctx, img, rms, mask, nx, ny, &d_img, &d_rms, &d_mask));
    const size_t ne = (size_t)(2 * half + 1) * (2 * half + 1), n = (size_t)npos;
    // x, y, the five float outputs, the model as doubles, then npix and flags
    double* d = nullptr;
    ZM_TRY(ctx->get("h_psf_io", sizeof(double) * (7 * n + ne) + sizeof(int32_t) * 2 * n, (void**)&d));
    double *d_x = d, *d_y = d + n, *d_o = d + 2 * n, *d_model = d + 7 * n;
    int32_t *d_np = reinterpret_cast<int32_t*>(d_model + ne), *d_fl = d_np + n;
    ZM_HIP(hipMemcpyAsync(d_x, x, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_y, y, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_model, model, sizeof(double) * ne, hipMemcpyHostToDevice, ctx->stream));
    ZM_TRY(zm_psf_photometry_dev(ctx, d_img, d_rms, d_mask, bad_bits, nx, ny, npos, d_x, d_y, d_model, half, fit_radius,
                                 fit_sky, d_o, d_o + n, d_o + 2 * n, d_o + 3 * n, d_o + 4 * n, d_np, d_fl));
    double* outs[5] = {out_flux, out_err, out_chi2, out_sky, out_cover};
    for (int k = 0; k < 5; ++k)
        ZM_HIP(hipMemcpyAsync(outs[k], d_o + k * n, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_npix, d_np, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_flags, d_fl, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int zm_psf_photometry_batch_dev(zm_ctx* ctx, int nimg, const zm_psf_image* images, const int64_t* offsets_dev,
                                           const int32_t* src_idx_dev, int64_t npairs, int nsrc, const double* ra_dev,
                                           const double* dec_dev, int32_t bad_bits, double fit_radius, int fit_sky,
                                           double* x_dev, double* y_dev, double* flux_dev, double* err_dev,
                                           double* chi2_dev, double* sky_dev, double* cover_dev, int32_t* npix_dev,
                                           int32_t* flags_dev) {
    const char* who = "zm_psf_photometry_batch_dev";
    ZM_CHECK(ctx, "%s: null argument", who);
    ZM_CHECK(nimg >= 0 && nimg <= 65535, "%s: nimg must be 0 .. 65535 (got %d)", who, nimg);
    ZM_CHECK(nsrc >= 0 && nsrc <= (1 << 30), "%s: nsrc must be 0 .. 2^30 (got %d)", who, nsrc);
    ZM_CHECK(npairs >= 0 && npairs <= 0x7fffffffll, "%s: npairs must be 0 .. 2^31 - 1 (got %lld)", who, (long long)npairs);
    ZM_CHECK(fit_radius > 0 && std::isfinite(fit_radius), "%s: fit radius %g must be positive", who, fit_radius);
    if (npairs == 0) return 0;
    ZM_CHECK(nimg > 0 && nsrc > 0, "%s: %lld pairs of %d images and %d sources", who, (long long)npairs, nimg, nsrc);
    ZM_CHECK(images && offsets_dev && src_idx_dev && ra_dev && dec_dev && x_dev && y_dev && flux_dev && err_dev && chi2_dev &&
                 sky_dev && cover_dev && npix_dev && flags_dev,
             "%s: null argument", who);
    ZM_HIP(hipSetDevice(ctx->device));
    // the pinned table is free to be rewritten once the copy the last call enqueued out of it has finished (the event
    // is the one lightcurve.hip guards its own table with: waiting for either call's copy is enough for both)
    if (ctx->lc_tab_event) ZM_HIP(hipEventSynchronize(ctx->lc_tab_event));
    else ZM_HIP(hipEventCreateWithFlags(&ctx->lc_tab_event, hipEventDisableTiming));
    psf_rec* rh = nullptr;
    ZM_TRY(ctx->get_pinned("psf_tab_h", sizeof(psf_rec) * (size_t)nimg, (void**)&rh));
    for (int i = 0; i < nimg; ++i) {
        char what[96];
        snprintf(what, sizeof(what), "%s: image %d", who, i);
        ZM_TRY(zm_check_wcs(&images[i].wcs, what));
        ZM_CHECK(images[i].img && images[i].model, "%s: null plane or model", what);
        ZM_CHECK(images[i].nx > 0 && images[i].ny > 0, "%s: bad sizes", what);
        ZM_TRY(psf_check_half(what, images[i].half));
        ZM_TRY(psf_check_radius(what, fit_radius, images[i].half));
        psf_rec& Q = rh[i];
        Q.img = images[i].img; Q.rms = images[i].rms; Q.mask = images[i].mask; Q.model = images[i].model;
        Q.nx = images[i].nx; Q.ny = images[i].ny; Q.half = images[i].half; Q.pad_ = 0;
        Q.wcs = images[i].wcs;
        zm_wcs_mark_order(&Q.wcs);
        zm_wcs_frame(&Q.wcs, Q.fr);
    }
    psf_rec* rd = nullptr;
    ZM_TRY(ctx->get("psf_tab", sizeof(psf_rec) * (size_t)nimg, (void**)&rd));
    zm_scope_timer timer(ctx, "psf_batch");
    ZM_HIP(hipMemcpyAsync(rd, rh, sizeof(psf_rec) * (size_t)nimg, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipEventRecord(ctx->lc_tab_event, ctx->stream));
    hipLaunchKernelGGL(k_psf_batch, dim3((unsigned)std::min<int64_t>(npairs, PSF_MAX_GRID)), dim3(64), 0, ctx->stream, rd,
                       nimg, (const long long*)offsets_dev, src_idx_dev, (long long)npairs, nsrc, ra_dev, dec_dev, bad_bits,
                       fit_radius, fit_sky ? 1 : 0, x_dev, y_dev, flux_dev, err_dev, chi2_dev, sky_dev, cover_dev, npix_dev,
                       flags_dev);
    ZM_HIP(hipGetLastError());
    return 0;
}
