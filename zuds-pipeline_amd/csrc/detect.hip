// Pixel-only pieces of the reference's seeing estimate and detection filter
// (SURVEY.md 8(f) row 4), so that `calculate_seeing=True` and the post-subtraction cuts
// run without SExtractor catalogs or the Gaia / Kowalski network queries:
//
//   zm_find_stars    isolated, unsaturated, unmasked local maxima above a threshold
//                    (stands in for "catalog sources matched to Gaia stars",
//                    zuds/seeing.py:10-103)
//   zm_star_fwhm     FWHM of each star from adaptive Gaussian-weighted second moments
//                    (stands in for SExtractor's FWHM_IMAGE, zuds/seeing.py:105-118)
//   zm_negpix_test   the "negative pixel next to a positive one" dipole cut of
//                    filter_sexcat (zuds/filterobjects.py:155-195)
//
//   zm_candidate_cuts_dev   the three pixel cuts of filter_sexcat (BPMCUT, RMSCUT against MEDCUT, the dipole
//                    cut) on planes that are already in HBM, frame statistics included, one wave per candidate
//
// Conventions (chosen, stated in oracle/detect.py): see there.
#include <algorithm>

#include "aperture_dev.h"

// out: candidates in no particular order (the host sorts by peak value, then y, then x)
__global__ __launch_bounds__(256) void k_find_stars(const float* __restrict__ img,
                                                    const uint8_t* __restrict__ bad, int nx, int ny,
                                                    float lo, float hi, int iso, int border,
                                                    int max_out, int* __restrict__ count,
                                                    int* __restrict__ ox, int* __restrict__ oy,
                                                    float* __restrict__ opeak) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x < border || x >= nx - border || y < border || y >= ny - border) return;
    const float v = img[(size_t)y * nx + x];
    if (!(v > lo) || !(v < hi)) return;
    for (int dy = -iso; dy <= iso; ++dy)
        for (int dx = -iso; dx <= iso; ++dx) {
            const size_t q = (size_t)(y + dy) * nx + (x + dx);
            const float n = img[q];
            if (!(n == n) || (bad && bad[q])) return;
            if (dx == 0 && dy == 0) continue;
            // strict maximum; ties go to the pixel that comes first in raster order
            const bool earlier = dy < 0 || (dy == 0 && dx < 0);
            if (earlier ? n >= v : n > v) return;
        }
    const int k = atomicAdd(count, 1);
    if (k < max_out) { ox[k] = x; oy[k] = y; opeak[k] = v; }
}

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one wave per star; window (2 half + 1)^2 around the peak pixel
__global__ __launch_bounds__(64) void k_star_fwhm(const float* __restrict__ img, int nx, int ny, int nstar,
                                                  const int* __restrict__ sx, const int* __restrict__ sy,
                                                  int half, int maxit, double* __restrict__ fwhm,
                                                  double* __restrict__ cxo, double* __restrict__ cyo) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= nstar) return;
    const int px = sx[k], py = sy[k], side = 2 * half + 1;
    double cx = px, cy = py, s2 = 4.0;                   // sigma_w^2 of the weight
    double out = __builtin_nan("");
    for (int it = 0; it < maxit; ++it) {
        double s0 = 0, s1x = 0, s1y = 0;
        for (int e = lane; e < side * side; e += 64) {
            const int j = py - half + e / side, i = px - half + e % side;
            if (i < 0 || i >= nx || j < 0 || j >= ny) continue;
            const double dx = i - cx, dy = j - cy;
            const double w = exp(-0.5 * (dx * dx + dy * dy) / s2) * (double)img[(size_t)j * nx + i];
            s0 += w; s1x += w * i; s1y += w * j;
        }
        s0 = wave_sum(s0); s1x = wave_sum(s1x); s1y = wave_sum(s1y);
        if (!(s0 > 0)) break;
        cx = s1x / s0; cy = s1y / s0;
        double sxx = 0, syy = 0, t0 = 0;
        for (int e = lane; e < side * side; e += 64) {
            const int j = py - half + e / side, i = px - half + e % side;
            if (i < 0 || i >= nx || j < 0 || j >= ny) continue;
            const double dx = i - cx, dy = j - cy;
            const double w = exp(-0.5 * (dx * dx + dy * dy) / s2) * (double)img[(size_t)j * nx + i];
            t0 += w; sxx += w * dx * dx; syy += w * dy * dy;
        }
        t0 = wave_sum(t0); sxx = wave_sum(sxx); syy = wave_sum(syy);
        if (!(t0 > 0)) break;
        const double m2 = 0.5 * (sxx + syy) / t0;        // measured sigma^2 under the weight
        const double inv = 1.0 / m2 - 1.0 / s2;
        if (!(m2 > 0) || !(inv > 0)) break;
        const double ns2 = 1.0 / inv;                    // de-weighted sigma^2
        const bool done = fabs(ns2 - s2) <= 1e-8 * ns2;
        s2 = ns2;
        out = 2.3548200450309493 * sqrt(s2);
        if (done) break;
    }
    if (lane == 0) { fwhm[k] = out; cxo[k] = cx; cyo[k] = cy; }
}

// x, y: SExtractor X_IMAGE / Y_IMAGE (1-based, float).  bad[k] = 1 when a pixel of the
// 11 x 11 cutout below -5 sigma has a neighbour (3 x 3) above +5 sigma.
__global__ void k_negpix(const float* __restrict__ img, int nx, int ny, int npos,
                         const double* __restrict__ xs, const double* __restrict__ ys, float med,
                         float sig, int half, int32_t* __restrict__ bad) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npos) return;
    // a position that is not finite has no cutout; a finite one is clamped while still double, as k_candidate_cuts
    // does: further than 64 pixels outside the frame no cutout pixel is inside it, wherever the centre lies
    if (!isfinite(xs[k]) || !isfinite(ys[k])) { bad[k] = 0; return; }
    const int xc = (int)fmin(fmax(rint(xs[k]), -64.0), nx + 64.0) - 1;  // np.round: half to even
    const int yc = (int)fmin(fmax(rint(ys[k]), -64.0), ny + 64.0) - 1;
    int b = 0;
    for (int j = yc - half; j <= yc + half && !b; ++j)
        for (int i = xc - half; i <= xc + half && !b; ++i) {
            if (i < 0 || i >= nx || j < 0 || j >= ny) continue;
            if (!((img[(size_t)j * nx + i] - med) / sig < -5.f)) continue;
            for (int dj = -1; dj <= 1 && !b; ++dj)
                for (int di = -1; di <= 1; ++di) {
                    const int ii = i + di, jj = j + dj;
                    // the 13 x 13 "big" cutout: neighbours outside it (or the frame) do not count
                    if (ii < xc - half - 1 || ii > xc + half + 1 || jj < yc - half - 1 || jj > yc + half + 1) continue;
                    if (ii < 0 || ii >= nx || jj < 0 || jj >= ny) continue;
                    if ((img[(size_t)jj * nx + ii] - med) / sig > 5.f) { b = 1; break; }
                }
        }
    bad[k] = b;
}

// ---- the three pixel cuts of filter_sexcat on resident planes, one wave per candidate -------------------------
// out = mask & bits: the select counts a pixel whose mask word is 0, the cuts count one without a bad bit
__global__ __launch_bounds__(256) void k_cc_mask(const int32_t* __restrict__ mask, int32_t bits, int64_t n,
                                                 int32_t* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) out[p] = mask[p] & bits;
}

#define CC_RADIUS 6.0        // zuds/filterobjects.py:102-104
#define CC_HALF 5            // CUTSIZE 11, zuds/filterobjects.py:12

// sel: the six doubles of zm_median_mad2_async_dev, {median, sigma, count} of the rms plane over the good pixels and
// of the image.  xs, ys: X_IMAGE / Y_IMAGE as SExtractor reports them (1-based), handed to the aperture unchanged
// as the reference hands them to photutils; the dipole test subtracts the 1 as the reference does.
// Lanes walk the bounding box of the aperture as k_aperture does (element e to lane e mod 64, float64 partials,
// xor-shuffle reduction); the overlap of a pixel is taken once and weighs both planes.
__global__ __launch_bounds__(64) void k_candidate_cuts(const float* __restrict__ img, const float* __restrict__ rms,
                                                       const int32_t* __restrict__ mask, int32_t bad_bits, int nx,
                                                       int ny, int npos, const double* __restrict__ xs,
                                                       const double* __restrict__ ys, const double* __restrict__ sel,
                                                       double* __restrict__ bpmcut, double* __restrict__ rmscut,
                                                       int32_t* __restrict__ negpix, double* __restrict__ stats) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= npos) return;
    const double medcut = 1.1 * sel[0];
    const double immed = sel[3];
    const double imsig = 1.48 * (sel[4] / 1.4826);
    if (k == 0 && lane == 0) {
        stats[0] = medcut; stats[1] = immed; stats[2] = imsig;
        stats[3] = sel[2]; stats[4] = sel[5];               // the two sample counts: the host refuses an empty frame
    }
    const double xc = xs[k], yc = ys[k], r = CC_RADIUS;
    const bool fin = isfinite(xc) && isfinite(yc);
    int ixmin = 0, ixmax = 0, iymin = 0, iymax = 0;
    if (fin) {
        // (k_aperture: clamped while still double)
        ixmin = max((int)fmin(fmax(floor(xc - r + 0.5), -1.0), nx + 1.0), 0);
        ixmax = min((int)fmin(fmax(ceil(xc + r + 0.5), -1.0), nx + 1.0), nx);
        iymin = max((int)fmin(fmax(floor(yc - r + 0.5), -1.0), ny + 1.0), 0);
        iymax = min((int)fmin(fmax(ceil(yc + r + 0.5), -1.0), ny + 1.0), ny);
    }
    const int bw = ixmax - ixmin, bh = iymax - iymin;
    double sr = 0.0, sb = 0.0;
    if (bw > 0 && bh > 0) {
        for (int e = lane; e < bw * bh; e += 64) {
            const int j = iymin + e / bw, i = ixmin + e % bw;
            const double x0 = i - 0.5 - xc, x1 = i + 0.5 - xc, y0 = j - 0.5 - yc, y1 = j + 0.5 - yc;
            const double frac = ap_signed(x1, y1, r) - ap_signed(x0, y1, r) - ap_signed(x1, y0, r) +
                                ap_signed(x0, y0, r);
            const size_t idx = (size_t)j * nx + i;
            sr += (double)rms[idx] * frac;
            if (mask[idx] & bad_bits) sb += frac;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        sr += __shfl_xor(sr, o);
        sb += __shfl_xor(sb, o);
    }
    // the dipole test (k_negpix's rule): lanes take the pixels of the 11 x 11 cutout, each looks at its 3 x 3
    // neighbours inside the 13 x 13 cutout and the frame.  The centre is clamped while still double: further than
    // 64 pixels outside the frame no cutout pixel is inside it, wherever the centre lies.
    bool hit = false;
    if (fin) {
        const int cx = (int)fmin(fmax(rint(xc), -64.0), nx + 64.0) - 1;     // np.round: half to even
        const int cy = (int)fmin(fmax(rint(yc), -64.0), ny + 64.0) - 1;
        const float med = (float)immed, sig = (float)imsig;
        const int side = 2 * CC_HALF + 1;
        for (int e = lane; e < side * side; e += 64) {
            const int j = cy - CC_HALF + e / side, i = cx - CC_HALF + e % side;
            if (i < 0 || i >= nx || j < 0 || j >= ny) continue;
            if (!((img[(size_t)j * nx + i] - med) / sig < -5.f)) continue;
            for (int dj = -1; dj <= 1; ++dj)
                for (int di = -1; di <= 1; ++di) {
                    const int ii = i + di, jj = j + dj;
                    if (ii < cx - CC_HALF - 1 || ii > cx + CC_HALF + 1 || jj < cy - CC_HALF - 1 || jj > cy + CC_HALF + 1) continue;
                    if (ii < 0 || ii >= nx || jj < 0 || jj >= ny) continue;
                    if ((img[(size_t)jj * nx + ii] - med) / sig > 5.f) hit = true;
                }
        }
    }
    const bool any = __ballot(hit) != 0ull;
    if (lane == 0) {
        bpmcut[k] = sb;
        rmscut[k] = sr / (M_PI * CC_RADIUS * CC_RADIUS);
        negpix[k] = any ? 1 : 0;
    }
}

// img / rms / mask: device planes.  Positions in, cuts and the three frame statistics out: host arrays, one copy.
extern "C" int zm_candidate_cuts_dev(zm_ctx* ctx, const float* d_img, const float* d_rms, const int32_t* d_mask,
                                     int32_t bad_bits, int nx, int ny, int npos, const double* x, const double* y,
                                     double* out_bpmcut, double* out_rmscut, int32_t* out_negpix, double* out_stats) {
    ZM_CHECK(ctx && d_img && d_rms && d_mask, "zm_candidate_cuts_dev: null plane");
    ZM_CHECK(nx > 0 && ny > 0 && npos >= 0, "zm_candidate_cuts_dev: bad sizes");
    if (npos == 0) return 0;
    ZM_CHECK(x && y && out_bpmcut && out_rmscut && out_negpix && out_stats, "zm_candidate_cuts_dev: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    const int64_t np = (int64_t)nx * ny;
    int32_t* d_good = nullptr;
    double* d_buf = nullptr;
    ZM_TRY(ctx->get("cc_mask", (size_t)np * 4, (void**)&d_good));
    // {select: 6 (+ 2)} {x, y} {bpmcut, rmscut, stats: 5 (+ 3), negpix}: what comes back is one contiguous run
    const size_t nback = sizeof(double) * (2 * (size_t)npos + 8) + sizeof(int32_t) * (size_t)npos;
    ZM_TRY(ctx->get("cc_buf", sizeof(double) * (8 + 2 * (size_t)npos) + nback, (void**)&d_buf));
    double *d_sel = d_buf, *d_x = d_buf + 8, *d_y = d_x + npos, *d_b = d_y + npos, *d_r = d_b + npos, *d_st = d_r + npos;
    int32_t* d_n = reinterpret_cast<int32_t*>(d_st + 8);
    char* h_back = nullptr;
    ZM_TRY(ctx->get_pinned("cc_back_h", nback, (void**)&h_back));
    hipStream_t s = ctx->stream;
    ZM_HIP(hipMemcpyAsync(d_x, x, sizeof(double) * npos, hipMemcpyHostToDevice, s));
    ZM_HIP(hipMemcpyAsync(d_y, y, sizeof(double) * npos, hipMemcpyHostToDevice, s));
    const int grid = (int)std::min<int64_t>((np + 255) / 256, 2048);
    hipLaunchKernelGGL(k_cc_mask, dim3(grid), dim3(256), 0, s, d_mask, bad_bits, np, d_good);
    ZM_HIP(hipGetLastError());
    // median of the rms plane over the good pixels and median + MAD of the image, left on the device
    ZM_TRY(zm_median_mad2_async_dev(ctx, d_rms, d_good, d_img, nullptr, np, d_sel));
    {
        zm_scope_timer t(ctx, "candidate_cuts");
        hipLaunchKernelGGL(k_candidate_cuts, dim3(npos), dim3(64), 0, s, d_img, d_rms, d_mask, bad_bits, nx, ny, npos,
                           d_x, d_y, d_sel, d_b, d_r, d_n, d_st);
        ZM_HIP(hipGetLastError());
    }
    ZM_HIP(hipMemcpyAsync(h_back, d_b, nback, hipMemcpyDeviceToHost, s));
    ZM_HIP(hipStreamSynchronize(s));
    const double* hd = reinterpret_cast<const double*>(h_back);
    const double* st = hd + 2 * (size_t)npos;
    ZM_CHECK(st[3] > 0 && st[4] > 0, "zm_candidate_cuts: every pixel is masked");
    ZM_CHECK(st[2] > 0, "zm_candidate_cuts: sigma must be positive");
    memcpy(out_bpmcut, hd, sizeof(double) * npos);
    memcpy(out_rmscut, hd + npos, sizeof(double) * npos);
    memcpy(out_negpix, st + 8, sizeof(int32_t) * npos);
    out_stats[0] = st[0]; out_stats[1] = st[1]; out_stats[2] = st[2];
    return 0;
}

// ---- host-pointer entry points (small outputs; the image is uploaded once) --------------
// img / bad: device planes; the candidate lists come back to host arrays (at most max_out entries)
extern "C" int zm_find_stars_dev(zm_ctx* ctx, const float* d_img, const uint8_t* d_bad, int nx, int ny,
                                 float thresh_lo, float thresh_hi, int isolation, int border, int max_out,
                                 int* out_x, int* out_y, float* out_peak, int* out_n) {
    ZM_CHECK(ctx && d_img && out_x && out_y && out_peak && out_n, "zm_find_stars: null argument");
    ZM_CHECK(nx > 0 && ny > 0 && max_out > 0, "zm_find_stars: bad sizes");
    ZM_CHECK(isolation >= 1 && isolation <= 32 && border >= isolation, "zm_find_stars: border >= isolation >= 1");
    ZM_HIP(hipSetDevice(ctx->device));
    char* d_out = nullptr;
    ZM_TRY(ctx->get("det_out", 16 + (size_t)max_out * 12, (void**)&d_out));
    int* d_n = (int*)d_out;
    int* d_x = (int*)(d_out + 16);
    int* d_y = d_x + max_out;
    float* d_p = (float*)(d_y + max_out);
    ZM_HIP(hipMemsetAsync(d_n, 0, 16, ctx->stream));
    hipLaunchKernelGGL(k_find_stars, dim3(zm_div_up(nx, 256), ny), dim3(256), 0, ctx->stream, d_img, d_bad, nx,
                       ny, thresh_lo, thresh_hi, isolation, border, max_out, d_n, d_x, d_y, d_p);
    ZM_HIP(hipGetLastError());
    int n = 0;
    ZM_HIP(hipMemcpyAsync(&n, d_n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    *out_n = n;                                           // may exceed max_out: caller raises the threshold
    const int m = n < max_out ? n : max_out;
    if (m > 0) {
        ZM_HIP(hipMemcpyAsync(out_x, d_x, sizeof(int) * m, hipMemcpyDeviceToHost, ctx->stream));
        ZM_HIP(hipMemcpyAsync(out_y, d_y, sizeof(int) * m, hipMemcpyDeviceToHost, ctx->stream));
        ZM_HIP(hipMemcpyAsync(out_peak, d_p, sizeof(float) * m, hipMemcpyDeviceToHost, ctx->stream));
        ZM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

extern "C" int zm_find_stars(zm_ctx* ctx, const float* img, const uint8_t* bad, int nx, int ny,
                             float thresh_lo, float thresh_hi, int isolation, int border, int max_out,
                             int* out_x, int* out_y, float* out_peak, int* out_n) {
    ZM_CHECK(ctx && img, "zm_find_stars: null argument");
    ZM_CHECK(nx > 0 && ny > 0, "zm_find_stars: bad sizes");
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t np = (size_t)nx * ny;
    float* d_img = nullptr;
    uint8_t* d_bad = nullptr;
    ZM_TRY(ctx->get("h_img", np * 4, (void**)&d_img));
    ZM_HIP(hipMemcpyAsync(d_img, img, np * 4, hipMemcpyHostToDevice, ctx->stream));
    if (bad) {
        ZM_TRY(ctx->get("h_bpm", np, (void**)&d_bad));
        ZM_HIP(hipMemcpyAsync(d_bad, bad, np, hipMemcpyHostToDevice, ctx->stream));
    }
    return zm_find_stars_dev(ctx, d_img, d_bad, nx, ny, thresh_lo, thresh_hi, isolation, border, max_out, out_x, out_y,
                             out_peak, out_n);
}

extern "C" int zm_star_fwhm(zm_ctx* ctx, const float* img, int nx, int ny, int nstar, const int* x,
                            const int* y, int half, double* out_fwhm, double* out_cx, double* out_cy) {
    ZM_CHECK(ctx && img, "zm_star_fwhm: null argument");
    ZM_CHECK(nx > 0 && ny > 0, "zm_star_fwhm: bad sizes");
    if (nstar == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t np = (size_t)nx * ny;
    float* d_img = nullptr;
    ZM_TRY(ctx->get("h_img", np * 4, (void**)&d_img));
    ZM_HIP(hipMemcpyAsync(d_img, img, np * 4, hipMemcpyHostToDevice, ctx->stream));
    return zm_star_fwhm_dev(ctx, d_img, nx, ny, nstar, x, y, half, out_fwhm, out_cx, out_cy);
}

// img: a device plane; star positions in, widths and centroids out: host arrays
extern "C" int zm_star_fwhm_dev(zm_ctx* ctx, const float* d_img, int nx, int ny, int nstar, const int* x,
                                const int* y, int half, double* out_fwhm, double* out_cx, double* out_cy) {
    ZM_CHECK(ctx && d_img && x && y && out_fwhm && out_cx && out_cy, "zm_star_fwhm: null argument");
    ZM_CHECK(nx > 0 && ny > 0 && nstar >= 0 && half >= 2 && half <= 64, "zm_star_fwhm: bad sizes");
    if (nstar == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    char* d_s = nullptr;
    ZM_TRY(ctx->get("det_star", (size_t)nstar * 32, (void**)&d_s));
    double* d_f = (double*)d_s;
    double* d_cx = d_f + nstar;
    double* d_cy = d_cx + nstar;
    int* d_x = (int*)(d_cy + nstar);
    int* d_y = d_x + nstar;
    ZM_HIP(hipMemcpyAsync(d_x, x, sizeof(int) * nstar, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_y, y, sizeof(int) * nstar, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_star_fwhm, dim3(nstar), dim3(64), 0, ctx->stream, d_img, nx, ny, nstar, d_x, d_y, half,
                       25, d_f, d_cx, d_cy);
    ZM_HIP(hipGetLastError());
    ZM_HIP(hipMemcpyAsync(out_fwhm, d_f, sizeof(double) * nstar, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_cx, d_cx, sizeof(double) * nstar, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_cy, d_cy, sizeof(double) * nstar, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int zm_negpix_test(zm_ctx* ctx, const float* img, int nx, int ny, int npos, const double* x,
                              const double* y, double median, double sigma, int32_t* out_bad) {
    ZM_CHECK(ctx && img && x && y && out_bad, "zm_negpix_test: null argument");
    ZM_CHECK(nx > 0 && ny > 0 && npos >= 0, "zm_negpix_test: bad sizes");
    ZM_CHECK(sigma > 0, "zm_negpix_test: sigma must be positive");
    if (npos == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t np = (size_t)nx * ny;
    float* d_img = nullptr;
    char* d_s = nullptr;
    ZM_TRY(ctx->get("h_img", np * 4, (void**)&d_img));
    ZM_HIP(hipMemcpyAsync(d_img, img, np * 4, hipMemcpyHostToDevice, ctx->stream));
    ZM_TRY(ctx->get("det_neg", (size_t)npos * 20, (void**)&d_s));
    double* d_x = (double*)d_s;
    double* d_y = d_x + npos;
    int32_t* d_b = (int32_t*)(d_y + npos);
    ZM_HIP(hipMemcpyAsync(d_x, x, sizeof(double) * npos, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_y, y, sizeof(double) * npos, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_negpix, dim3(zm_div_up(npos, 64)), dim3(64), 0, ctx->stream, d_img, nx, ny, npos, d_x,
                       d_y, (float)median, (float)sigma, 5, d_b);
    ZM_HIP(hipGetLastError());
    ZM_HIP(hipMemcpyAsync(out_bad, d_b, sizeof(int32_t) * npos, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
