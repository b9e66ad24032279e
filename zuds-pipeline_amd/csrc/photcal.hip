// Photometric calibration on resident planes (DESIGN.md "Photometric calibration"): what APCORk, MAGZP and MAGLIM are
// made of.  This operator is the project's own; the reference inherits the three cards from IPAC's headers.
//
//   k_growth          one wave per star: the sky annulus into LDS, an exact clipped median / MAD of it, then one pass over
//                     the bounding box of the largest aperture that sums every radius at once (ap_signed overlaps, fp64)
//   k_clipped_median  one workgroup per column of doubles: the column in LDS (up to 128 KB), the same clipped statistics
//   k_maglim_points   one wave per lattice point: sqrt(sum(rms^2 frac)) over an aperture, NaN where the box is unusable;
//                     its median is k_clipped_median with maxiter 0
//
// The select is exact and the same in both kernels: a bitonic sort of the values in LDS, after which the survivors of
// every clipping round are a contiguous range [lo, hi) of the sorted array (|v - median| > t cuts from the two ends).
// The median is the middle of the range; the MAD needs no second array: |v - median| falls along the left half and
// rises along the right half, so every thread finds the rank of its own deviation in the union of the two runs with one
// binary search in the other run, and the thread(s) that hold the middle rank(s) publish it.  No float atomics, no
// global scratch.
#include "aperture_dev.h"

// comparisons against thresholds and radii are meant as the plain IEEE operations a float64 restatement performs
#pragma clang fp contract(off)

#define PC_SKY_CAP 2048          // floats per star: pixel centres within 20 px of a point number 1347 at the most
#define PC_GROWTH_NT 64          // one wave per workgroup (stars per workgroup: 1)
#define PC_CM_NT 1024

struct pc_radii {
    double r[ZM_GROWTH_NAPER_MAX];
};

template <class T>
__device__ __forceinline__ void pc_sort(T* a, int npad) {
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (npad >> 1); t += blockDim.x) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;        // bit j of i is clear
                const bool up = (i & k) == 0;
                const T x = a[i], y = a[l];
                if ((x > y) == up) {
                    a[i] = y;
                    a[l] = x;
                }
            }
            __syncthreads();
        }
    }
}

template <class T>
__device__ __forceinline__ double pc_dev(const T* a, int i, double med) {
    return fabs((double)a[i] - med);
}

// Clipped median / 1.4826 MAD of the ascending a[0 .. nvalid): every thread of the workgroup calls it and gets the same
// results.  hit: two doubles in LDS.
template <class T>
__device__ __forceinline__ void pc_clip(const T* a, int nvalid, double kappa, int maxiter, double* hit, double* out_med,
                                        double* out_sig, int* out_n) {
    int lo = 0, hi = nvalid;
    double med = NAN, sig = NAN;
    for (int it = 0;; ++it) {
        const int m = hi - lo;
        if (m <= 0) {
            med = sig = NAN;
            break;
        }
        const int p = lo + (m >> 1);
        med = (m & 1) ? (double)a[p] : 0.5 * ((double)a[p - 1] + (double)a[p]);
        const int k0 = (m - 1) >> 1, k1 = m >> 1;
        for (int i = lo + (int)threadIdx.x; i < hi; i += blockDim.x) {
            const double d = pc_dev(a, i, med);
            int rank;
            if (i < p) {                       // left run (falls with i): right entries strictly below d come first
                int l = p, h = hi;
                while (l < h) {
                    const int c = (l + h) >> 1;
                    if (pc_dev(a, c, med) < d) l = c + 1; else h = c;
                }
                rank = (p - 1 - i) + (l - p);
            } else {                           // right run (rises with i): left entries at or below d come first
                int l = lo, h = p;
                while (l < h) {
                    const int c = (l + h) >> 1;
                    if (pc_dev(a, c, med) > d) l = c + 1; else h = c;
                }
                rank = (i - p) + (p - l);
            }
            if (rank == k0) hit[0] = d;
            if (rank == k1) hit[1] = d;
        }
        __syncthreads();
        sig = 1.4826 * (0.5 * (hit[0] + hit[1]));
        __syncthreads();                       // hit is written again in the next round
        if (it >= maxiter) break;
        const double thr = kappa * sig;
        int l = lo, h = p;                     // the dropped ones are the outer ends of the two runs
        while (l < h) {
            const int c = (l + h) >> 1;
            if (pc_dev(a, c, med) > thr) l = c + 1; else h = c;
        }
        const int nlo = l;
        l = p, h = hi;
        while (l < h) {
            const int c = (l + h) >> 1;
            if (pc_dev(a, c, med) <= thr) l = c + 1; else h = c;
        }
        if (nlo == lo && l == hi) break;
        lo = nlo;
        hi = l;
    }
    *out_med = med;
    *out_sig = sig;
    *out_n = hi > lo ? hi - lo : 0;
}

__device__ __forceinline__ int pc_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

__global__ __launch_bounds__(PC_GROWTH_NT) void k_growth(
    const float* __restrict__ img, const float* __restrict__ rms, const int32_t* __restrict__ mask, int32_t bad_bits,
    float saturate, int nx, int ny, int nstar, const double* __restrict__ xs, const double* __restrict__ ys, int naper,
    pc_radii R, double r_in, double r_out, double kappa, int maxiter, int nsky_min, double* __restrict__ flux,
    double* __restrict__ err, double* __restrict__ sky_out, double* __restrict__ sig_out, int32_t* __restrict__ nsky_out,
    int32_t* __restrict__ flags_out) {
    __shared__ float sv[PC_SKY_CAP];
    __shared__ double hit[2];
    __shared__ int cnt[2];
    __shared__ double sr[ZM_GROWTH_NAPER_MAX];       // the radii: read from LDS in the loops, not held in 16 SGPRs
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= nstar) return;
    const double xc = xs[s], yc = ys[s];
    if (!(isfinite(xc) && isfinite(yc))) {
        if (lane == 0) {
            for (int k = 0; k < naper; ++k) flux[(size_t)s * naper + k] = err[(size_t)s * naper + k] = NAN;
            sky_out[s] = sig_out[s] = NAN;
            nsky_out[s] = 0;
            flags_out[s] = ZM_GROWTH_BADPOS;
        }
        return;
    }
    if (lane == 0) {
        cnt[0] = cnt[1] = 0;
#pragma unroll
        for (int k = 0; k < ZM_GROWTH_NAPER_MAX; ++k) sr[k] = R.r[k];
    }
    __syncthreads();
    // ---- the annulus: pixel centres at r_in <= d < r_out (compared as squares), those off the frame only noted
    {
        const double ax0 = ceil(xc - r_out), ay0 = ceil(yc - r_out);
        const int aw = min(max((int)(floor(xc + r_out) - ax0) + 1, 0), 42);
        const int ah = min(max((int)(floor(yc + r_out) - ay0) + 1, 0), 42);
        const double rin2 = r_in * r_in, rout2 = r_out * r_out;
        for (int e = lane; e < aw * ah; e += PC_GROWTH_NT) {
            const double px = ax0 + (e % aw), py = ay0 + (e / aw);
            const double dx = px - xc, dy = py - yc, d2 = dx * dx + dy * dy;
            if (!(d2 >= rin2 && d2 < rout2)) continue;
            if (px < 0.0 || py < 0.0 || px >= (double)nx || py >= (double)ny) {
                atomicOr(&cnt[1], 1);
                continue;
            }
            const size_t idx = (size_t)(int)py * nx + (int)px;
            const float v = img[idx];
            if (isfinite(v) && !(mask && (mask[idx] & bad_bits))) {
                const int slot = atomicAdd(&cnt[0], 1);
                if (slot < PC_SKY_CAP) sv[slot] = v;
            }
        }
    }
    __syncthreads();
    const int nval = min(cnt[0], PC_SKY_CAP);
    const int annclip = cnt[1];
    const int npad = pc_pow2(nval);
    for (int i = nval + lane; i < npad; i += PC_GROWTH_NT) sv[i] = INFINITY;
    __syncthreads();
    pc_sort(sv, npad);
    double sky, sig;
    int nsky;
    pc_clip(sv, nval, kappa, maxiter, hit, &sky, &sig, &nsky);

    // ---- every aperture in one pass over the box of the largest
    const double rmax = sr[naper - 1];
    const double bx0 = floor(xc - rmax + 0.5), bx1 = ceil(xc + rmax + 0.5);
    const double by0 = floor(yc - rmax + 0.5), by1 = ceil(yc + rmax + 0.5);
    const int boxclip = bx0 < 0.0 || by0 < 0.0 || bx1 > (double)nx || by1 > (double)ny;
    const int ixmin = max((int)fmin(fmax(bx0, -1.0), nx + 1.0), 0), ixmax = min((int)fmin(fmax(bx1, -1.0), nx + 1.0), nx);
    const int iymin = max((int)fmin(fmax(by0, -1.0), ny + 1.0), 0), iymax = min((int)fmin(fmax(by1, -1.0), ny + 1.0), ny);
    const int bw = ixmax - ixmin, bh = iymax - iymin;
    double f[ZM_GROWTH_NAPER_MAX], v[ZM_GROWTH_NAPER_MAX];
#pragma unroll
    for (int k = 0; k < ZM_GROWTH_NAPER_MAX; ++k) f[k] = v[k] = 0.0;
    int fl = 0, nanmask = 0;
    if (bw > 0 && bh > 0) {
        const double rmax2 = rmax * rmax;
        for (int e = lane; e < bw * bh; e += PC_GROWTH_NT) {
            const int j = iymin + e / bw, i = ixmin + e % bw;
            const double x0 = i - 0.5 - xc, x1 = i + 0.5 - xc, y0 = j - 0.5 - yc, y1 = j + 0.5 - yc;
            const double fx = fmax(fabs(x0), fabs(x1)), fy = fmax(fabs(y0), fabs(y1));
            const double qx = fmin(fmax(0.0, x0), x1), qy = fmin(fmax(0.0, y0), y1);      // nearest point of the pixel
            const double far2 = fx * fx + fy * fy, near2 = qx * qx + qy * qy;
            if (near2 >= rmax2) continue;
            const size_t idx = (size_t)j * nx + i;
            const float val = img[idx];
            const bool fin = isfinite(val);
            if (mask && (mask[idx] & bad_bits)) fl |= ZM_GROWTH_BAD;
            if (saturate > 0.f && val >= saturate) fl |= ZM_GROWTH_SATURATED;
            if (!fin) fl |= ZM_GROWTH_NONFINITE;
            const double dv = (double)val - sky;
            double rv = 1.0;
            if (rms) {
                const double sg = rms[idx];
                rv = isfinite(sg) ? sg * sg : NAN;        // an rms value that is not finite: the errors it touches are NaN
            }
#pragma unroll
            for (int k = 0; k < ZM_GROWTH_NAPER_MAX; ++k) {
                if (k >= naper) continue;
                const double r = sr[k], r2 = r * r;
                if (near2 >= r2) continue;
                double frac = 1.0;
                if (far2 > r2)
                    frac = ap_signed(x1, y1, r) - ap_signed(x0, y1, r) - ap_signed(x1, y0, r) + ap_signed(x0, y0, r);
                if (fin) f[k] += dv * frac; else nanmask |= 1 << k;
                v[k] += rv * frac;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < ZM_GROWTH_NAPER_MAX; ++k) {
            f[k] += __shfl_xor(f[k], o);
            v[k] += __shfl_xor(v[k], o);
        }
        fl |= __shfl_xor(fl, o);
        nanmask |= __shfl_xor(nanmask, o);
    }
    if (lane == 0) {
        const bool nosky = nsky == 0;
#pragma unroll
        for (int k = 0; k < ZM_GROWTH_NAPER_MAX; ++k) {
            if (k >= naper) continue;
            const double var = isfinite(v[k]) ? fmax(v[k], 0.0) : v[k];
            flux[(size_t)s * naper + k] = (nosky || ((nanmask >> k) & 1)) ? NAN : f[k];
            err[(size_t)s * naper + k] = nosky ? NAN : (rms ? sqrt(var) : sqrt(var) * sig);
        }
        sky_out[s] = sky;
        sig_out[s] = sig;
        nsky_out[s] = nsky;
        flags_out[s] = fl | (boxclip ? ZM_GROWTH_BOXCLIP : 0) | (annclip ? ZM_GROWTH_ANNCLIP : 0) |
                       (nsky < nsky_min ? ZM_GROWTH_FEWSKY : 0);
    }
}

__global__ __launch_bounds__(PC_CM_NT) void k_clipped_median(const double* __restrict__ values, int n, int64_t stride,
                                                             int npad, double kappa, int maxiter,
                                                             double* __restrict__ out) {
    extern __shared__ double cm[];
    __shared__ double hit[2];
    __shared__ int cnt;
    const int c = blockIdx.x;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < npad; i += blockDim.x) {
        double x = INFINITY;
        if (i < n) {
            x = values[(size_t)i * stride + c];
            if (isfinite(x)) ++mine; else x = INFINITY;
        }
        cm[i] = x;
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    const int nvalid = cnt;
    pc_sort(cm, npad);
    double med, sig;
    int nused;
    pc_clip(cm, nvalid, kappa, maxiter, hit, &med, &sig, &nused);
    if (threadIdx.x == 0) {
        out[4 * (size_t)c + 0] = med;
        out[4 * (size_t)c + 1] = sig;
        out[4 * (size_t)c + 2] = (double)nused;
        out[4 * (size_t)c + 3] = (double)nvalid;
    }
}

__global__ __launch_bounds__(64) void k_maglim_points(const float* __restrict__ rms, const int32_t* __restrict__ mask,
                                                     int32_t bad_bits, int nx, int ny, double r, double x_first,
                                                     double y_first, int step, int npx, int npts,
                                                     double* __restrict__ col) {
    const int pt = blockIdx.x, lane = threadIdx.x;
    if (pt >= npts) return;
    const double xc = x_first + (double)(pt % npx) * step, yc = y_first + (double)(pt / npx) * step;
    const int ixmin = max((int)fmin(fmax(floor(xc - r + 0.5), -1.0), nx + 1.0), 0);
    const int ixmax = min((int)fmin(fmax(ceil(xc + r + 0.5), -1.0), nx + 1.0), nx);
    const int iymin = max((int)fmin(fmax(floor(yc - r + 0.5), -1.0), ny + 1.0), 0);
    const int iymax = min((int)fmin(fmax(ceil(yc + r + 0.5), -1.0), ny + 1.0), ny);
    const int bw = ixmax - ixmin, bh = iymax - iymin;
    double v = 0.0;
    int bad = 0;
    if (bw > 0 && bh > 0) {
        for (int e = lane; e < bw * bh; e += 64) {
            const int j = iymin + e / bw, i = ixmin + e % bw;
            const double x0 = i - 0.5 - xc, x1 = i + 0.5 - xc, y0 = j - 0.5 - yc, y1 = j + 0.5 - yc;
            const double frac = ap_signed(x1, y1, r) - ap_signed(x0, y1, r) - ap_signed(x1, y0, r) + ap_signed(x0, y0, r);
            const size_t idx = (size_t)j * nx + i;
            const float sg = rms[idx];
            if (!(isfinite(sg) && sg > 0.f)) bad = 1;
            if (mask && (mask[idx] & bad_bits)) bad = 1;
            v += (double)sg * (double)sg * frac;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        v += __shfl_xor(v, o);
        bad |= __shfl_xor(bad, o);
    }
    if (lane == 0) col[pt] = bad ? NAN : sqrt(fmax(v, 0.0));
}

__global__ void k_maglim_pack(const double* __restrict__ o4, int npts, double* __restrict__ out3) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        out3[0] = o4[0];
        out3[1] = o4[3];
        out3[2] = (double)npts;
    }
}

static int pc_growth_check(const char* who, zm_ctx* ctx, const float* img, int nx, int ny, int nstar, const double* x,
                           const double* y, int naper, const double* radii, double r_in, double r_out, double kappa,
                           int maxiter, const void* o1, const void* o2, const void* o3, const void* o4, const void* o5,
                           const void* o6) {
    ZM_CHECK(ctx && img && radii && o1 && o2 && o3 && o4 && o5 && o6, "%s: null argument", who);
    ZM_CHECK(nx > 0 && ny > 0 && nstar >= 0, "%s: bad sizes", who);
    ZM_CHECK(nstar == 0 || (x && y), "%s: null positions", who);
    ZM_CHECK(naper >= 1 && naper <= ZM_GROWTH_NAPER_MAX, "%s: naper %d outside 1 .. %d", who, naper, ZM_GROWTH_NAPER_MAX);
    for (int k = 0; k < naper; ++k) {
        ZM_CHECK(radii[k] > 0 && radii[k] <= 64.0, "%s: radius %g outside (0, 64]", who, radii[k]);
        ZM_CHECK(k == 0 || radii[k] > radii[k - 1], "%s: the radii must ascend", who);
    }
    ZM_CHECK(r_in >= 0 && r_in < r_out, "%s: annulus %g .. %g: need 0 <= r_in < r_out", who, r_in, r_out);
    ZM_CHECK(r_out <= ZM_GROWTH_ROUT_MAX, "%s: r_out %g beyond the largest supported annulus radius, %g px", who, r_out,
             (double)ZM_GROWTH_ROUT_MAX);
    ZM_CHECK(kappa > 0 && kappa < 1e30 && maxiter >= 0, "%s: bad kappa %g or maxiter %d", who, kappa, maxiter);
    return 0;
}

extern "C" int zm_growth_dev(zm_ctx* ctx, const float* img, const float* rms, const int32_t* mask, int32_t bad_bits,
                             float saturate, int nx, int ny, int nstar, const double* x, const double* y, int naper,
                             const double* radii, double r_in, double r_out, double kappa, int maxiter, int nsky_min,
                             double* out_flux, double* out_err, double* out_sky, double* out_sky_sigma,
                             int32_t* out_nsky, int32_t* out_flags) {
    ZM_TRY(pc_growth_check("zm_growth_dev", ctx, img, nx, ny, nstar, x, y, naper, radii, r_in, r_out, kappa, maxiter,
                           out_flux, out_err, out_sky, out_sky_sigma, out_nsky, out_flags));
    if (nstar == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    pc_radii R;
    for (int k = 0; k < ZM_GROWTH_NAPER_MAX; ++k) R.r[k] = radii[k < naper ? k : naper - 1];
    zm_scope_timer t(ctx, "growth");
    hipLaunchKernelGGL(k_growth, dim3(nstar), dim3(PC_GROWTH_NT), 0, ctx->stream, img, rms, mask, bad_bits, saturate, nx,
                       ny, nstar, x, y, naper, R, r_in, r_out, kappa, maxiter, nsky_min, out_flux, out_err, out_sky,
                       out_sky_sigma, out_nsky, out_flags);
    ZM_HIP(hipGetLastError());
    return 0;
}

extern "C" int zm_growth(zm_ctx* ctx, const float* img, const float* rms, const int32_t* mask, int32_t bad_bits,
                         float saturate, int nx, int ny, int nstar, const double* x, const double* y, int naper,
                         const double* radii, double r_in, double r_out, double kappa, int maxiter, int nsky_min,
                         double* out_flux, double* out_err, double* out_sky, double* out_sky_sigma, int32_t* out_nsky,
                         int32_t* out_flags) {
    ZM_TRY(pc_growth_check("zm_growth", ctx, img, nx, ny, nstar, x, y, naper, radii, r_in, r_out, kappa, maxiter,
                           out_flux, out_err, out_sky, out_sky_sigma, out_nsky, out_flags));
    if (nstar == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t np = (size_t)nx * ny, ns = (size_t)nstar;
    float *d_img = nullptr, *d_rms = nullptr;
    int32_t* d_mask = nullptr;
    double* d = nullptr;
    ZM_TRY(ctx->get("h_img", np * 4, (void**)&d_img));
    ZM_HIP(hipMemcpyAsync(d_img, img, np * 4, hipMemcpyHostToDevice, ctx->stream));
    if (rms) {
        ZM_TRY(ctx->get("h_wgt", np * 4, (void**)&d_rms));
        ZM_HIP(hipMemcpyAsync(d_rms, rms, np * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (mask) {
        ZM_TRY(ctx->get("h_mask", np * 4, (void**)&d_mask));
        ZM_HIP(hipMemcpyAsync(d_mask, mask, np * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    // x, y, sky, sigma, flux[naper], err[naper] as doubles, then nsky and flags
    ZM_TRY(ctx->get("pc_growth", sizeof(double) * ns * (4 + 2 * (size_t)naper) + sizeof(int32_t) * 2 * ns, (void**)&d));
    double *d_x = d, *d_y = d + ns, *d_sky = d + 2 * ns, *d_sig = d + 3 * ns, *d_f = d + 4 * ns, *d_e = d_f + ns * naper;
    int32_t *d_n = reinterpret_cast<int32_t*>(d_e + ns * naper), *d_fl = d_n + ns;
    ZM_HIP(hipMemcpyAsync(d_x, x, sizeof(double) * ns, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_y, y, sizeof(double) * ns, hipMemcpyHostToDevice, ctx->stream));
    ZM_TRY(zm_growth_dev(ctx, d_img, d_rms, d_mask, bad_bits, saturate, nx, ny, nstar, d_x, d_y, naper, radii, r_in,
                         r_out, kappa, maxiter, nsky_min, d_f, d_e, d_sky, d_sig, d_n, d_fl));
    ZM_HIP(hipMemcpyAsync(out_flux, d_f, sizeof(double) * ns * naper, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_err, d_e, sizeof(double) * ns * naper, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_sky, d_sky, sizeof(double) * ns, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_sky_sigma, d_sig, sizeof(double) * ns, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_nsky, d_n, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_flags, d_fl, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

static int pc_cm_launch(zm_ctx* ctx, const double* values, int n, int ncol, int64_t stride, double kappa, int maxiter,
                        double* out) {
    int npad = 1;
    while (npad < n) npad <<= 1;
    const size_t shmem = sizeof(double) * (size_t)npad;
    static bool attr_set[64] = {};
    // (the static 24 bytes beside the column count towards the 64 KB a kernel gets without asking)
    if (shmem + 64 > 65536 && !attr_set[ctx->device & 63]) {
        ZM_HIP(hipFuncSetAttribute((const void*)k_clipped_median, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(sizeof(double) * ZM_CLIPMED_NMAX)));
        attr_set[ctx->device & 63] = true;
    }
    int nt = npad / 2;
    nt = nt < 64 ? 64 : (nt > PC_CM_NT ? PC_CM_NT : nt);
    hipLaunchKernelGGL(k_clipped_median, dim3(ncol), dim3(nt), shmem, ctx->stream, values, n, stride, npad, kappa,
                       maxiter, out);
    ZM_HIP(hipGetLastError());
    return 0;
}

static int pc_cm_check(const char* who, zm_ctx* ctx, const double* values, int n, int ncol, int64_t stride, double kappa,
                       int maxiter, const double* out) {
    ZM_CHECK(ctx && out, "%s: null argument", who);
    ZM_CHECK(n >= 0 && ncol >= 0 && stride >= ncol, "%s: bad sizes (n %d, ncol %d, stride %lld)", who, n, ncol,
             (long long)stride);
    ZM_CHECK(n <= ZM_CLIPMED_NMAX, "%s: %d rows, a launch holds at most %d in LDS", who, n, ZM_CLIPMED_NMAX);
    ZM_CHECK(values || n == 0 || ncol == 0, "%s: null values", who);
    ZM_CHECK(kappa > 0 && kappa < 1e30 && maxiter >= 0, "%s: bad kappa %g or maxiter %d", who, kappa, maxiter);
    return 0;
}

extern "C" int zm_clipped_median_dev(zm_ctx* ctx, const double* values, int n, int ncol, int64_t stride, double kappa,
                                     int maxiter, double* out) {
    ZM_TRY(pc_cm_check("zm_clipped_median_dev", ctx, values, n, ncol, stride, kappa, maxiter, out));
    if (ncol == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    zm_scope_timer t(ctx, "clipped_median");
    return pc_cm_launch(ctx, values, n, ncol, stride, kappa, maxiter, out);
}

extern "C" int zm_clipped_median(zm_ctx* ctx, const double* values, int n, int ncol, int64_t stride, double kappa,
                                 int maxiter, double* out) {
    ZM_TRY(pc_cm_check("zm_clipped_median", ctx, values, n, ncol, stride, kappa, maxiter, out));
    if (ncol == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t nel = n ? (size_t)(n - 1) * stride + ncol : 0;
    double* d = nullptr;
    ZM_TRY(ctx->get("pc_cm", sizeof(double) * (nel + 4 * (size_t)ncol), (void**)&d));
    double* d_out = d + nel;
    if (nel) ZM_HIP(hipMemcpyAsync(d, values, sizeof(double) * nel, hipMemcpyHostToDevice, ctx->stream));
    ZM_TRY(pc_cm_launch(ctx, d, n, ncol, stride, kappa, maxiter, d_out));
    ZM_HIP(hipMemcpyAsync(out, d_out, sizeof(double) * 4 * ncol, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// centres c = step / 2 + i step with c + 0.5 >= margin and n - 0.5 - c >= margin: the first, and how many
static void pc_lattice(int n, int step, double margin, double* first, int* count) {
    const double h = 0.5 * step;
    long i0 = (long)ceil((margin - 0.5 - h) / step);
    if (i0 < 0) i0 = 0;
    long i1 = (long)floor((n - 0.5 - margin - h) / step);
    *first = h + (double)i0 * step;
    *count = i1 >= i0 ? (int)(i1 - i0 + 1) : 0;
}

extern "C" int zm_maglim_dev(zm_ctx* ctx, const float* rms, const int32_t* mask, int32_t bad_bits, int nx, int ny,
                             double radius, int step, double* out3_dev) {
    ZM_CHECK(ctx && rms && out3_dev, "zm_maglim_dev: null argument");
    ZM_CHECK(nx > 0 && ny > 0 && step > 0, "zm_maglim_dev: bad sizes");
    ZM_CHECK(radius > 0 && radius <= 64.0, "zm_maglim_dev: radius %g outside (0, 64]", radius);
    double xf, yf;
    int npx, npy;
    pc_lattice(nx, step, radius + 1.0, &xf, &npx);
    pc_lattice(ny, step, radius + 1.0, &yf, &npy);
    const long long npts = (long long)npx * npy;
    ZM_CHECK(npts <= ZM_CLIPMED_NMAX, "zm_maglim_dev: %lld lattice points with step %d, at most %d: take a coarser step",
             npts, step, ZM_CLIPMED_NMAX);
    ZM_HIP(hipSetDevice(ctx->device));
    double* d = nullptr;
    ZM_TRY(ctx->get("pc_maglim", sizeof(double) * ((size_t)npts + 4), (void**)&d));
    double *d_o4 = d, *d_col = d + 4;
    zm_scope_timer t(ctx, "maglim");
    if (npts > 0) {
        hipLaunchKernelGGL(k_maglim_points, dim3((int)npts), dim3(64), 0, ctx->stream, rms, mask, bad_bits, nx, ny,
                           radius, xf, yf, step, npx, (int)npts, d_col);
        ZM_HIP(hipGetLastError());
    }
    ZM_TRY(pc_cm_launch(ctx, d_col, (int)npts, 1, 1, 3.0, 0, d_o4));
    hipLaunchKernelGGL(k_maglim_pack, dim3(1), dim3(64), 0, ctx->stream, d_o4, (int)npts, out3_dev);
    ZM_HIP(hipGetLastError());
    return 0;
}
