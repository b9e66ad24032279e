// Light curves on gfx950: which sources lie inside which image footprint, and forced photometry of every such pair in
// one launch.
//
// Replaces the per-subtraction loop of the reference's scripts/dophot.py: q3c_poly_query(Source.ra, Source.dec,
// wcs.calc_footprint()) and raw_aperture_photometry at the positions it returns.  The operator is stated in DESIGN.md
// ("Light curves").
//
// Footprint.  The spherical quadrilateral whose vertices are the unit vectors of the centres of the four corner pixels
// (order and center = True convention of WCS.calc_footprint), joined by great circles - the polygon q3c tests, its face
// projection being gnomonic.  The host makes the vertices (zm_wcs_pix2vec) and the four inward unit normals of the edge
// planes in fp64; the side that is "inward" comes from the polygon's own orientation, so det(CD) of either sign works.
// A source is inside when its unit vector is on the inner side of all four planes (>= 0: the boundary belongs to the
// footprint) and in the hemisphere of the vertex sum.  A cap around the normalised vertex sum whose cosine is that of
// the farthest vertex, less a few ulp, rejects most pairs with one dot product.
//
//   k_lc_unit     (ra, dec) -> unit vector, once per source; a value that is not finite gives NaN, which joins nothing
//   k_lc_join<0>  one thread per (image, source): the test, and per wave the number of hits (ballot) -> cnt[image][wave]
//   k_lc_scan_*   exclusive scan of cnt in (image, wave) order, int32 in, int64 out (three launches)
//   k_lc_offsets  offsets[image] = the scan at the image's first wave, offsets[nimg] = the total
//   k_lc_join<1>  the test again; a hit goes to base[image][wave] + its rank among the wave's hits, if that is below the
//                 capacity.  Within an image src_idx is ascending, and the bytes are the same on every run: no atomics.
//   k_lc_batch    one wave per pair: image of the pair (binary search of offsets), sky -> pixel with the image's WCS
//                 (zm_plane2pix, TPV inverse included), then ap_wave_sum - the body of k_aperture
//
// Brute force: nimg x nsrc tests of <= 15 fp64 multiply-adds on 24 bytes each (DESIGN.md has the arithmetic).
#include <algorithm>
#include <cmath>

#include "aperture_dev.h"
#include "wcs_math.h"

#define LC_SCAN_PER_BLOCK 1024        // elements of one block of the scan (256 threads x 4)
#define LC_MAX_GRID (1 << 24)         // workgroups of k_lc_batch: 2^30 work-items, below the 2^32 a launch takes
#define LC_D2R 0.017453292519943295   // (wcs_host.hip's D2R: sky -> pixel here follows zm_wcs_sky2pix step by step)

struct lc_foot {                      // one image of the join, 16 doubles, uniform across a workgroup
    double n[4][3];                   // inward unit normals of the edge planes
    double c[3];                      // normalised vertex sum
    double cosr;                      // cosine of the cap's radius, widened
};

struct lc_rec {                       // one image of the batch, uniform across a wave
    const float* img;
    const float* rms;                 // or NULL
    const int32_t* mask;              // or NULL
    int32_t nx, ny;
    double fr[9];                     // zm_wcs_frame of wcs
    zm_wcs wcs;                       // private copy, TPV order marked
};

__device__ __forceinline__ bool lc_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

__global__ __launch_bounds__(256) void k_lc_unit(const double* __restrict__ ra, const double* __restrict__ dec, int n,
                                                 double* __restrict__ vx, double* __restrict__ vy, double* __restrict__ vz) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double a = ra[i], d = dec[i];
    double x = __builtin_nan(""), y = x, z = x;
    if (lc_finite(a) && lc_finite(d)) {
        const double ar = a * LC_D2R, dr = d * LC_D2R, cd = cos(dr);
        x = cd * cos(ar);
        y = cd * sin(ar);
        z = sin(dr);
    }
    vx[i] = x; vy[i] = y; vz[i] = z;
}

// grid (ceil(nsrc / 256), nimg); nwave = 4 gridDim.x waves per image.  A NaN vector fails every comparison.
template <bool FILL>
__global__ __launch_bounds__(256) void k_lc_join(const lc_foot* __restrict__ foot, const double* __restrict__ vx,
                                                 const double* __restrict__ vy, const double* __restrict__ vz, int nsrc,
                                                 int32_t* __restrict__ cnt, const long long* __restrict__ base,
                                                 long long capacity, int32_t* __restrict__ src_idx) {
    const lc_foot* __restrict__ F = foot + blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool in = false;
    if (i < nsrc) {
        const double x = vx[i], y = vy[i], z = vz[i];
        const double dc = F->c[0] * x + F->c[1] * y + F->c[2] * z;
        if (dc >= F->cosr && dc > 0.0) {
            in = true;
#pragma unroll
            for (int k = 0; k < 4; ++k) in = in && (F->n[k][0] * x + F->n[k][1] * y + F->n[k][2] * z >= 0.0);
        }
    }
    const unsigned long long hits = __ballot(in);
    const size_t w = (size_t)blockIdx.y * (gridDim.x * 4) + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (!FILL) {
        if (lane == 0) cnt[w] = __popcll(hits);
    } else if (in) {
        const long long pos = base[w] + __popcll(hits & ((1ull << lane) - 1ull));
        if (pos < capacity) src_idx[pos] = i;
    }
}

// ---- exclusive scan, int32 in, int64 out (per block, the block totals, add) ------------------------------------------
__device__ __forceinline__ long long lc_block_scan(long long v, long long* sh, long long* total) {    // exclusive, 256 threads
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int of = 1; of < 256; of <<= 1) {
        const long long a = t >= of ? sh[t - of] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const long long incl = sh[t];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void k_lc_scan_local(const int32_t* __restrict__ in, long long n, long long* __restrict__ out,
                                                       long long* __restrict__ bsum) {
    __shared__ long long sh[256];
    const long long b0 = (long long)blockIdx.x * LC_SCAN_PER_BLOCK + threadIdx.x * 4;
    long long v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = b0 + k < n ? in[b0 + k] : 0;
        s += v[k];
    }
    long long total;
    long long ex = lc_block_scan(s, sh, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (b0 + k < n) out[b0 + k] = ex;
        ex += v[k];
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_lc_scan_tops(long long* __restrict__ bsum, int nb, long long* __restrict__ total_out) {
    __shared__ long long sh[256];
    long long carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int k = b0 + threadIdx.x;
        const long long v = k < nb ? bsum[k] : 0;
        long long total;
        const long long ex = lc_block_scan(v, sh, &total);
        if (k < nb) bsum[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(256) void k_lc_scan_add(long long* __restrict__ out, long long n, const long long* __restrict__ bsum) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] += bsum[i / LC_SCAN_PER_BLOCK];
}

__global__ __launch_bounds__(256) void k_lc_offsets(const long long* __restrict__ base, const long long* __restrict__ total,
                                                    int nimg, int nwave, long long* __restrict__ offsets) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nimg) offsets[i] = base[(size_t)i * nwave];
    else if (i == nimg) offsets[i] = *total;
}

// ---- batched forced photometry -----------------------------------------------------------------------------------------
// One wave per pair (grid = npairs, strided beyond LC_MAX_GRID).  The pair index comes from blockIdx.x, so the search and every field of the image's record are
// uniform: they stay in SGPRs (scalar loads), and the fp64 sin / cos of the position are the only transcendentals
// (the frame of the WCS comes from the host).
__global__ __launch_bounds__(64) void k_lc_batch(const lc_rec* __restrict__ recs, int nimg,
                                                 const long long* __restrict__ offsets, const int32_t* __restrict__ src_idx,
                                                 long long npairs, int nsrc, const double* __restrict__ ra, const double* __restrict__ dec,
                                                 double r, double* __restrict__ xo, double* __restrict__ yo,
                                                 double* __restrict__ flux, double* __restrict__ err,
                                                 int32_t* __restrict__ flags) {
    const int lane = threadIdx.x;
    for (long long p = blockIdx.x; p < npairs; p += gridDim.x) {
        int lo = 0, hi = nimg;                           // offsets[lo] <= p < offsets[hi], whatever lies between
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= p) lo = mid; else hi = mid;
        }
        const lc_rec* __restrict__ R = recs + lo;
        const int s = src_idx[p];
        double x = __builtin_nan(""), y = x;
        if (s >= 0 && s < nsrc) {
            // zm_wcs_sky2pix, step by step
            const double a = ra[s] * LC_D2R, d = dec[s] * LC_D2R;
            const double v[3] = {cos(d) * cos(a), cos(d) * sin(a), sin(d)};
            double ta = 0, tb = 0, tc = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ta += v[k] * R->fr[k];
                tb += v[k] * R->fr[3 + k];
                tc += v[k] * R->fr[6 + k];
            }
            zm_plane2pix(&R->wcs, ta / tc / LC_D2R, tb / tc / LC_D2R, &x, &y);
            x -= 1.0;                                    // FITS 1-based -> 0-based, as all_world2pix(.., 0)
            y -= 1.0;
        }
        double f, e;
        int32_t fl;
        ap_wave_sum(R->img, R->rms, R->mask, R->nx, R->ny, x, y, r, lane, &f, &e, &fl);
        if (lane == 0) {
            xo[p] = x;
            yo[p] = y;
            flux[p] = f;
            err[p] = e;
            flags[p] = fl;
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
static size_t lc_up(size_t b) { return (b + 255) & ~(size_t)255; }

static double lc_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// vertices, inward normals and cap of one footprint; a polygon that is degenerate or not convex is an error
static int lc_make_foot(const char* who, int index, const zm_wcs* w, lc_foot* F) {
    char what[96];
    snprintf(what, sizeof(what), "%s: image %d", who, index);
    ZM_TRY(zm_check_wcs(w, what));
    double fr[9], c[4][3];
    zm_wcs_frame(w, fr);
    const double nx = w->naxis[0], ny = w->naxis[1];
    const double px[4] = {1.0, 1.0, nx, nx}, py[4] = {1.0, ny, ny, 1.0};        // WCS.calc_footprint's order
    for (int k = 0; k < 4; ++k) {
        zm_wcs_pix2vec(w, fr, px[k], py[k], c[k]);
        ZM_CHECK(std::isfinite(c[k][0]) && std::isfinite(c[k][1]) && std::isfinite(c[k][2]), "%s: corner %d is not finite", what, k);
    }
    const double tiny = 1e-14;                           // (a corner pixel of a ZTF frame is 5e-6 rad from the next)
    double n[4][3];
    for (int k = 0; k < 4; ++k) {
        const double *a = c[k], *b = c[(k + 1) & 3];
        n[k][0] = a[1] * b[2] - a[2] * b[1];
        n[k][1] = a[2] * b[0] - a[0] * b[2];
        n[k][2] = a[0] * b[1] - a[1] * b[0];
        const double len = sqrt(lc_dot(n[k], n[k]));
        ZM_CHECK(len > tiny, "%s: the footprint is degenerate (corners %d and %d coincide)", what, k, (k + 1) & 3);
        for (int j = 0; j < 3; ++j) n[k][j] /= len;
    }
    const double s = lc_dot(n[0], c[2]) > 0.0 ? 1.0 : -1.0;      // the polygon's own orientation
    for (int k = 0; k < 4; ++k)
        for (int j = 2; j <= 3; ++j)
            ZM_CHECK(s * lc_dot(n[k], c[(k + j) & 3]) > tiny, "%s: the footprint is degenerate or not convex (corner %d against edge %d)",
                     what, (k + j) & 3, k);
    double sum[3];
    for (int j = 0; j < 3; ++j) sum[j] = c[0][j] + c[1][j] + c[2][j] + c[3][j];
    const double len = sqrt(lc_dot(sum, sum));
    ZM_CHECK(len > tiny, "%s: the footprint has no centre", what);
    double cosr = 1.0;
    for (int j = 0; j < 3; ++j) F->c[j] = sum[j] / len;
    for (int k = 0; k < 4; ++k) cosr = std::min(cosr, lc_dot(F->c, c[k]));
    ZM_CHECK(cosr > 0.0, "%s: the footprint spans a hemisphere", what);
    F->cosr = cosr - 8.0 * 2.220446049250313e-16;        // a few ulp of 1: the pre-test must never reject what the planes accept
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 3; ++j) F->n[k][j] = s * n[k][j];
    return 0;
}

// the pinned image table ("lc_tab_h"), free to be rewritten: the copy the last call enqueued out of it has finished
static int lc_pinned_table(zm_ctx* ctx, size_t bytes, void** out) {
    if (ctx->lc_tab_event) ZM_HIP(hipEventSynchronize(ctx->lc_tab_event));
    else ZM_HIP(hipEventCreateWithFlags(&ctx->lc_tab_event, hipEventDisableTiming));
    return ctx->get_pinned("lc_tab_h", bytes, out);
}

extern "C" int zm_footprint_join_dev(zm_ctx* ctx, int nimg, const zm_wcs* wcs, int nsrc, const double* ra_dev,
                                     const double* dec_dev, int64_t capacity, int64_t* offsets_dev, int32_t* src_idx_dev,
                                     int64_t* out_npairs) {
    ZM_CHECK(ctx && offsets_dev && out_npairs, "zm_footprint_join_dev: null argument");
    ZM_CHECK(nimg >= 0 && nimg <= 65535, "zm_footprint_join_dev: nimg must be 0 .. 65535 (got %d)", nimg);
    ZM_CHECK(nsrc >= 0 && nsrc <= (1 << 30), "zm_footprint_join_dev: nsrc must be 0 .. 2^30 (got %d)", nsrc);
    ZM_CHECK(capacity >= 0, "zm_footprint_join_dev: negative capacity");
    ZM_CHECK(nimg == 0 || wcs, "zm_footprint_join_dev: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    *out_npairs = 0;
    lc_foot* fh = nullptr;
    if (nimg) {                                          // geometry first: a bad footprint is an error whatever nsrc is
        ZM_TRY(lc_pinned_table(ctx, sizeof(lc_foot) * (size_t)nimg, (void**)&fh));
        for (int i = 0; i < nimg; ++i) ZM_TRY(lc_make_foot("zm_footprint_join_dev", i, &wcs[i], &fh[i]));
    }
    if (nimg == 0 || nsrc == 0) {
        ZM_HIP(hipMemsetAsync(offsets_dev, 0, sizeof(int64_t) * ((size_t)nimg + 1), ctx->stream));
        return 0;
    }
    ZM_CHECK(ra_dev && dec_dev && (capacity == 0 || src_idx_dev), "zm_footprint_join_dev: null argument");
    const int nblk = zm_div_up(nsrc, 256), nwave = nblk * 4;
    const size_t N = (size_t)nsrc, M = (size_t)nimg * nwave;
    ZM_CHECK(M <= ((size_t)1 << 30), "zm_footprint_join_dev: %d images x %d sources is more than one call takes", nimg, nsrc);
    const int nb = (int)((M + LC_SCAN_PER_BLOCK - 1) / LC_SCAN_PER_BLOCK);
    const size_t o_v = 0, o_foot = o_v + lc_up(3 * N * 8), o_cnt = o_foot + lc_up(sizeof(lc_foot) * (size_t)nimg),
                 o_base = o_cnt + lc_up(M * 4), o_bsum = o_base + lc_up(M * 8), o_tot = o_bsum + lc_up((size_t)nb * 8),
                 total = o_tot + 256;
    char* w = nullptr;
    ZM_TRY(ctx->get("lc_join", total, (void**)&w));
    double *vx = (double*)(w + o_v), *vy = vx + N, *vz = vy + N;
    lc_foot* fd = (lc_foot*)(w + o_foot);
    int32_t* cnt = (int32_t*)(w + o_cnt);
    long long *base = (long long*)(w + o_base), *bsum = (long long*)(w + o_bsum), *tot = (long long*)(w + o_tot);
    long long* th = nullptr;
    ZM_TRY(ctx->get_pinned("lc_total_h", sizeof(long long), (void**)&th));
    {
        zm_scope_timer timer(ctx, "lc_join");
        ZM_HIP(hipMemcpyAsync(fd, fh, sizeof(lc_foot) * (size_t)nimg, hipMemcpyHostToDevice, ctx->stream));
        ZM_HIP(hipEventRecord(ctx->lc_tab_event, ctx->stream));
        const dim3 grid((unsigned)nblk, (unsigned)nimg), block(256);
        hipLaunchKernelGGL(k_lc_unit, dim3((unsigned)nblk), block, 0, ctx->stream, ra_dev, dec_dev, nsrc, vx, vy, vz);
        hipLaunchKernelGGL(k_lc_join<false>, grid, block, 0, ctx->stream, fd, vx, vy, vz, nsrc, cnt, (const long long*)nullptr,
                           0ll, (int32_t*)nullptr);
        hipLaunchKernelGGL(k_lc_scan_local, dim3((unsigned)nb), block, 0, ctx->stream, cnt, (long long)M, base, bsum);
        hipLaunchKernelGGL(k_lc_scan_tops, dim3(1), block, 0, ctx->stream, bsum, nb, tot);
        hipLaunchKernelGGL(k_lc_scan_add, dim3((unsigned)((M + 255) / 256)), block, 0, ctx->stream, base, (long long)M, bsum);
        hipLaunchKernelGGL(k_lc_offsets, dim3((unsigned)zm_div_up(nimg + 1, 256)), block, 0, ctx->stream, base, tot, nimg, nwave,
                           (long long*)offsets_dev);
        if (capacity > 0)
            hipLaunchKernelGGL(k_lc_join<true>, grid, block, 0, ctx->stream, fd, vx, vy, vz, nsrc, (int32_t*)nullptr, base,
                               (long long)capacity, src_idx_dev);
        ZM_HIP(hipGetLastError());
        ZM_HIP(hipMemcpyAsync(th, tot, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    }
    ZM_HIP(hipStreamSynchronize(ctx->stream));           // the one word the caller sizes its next call by
    *out_npairs = (int64_t)*th;
    return 0;
}

extern "C" int zm_footprint_join(zm_ctx* ctx, int nimg, const zm_wcs* wcs, int nsrc, const double* ra, const double* dec,
                                 int64_t capacity, int64_t* offsets, int32_t* src_idx, int64_t* out_npairs) {
    ZM_CHECK(ctx && offsets && out_npairs, "zm_footprint_join: null argument");
    ZM_CHECK(nimg >= 0 && nimg <= 65535, "zm_footprint_join: nimg must be 0 .. 65535 (got %d)", nimg);
    ZM_CHECK(nsrc >= 0 && nsrc <= (1 << 30), "zm_footprint_join: nsrc must be 0 .. 2^30 (got %d)", nsrc);
    ZM_CHECK(capacity >= 0 && (capacity == 0 || src_idx), "zm_footprint_join: bad capacity or null pair list");
    ZM_CHECK(nsrc == 0 || (ra && dec), "zm_footprint_join: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)nsrc, K = (size_t)nimg + 1, cap = (size_t)capacity;
    const size_t o_ra = 0, o_dec = o_ra + lc_up(N * 8), o_off = o_dec + lc_up(N * 8), o_idx = o_off + lc_up(K * 8),
                 total = o_idx + lc_up(cap * 4) + 256;
    char* d = nullptr;
    ZM_TRY(ctx->get("h_lc_io", total, (void**)&d));
    if (nsrc) {
        ZM_HIP(hipMemcpyAsync(d + o_ra, ra, N * 8, hipMemcpyHostToDevice, ctx->stream));
        ZM_HIP(hipMemcpyAsync(d + o_dec, dec, N * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    ZM_TRY(zm_footprint_join_dev(ctx, nimg, wcs, nsrc, (const double*)(d + o_ra), (const double*)(d + o_dec), capacity,
                                 (int64_t*)(d + o_off), (int32_t*)(d + o_idx), out_npairs));
    ZM_HIP(hipMemcpyAsync(offsets, d + o_off, K * 8, hipMemcpyDeviceToHost, ctx->stream));
    const size_t got = std::min((size_t)*out_npairs, cap);
    if (got) ZM_HIP(hipMemcpyAsync(src_idx, d + o_idx, got * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int zm_forced_photometry_batch_dev(zm_ctx* ctx, int nimg, const zm_lc_image* images, const int64_t* offsets_dev,
                                              const int32_t* src_idx_dev, int64_t npairs, int nsrc, const double* ra_dev,
                                              const double* dec_dev, double radius, double* x_dev, double* y_dev,
                                              double* flux_dev, double* err_dev, int32_t* flags_dev) {
    ZM_CHECK(ctx, "zm_forced_photometry_batch_dev: null argument");
    ZM_CHECK(nimg >= 0 && nimg <= 65535, "zm_forced_photometry_batch_dev: nimg must be 0 .. 65535 (got %d)", nimg);
    ZM_CHECK(nsrc >= 0 && nsrc <= (1 << 30), "zm_forced_photometry_batch_dev: nsrc must be 0 .. 2^30 (got %d)", nsrc);
    ZM_CHECK(npairs >= 0 && npairs <= 0x7fffffffll, "zm_forced_photometry_batch_dev: npairs must be 0 .. 2^31 - 1 (got %lld)",
             (long long)npairs);
    ZM_CHECK(radius > 0 && radius < 512, "zm_forced_photometry_batch_dev: radius %g outside (0, 512)", radius);
    if (npairs == 0) return 0;
    ZM_CHECK(nimg > 0 && nsrc > 0, "zm_forced_photometry_batch_dev: %lld pairs of %d images and %d sources", (long long)npairs, nimg,
             nsrc);
    ZM_CHECK(images && offsets_dev && src_idx_dev && ra_dev && dec_dev && x_dev && y_dev && flux_dev && err_dev && flags_dev,
             "zm_forced_photometry_batch_dev: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    lc_rec* rh = nullptr;
    ZM_TRY(lc_pinned_table(ctx, sizeof(lc_rec) * (size_t)nimg, (void**)&rh));
    for (int i = 0; i < nimg; ++i) {
        char what[96];
        snprintf(what, sizeof(what), "zm_forced_photometry_batch_dev: image %d", i);
        ZM_TRY(zm_check_wcs(&images[i].wcs, what));
        ZM_CHECK(images[i].img, "%s: null plane", what);
        ZM_CHECK(images[i].nx > 0 && images[i].ny > 0, "%s: bad sizes", what);
        lc_rec& R = rh[i];
        R.img = images[i].img; R.rms = images[i].rms; R.mask = images[i].mask;
        R.nx = images[i].nx; R.ny = images[i].ny;
        R.wcs = images[i].wcs;
        zm_wcs_mark_order(&R.wcs);
        zm_wcs_frame(&R.wcs, R.fr);
    }
    lc_rec* rd = nullptr;
    ZM_TRY(ctx->get("lc_tab", sizeof(lc_rec) * (size_t)nimg, (void**)&rd));
    zm_scope_timer timer(ctx, "lc_batch");
    // the device table is rewritten in stream order behind the kernel of an earlier call; the pinned one is guarded by the event
    ZM_HIP(hipMemcpyAsync(rd, rh, sizeof(lc_rec) * (size_t)nimg, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipEventRecord(ctx->lc_tab_event, ctx->stream));
    hipLaunchKernelGGL(k_lc_batch, dim3((unsigned)std::min<int64_t>(npairs, LC_MAX_GRID)), dim3(64), 0, ctx->stream, rd, nimg,
                       (const long long*)offsets_dev, src_idx_dev, (long long)npairs, nsrc, ra_dev, dec_dev, radius, x_dev, y_dev, flux_dev, err_dev, flags_dev);
    ZM_HIP(hipGetLastError());
    return 0;
}
