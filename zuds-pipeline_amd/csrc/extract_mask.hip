// MASK_TYPE BLANK / CORRECT of sextractor.conf for the extractor's second pass: the Kron, windowed and aperture sums of
// an object with the pixels of its neighbours (and its own bad pixels) taken out or replaced by their mirror about the
// object's centre.  The operator is a chosen convention, stated in DESIGN.md ("MASK_TYPE") and restated in numpy in
// tests/mask_ref.py.  Opt-in: zm_extract_measure and its kernels (extract_measure.hip) are what they were.
//
//   k_ex_kron_m<CORRECT>   k_ex_kron with the replacement step in both flux walks (about the isophotal barycentre)
//   k_ex_win_m<CORRECT>    k_ex_win with the replacement step in every pass (about that pass's centre)
//   k_ex_aper_m<CORRECT>   the circular aperture about the barycentre: exact overlap, replaced values, lost pixels left out
// A pixel is unusable for object k when it is bad (mx_isbad) or belongs to another object (seg != 0 && seg != NUMBER).
// CORRECT: it takes value and sigma of its mirror where that lies in the frame and is usable for k (counted in nrepl),
// otherwise it adds nothing (nlost).  BLANK: every unusable pixel is lost.  Weights that depend on position (ellipse
// radius, circle overlap, the window's Gaussian) are taken at the pixel itself.
// Summation as in extract_measure.hip: one 256-thread workgroup per object, element e of a row-major clipped box on
// lane e % 256, float64 partials, xor shuffles, waves added in order through LDS, every decision uniform over the
// workgroup.  An object without an unusable pixel in its footprints sums the same values in the same order as the
// unmasked kernels: the same bits.  Every read is of a pixel inside the frame: boxes are clipped, mirrors are tested.
#include "aperture_dev.h"

// one rounding per operation in everything below, as in extract_measure.hip
#pragma clang fp contract(off)

#include "measure_dev.h"

struct mk_out {                      // what the masked pass has beyond mx_kout / mx_wout; each kernel writes its own fields
    double flux_aper, fluxerr_aper;
    int nrepl_auto, nap, nrepl_aper, nlost_aper, nrepl_win, nlost_win;
};

#define MK_USE 0                     // the pixel itself
#define MK_REPL 1                    // its mirror
#define MK_LOST 2                    // nothing

__device__ __forceinline__ bool mk_unusable(const float* __restrict__ img, const float* __restrict__ sig,
                                            const uint8_t* __restrict__ bad, const int* __restrict__ seg, int number,
                                            size_t p) {
    const int s = seg[p];
    return mx_bad_at(img, sig, bad, p) || (s != 0 && s != number);
}

// where pixel (i, j) (index p, inside the frame) of object `number` takes its value from: *q is p (MK_USE) or the mirror
// about (cx, cy) (MK_REPL); MK_LOST leaves *q = p
template <bool CORRECT>
__device__ __forceinline__ int mk_source(const float* __restrict__ img, const float* __restrict__ sig,
                                         const uint8_t* __restrict__ bad, const int* __restrict__ seg, int nx, int ny,
                                         int number, int i, int j, size_t p, double cx, double cy, size_t* q) {
    *q = p;
    if (!mk_unusable(img, sig, bad, seg, number, p)) return MK_USE;
    if (!CORRECT) return MK_LOST;
    const double mi = floor((2.0 * cx - i) + 0.5), mj = floor((2.0 * cy - j) + 0.5);
    if (!isfinite(mi) || !isfinite(mj)) return MK_LOST;
    const int ii = mx_int(mi, nx), jj = mx_int(mj, ny);
    if (ii < 0 || ii >= nx || jj < 0 || jj >= ny) return MK_LOST;
    const size_t m = (size_t)jj * nx + ii;
    if (mk_unusable(img, sig, bad, seg, number, m)) return MK_LOST;
    *q = m;
    return MK_REPL;
}

// "frac > 0" for the counts: the pixel's square reaches inside the circle (the point of the square nearest to the centre
// lies inside the radius: the rule of FLAGS bit 16).  The computed overlap of a pixel outside the circle is a rounding
// residue of either sign, so its sign is not asked.
__device__ __forceinline__ bool mk_reaches(double dx, double dy, double r) {
    const double ax = fmax(fabs(dx) - 0.5, 0.0), ay = fmax(fabs(dy) - 0.5, 0.0);
    return ax * ax + ay * ay < r * r;
}

template <bool CORRECT>
__global__ __launch_bounds__(256) void k_ex_kron_m(const float* __restrict__ img, const float* __restrict__ sig,
                                                   const uint8_t* __restrict__ bad, const int* __restrict__ seg, int nx,
                                                   int ny, const mx_obj* __restrict__ obj, int nobj, double kfact,
                                                   double kmin, int use_filter, mx_kout* __restrict__ out,
                                                   mk_out* __restrict__ mout) {
    __shared__ double sh2[4][2], sh7[4][7];
    __shared__ int shi[4][3];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (k >= nobj) return;
    const mx_obj o = obj[k];
    // ---- walk 1: s0 = sum v', s1 = sum sqrt(r2) v' over r2 <= 36 ------------------------------------------------
    double s[2] = {0.0, 0.0};
    {
        const int bw = o.sx1 - o.sx0, bh = o.sy1 - o.sy0;
        const int total = (o.valid && bw > 0 && bh > 0) ? bw * bh : 0;
        for (int e = tid; e < total; e += 256) {
            const int j = o.sy0 + e / bw, i = o.sx0 + e % bw;
            const size_t p = (size_t)j * nx + i;
            const double dx = i - o.xc, dy = j - o.yc;
            const double r2 = o.cxx * dx * dx + o.cyy * dy * dy + o.cxy * dx * dy;
            if (!(r2 <= 36.0)) continue;
            size_t q;
            if (mk_source<CORRECT>(img, sig, bad, seg, nx, ny, o.number, i, j, p, o.xc, o.yc, &q) == MK_LOST) continue;
            const double v = img[q];
            s[0] += v;
            s[1] += sqrt(fmax(r2, 0.0)) * v;
        }
    }
    mx_reduce<2>(s, sh2, lane, wave);
    const double r1 = (s[0] > 0.0 && s[1] > 0.0) ? s[1] / s[0] : 0.0;
    const double R = fmax(kfact * r1, kmin), R2 = R * R;
    // ---- walk 2: the flux sums over r2 <= R^2 -------------------------------------------------------------------
    double f[2] = {0.0, 0.0};
    int np = 0, nl = 0, nr = 0;
    {
        const double hx = R * o.sx, hy = R * o.sy;
        const int i0 = max(mx_int(floor(o.xc - hx), nx), 0), i1 = min(mx_int(ceil(o.xc + hx), nx) + 1, nx);
        const int j0 = max(mx_int(floor(o.yc - hy), ny), 0), j1 = min(mx_int(ceil(o.yc + hy), ny) + 1, ny);
        const int bw = i1 - i0, bh = j1 - j0;
        const int total = (o.valid && bw > 0 && bh > 0) ? bw * bh : 0;
        for (int e = tid; e < total; e += 256) {
            const int j = j0 + e / bw, i = i0 + e % bw;
            const size_t p = (size_t)j * nx + i;
            const double dx = i - o.xc, dy = j - o.yc;
            const double r2 = o.cxx * dx * dx + o.cyy * dy * dy + o.cxy * dx * dy;
            if (!(r2 <= R2)) continue;
            size_t q;
            const int how = mk_source<CORRECT>(img, sig, bad, seg, nx, ny, o.number, i, j, p, o.xc, o.yc, &q);
            if (how == MK_LOST) { ++nl; continue; }
            if (how == MK_REPL) ++nr;
            const double sg = sig[q];
            f[0] += (double)img[q];
            f[1] += sg * sg;
            ++np;
        }
    }
    mx_reduce<2>(f, sh2, lane, wave);
    np = mx_wsumi(np);
    nl = mx_wsumi(nl);
    nr = mx_wsumi(nr);
    if (lane == 0) { shi[wave][0] = np; shi[wave][1] = nl; shi[wave][2] = nr; }
    // ---- walk 3: the isophotal error sums over the members (unchanged) ------------------------------------------
    double m[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    mx_iso_sums(img, sig, bad, seg, nx, ny, o, use_filter, tid, m);
    mx_reduce<7>(m, sh7, lane, wave);                    // (its barriers also publish shi)
    if (tid == 0) {
        mx_kout r;
        r.r1 = r1; r.radius = R; r.flux = f[0]; r.var = f[1];
        r.sumf = m[0];
#pragma unroll
        for (int q = 0; q < 6; ++q) r.e[q] = m[q + 1];
        r.npix = shi[0][0] + shi[1][0] + shi[2][0] + shi[3][0];
        r.nskip = shi[0][1] + shi[1][1] + shi[2][1] + shi[3][1];
        out[k] = r;
        mout[k].nrepl_auto = shi[0][2] + shi[1][2] + shi[2][2] + shi[3][2];
    }
}

// mx_win_pass with the replacement step about (cx, cy).  FINAL also counts, over the pixels the circle reaches (mk_reaches), the replaced
// (*nrepl) and the lost (*nlost) ones, per lane
template <bool FINAL, bool CORRECT, int N>
__device__ __forceinline__ void mk_win_pass(const float* __restrict__ img, const float* __restrict__ sig,
                                            const uint8_t* __restrict__ bad, const int* __restrict__ seg, int nx, int ny,
                                            int number, double cx, double cy, double r, double tw, int tid,
                                            double (&s)[N], int* nrepl, int* nlost) {
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] = 0.0;
    const int i0 = max(mx_int(floor(cx - r + 0.5), nx), 0), i1 = min(mx_int(ceil(cx + r + 0.5), nx), nx);
    const int j0 = max(mx_int(floor(cy - r + 0.5), ny), 0), j1 = min(mx_int(ceil(cy + r + 0.5), ny), ny);
    const int bw = i1 - i0, bh = j1 - j0;
    const int total = (bw > 0 && bh > 0) ? bw * bh : 0;
    for (int e = tid; e < total; e += 256) {
        const int j = j0 + e / bw, i = i0 + e % bw;
        const size_t p = (size_t)j * nx + i;
        size_t q;
        const int how = mk_source<CORRECT>(img, sig, bad, seg, nx, ny, number, i, j, p, cx, cy, &q);
        if (!FINAL && how == MK_LOST) continue;
        const double dx = i - cx, dy = j - cy;
        const double x0 = i - 0.5 - cx, x1 = i + 0.5 - cx, y0 = j - 0.5 - cy, y1 = j + 0.5 - cy;
        const double frac = ap_signed(x1, y1, r) - ap_signed(x0, y1, r) - ap_signed(x1, y0, r) + ap_signed(x0, y0, r);
        if (FINAL) {
            if (mk_reaches(dx, dy, r)) {
                if (how == MK_REPL) ++*nrepl;
                if (how == MK_LOST) ++*nlost;
            }
            if (how == MK_LOST) continue;
        }
        const double w = frac * exp(-((dx * dx + dy * dy) / tw));
        const double v = img[q], wv = w * v;
        s[0] += wv;
        if (!FINAL) {
            s[1] += wv * dx;
            s[2] += wv * dy;
        } else {
            const double sg = sig[q], ws = w * w * (sg * sg);
            s[1] += wv * dx * dx;
            s[2] += wv * dy * dy;
            s[3] += wv * dx * dy;
            s[4] += ws * dx * dx;
            s[5] += ws * dy * dy;
            s[6] += ws * dx * dy;
        }
    }
}

template <bool CORRECT>
__global__ __launch_bounds__(256) void k_ex_win_m(const float* __restrict__ img, const float* __restrict__ sig,
                                                  const uint8_t* __restrict__ bad, const int* __restrict__ seg, int nx,
                                                  int ny, const mx_obj* __restrict__ obj, int nobj,
                                                  mx_wout* __restrict__ out, mk_out* __restrict__ mout) {
    __shared__ double sh3[4][3], sh7[4][7];
    __shared__ int shi[4][2];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (k >= nobj) return;
    const mx_obj o = obj[k];
    double cx = o.xc, cy = o.yc;
    const double r = 4.0 * o.sw;
    const bool usable = o.sw > 0.0 && r < 1e9;           // false for NaN as well
    int niter = 0, flags = usable ? 0 : 1;
    bool converged = false;
    int nr = 0, nl = 0;
    // every thread holds the same reduced sums after mx_reduce, so every branch below is uniform over the workgroup
    for (int it = 0; it < MX_WIN_ITER && flags == 0 && !converged; ++it) {
        double s[3];
        mk_win_pass<false, CORRECT>(img, sig, bad, seg, nx, ny, o.number, cx, cy, r, o.tw, tid, s, &nr, &nl);
        mx_reduce<3>(s, sh3, lane, wave);
        niter = it + 1;
        if (!(s[0] > 0.0)) { flags |= 1; break; }
        const double stx = 2.0 * s[1] / s[0], sty = 2.0 * s[2] / s[0];
        cx += stx;
        cy += sty;
        converged = stx * stx + sty * sty < MX_WIN_STEP2;
    }
    if (flags == 0 && !converged) flags |= 2;
    double m[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool final_pass = !(flags & 1);                // (counts of a final pass stay where its sum then falls back)
    if (final_pass) {
        mk_win_pass<true, CORRECT>(img, sig, bad, seg, nx, ny, o.number, cx, cy, r, o.tw, tid, m, &nr, &nl);
        nr = mx_wsumi(nr);
        nl = mx_wsumi(nl);
        if (lane == 0) { shi[wave][0] = nr; shi[wave][1] = nl; }
        mx_reduce<7>(m, sh7, lane, wave);                // (its barriers also publish shi)
        if (!(m[0] > 0.0)) flags |= 1;
    }
    if (tid == 0) {
        mx_wout w;
        w.cx = cx; w.cy = cy;
#pragma unroll
        for (int q = 0; q < 7; ++q) w.m[q] = m[q];
        w.niter = niter; w.flags = flags;
        out[k] = w;
        mout[k].nrepl_win = final_pass ? shi[0][0] + shi[1][0] + shi[2][0] + shi[3][0] : 0;
        mout[k].nlost_win = final_pass ? shi[0][1] + shi[1][1] + shi[2][1] + shi[3][1] : 0;
    }
}

// The circle of radius r about the barycentre, box rule of ap_wave_sum (aperture_dev.h): flux = sum frac v',
// var = sum frac sigma'^2; over the pixels of the clipped box that the circle reaches (mk_reaches): nap, the replaced and the lost ones
template <bool CORRECT>
__global__ __launch_bounds__(256) void k_ex_aper_m(const float* __restrict__ img, const float* __restrict__ sig,
                                                   const uint8_t* __restrict__ bad, const int* __restrict__ seg, int nx,
                                                   int ny, const mx_obj* __restrict__ obj, int nobj, double r,
                                                   mk_out* __restrict__ mout) {
    __shared__ double sh2[4][2];
    __shared__ int shi[4][3];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (k >= nobj) return;
    const mx_obj o = obj[k];
    const double cx = o.xc, cy = o.yc;
    double f[2] = {0.0, 0.0};
    int na = 0, nr = 0, nl = 0;
    {
        const int i0 = max(mx_int(floor(cx - r + 0.5), nx), 0), i1 = min(mx_int(ceil(cx + r + 0.5), nx), nx);
        const int j0 = max(mx_int(floor(cy - r + 0.5), ny), 0), j1 = min(mx_int(ceil(cy + r + 0.5), ny), ny);
        const int bw = i1 - i0, bh = j1 - j0;
        const int total = (o.valid && bw > 0 && bh > 0) ? bw * bh : 0;
        for (int e = tid; e < total; e += 256) {
            const int j = j0 + e / bw, i = i0 + e % bw;
            const size_t p = (size_t)j * nx + i;
            const double x0 = i - 0.5 - cx, x1 = i + 0.5 - cx, y0 = j - 0.5 - cy, y1 = j + 0.5 - cy;
            const double frac = ap_signed(x1, y1, r) - ap_signed(x0, y1, r) - ap_signed(x1, y0, r) + ap_signed(x0, y0, r);
            size_t q;
            const int how = mk_source<CORRECT>(img, sig, bad, seg, nx, ny, o.number, i, j, p, cx, cy, &q);
            if (mk_reaches(i - cx, j - cy, r)) {
                ++na;
                if (how == MK_REPL) ++nr;
                if (how == MK_LOST) ++nl;
            }
            if (how == MK_LOST) continue;
            const double v = img[q], sg = sig[q];
            f[0] += frac * v;
            f[1] += frac * (sg * sg);
        }
    }
    mx_reduce<2>(f, sh2, lane, wave);
    na = mx_wsumi(na);
    nr = mx_wsumi(nr);
    nl = mx_wsumi(nl);
    if (lane == 0) { shi[wave][0] = na; shi[wave][1] = nr; shi[wave][2] = nl; }
    __syncthreads();
    if (tid == 0) {
        mout[k].flux_aper = f[0];
        // a finite sum that rounds below 0 is 0; one that is not finite stays so (the rule of ap_wave_sum)
        mout[k].fluxerr_aper = sqrt(isfinite(f[1]) ? fmax(f[1], 0.0) : f[1]);
        mout[k].nap = shi[0][0] + shi[1][0] + shi[2][0] + shi[3][0];
        mout[k].nrepl_aper = shi[0][1] + shi[1][1] + shi[2][1] + shi[3][1];
        mout[k].nlost_aper = shi[0][2] + shi[1][2] + shi[2][2] + shi[3][2];
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------
extern "C" void zm_mask_params_default(zm_mask_params* p) {
    if (!p) return;
    p->type = ZM_MASK_CORRECT;
    p->pad_ = 0;
    p->aper_radius = 3.0;
}

template <bool CORRECT>
static void mk_launch(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad, const int32_t* seg, int nx,
                      int ny, const mx_obj* d_obj, int n, const zm_measure_params* params, double aper_radius, mx_kout* d_k,
                      mx_wout* d_w, mk_out* d_m) {
    hipLaunchKernelGGL(k_ex_kron_m<CORRECT>, dim3(n), dim3(256), 0, ctx->stream, img, sigma, bad, seg, nx, ny, d_obj, n,
                       params->kron_fact, params->kron_min_radius, params->filter, d_k, d_m);
    hipLaunchKernelGGL(k_ex_win_m<CORRECT>, dim3(n), dim3(256), 0, ctx->stream, img, sigma, bad, seg, nx, ny, d_obj, n,
                       d_w, d_m);
    hipLaunchKernelGGL(k_ex_aper_m<CORRECT>, dim3(n), dim3(256), 0, ctx->stream, img, sigma, bad, seg, nx, ny, d_obj, n,
                       aper_radius, d_m);
}

static int mk_check_mask(const zm_mask_params* mask) {
    ZM_CHECK(mask, "zm_extract_measure_masked: null argument");
    ZM_CHECK(mask->type == ZM_MASK_BLANK || mask->type == ZM_MASK_CORRECT,
             "zm_extract_measure_masked: bad mask type %d (ZM_MASK_BLANK, ZM_MASK_CORRECT)", mask->type);
    ZM_CHECK(mask->aper_radius > 0 && mask->aper_radius < 512, "zm_extract_measure_masked: bad aperture radius %g",
             mask->aper_radius);
    return 0;
}

extern "C" int zm_extract_measure_masked_dev(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                                             const int32_t* segm_dev, int nx, int ny, const zm_wcs* wcs,
                                             const zm_measure_params* params, int n, const zm_object* rows,
                                             zm_object_ext* out, const zm_mask_params* mask, zm_object_mask* out_mask) {
    ZM_TRY(mx_check_args("zm_extract_measure_masked", ctx, img, sigma, segm_dev, nx, ny, params, n));
    ZM_TRY(mk_check_mask(mask));
    if (n == 0) return 0;
    ZM_CHECK(rows && out && out_mask, "zm_extract_measure_masked: %d rows need a row array and both output arrays", n);
    ZM_HIP(hipSetDevice(ctx->device));
    std::vector<mx_obj> objs;
    mx_prepare(rows, n, nx, ny, objs);
    char* d = nullptr;
    const size_t b_obj = ((size_t)n * sizeof(mx_obj) + 15) & ~(size_t)15, b_k = ((size_t)n * sizeof(mx_kout) + 15) & ~(size_t)15,
                 b_w = ((size_t)n * sizeof(mx_wout) + 15) & ~(size_t)15;
    ZM_TRY(ctx->get("mx_buf", b_obj + b_k + b_w + (size_t)n * sizeof(mk_out), (void**)&d));
    mx_obj* d_obj = (mx_obj*)d;
    mx_kout* d_k = (mx_kout*)(d + b_obj);
    mx_wout* d_w = (mx_wout*)(d + b_obj + b_k);
    mk_out* d_m = (mk_out*)(d + b_obj + b_k + b_w);
    ZM_HIP(hipMemcpyAsync(d_obj, objs.data(), (size_t)n * sizeof(mx_obj), hipMemcpyHostToDevice, ctx->stream));
    if (mask->type == ZM_MASK_CORRECT)
        mk_launch<true>(ctx, img, sigma, bad, segm_dev, nx, ny, d_obj, n, params, mask->aper_radius, d_k, d_w, d_m);
    else
        mk_launch<false>(ctx, img, sigma, bad, segm_dev, nx, ny, d_obj, n, params, mask->aper_radius, d_k, d_w, d_m);
    ZM_HIP(hipGetLastError());
    std::vector<mx_kout> kout(n);
    std::vector<mx_wout> wout(n);
    std::vector<mk_out> mo(n);
    ZM_HIP(hipMemcpyAsync(kout.data(), d_k, (size_t)n * sizeof(mx_kout), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(wout.data(), d_w, (size_t)n * sizeof(mx_wout), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(mo.data(), d_m, (size_t)n * sizeof(mk_out), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    // nskip = nlost in kout: mx_finish takes FLAGS_AUTO bits 1, 2 and 4 by their formulas
    ZM_TRY(mx_finish(rows, n, nx, ny, wcs, objs, kout, wout, out));
    for (int k = 0; k < n; ++k) {
        const mk_out& q = mo[k];
        zm_object_mask* m = out_mask + k;
        memset(m, 0, sizeof(*m));
        m->number = rows[k].number;
        m->nrepl_auto = q.nrepl_auto;
        m->nlost_auto = kout[k].nskip;
        m->nap = q.nap;
        m->nrepl_aper = q.nrepl_aper;
        m->nlost_aper = q.nlost_aper;
        m->nrepl_win = q.nrepl_win;
        m->nlost_win = q.nlost_win;
        m->flux_aper = q.flux_aper;
        m->fluxerr_aper = q.fluxerr_aper;
        if ((int64_t)10 * ((int64_t)q.nrepl_auto + kout[k].nskip) > (int64_t)kout[k].npix + kout[k].nskip)
            out[k].flags_auto |= ZM_AUTO_CROWDED;
        const bool aper_crowded = (int64_t)10 * ((int64_t)q.nrepl_aper + q.nlost_aper) > (int64_t)q.nap;
        m->crowded = ((out[k].flags_auto & ZM_AUTO_CROWDED) || aper_crowded) ? 1 : 0;
    }
    return 0;
}

extern "C" int zm_extract_measure_masked(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                                         const int32_t* segm, int nx, int ny, const zm_wcs* wcs,
                                         const zm_measure_params* params, int n, const zm_object* rows,
                                         zm_object_ext* out, const zm_mask_params* mask, zm_object_mask* out_mask) {
    ZM_CHECK(ctx && img && sigma && segm, "zm_extract_measure_masked: null argument");
    ZM_CHECK(nx > 0 && ny > 0 && (int64_t)nx * ny <= (int64_t)1 << 30, "zm_extract_measure_masked: bad sizes %d x %d", nx, ny);
    ZM_TRY(mk_check_mask(mask));
    if (n == 0) return 0;
    float *d_img = nullptr, *d_sig = nullptr;
    uint8_t* d_bad = nullptr;
    int32_t* d_seg = nullptr;
    ZM_TRY(mx_stage(ctx, img, sigma, bad, segm, nx, ny, &d_img, &d_sig, &d_bad, &d_seg));
    return zm_extract_measure_masked_dev(ctx, d_img, d_sig, d_bad, d_seg, nx, ny, wcs, params, n, rows, out, mask, out_mask);
}
