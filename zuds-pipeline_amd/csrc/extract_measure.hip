// The second, opt-in measurement pass behind the source extractor: the Kron (*_AUTO) and windowed (*WIN*) columns of
// zuds/astromatic/sextractor.param and the isophotal position errors behind ERR*_WORLD.  The arithmetic is a chosen
// convention, stated in DESIGN.md ("Source extraction", "The wide table") and restated in numpy in tests/measure_ref.py.
//
//   k_ex_kron   one workgroup per object: the sums of the first-moment radius over the clipped search box, the radius
//               (every thread, from the same reduced values), the flux sums over the clipped box of the Kron ellipse,
//               then the isophotal error sums over the object's own bounding box
//   k_ex_win    one workgroup per object: at most 16 centring passes and one moment pass over the clipped box of the
//               window's circle; after every pass the reduced sums go through LDS to every thread, which all take the
//               same decision
// Summation as in k_ex_measure: element e of a row-major box belongs to lane e % 256, float64 partial sums per lane,
// xor shuffles inside a wave, waves 0..3 added in order: no float atomics, the same bits on every run.  Every box is
// clipped to the frame, so an object costs at most 3 (Kron) or 17 (window) walks over the frame.
#include "aperture_dev.h"

// one rounding per operation in everything below (the per-pixel radii decide which pixels are summed: the restatement
// evaluates the same expressions); aperture_dev.h above keeps the contraction k_aperture compiles it with
#pragma clang fp contract(off)

#include "measure_dev.h"             // structs, bad-pixel rule, reduction, error sums: shared with extract_mask.hip

__global__ __launch_bounds__(256) void k_ex_kron(const float* __restrict__ img, const float* __restrict__ sig,
                                                 const uint8_t* __restrict__ bad, const int* __restrict__ seg, int nx,
                                                 int ny, const mx_obj* __restrict__ obj, int nobj, double kfact,
                                                 double kmin, int use_filter, mx_kout* __restrict__ out) {
    __shared__ double sh2[4][2], sh7[4][7];
    __shared__ int shi[4][2];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (k >= nobj) return;
    const mx_obj o = obj[k];
    // ---- walk 1: s0 = sum v, s1 = sum sqrt(r2) v over r2 <= 36 -------------------------------------------------
    double s[2] = {0.0, 0.0};
    {
        const int bw = o.sx1 - o.sx0, bh = o.sy1 - o.sy0;
        const int total = (o.valid && bw > 0 && bh > 0) ? bw * bh : 0;
        for (int e = tid; e < total; e += 256) {
            const int j = o.sy0 + e / bw, i = o.sx0 + e % bw;
            const size_t p = (size_t)j * nx + i;
            const double dx = i - o.xc, dy = j - o.yc;
            const double r2 = o.cxx * dx * dx + o.cyy * dy * dy + o.cxy * dx * dy;
            if (!(r2 <= 36.0) || mx_bad_at(img, sig, bad, p)) continue;
            const double v = img[p];
            s[0] += v;
            s[1] += sqrt(fmax(r2, 0.0)) * v;
        }
    }
    mx_reduce<2>(s, sh2, lane, wave);
    const double r1 = (s[0] > 0.0 && s[1] > 0.0) ? s[1] / s[0] : 0.0;
    const double R = fmax(kfact * r1, kmin), R2 = R * R;
    // ---- walk 2: the flux sums over r2 <= R^2 -------------------------------------------------------------------
    double f[2] = {0.0, 0.0};
    int np = 0, ns = 0;
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
            if (mx_bad_at(img, sig, bad, p)) { ++ns; continue; }
            const double sg = sig[p];
            f[0] += (double)img[p];
            f[1] += sg * sg;
            ++np;
        }
    }
    mx_reduce<2>(f, sh2, lane, wave);
    np = mx_wsumi(np);
    ns = mx_wsumi(ns);
    if (lane == 0) { shi[wave][0] = np; shi[wave][1] = ns; }
    // ---- walk 3: the isophotal error sums over the members -----------------------------------------------------
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
    }
}

// one pass over the clipped box of the circle of radius r about (cx, cy): w = frac * exp(-r^2 / tw) per good pixel.
// FINAL = false: s = {tv, sum w v dx, sum w v dy}; FINAL = true: the seven sums of mx_wout::m
template <bool FINAL, int N>
__device__ __forceinline__ void mx_win_pass(const float* __restrict__ img, const float* __restrict__ sig,
                                            const uint8_t* __restrict__ bad, int nx, int ny, double cx, double cy,
                                            double r, double tw, int tid, double (&s)[N]) {
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] = 0.0;
    const int i0 = max(mx_int(floor(cx - r + 0.5), nx), 0), i1 = min(mx_int(ceil(cx + r + 0.5), nx), nx);
    const int j0 = max(mx_int(floor(cy - r + 0.5), ny), 0), j1 = min(mx_int(ceil(cy + r + 0.5), ny), ny);
    const int bw = i1 - i0, bh = j1 - j0;
    const int total = (bw > 0 && bh > 0) ? bw * bh : 0;
    for (int e = tid; e < total; e += 256) {
        const int j = j0 + e / bw, i = i0 + e % bw;
        const size_t p = (size_t)j * nx + i;
        if (mx_bad_at(img, sig, bad, p)) continue;
        const double dx = i - cx, dy = j - cy;
        const double x0 = i - 0.5 - cx, x1 = i + 0.5 - cx, y0 = j - 0.5 - cy, y1 = j + 0.5 - cy;
        const double frac = ap_signed(x1, y1, r) - ap_signed(x0, y1, r) - ap_signed(x1, y0, r) + ap_signed(x0, y0, r);
        const double w = frac * exp(-((dx * dx + dy * dy) / tw));
        const double v = img[p], wv = w * v;
        s[0] += wv;
        if (!FINAL) {
            s[1] += wv * dx;
            s[2] += wv * dy;
        } else {
            const double sg = sig[p], ws = w * w * (sg * sg);
            s[1] += wv * dx * dx;
            s[2] += wv * dy * dy;
            s[3] += wv * dx * dy;
            s[4] += ws * dx * dx;
            s[5] += ws * dy * dy;
            s[6] += ws * dx * dy;
        }
    }
}

__global__ __launch_bounds__(256) void k_ex_win(const float* __restrict__ img, const float* __restrict__ sig,
                                                const uint8_t* __restrict__ bad, int nx, int ny,
                                                const mx_obj* __restrict__ obj, int nobj, mx_wout* __restrict__ out) {
    __shared__ double sh3[4][3], sh7[4][7];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (k >= nobj) return;
    const mx_obj o = obj[k];
    double cx = o.xc, cy = o.yc;
    const double r = 4.0 * o.sw;
    const bool usable = o.sw > 0.0 && r < 1e9;           // false for NaN as well
    int niter = 0, flags = usable ? 0 : 1;
    bool converged = false;
    // every thread holds the same reduced sums after mx_reduce, so every branch below is uniform over the workgroup
    for (int it = 0; it < MX_WIN_ITER && flags == 0 && !converged; ++it) {
        double s[3];
        mx_win_pass<false>(img, sig, bad, nx, ny, cx, cy, r, o.tw, tid, s);
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
    if (!(flags & 1)) {
        mx_win_pass<true>(img, sig, bad, nx, ny, cx, cy, r, o.tw, tid, m);
        mx_reduce<7>(m, sh7, lane, wave);
        if (!(m[0] > 0.0)) flags |= 1;
    }
    if (tid == 0) {
        mx_wout w;
        w.cx = cx; w.cy = cy;
#pragma unroll
        for (int q = 0; q < 7; ++q) w.m[q] = m[q];
        w.niter = niter; w.flags = flags;
        out[k] = w;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------
extern "C" void zm_measure_params_default(zm_measure_params* p) {
    if (!p) return;
    p->kron_fact = 2.5;
    p->kron_min_radius = 3.5;
    p->filter = 1;
    p->pad_ = 0;
}

// A, B, THETA of second moments as ex_finish_row takes them (the 1/12 rule included when `thin` is set)
static void mx_ellipse(double x2, double y2, double xy, bool thin, double* a, double* b, double* theta) {
    if (thin && x2 * y2 - xy * xy < 0.00694) { x2 += 1.0 / 12.0; y2 += 1.0 / 12.0; }
    const double pm = 0.5 * (x2 + y2), dm = 0.5 * (x2 - y2);
    const double rt = sqrt(dm * dm + xy * xy);
    *a = sqrt(pm + rt);
    *b = sqrt(fmax(pm - rt, 0.0));
    *theta = 0.5 * atan2(2.0 * xy, x2 - y2) * (180.0 / M_PI);
}

static int mx_clip(double v, int n) {                    // v rounded down into [0, n]
    if (!(v > 0.0)) return 0;
    if (v >= (double)n) return n;
    return (int)v;
}

int mx_check_args(const char* who, const zm_ctx* ctx, const float* img, const float* sigma, const int32_t* segm_dev,
                  int nx, int ny, const zm_measure_params* params, int n) {
    ZM_CHECK(ctx && img && sigma && segm_dev && params, "%s: null argument", who);
    ZM_CHECK(nx > 0 && ny > 0 && (int64_t)nx * ny <= (int64_t)1 << 30, "%s: bad sizes %d x %d", who, nx, ny);
    ZM_CHECK(n >= 0 && n <= (1 << 24), "%s: bad row count %d", who, n);
    ZM_CHECK(params->kron_fact > 0 && params->kron_min_radius > 0 && params->kron_fact < 1e6 &&
                 params->kron_min_radius < 1e6 && (params->filter == 0 || params->filter == 1),
             "%s: bad parameters (PHOT_AUTOPARAMS %g, %g; filter %d)", who, params->kron_fact,
             params->kron_min_radius, params->filter);
    return 0;
}

void mx_prepare(const zm_object* rows, int n, int nx, int ny, std::vector<mx_obj>& objs) {
    objs.resize(n);
    for (int k = 0; k < n; ++k) {
        const zm_object& r = rows[k];
        mx_obj& o = objs[k];
        memset(&o, 0, sizeof(o));
        o.xc = r.x_image - 1.0;
        o.yc = r.y_image - 1.0;
        const double D = r.x2 * r.y2 - r.xy * r.xy;
        o.valid = std::isfinite(o.xc) && std::isfinite(o.yc) && std::isfinite(D) && D > 0.0 && r.x2 > 0.0 && r.y2 > 0.0;
        if (o.valid) {
            o.cxx = r.y2 / D;
            o.cyy = r.x2 / D;
            o.cxy = -2.0 * r.xy / D;
            o.sx = sqrt(r.x2);
            o.sy = sqrt(r.y2);
            o.sx0 = mx_clip(floor(o.xc - 6.0 * o.sx), nx);
            o.sx1 = mx_clip(ceil(o.xc + 6.0 * o.sx) + 1.0, nx);
            o.sy0 = mx_clip(floor(o.yc - 6.0 * o.sy), ny);
            o.sy1 = mx_clip(ceil(o.yc + 6.0 * o.sy) + 1.0, ny);
        } else {
            o.xc = o.yc = 0.0;
        }
        o.sw = r.fwhm_image > 0.0 ? r.fwhm_image / 2.35482 : sqrt((r.x2 + r.y2) / 2.0);
        if (!o.valid) o.sw = 0.0;
        o.tw = 2.0 * o.sw * o.sw;
        // the bounding box comes from the caller: nothing outside the frame is ever read
        o.ix0 = mx_clip((double)r.xmin - 1.0, nx);
        o.ix1 = mx_clip((double)r.xmax, nx);
        o.iy0 = mx_clip((double)r.ymin - 1.0, ny);
        o.iy1 = mx_clip((double)r.ymax, ny);
        o.number = r.number;
    }
}

extern "C" int zm_extract_measure_dev(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                                      const int32_t* segm_dev, int nx, int ny, const zm_wcs* wcs,
                                      const zm_measure_params* params, int n, const zm_object* rows,
                                      zm_object_ext* out) {
    ZM_TRY(mx_check_args("zm_extract_measure", ctx, img, sigma, segm_dev, nx, ny, params, n));
    if (n == 0) return 0;
    ZM_CHECK(rows && out, "zm_extract_measure: %d rows need a row array and an output array", n);
    ZM_HIP(hipSetDevice(ctx->device));
    std::vector<mx_obj> objs;
    mx_prepare(rows, n, nx, ny, objs);
    char* d = nullptr;
    const size_t b_obj = ((size_t)n * sizeof(mx_obj) + 15) & ~(size_t)15, b_k = ((size_t)n * sizeof(mx_kout) + 15) & ~(size_t)15;
    ZM_TRY(ctx->get("mx_buf", b_obj + b_k + (size_t)n * sizeof(mx_wout), (void**)&d));
    mx_obj* d_obj = (mx_obj*)d;
    mx_kout* d_k = (mx_kout*)(d + b_obj);
    mx_wout* d_w = (mx_wout*)(d + b_obj + b_k);
    ZM_HIP(hipMemcpyAsync(d_obj, objs.data(), (size_t)n * sizeof(mx_obj), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_ex_kron, dim3(n), dim3(256), 0, ctx->stream, img, sigma, bad, segm_dev, nx, ny, d_obj, n,
                       params->kron_fact, params->kron_min_radius, params->filter, d_k);
    hipLaunchKernelGGL(k_ex_win, dim3(n), dim3(256), 0, ctx->stream, img, sigma, bad, nx, ny, d_obj, n, d_w);
    ZM_HIP(hipGetLastError());
    std::vector<mx_kout> kout(n);
    std::vector<mx_wout> wout(n);
    ZM_HIP(hipMemcpyAsync(kout.data(), d_k, (size_t)n * sizeof(mx_kout), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(wout.data(), d_w, (size_t)n * sizeof(mx_wout), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return mx_finish(rows, n, nx, ny, wcs, objs, kout, wout, out);
}

int mx_finish(const zm_object* rows, int n, int nx, int ny, const zm_wcs* wcs, const std::vector<mx_obj>& objs,
              const std::vector<mx_kout>& kout, const std::vector<mx_wout>& wout, zm_object_ext* out) {
    for (int k = 0; k < n; ++k) {
        const zm_object& r = rows[k];
        const mx_obj& o = objs[k];
        const mx_kout& q = kout[k];
        const mx_wout& w = wout[k];
        zm_object_ext* x = out + k;
        memset(x, 0, sizeof(*x));
        x->number = r.number;
        // Kron
        x->kron_radius = q.radius;
        x->flux_auto = q.flux;
        x->fluxerr_auto = sqrt(q.var);
        x->npix_auto = q.npix;
        x->nskip_auto = q.nskip;
        if (q.flux > 0.0) {
            x->mag_auto = -2.5 * log10(q.flux);
            x->magerr_auto = 1.0857362 * x->fluxerr_auto / q.flux;
        } else {
            x->mag_auto = x->magerr_auto = 99.0;
        }
        int fa = 0;
        if ((int64_t)10 * q.nskip > (int64_t)q.npix + q.nskip) fa |= 1;
        const double hx = q.radius * o.sx, hy = q.radius * o.sy;
        if (!o.valid || o.xc - hx < -0.5 || o.xc + hx > nx - 0.5 || o.yc - hy < -0.5 || o.yc + hy > ny - 0.5) fa |= 2;
        if (q.r1 == 0.0) fa |= 4;
        x->flags_auto = fa;
        // isophotal position errors
        const double S2 = q.sumf * q.sumf, xb = o.xc - o.ix0, yb = o.yc - o.iy0;
        x->errx2 = (q.e[0] - 2.0 * xb * q.e[3] + xb * xb * q.e[5]) / S2;
        x->erry2 = (q.e[1] - 2.0 * yb * q.e[4] + yb * yb * q.e[5]) / S2;
        x->errxy = (q.e[2] - xb * q.e[4] - yb * q.e[3] + xb * yb * q.e[5]) / S2;
        // window
        x->sigma_win = o.sw;
        x->niter_win = w.niter;
        x->flags_win = w.flags;
        if (w.flags & 1) {
            x->xwin_image = r.x_image;
            x->ywin_image = r.y_image;
            x->x2win = r.x2; x->y2win = r.y2; x->xywin = r.xy;
            x->errx2win = x->errx2; x->erry2win = x->erry2; x->errxywin = x->errxy;
            x->awin_image = r.a_image;
            x->bwin_image = r.b_image;
            x->thetawin_image = r.theta_image;
        } else {
            const double tv = w.m[0];
            x->xwin_image = w.cx + 1.0;
            x->ywin_image = w.cy + 1.0;
            x->x2win = 2.0 * w.m[1] / tv;
            x->y2win = 2.0 * w.m[2] / tv;
            x->xywin = 2.0 * w.m[3] / tv;
            x->errx2win = 4.0 * w.m[4] / (tv * tv);
            x->erry2win = 4.0 * w.m[5] / (tv * tv);
            x->errxywin = 4.0 * w.m[6] / (tv * tv);
            mx_ellipse(x->x2win, x->y2win, x->xywin, true, &x->awin_image, &x->bwin_image, &x->thetawin_image);
        }
        mx_ellipse(x->errx2win, x->erry2win, x->errxywin, true, &x->errawin_image, &x->errbwin_image,
                   &x->errthetawin_image);
        x->xwin_world = x->ywin_world = x->erra_world = x->errb_world = x->errtheta_world = NAN;
    }
    if (wcs) {
        // five positions per row: the window's, and the barycentre +- 0.5 px along either axis
        std::vector<double> p((size_t)n * 20);
        double *px = p.data(), *py = px + 5 * (size_t)n, *ra = py + 5 * (size_t)n, *de = ra + 5 * (size_t)n;
        for (int k = 0; k < n; ++k) {
            const double xb = rows[k].x_image, yb = rows[k].y_image;
            double* X = px + 5 * (size_t)k;
            double* Y = py + 5 * (size_t)k;
            X[0] = out[k].xwin_image; Y[0] = out[k].ywin_image;
            X[1] = xb + 0.5; Y[1] = yb;
            X[2] = xb - 0.5; Y[2] = yb;
            X[3] = xb; Y[3] = yb + 0.5;
            X[4] = xb; Y[4] = yb - 0.5;
        }
        ZM_TRY(zm_wcs_pix2sky(wcs, 5 * n, px, py, ra, de));
        for (int k = 0; k < n; ++k) {
            zm_object_ext* x = out + k;
            const double* A = ra + 5 * (size_t)k;
            const double* Dd = de + 5 * (size_t)k;
            x->xwin_world = A[0];
            x->ywin_world = Dd[0];
            auto wrap = [](double d) { return d > 180.0 ? d - 360.0 : (d < -180.0 ? d + 360.0 : d); };
            const double cd = cos(0.5 * (Dd[1] + Dd[2]) * (M_PI / 180.0));
            const double j00 = wrap(A[1] - A[2]) * cd, j01 = wrap(A[3] - A[4]) * cd;      // d(ra cos dec) / dx, / dy
            const double j10 = Dd[1] - Dd[2], j11 = Dd[3] - Dd[4];                        // d dec / dx, / dy
            const double c00 = x->errx2, c11 = x->erry2, c01 = x->errxy;
            const double w00 = j00 * (j00 * c00 + j01 * c01) + j01 * (j00 * c01 + j01 * c11);
            const double w11 = j10 * (j10 * c00 + j11 * c01) + j11 * (j10 * c01 + j11 * c11);
            const double w01 = j10 * (j00 * c00 + j01 * c01) + j11 * (j00 * c01 + j01 * c11);
            mx_ellipse(w00, w11, w01, false, &x->erra_world, &x->errb_world, &x->errtheta_world);
        }
    }
    return 0;
}

int mx_stage(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad, const int32_t* segm, int nx, int ny,
             float** d_img, float** d_sig, uint8_t** d_bad, int32_t** d_seg) {
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t np = (size_t)nx * ny;
    *d_bad = nullptr;
    ZM_TRY(ctx->get("h_img", np * 4, (void**)d_img));
    ZM_TRY(ctx->get("h_wgt", np * 4, (void**)d_sig));
    ZM_TRY(ctx->get("ex_seg", np * 4, (void**)d_seg));
    ZM_HIP(hipMemcpyAsync(*d_img, img, np * 4, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(*d_sig, sigma, np * 4, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(*d_seg, segm, np * 4, hipMemcpyHostToDevice, ctx->stream));
    if (bad) {
        ZM_TRY(ctx->get("h_bpm", np, (void**)d_bad));
        ZM_HIP(hipMemcpyAsync(*d_bad, bad, np, hipMemcpyHostToDevice, ctx->stream));
    }
    return 0;
}

extern "C" int zm_extract_measure(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                                  const int32_t* segm, int nx, int ny, const zm_wcs* wcs,
                                  const zm_measure_params* params, int n, const zm_object* rows, zm_object_ext* out) {
    ZM_CHECK(ctx && img && sigma && segm, "zm_extract_measure: null argument");
    ZM_CHECK(nx > 0 && ny > 0 && (int64_t)nx * ny <= (int64_t)1 << 30, "zm_extract_measure: bad sizes %d x %d", nx, ny);
    if (n == 0) return 0;
    float *d_img = nullptr, *d_sig = nullptr;
    uint8_t* d_bad = nullptr;
    int32_t* d_seg = nullptr;
    ZM_TRY(mx_stage(ctx, img, sigma, bad, segm, nx, ny, &d_img, &d_sig, &d_bad, &d_seg));
    return zm_extract_measure_dev(ctx, d_img, d_sig, d_bad, d_seg, nx, ny, wcs, params, n, rows, out);
}
