// Fake sources on resident planes (DESIGN.md "Fake sources"): PSF-model point sources added to an image and its rms plane.
// This operator is the project's own; the reference left fake-source tests to offline work.
//
//   zm_inject_layers   host only: the layer of every fake, 1 + the largest layer among the EARLIER fakes whose box shares a
//                      pixel with its own (cell hashing, cells of one box width: a partner lies in the 3 x 3 cells around)
//   k_inject           one wave per fake of one layer: the model into LDS, the lanes stride over the box of
//                      (2 (half + 3) + 1)^2 pixels, read - add - write of img (and rms); the sum deposited and the flags
//                      by the xor-shuffle trees of psf_dev.h
//
// Within a layer no two boxes share a pixel, and of every overlapping pair the earlier index lies in an earlier layer: one
// launch per layer, in order on the context's stream, gives the result of adding the fakes one at a time in index order -
// without a float atomic, the same bytes on every run.
#include <algorithm>
#include <cmath>
#include <unordered_map>

#include "psf_dev.h"

#define INJ_MODEL_MAX ((2 * ZM_PSF_HALF_MAX + 1) * (2 * ZM_PSF_HALF_MAX + 1))
#define INJ_PAD 3                    // the box reaches half + INJ_PAD pixels from the centre pixel: the taps' reach
#define INJ_NMAX (1 << 24)

// P at the box offset (i, j): the six-by-six walk of psf_wave_fit in its order - rows outer, ty[a] * (sum_b tx[b] * m) -
// over the model samples (j + oy + a, i + ox + b), 0 outside the model's grid.  fp contract is off (psf_dev.h).
__device__ __forceinline__ double inj_profile(const double* sm, int mw, const double tx[6], const double ty[6], int i, int j,
                                              int ox, int oy) {
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
    return P;
}

// list[blockIdx.x]: the fake of this wave (the launch covers one layer's slice of the work list)
__global__ __launch_bounds__(64) void k_inject(float* __restrict__ img, float* __restrict__ rms,
                                               const int32_t* __restrict__ mask, int32_t bad_bits, int nx, int ny,
                                               const int32_t* __restrict__ list, int count, const double* __restrict__ xs,
                                               const double* __restrict__ ys, const double* __restrict__ fluxes,
                                               const double* __restrict__ model, int half, double gain, double core2,
                                               double* __restrict__ out_sum, int32_t* __restrict__ out_flags) {
    __shared__ double sm[INJ_MODEL_MAX];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= count) return;
    const int s = list[blockIdx.x];
    const int mw = 2 * half + 1;
    for (int e = lane; e < mw * mw; e += 64) sm[e] = model[e];
    __syncthreads();
    const double x = xs[s], y = ys[s], flux = fluxes[s];
    if (!(isfinite(x) && isfinite(y) && isfinite(flux))) {
        if (lane == 0) {
            if (out_sum) out_sum[s] = __builtin_nan("");
            out_flags[s] = ZM_INJ_BADPOS;
        }
        return;
    }
    const double ixd = floor(x + 0.5), iyd = floor(y + 0.5);
    const double fx = x - ixd, fy = y - iyd;
    // the model at (i - fx, j - fy): floor sample i + ox, fractional part dx, the same for every pixel of the box
    const double dx = fx > 0.0 ? 1.0 - fx : -fx, dy = fy > 0.0 ? 1.0 - fy : -fy;
    const int ox = (fx > 0.0 ? -1 : 0) + half - 2, oy = (fy > 0.0 ? -1 : 0) + half - 2;
    double tx[6], ty[6];
    psf_taps(dx, tx);
    psf_taps(dy, ty);
    const int m = half + INJ_PAD, bw = 2 * m + 1;
    double Psum = 0.0;
    int fl = 0, inside = 0;
    for (int e = lane; e < bw * bw; e += 64) {
        const int j = e / bw - m, i = e % bw - m;
        const double px = ixd + (double)i, py = iyd + (double)j;
        if (px < 0.0 || py < 0.0 || px >= (double)nx || py >= (double)ny) {
            fl |= ZM_INJ_CLIPPED;
            continue;
        }
        inside = 1;
        const size_t idx = (size_t)(int)py * nx + (int)px;
        if (mask) {
            const double ddx = (double)i - fx, ddy = (double)j - fy;
            if (ddx * ddx + ddy * ddy <= core2 && (mask[idx] & bad_bits)) fl |= ZM_INJ_BAD;
        }
        const double P = inj_profile(sm, mw, tx, ty, i, j, ox, oy);
        const double v = flux * P;
        if (v == 0.0) continue;
        const float old = img[idx];
        if (!isfinite(old)) fl |= ZM_INJ_NONFINITE;
        img[idx] = (float)((double)old + v);
        Psum += P;
        if (rms && gain > 0.0 && v > 0.0) {
            const float sg = rms[idx];
            if (isfinite(sg) && sg > 0.0f) rms[idx] = (float)sqrt((double)sg * (double)sg + v / gain);
        }
    }
    Psum = psf_wave_add(Psum);
    fl = psf_wave_or(fl);
    inside = psf_wave_or(inside);
    if (!inside) fl |= ZM_INJ_OUTSIDE;
    if (lane == 0) {
        if (out_sum) out_sum[s] = inside ? flux * Psum : 0.0;
        out_flags[s] = fl;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
namespace {
struct inj_cell_hash {
    size_t operator()(const std::pair<long long, long long>& c) const {
        return (size_t)((unsigned long long)c.first * 0x9E3779B97F4A7C15ull ^ ((unsigned long long)c.second + 0x7F4A7C15ull +
                                                                               ((unsigned long long)c.first << 6)));
    }
};

// the cell of a centre pixel; clamped far outside any frame (monotone, so neighbours stay neighbours: pairs are compared
// on the unclamped doubles)
long long inj_cell(double ipix, int cell) {
    const double c = std::floor(ipix / (double)cell), lim = 1125899906842624.0;      // 2^50
    return (long long)std::min(std::max(c, -lim), lim);
}
}   // namespace

extern "C" int zm_inject_layers(int n, const double* x, const double* y, int half, int32_t* out_layer, int* out_nlayers) {
    const char* who = "zm_inject_layers";
    ZM_CHECK(n >= 0, "%s: n %d is negative", who, n);
    ZM_CHECK(half >= 1 && half <= ZM_PSF_HALF_MAX, "%s: half %d outside 1 .. %d", who, half, ZM_PSF_HALF_MAX);
    ZM_CHECK(out_nlayers, "%s: null argument", who);
    *out_nlayers = 0;
    if (n == 0) return 0;
    ZM_CHECK(x && y && out_layer, "%s: null argument", who);
    const int sep = 2 * (half + INJ_PAD), cell = sep + 1;
    std::unordered_map<std::pair<long long, long long>, std::vector<int>, inj_cell_hash> cells;
    std::vector<double> ix(n), iy(n);
    int nl = 0;
    for (int k = 0; k < n; ++k) {
        if (!(std::isfinite(x[k]) && std::isfinite(y[k]))) {      // writes nothing: layer 0, a partner of nobody
            out_layer[k] = 0;
            continue;
        }
        ix[k] = std::floor(x[k] + 0.5);
        iy[k] = std::floor(y[k] + 0.5);
        const long long cx = inj_cell(ix[k], cell), cy = inj_cell(iy[k], cell);
        int top = 0;
        for (long long a = cy - 1; a <= cy + 1; ++a)
            for (long long b = cx - 1; b <= cx + 1; ++b) {
                auto it = cells.find({b, a});
                if (it == cells.end()) continue;
                for (int e : it->second)
                    if (std::fabs(ix[e] - ix[k]) <= (double)sep && std::fabs(iy[e] - iy[k]) <= (double)sep)
                        top = std::max(top, out_layer[e]);
            }
        out_layer[k] = top + 1;
        nl = std::max(nl, top + 1);
        cells[{cx, cy}].push_back(k);
    }
    *out_nlayers = nl;
    return 0;
}

static int inj_check(const char* who, zm_ctx* ctx, const float* img, int nx, int ny, int n, int half, double gain,
                     double core_radius) {
    ZM_CHECK(ctx && img, "%s: null argument", who);
    ZM_CHECK(nx > 0 && ny > 0 && n >= 0, "%s: bad sizes", who);
    ZM_CHECK(n <= INJ_NMAX, "%s: %d fakes, at most %d in one call", who, n, INJ_NMAX);
    ZM_CHECK(half >= 1 && half <= ZM_PSF_HALF_MAX, "%s: half %d outside 1 .. %d", who, half, ZM_PSF_HALF_MAX);
    ZM_CHECK(std::isfinite(gain) && gain >= 0.0, "%s: gain %g must be finite and not negative", who, gain);
    ZM_CHECK(std::isfinite(core_radius) && core_radius >= 0.0, "%s: core radius %g must be finite and not negative", who,
             core_radius);
    return 0;
}

extern "C" int zm_inject_dev(zm_ctx* ctx, float* img, float* rms, const int32_t* mask, int32_t bad_bits, int nx, int ny,
                             int n, const double* x, const double* y, const double* flux, const double* model, int half,
                             double gain, double core_radius, double* out_sum, int32_t* out_flags) {
    const char* who = "zm_inject_dev";
    ZM_TRY(inj_check(who, ctx, img, nx, ny, n, half, gain, core_radius));
    if (n == 0) return 0;
    ZM_CHECK(x && y && flux && model && out_flags, "%s: null argument", who);
    std::vector<int32_t> layer(n);
    int nl = 0;
    ZM_TRY(zm_inject_layers(n, x, y, half, layer.data(), &nl));
    // the work list: the fakes of layer 0 (no finite position: flags only), 1, 2, ... each in index order
    std::vector<int> start(nl + 2, 0);
    for (int k = 0; k < n; ++k) ++start[layer[k] + 1];
    for (int l = 0; l <= nl; ++l) start[l + 1] += start[l];
    ZM_HIP(hipSetDevice(ctx->device));
    // one staging buffer {x, y, flux, list}: pinned, guarded by an event so that a later call cannot overwrite a copy still
    // in flight (as zm_stamps_dev stages its origins)
    const size_t ns = (size_t)n, total = sizeof(double) * 3 * ns + sizeof(int32_t) * ns;
    hipEvent_t* ev = nullptr;
    ZM_TRY(zm_get_sync_events(ctx, 13, &ev));
    ZM_HIP(hipEventSynchronize(ev[12]));
    char *pin = nullptr, *dev = nullptr;
    ZM_TRY(ctx->get_pinned("inject_args_h", total, (void**)&pin));
    ZM_TRY(ctx->get("inject_args", total, (void**)&dev));
    double* hx = reinterpret_cast<double*>(pin);
    int32_t* hl = reinterpret_cast<int32_t*>(pin + sizeof(double) * 3 * ns);
    memcpy(hx, x, sizeof(double) * ns);
    memcpy(hx + ns, y, sizeof(double) * ns);
    memcpy(hx + 2 * ns, flux, sizeof(double) * ns);
    {
        std::vector<int> at(start.begin(), start.end() - 1);
        for (int k = 0; k < n; ++k) hl[at[layer[k]]++] = k;
    }
    ZM_HIP(hipMemcpyAsync(dev, pin, total, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipEventRecord(ev[12], ctx->stream));
    const double *d_x = reinterpret_cast<const double*>(dev), *d_y = d_x + ns, *d_f = d_x + 2 * ns;
    const int32_t* d_list = reinterpret_cast<const int32_t*>(dev + sizeof(double) * 3 * ns);
    zm_scope_timer t(ctx, "inject");
    for (int l = 0; l <= nl; ++l) {
        const int count = start[l + 1] - start[l];
        if (count == 0) continue;
        hipLaunchKernelGGL(k_inject, dim3((unsigned)count), dim3(64), 0, ctx->stream, img, rms, mask, bad_bits, nx, ny,
                           d_list + start[l], count, d_x, d_y, d_f, model, half, gain, core_radius * core_radius, out_sum,
                           out_flags);
        ZM_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int zm_inject(zm_ctx* ctx, float* img, float* rms, const int32_t* mask, int32_t bad_bits, int nx, int ny, int n,
                         const double* x, const double* y, const double* flux, const double* model, int half, double gain,
                         double core_radius, double* out_sum, int32_t* out_flags) {
    const char* who = "zm_inject";
    ZM_TRY(inj_check(who, ctx, img, nx, ny, n, half, gain, core_radius));
    if (n == 0) return 0;
    ZM_CHECK(x && y && flux && model && out_flags, "%s: null argument", who);
    ZM_HIP(hipSetDevice(ctx->device));
    // the planes as zm_psf_photometry stages them
    const size_t np = (size_t)nx * ny, ne = (size_t)(2 * half + 1) * (2 * half + 1), ns = (size_t)n;
    float *d_img = nullptr, *d_rms = nullptr;
    int32_t* d_mask = nullptr;
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
    // the model and the sums as doubles, then the flags
    double* d = nullptr;
    ZM_TRY(ctx->get("h_inject_io", sizeof(double) * (ne + ns) + sizeof(int32_t) * ns, (void**)&d));
    double *d_model = d, *d_sum = d + ne;
    int32_t* d_fl = reinterpret_cast<int32_t*>(d_sum + ns);
    ZM_HIP(hipMemcpyAsync(d_model, model, sizeof(double) * ne, hipMemcpyHostToDevice, ctx->stream));
    ZM_TRY(zm_inject_dev(ctx, d_img, d_rms, d_mask, bad_bits, nx, ny, n, x, y, flux, d_model, half, gain, core_radius, d_sum,
                         d_fl));
    ZM_HIP(hipMemcpyAsync(img, d_img, np * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (rms) ZM_HIP(hipMemcpyAsync(rms, d_rms, np * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_sum) ZM_HIP(hipMemcpyAsync(out_sum, d_sum, sizeof(double) * ns, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(out_flags, d_fl, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
