// FITS data blocks <-> native planes on the device: the byte swap and BSCALE / BZERO
// arithmetic that astropy / fitsio do on the host in the reference's
// FITSFile.load_data / save (zuds/fitsfile.py:69-94,146-206).  The raw big-endian data
// block of a primary HDU goes over PCIe as it lies on disk (pinned staging, async copy);
// decoding to the float32 / int32 / uint8 planes the kernels take, and encoding the
// products back, are streaming kernels (HBM bound, one pass).
#include "zm_internal.h"

__device__ inline uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
__device__ inline uint16_t bswap16(uint16_t v) { return (uint16_t)((v << 8) | (v >> 8)); }

// The contract is written above zm_fits_decode_dev in include/zudsmi.h; tests/fits_ref.py restates it.

// physical = fl(fl(bscale * stored) + bzero): two roundings, as the host reader's numpy expression.  A fused
// multiply-add would round once and differ from it (BSCALE 0.1, BZERO -3: stored 30 gives 0 here, 1.7e-16 fused).
__device__ inline double fits_scale(double v, double bscale, double bzero) {
#pragma clang fp contract(off)
    const double t = bscale * v;
    return t + bzero;
}

// Integer planes saturate at the ends of their type, from an integer and from a real value alike; NaN gives 0.
__device__ inline void fits_store_int(void* __restrict__ out, int64_t p, int out_kind, int64_t s) {
    if (out_kind == 1) reinterpret_cast<int32_t*>(out)[p] = (int32_t)(s < INT32_MIN ? INT32_MIN : (s > INT32_MAX ? INT32_MAX : s));
    else if (out_kind == 3) reinterpret_cast<int16_t*>(out)[p] = (int16_t)(s < INT16_MIN ? INT16_MIN : (s > INT16_MAX ? INT16_MAX : s));
    else reinterpret_cast<uint8_t*>(out)[p] = (uint8_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

__device__ inline void fits_store_real(void* __restrict__ out, int64_t p, int out_kind, double v) {
    const double lo = out_kind == 1 ? -2147483648.0 : (out_kind == 3 ? -32768.0 : 0.0);
    const double hi = out_kind == 1 ? 2147483647.0 : (out_kind == 3 ? 32767.0 : 255.0);
    int32_t r = 0;                                   // NaN
    if (v <= lo) r = (int32_t)lo;
    else if (v >= hi) r = (int32_t)hi;
    else if (v == v) r = (int32_t)v;                 // in range: the cast truncates toward zero
    if (out_kind == 1) reinterpret_cast<int32_t*>(out)[p] = r;
    else if (out_kind == 3) reinterpret_cast<int16_t*>(out)[p] = (int16_t)r;
    else reinterpret_cast<uint8_t*>(out)[p] = (uint8_t)r;
}

// BITPIX: 8, 16, 32, 64, -32, -64.  out_kind: 0 float32, 1 int32, 2 uint8, 3 int16 (a BITPIX 16 mask kept at 16 bits).
__global__ __launch_bounds__(256) void k_fits_decode(const uint8_t* __restrict__ raw, int bitpix,
                                                     double bscale, double bzero, int64_t n,
                                                     int out_kind, void* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const bool scaled = (bscale != 1.0) || (bzero != 0.0);
    double v;
    int64_t iv = 0;
    bool is_int = true;
    switch (bitpix) {
        case 8: iv = raw[p]; break;
        case 16: iv = (int16_t)bswap16(reinterpret_cast<const uint16_t*>(raw)[p]); break;
        case 32: iv = (int32_t)bswap32(reinterpret_cast<const uint32_t*>(raw)[p]); break;
        case 64: {
            const uint32_t hi = bswap32(reinterpret_cast<const uint32_t*>(raw)[2 * p]);
            const uint32_t lo = bswap32(reinterpret_cast<const uint32_t*>(raw)[2 * p + 1]);
            iv = (int64_t)(((uint64_t)hi << 32) | lo);
            break;
        }
        case -32: {
            is_int = false;
            const uint32_t bits = bswap32(reinterpret_cast<const uint32_t*>(raw)[p]);
            if (out_kind == 0 && !scaled) {          // the bits of the file: NaN payloads, -0.0 and subnormals as they are
                reinterpret_cast<uint32_t*>(out)[p] = bits;
                return;
            }
            v = (double)__uint_as_float(bits);
            break;
        }
        default: {   // -64
            is_int = false;
            const uint32_t hi = bswap32(reinterpret_cast<const uint32_t*>(raw)[2 * p]);
            const uint32_t lo = bswap32(reinterpret_cast<const uint32_t*>(raw)[2 * p + 1]);
            v = __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
            break;
        }
    }
    if (is_int) {
        if (out_kind != 0 && bscale == 1.0 && bzero == floor(bzero) && fabs(bzero) <= 0x1p63) {
            // exact integers: stored + BZERO (the unsigned 16 / 32 / 64 bit and signed-byte conventions), saturating
            int64_t s;
            if (bzero == 0x1p63) {                   // stored + 2^63 lies in 0 .. 2^64 - 1
                const uint64_t u = (uint64_t)iv ^ 0x8000000000000000ull;
                s = u > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)u;
            } else {
                const int64_t bz = (int64_t)bzero;
                if (__builtin_add_overflow(iv, bz, &s)) s = bz < 0 ? INT64_MIN : INT64_MAX;
            }
            fits_store_int(out, p, out_kind, s);
            return;
        }
        if (out_kind == 0 && !scaled) {              // one rounding, integer -> float32, never through fp64
            reinterpret_cast<float*>(out)[p] = bitpix == 64 ? (float)iv : (float)(int32_t)iv;
            return;
        }
        v = (double)iv;
    }
    if (scaled) v = fits_scale(v, bscale, bzero);
    if (out_kind == 0) reinterpret_cast<float*>(out)[p] = (float)v;
    else fits_store_real(out, p, out_kind, v);
}

// in_kind: 0 float32 -> BITPIX -32, 1 int32 -> BITPIX 32, 2 uint8 -> BITPIX 8,
// 3 int32 -> BITPIX 16 (values must fit)
__global__ __launch_bounds__(256) void k_fits_encode(const void* __restrict__ in, int in_kind,
                                                     int64_t n, uint8_t* __restrict__ raw) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    switch (in_kind) {
        case 0: reinterpret_cast<uint32_t*>(raw)[p] = bswap32(__float_as_uint(reinterpret_cast<const float*>(in)[p])); break;
        case 1: reinterpret_cast<uint32_t*>(raw)[p] = bswap32((uint32_t)reinterpret_cast<const int32_t*>(in)[p]); break;
        case 2: raw[p] = reinterpret_cast<const uint8_t*>(in)[p]; break;
        default: reinterpret_cast<uint16_t*>(raw)[p] = bswap16((uint16_t)(int16_t)reinterpret_cast<const int32_t*>(in)[p]); break;
    }
}

extern "C" int zm_fits_decode_dev(zm_ctx* ctx, const void* raw_dev, int bitpix, double bscale,
                                  double bzero, int64_t n, int out_kind, void* out_dev) {
    ZM_CHECK(ctx && raw_dev && out_dev && n > 0, "zm_fits_decode_dev: bad argument");
    ZM_CHECK(bitpix == 8 || bitpix == 16 || bitpix == 32 || bitpix == 64 || bitpix == -32 || bitpix == -64,
             "zm_fits_decode_dev: unsupported BITPIX %d", bitpix);
    ZM_CHECK(out_kind >= 0 && out_kind <= 3, "zm_fits_decode_dev: unknown output kind %d", out_kind);
    ZM_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_fits_decode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const uint8_t*)raw_dev, bitpix, bscale, bzero, n, out_kind, out_dev);
    ZM_HIP(hipGetLastError());
    return 0;
}

extern "C" int zm_fits_encode_dev(zm_ctx* ctx, const void* in_dev, int in_kind, int64_t n,
                                  void* raw_dev) {
    ZM_CHECK(ctx && in_dev && raw_dev && n > 0, "zm_fits_encode_dev: bad argument");
    ZM_CHECK(in_kind >= 0 && in_kind <= 3, "zm_fits_encode_dev: unknown input kind %d", in_kind);
    ZM_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_fits_encode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       in_dev, in_kind, n, (uint8_t*)raw_dev);
    ZM_HIP(hipGetLastError());
    return 0;
}
