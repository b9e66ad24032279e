// What the units of the extractor's second pass share: extract_measure.hip (k_ex_kron, k_ex_win) and extract_mask.hip
// (their masked forms and the masked aperture).  Row and result structs, the bad-pixel rule, the workgroup reduction, the
// isophotal error sums, and the two host steps around the kernels (rows -> mx_obj, kernel results -> zm_object_ext).
//
// Include it BELOW `#pragma clang fp contract(off)`: the per-pixel radii decide which pixels are summed and the
// restatements (tests/measure_ref.py, tests/mask_ref.py) evaluate the same expressions with one rounding per operation.
#pragma once
#include <climits>
#include <cmath>
#include <vector>

#include "zm_internal.h"

struct mx_obj {                      // what the kernels need of one row, prepared on the host
    double xc, yc;                   // isophotal barycentre, 0-based
    double cxx, cyy, cxy;            // ellipse coefficients of the isophotal moments
    double sx, sy;                   // sqrt(x2), sqrt(y2): half extents of the unit ellipse
    double sw, tw;                   // sigma_win, 2 sigma_win^2
    int sx0, sx1, sy0, sy1;          // search box of the Kron radius, clipped, half-open
    int ix0, ix1, iy0, iy1;          // the object's bounding box, clipped, half-open
    int number, valid;               // NUMBER; 0: the moments give no ellipse (nothing is summed)
};

struct mx_kout {
    double r1, radius, flux, var;    // first-moment radius, KRON_RADIUS, sum v, sum sigma^2
    double sumf, e[6];               // over the members, offsets (di, dj) from the box's corner: sum of the filtered
                                     // values; sum sigma^2 di^2, dj^2, di dj, di, dj, 1
    int npix, nskip;
};

struct mx_wout {
    double cx, cy;                   // final centre, 0-based
    double m[7];                     // tv, sum w v dx^2, dy^2, dx dy, sum w^2 sigma^2 dx^2, dy^2, dx dy
    int niter, flags;
};

#define MX_WIN_ITER 16
#define MX_WIN_STEP2 1e-8            // (1e-4 px)^2

__device__ __forceinline__ bool mx_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool mx_isbad(float v, float s, unsigned b) {
    return b != 0 || mx_nonfinite(v) || mx_nonfinite(s) || !(s > 0.f);
}
__device__ __forceinline__ bool mx_bad_at(const float* __restrict__ img, const float* __restrict__ sig,
                                          const uint8_t* __restrict__ bad, size_t p) {
    return mx_isbad(img[p], sig[p], bad ? bad[p] : 0u);
}

// a double clamped to [-1, n + 1] before it becomes an int (a double outside int's range has no defined conversion)
__device__ __forceinline__ int mx_int(double v, int n) { return (int)fmin(fmax(v, -1.0), n + 1.0); }

// the filtered value of k_ex_filter at (x, y): float32, taps in row-major order, bad and outside pixels enter as 0
__device__ __forceinline__ float mx_filtered(const float* __restrict__ img, const float* __restrict__ sig,
                                             const uint8_t* __restrict__ bad, int nx, int ny, int x, int y) {
    const float coef[3][3] = {{1.f, 2.f, 1.f}, {2.f, 4.f, 2.f}, {1.f, 2.f, 1.f}};
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int xx = x + d - 1, yy = y + r - 1;
            float v = 0.f;
            if (xx >= 0 && xx < nx && yy >= 0 && yy < ny) {
                const size_t p = (size_t)yy * nx + xx;
                if (!mx_bad_at(img, sig, bad, p)) v = img[p];
            }
            acc += coef[r][d] * v;
        }
    return acc * 0.0625f;
}

__device__ __forceinline__ double mx_wsum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int mx_wsumi(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the sums of all 256 lanes, on every thread: the waves' results are added in order by everyone from the same LDS words
template <int N>
__device__ __forceinline__ void mx_reduce(double (&s)[N], double (*sh)[N], int lane, int wave) {
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] = mx_wsum(s[q]);
    __syncthreads();                                     // the readers of the round before are done
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) sh[wave][q] = s[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] = ((sh[0][q] + sh[1][q]) + sh[2][q]) + sh[3][q];
}

// the isophotal error sums over the members of object o (walk 3 of the Kron kernels), per lane
// (offsets from the box's corner are small integers and sigma^2 of a float32 has 48 bits: like the barycentre's sums
// these are exact in any order for all but very large objects; the shift to the barycentre happens on the host)
__device__ __forceinline__ void mx_iso_sums(const float* __restrict__ img, const float* __restrict__ sig,
                                            const uint8_t* __restrict__ bad, const int* __restrict__ seg, int nx, int ny,
                                            const mx_obj& o, int use_filter, int tid, double (&m)[7]) {
    const int bw = o.ix1 - o.ix0, bh = o.iy1 - o.iy0;
    const int total = (bw > 0 && bh > 0) ? bw * bh : 0;
    for (int e = tid; e < total; e += 256) {
        const int j = o.iy0 + e / bw, i = o.ix0 + e % bw;
        const size_t p = (size_t)j * nx + i;
        if (seg[p] != o.number) continue;
        const double dx = i - o.ix0, dy = j - o.iy0;
        const double sg = sig[p], sg2 = sg * sg;
        const float fv = use_filter ? mx_filtered(img, sig, bad, nx, ny, i, j) : img[p];
        m[0] += (double)fv;
        m[1] += sg2 * dx * dx;
        m[2] += sg2 * dy * dy;
        m[3] += sg2 * dx * dy;
        m[4] += sg2 * dx;
        m[5] += sg2 * dy;
        m[6] += sg2;
    }
}

// ---- host (extract_measure.hip) -------------------------------------------------------------------------------------
// rows -> what the kernels take
void mx_prepare(const zm_object* rows, int n, int nx, int ny, std::vector<mx_obj>& objs);
// kernel results -> zm_object_ext rows (flags_auto from npix / nskip as they stand in kout), world columns with a WCS
int mx_finish(const zm_object* rows, int n, int nx, int ny, const zm_wcs* wcs, const std::vector<mx_obj>& objs,
              const std::vector<mx_kout>& kout, const std::vector<mx_wout>& wout, zm_object_ext* out);
// the argument checks of zm_extract_measure_dev, under the name `who`
int mx_check_args(const char* who, const zm_ctx* ctx, const float* img, const float* sigma, const int32_t* segm_dev,
                  int nx, int ny, const zm_measure_params* params, int n);
// host planes -> the context's staging planes
int mx_stage(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad, const int32_t* segm, int nx, int ny,
             float** d_img, float** d_sig, uint8_t** d_bad, int32_t** d_seg);
