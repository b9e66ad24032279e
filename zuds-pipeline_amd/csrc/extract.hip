// Source extraction on resident planes: the detection catalog and the segmentation map that the reference gets
// from SExtractor (PipelineFITSCatalog.from_image, zuds/catalog.py:96-130; settings of
// zuds/astromatic/sextractor.conf, sextractor.param, default.conv).  The arithmetic is a chosen convention, stated in
// DESIGN.md ("Source extraction") and restated in numpy in tests/extract_ref.py.
//
// Phases, each a launch of its own on the context's stream (no workgroup ever waits for another one):
//   k_ex_filter    3 x 3 filter + threshold, four pixels per lane; writes the filtered plane, the initial labels
//                  (own index / -1), a zeroed counter plane and the bad-pixel plane as int32
//   k_ex_local     union-find inside a 32 x 8 tile in LDS; labels become the tile-local root's global index
//   k_ex_border    unions across tile borders with integer atomicMin on the global labels
//   k_ex_flatten   every foreground pixel points at its root = the smallest linear index of its component
//   k_ex_count     pixels per root (integer atomics, one per wave where a wave sees one root)
//   k_ex_scan1/2/3 raster-order numbering of the roots with at least DETECT_MINAREA pixels
//   k_ex_relabel   segmentation map + bounding box, flag OR, saturation and bad-neighbour bits (integer atomics)
//   k_ex_measure   one workgroup per object walks its bounding box row-major: lane-fixed float64 partial sums, a
//                  fixed-shape reduction (xor shuffles, then waves 0..3 in order): no float atomics, same bits every run
//   k_ex_apbad     does the aperture's circle reach a bad pixel (FLAGS bit 16)
// Every walk along a label chain is bounded by the pixel count; a walk that reaches its bound sets ZM_EXTRACT_CHAIN in the
// status word and returns.
#include <climits>
#include <cmath>

#include "zm_internal.h"

#define EX_TW 32
#define EX_TH 8
#define EX_SCAN_ROUNDS 8
#define EX_SCAN_SPAN (256 * EX_SCAN_ROUNDS)
#define EX_BIT_SAT 4
#define EX_BIT_BADNBR 256

struct ex_meas {
    double s[7];                     // sum v, v dx, v dy, v dx^2, v dy^2, v dx dy (filtered); sum of the unfiltered values
    float peak, fmax;
    int peakidx, nthr;
    float level;                     // the level nthr was counted at
    int pad_;
};

__device__ __forceinline__ bool ex_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool ex_isbad(float v, float s, unsigned b) {
    return b != 0 || ex_nonfinite(v) || ex_nonfinite(s) || !(s > 0.f);
}

// one image row of the six columns x0 - 1 .. x0 + 4: unfiltered values, noise, badness; outside the frame: 0 and bad
__device__ __forceinline__ void ex_row(const float* __restrict__ img, const float* __restrict__ sig,
                                       const uint8_t* __restrict__ bad, int nx, int ny, int y, int x0, bool vec,
                                       float (&raw)[6], float (&s)[6], unsigned& badbits) {
#pragma unroll
    for (int j = 0; j < 6; ++j) { raw[j] = 0.f; s[j] = 0.f; }
    badbits = 0x3f;
    if (y < 0 || y >= ny) return;
    const size_t row = (size_t)y * nx;
    unsigned b[6] = {0, 0, 0, 0, 0, 0};
    bool in[6];
    if (vec) {                                           // nx % 4 == 0, aligned planes: x0 + 3 < nx
        const float4 a = *reinterpret_cast<const float4*>(img + row + x0);
        const float4 c = *reinterpret_cast<const float4*>(sig + row + x0);
        raw[1] = a.x; raw[2] = a.y; raw[3] = a.z; raw[4] = a.w;
        s[1] = c.x; s[2] = c.y; s[3] = c.z; s[4] = c.w;
        if (bad) {
            const unsigned w = *reinterpret_cast<const unsigned*>(bad + row + x0);
            b[1] = w & 0xffu; b[2] = (w >> 8) & 0xffu; b[3] = (w >> 16) & 0xffu; b[4] = w >> 24;
        }
        in[1] = in[2] = in[3] = in[4] = true;
    } else {
#pragma unroll
        for (int j = 1; j <= 4; ++j) {
            const int x = x0 + j - 1;
            in[j] = x < nx;
            if (in[j]) { raw[j] = img[row + x]; s[j] = sig[row + x]; b[j] = bad ? bad[row + x] : 0u; }
        }
    }
    in[0] = x0 - 1 >= 0 && x0 - 1 < nx;
    in[5] = x0 + 4 < nx;
    if (in[0]) { raw[0] = img[row + x0 - 1]; s[0] = sig[row + x0 - 1]; b[0] = bad ? bad[row + x0 - 1] : 0u; }
    if (in[5]) { raw[5] = img[row + x0 + 4]; s[5] = sig[row + x0 + 4]; b[5] = bad ? bad[row + x0 + 4] : 0u; }
    badbits = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
        if (!in[j] || ex_isbad(raw[j], s[j], b[j])) badbits |= 1u << j;
}

// block (64, 4): lane -> four pixels of one row
__global__ __launch_bounds__(256) void k_ex_filter(const float* __restrict__ img, const float* __restrict__ sig,
                                                   const uint8_t* __restrict__ bad, int nx, int ny, float thr,
                                                   int use_filter, int vec, float* __restrict__ filt,
                                                   int* __restrict__ label, int* __restrict__ cnt,
                                                   int* __restrict__ bad32) {
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= nx || y >= ny) return;
    float raw[3][6], s[3][6];
    unsigned bb[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) ex_row(img, sig, bad, nx, ny, y + r - 1, x0, vec != 0, raw[r], s[r], bb[r]);
    const float coef[3][3] = {{1.f, 2.f, 1.f}, {2.f, 4.f, 2.f}, {1.f, 2.f, 1.f}};
    float f[4];
    int lab[4], isb[4];
    const size_t row = (size_t)y * nx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float v = ((bb[r] >> (k + d)) & 1u) ? 0.f : raw[r][k + d];
                acc += coef[r][d] * v;                   // products by powers of two: exact with or without FMA
            }
        acc *= 0.0625f;
        f[k] = use_filter ? acc : raw[1][k + 1];
        isb[k] = (bb[1] >> (k + 1)) & 1u;
        const bool fg = !isb[k] && f[k] > thr * s[1][k + 1];
        lab[k] = fg ? (int)(row + x0 + k) : -1;
    }
    if (vec) {
        *reinterpret_cast<float4*>(filt + row + x0) = make_float4(f[0], f[1], f[2], f[3]);
        *reinterpret_cast<int4*>(label + row + x0) = make_int4(lab[0], lab[1], lab[2], lab[3]);
        *reinterpret_cast<int4*>(cnt + row + x0) = make_int4(0, 0, 0, 0);
        *reinterpret_cast<int4*>(bad32 + row + x0) = make_int4(isb[0], isb[1], isb[2], isb[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < nx) {
                filt[row + x0 + k] = f[k];
                label[row + x0 + k] = lab[k];
                cnt[row + x0 + k] = 0;
                bad32[row + x0 + k] = isb[k];
            }
    }
}

// ---- labelling --------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ex_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of a (labels only ever decrease along a chain); -1 when the walk passes its bound
__device__ __forceinline__ int ex_find(const int* label, int a, int bound) {
    for (int it = 0; it <= bound; ++it) {
        const int l = ex_ld(label + a);
        if (l == a) return a;
        a = l;
    }
    return -1;
}

// unite the sets of a and b: the larger root is linked under the smaller one.  A retry happens only when another lane
// has linked the same root in between, which at most `bound` roots can undergo.
__device__ __forceinline__ void ex_union(int* label, int a, int b, int bound, int* status) {
    for (int it = 0; it <= bound; ++it) {
        a = ex_find(label, a, bound);
        b = ex_find(label, b, bound);
        if (a < 0 || b < 0) break;
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(label + a, b);
        if (old == a) return;
        a = old;                                         // a had a parent already: go on with that one and b
    }
    atomicOr(status, ZM_EXTRACT_CHAIN);
}

__device__ __forceinline__ int ex_find_lds(const int* lab, int a) {
    for (int it = 0; it <= EX_TW * EX_TH; ++it) {
        const int l = __hip_atomic_load(lab + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (l == a) return a;
        a = l;
    }
    return -1;
}

__device__ __forceinline__ void ex_union_lds(int* lab, int a, int b, int* status) {
    for (int it = 0; it <= EX_TW * EX_TH; ++it) {
        a = ex_find_lds(lab, a);
        b = ex_find_lds(lab, b);
        if (a < 0 || b < 0) break;
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;
    }
    atomicOr(status, ZM_EXTRACT_CHAIN);
}

// block (32, 8) = one tile.  The backward neighbours W, NW, N, NE name every 8-adjacent pair once.
__global__ __launch_bounds__(256) void k_ex_local(int* __restrict__ label, int nx, int ny, int* __restrict__ status) {
    __shared__ int lab[EX_TW * EX_TH];
    const int tx = threadIdx.x, ty = threadIdx.y, t = ty * EX_TW + tx;
    const int x = blockIdx.x * EX_TW + tx, y = blockIdx.y * EX_TH + ty;
    const bool inb = x < nx && y < ny;
    const size_t p = (size_t)y * nx + x;
    const bool fg = inb && label[p] >= 0;
    lab[t] = fg ? t : -1;
    __syncthreads();
    if (fg) {
        if (tx > 0 && lab[t - 1] >= 0) ex_union_lds(lab, t, t - 1, status);
        if (ty > 0) {
            if (tx > 0 && lab[t - EX_TW - 1] >= 0) ex_union_lds(lab, t, t - EX_TW - 1, status);
            if (lab[t - EX_TW] >= 0) ex_union_lds(lab, t, t - EX_TW, status);
            if (tx < EX_TW - 1 && lab[t - EX_TW + 1] >= 0) ex_union_lds(lab, t, t - EX_TW + 1, status);
        }
    }
    __syncthreads();
    if (fg) {
        const int r = ex_find_lds(lab, t);
        if (r < 0) { atomicOr(status, ZM_EXTRACT_CHAIN); return; }
        // raster order inside the tile follows raster order in the frame: the local root is the smallest index of its piece
        label[p] = (blockIdx.y * EX_TH + r / EX_TW) * nx + blockIdx.x * EX_TW + r % EX_TW;
    }
}

__global__ __launch_bounds__(256) void k_ex_border(int* __restrict__ label, int nx, int ny, int bound,
                                                   int* __restrict__ status) {
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x = blockIdx.x * EX_TW + tx, y = blockIdx.y * EX_TH + ty;
    if (x >= nx || y >= ny) return;
    if (tx != 0 && ty != 0 && tx != EX_TW - 1) return;     // only these have a backward neighbour in another tile
    const int p = y * nx + x;
    if (ex_ld(label + p) < 0) return;
    if (tx == 0 && x > 0 && ex_ld(label + p - 1) >= 0) ex_union(label, p, p - 1, bound, status);
    if (y > 0) {
        if ((tx == 0 || ty == 0) && x > 0 && ex_ld(label + p - nx - 1) >= 0) ex_union(label, p, p - nx - 1, bound, status);
        if (ty == 0 && ex_ld(label + p - nx) >= 0) ex_union(label, p, p - nx, bound, status);
        if ((tx == EX_TW - 1 || ty == 0) && x + 1 < nx && ex_ld(label + p - nx + 1) >= 0)
            ex_union(label, p, p - nx + 1, bound, status);
    }
}

__global__ __launch_bounds__(256) void k_ex_flatten(int* __restrict__ label, int np, int bound, int* __restrict__ status) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    if (ex_ld(label + p) < 0) return;
    const int r = ex_find(label, p, bound);
    if (r < 0) { atomicOr(status, ZM_EXTRACT_CHAIN); return; }
    // a shortcut to the root: chains that pass through p still end at the same root
    __hip_atomic_store(label + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- pixels per root ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ex_count(const int* __restrict__ label, int np, int* __restrict__ cnt) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int l = p < np ? label[p] : -1;
    const unsigned long long m = __ballot(l >= 0);
    if (m == 0) return;
    const int leader = __ffsll((long long)m) - 1;
    const int l0 = __shfl(l, leader);
    if (__all(l < 0 || l == l0)) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(cnt + l0, __popcll(m));
    } else if (l >= 0) {
        atomicAdd(cnt + l, 1);
    }
}

// ---- raster-order numbering of the roots that stay ------------------------------------------------------------------
__device__ __forceinline__ bool ex_keeps(const int* label, const int* cnt, int p, int np, int minarea) {
    return p < np && label[p] == p && cnt[p] >= minarea;
}

__global__ __launch_bounds__(256) void k_ex_scan1(const int* __restrict__ label, const int* __restrict__ cnt, int np,
                                                  int minarea, int* __restrict__ blockcount) {
    int tot = 0;
    for (int r = 0; r < EX_SCAN_ROUNDS; ++r) {
        const int p = blockIdx.x * EX_SCAN_SPAN + r * 256 + threadIdx.x;
        tot += __syncthreads_count(ex_keeps(label, cnt, p, np, minarea));
    }
    if (threadIdx.x == 0) blockcount[blockIdx.x] = tot;
}

// one workgroup: exclusive prefix of the block counts in place, the total into *nobj
__global__ __launch_bounds__(1024) void k_ex_scan2(int* __restrict__ blockcount, int nblocks, int* __restrict__ nobj) {
    __shared__ int sh[1024];
    int carry = 0;
    for (int base = 0; base < nblocks; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nblocks ? blockcount[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int a = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < nblocks) blockcount[i] = carry + sh[threadIdx.x] - v;
        carry += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *nobj = carry;
}

__global__ __launch_bounds__(256) void k_ex_objinit(int* __restrict__ obj, int cap) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= cap) return;
    int* o = obj + (size_t)k * EX_OI;
    o[0] = INT_MAX; o[1] = -1; o[2] = INT_MAX; o[3] = -1; o[4] = 0; o[5] = 0; o[6] = 0; o[7] = -1;
}

// cnt[root] becomes the object's NUMBER (0: dropped); npix and the root of the first `cap` objects go to the table
__global__ __launch_bounds__(256) void k_ex_scan3(const int* __restrict__ label, int* __restrict__ cnt, int np, int minarea,
                                                  const int* __restrict__ blockoff, int cap, int* __restrict__ obj) {
    __shared__ int wtot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int running = blockoff[blockIdx.x];
    for (int r = 0; r < EX_SCAN_ROUNDS; ++r) {
        const int p = blockIdx.x * EX_SCAN_SPAN + r * 256 + threadIdx.x;
        const bool root = p < np && label[p] == p;
        const int c = root ? cnt[p] : 0;
        const bool q = root && c >= minarea;
        const unsigned long long m = __ballot(q);
        if (lane == 0) wtot[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { before += w < wave ? wtot[w] : 0; all += wtot[w]; }
        if (root) {
            int number = 0;
            if (q) {
                number = running + before + __popcll(m & ((1ull << lane) - 1ull)) + 1;
                if (number <= cap) { obj[(size_t)(number - 1) * EX_OI + 4] = c; obj[(size_t)(number - 1) * EX_OI + 7] = p; }
            }
            cnt[p] = number;
        }
        running += all;
        __syncthreads();
    }
}

// ---- segmentation map and the integer reductions -----------------------------------------------------------------
__device__ __forceinline__ int ex_wmin(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int ex_wmax(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int ex_wor(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void k_ex_relabel(const int* __restrict__ label, const int* __restrict__ num,
                                                    const float* __restrict__ img, const int32_t* __restrict__ flag,
                                                    const int* __restrict__ bad32, int nx, int ny, float satur, int cap,
                                                    int* __restrict__ seg, int* __restrict__ obj) {
    const int np = nx * ny;
    const int p = blockIdx.x * 256 + threadIdx.x;
    int n = 0;
    if (p < np) {
        const int l = label[p];
        n = l >= 0 ? num[l] : 0;
        seg[p] = n;
    }
    const bool member = n > 0 && n <= cap;
    int x = 0, y = 0, fl = 0, bits = 0;
    if (member) {
        y = p / nx;
        x = p - y * nx;
        fl = flag ? flag[p] : 0;
        if (img[p] >= satur) bits |= EX_BIT_SAT;
        int nb = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = x + dx, yy = y + dy;
                if (xx >= 0 && xx < nx && yy >= 0 && yy < ny) nb |= bad32[yy * nx + xx];
            }
        if (nb) bits |= EX_BIT_BADNBR;
    }
    const unsigned long long m = __ballot(member);
    if (m == 0) return;
    const int leader = __ffsll((long long)m) - 1;
    const int n0 = __shfl(n, leader);
    if (__all(!member || n == n0)) {                    // one object in this wave: one set of atomics
        const int x0 = ex_wmin(member ? x : INT_MAX), x1 = ex_wmax(member ? x : -1);
        const int y0 = ex_wmin(member ? y : INT_MAX), y1 = ex_wmax(member ? y : -1);
        fl = ex_wor(fl);
        bits = ex_wor(bits);
        if ((int)(threadIdx.x & 63) == leader) {
            int* o = obj + (size_t)(n0 - 1) * EX_OI;
            atomicMin(o + 0, x0); atomicMax(o + 1, x1); atomicMin(o + 2, y0); atomicMax(o + 3, y1);
            if (fl) atomicOr(o + 5, fl);
            if (bits) atomicOr(o + 6, bits);
        }
    } else if (member) {
        int* o = obj + (size_t)(n - 1) * EX_OI;
        atomicMin(o + 0, x); atomicMax(o + 1, x); atomicMin(o + 2, y); atomicMax(o + 3, y);
        if (fl) atomicOr(o + 5, fl);
        if (bits) atomicOr(o + 6, bits);
    }
}

// ---- isophotal sums -------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ex_wsum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one workgroup of four waves per object; element e of the row-major bounding box belongs to lane e % 256
__global__ __launch_bounds__(256) void k_ex_measure(const int* __restrict__ seg, const float* __restrict__ filt,
                                                    const float* __restrict__ img, const float* __restrict__ sig,
                                                    int nx, float thr, const int* __restrict__ obj, int nobj,
                                                    ex_meas* __restrict__ out) {
    __shared__ double sh[4][7];
    __shared__ float shp[4], shm[4];
    __shared__ int shi[4], shn[4];
    __shared__ float level;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (k >= nobj) return;
    const int* o = obj + (size_t)k * EX_OI;
    const int xmin = o[0], xmax = o[1], ymin = o[2], ymax = o[3];
    const int bw = xmax - xmin + 1, bh = ymax - ymin + 1;
    const int total = (bw > 0 && bh > 0) ? bw * bh : 0;
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    float peak = -INFINITY, fmx = -INFINITY;
    int pidx = INT_MAX;
    for (int e = tid; e < total; e += 256) {
        const int j = e / bw, i = e - j * bw;
        const int p = (ymin + j) * nx + xmin + i;
        if (seg[p] != k + 1) continue;
        const float vf = filt[p], rf = img[p];
        const double v = vf, dx = i, dy = j;
        s[0] += v; s[1] += v * dx; s[2] += v * dy; s[3] += v * dx * dx; s[4] += v * dy * dy; s[5] += v * dx * dy;
        s[6] += (double)rf;
        if (vf > peak) { peak = vf; pidx = p; }          // p grows along the walk: the first pixel of a tie stays
        fmx = fmaxf(fmx, rf);
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) s[q] = ex_wsum(s[q]);
#pragma unroll
    for (int of = 32; of >= 1; of >>= 1) {
        const float op = __shfl_xor(peak, of);
        const int oi = __shfl_xor(pidx, of);
        if (op > peak || (op == peak && oi < pidx)) { peak = op; pidx = oi; }
        fmx = fmaxf(fmx, __shfl_xor(fmx, of));
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 7; ++q) sh[wave][q] = s[q];
        shp[wave] = peak; shi[wave] = pidx; shm[wave] = fmx;
    }
    __syncthreads();
    if (tid == 0) {
        ex_meas r;
#pragma unroll
        for (int q = 0; q < 7; ++q) r.s[q] = ((sh[0][q] + sh[1][q]) + sh[2][q]) + sh[3][q];
        float pk = shp[0], fm = shm[0];
        int pi = shi[0];
        for (int w = 1; w < 4; ++w) {
            if (shp[w] > pk || (shp[w] == pk && shi[w] < pi)) { pk = shp[w]; pi = shi[w]; }
            fm = fmaxf(fm, shm[w]);
        }
        r.peak = pk; r.fmax = fm; r.peakidx = pi; r.nthr = 0; r.pad_ = 0;
        // the level the FWHM area is counted at: the detection threshold at the peak pixel, or half the peak
        level = pi != INT_MAX ? fmaxf(thr * sig[pi], 0.5f * pk) : INFINITY;
        r.level = level;
        out[k] = r;
    }
    __syncthreads();
    const float t = level;
    int n = 0;
    for (int e = tid; e < total; e += 256) {
        const int j = e / bw, i = e - j * bw;
        const int p = (ymin + j) * nx + xmin + i;
        if (seg[p] == k + 1 && filt[p] >= t) ++n;
    }
#pragma unroll
    for (int of = 32; of >= 1; of >>= 1) n += __shfl_xor(n, of);
    if (lane == 0) shn[wave] = n;
    __syncthreads();
    if (tid == 0) out[k].nthr = shn[0] + shn[1] + shn[2] + shn[3];
}

// FLAGS bit 16, second half: does the aperture's circle reach a bad pixel?  One wave per object over the clipped bounding
// box of the circle; a pixel is reached when the point of its square nearest to the centre lies inside the radius
// (single roundings, no contraction: the numpy restatement evaluates the same expression).
__global__ __launch_bounds__(64) void k_ex_apbad(const int* __restrict__ bad32, int nx, int ny, int nobj,
                                                 const double* __restrict__ xs, const double* __restrict__ ys, double r,
                                                 int32_t* __restrict__ hit) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= nobj) return;
    const double xc = xs[k], yc = ys[k];
    int i0 = (int)floor(xc - r + 0.5), i1 = (int)ceil(xc + r + 0.5);
    int j0 = (int)floor(yc - r + 0.5), j1 = (int)ceil(yc + r + 0.5);
    i0 = max(i0, 0); i1 = min(i1, nx); j0 = max(j0, 0); j1 = min(j1, ny);
    const int bw = i1 - i0, bh = j1 - j0;
    int h = 0;
    if (bw > 0 && bh > 0)
        for (int e = lane; e < bw * bh; e += 64) {
            const int j = j0 + e / bw, i = i0 + e % bw;
            if (!bad32[(size_t)j * nx + i]) continue;
            const double dx = fmax(fabs((double)i - xc) - 0.5, 0.0), dy = fmax(fabs((double)j - yc) - 0.5, 0.0);
            if (__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) < __dmul_rn(r, r)) h = 1;
        }
    h = ex_wor(h);
    if (lane == 0) hit[k] = h;
}

// ---- host ----------------------------------------------------------------------------------------------------------
extern "C" void zm_extract_params_default(zm_extract_params* p) {
    if (!p) return;
    p->detect_thresh = 1.5f;
    p->satur_level = 50000.f;
    p->detect_minarea = 5;
    p->filter = 1;
    p->aper_radius = 3.0;
}

static void ex_finish_row(zm_object* r, const int* o, const ex_meas& m, int number, int nx, int ny, double radius) {
    memset(r, 0, sizeof(*r));
    const int xmin = o[0], xmax = o[1], ymin = o[2], ymax = o[3];
    r->number = number;
    r->npix = o[4];
    r->xmin = xmin + 1; r->xmax = xmax + 1; r->ymin = ymin + 1; r->ymax = ymax + 1;
    r->imaflags_iso = o[5];
    r->flags_weight = (o[6] & EX_BIT_BADNBR) ? 1 : 0;
    r->first = o[7];
    r->nthresh = m.nthr;
    const double S = m.s[0];
    const double xb = m.s[1] / S, yb = m.s[2] / S;
    double x2 = m.s[3] / S - xb * xb, y2 = m.s[4] / S - yb * yb;
    const double xy = m.s[5] / S - xb * yb;
    if (x2 * y2 - xy * xy < 0.00694) { x2 += 1.0 / 12.0; y2 += 1.0 / 12.0; }
    const double pm = 0.5 * (x2 + y2), dm = 0.5 * (x2 - y2);
    const double rt = sqrt(dm * dm + xy * xy);
    r->x_image = xmin + xb + 1.0;
    r->y_image = ymin + yb + 1.0;
    r->x2 = x2; r->y2 = y2; r->xy = xy;
    r->a_image = sqrt(pm + rt);
    r->b_image = sqrt(fmax(pm - rt, 0.0));
    r->theta_image = 0.5 * atan2(2.0 * xy, x2 - y2) * (180.0 / M_PI);
    r->elongation = r->a_image / r->b_image;
    r->peak = m.peak;
    // FWHM of a Gaussian from its area above a level: nthr pixels at or above `level` under the peak
    r->fwhm_image = m.peak > m.level ? sqrt(4.0 * M_LN2 * m.nthr / (M_PI * log((double)m.peak / (double)m.level))) : 0.0;
    r->flux_iso = m.s[6];
    r->flux_max = m.fmax;
    int fl = (o[6] & EX_BIT_SAT) ? 4 : 0;
    if (xmin == 0 || ymin == 0 || xmax == nx - 1 || ymax == ny - 1) fl |= 8;
    const double xc = r->x_image - 1.0, yc = r->y_image - 1.0;
    // the aperture's circle leaves the frame (pixel i covers [i - 0.5, i + 0.5]); a bad pixel under it: k_ex_apbad
    if (xc - radius < -0.5 || xc + radius > nx - 0.5 || yc - radius < -0.5 || yc + radius > ny - 0.5) fl |= 16;
    r->flags = fl;
    r->x_world = r->y_world = NAN;
}

// The stages of zm_ex_first_pass (declared in zm_internal.h; deblend.hip and clean.hip call them too).
int zm_ex_check(zm_ctx* ctx, const float* img, const float* sigma, int nx, int ny, const zm_extract_params* params,
                int max_objects, const zm_object* out_rows, const int* out_nwritten, const int* out_nfound) {
    ZM_CHECK(ctx && img && sigma && params && out_nwritten && out_nfound, "zm_extract: null argument");
    // rows go on gridDim.y, four per workgroup of the filter: 65535 x 4 rows at the most
    ZM_CHECK(nx > 0 && ny > 0 && (int64_t)nx * ny <= (int64_t)1 << 30 && ny <= 65535 * 4,
             "zm_extract: bad sizes %d x %d (at most 2^30 pixels and 262140 rows)", nx, ny);
    ZM_CHECK(max_objects >= 0 && max_objects <= (1 << 24) && (out_rows || max_objects == 0),
             "zm_extract: max_objects %d needs a row array (and at most 2^24 rows)", max_objects);
    ZM_CHECK(params->detect_thresh > 0.f && params->detect_minarea >= 1 && (params->filter == 0 || params->filter == 1) &&
                 params->aper_radius > 0 && params->aper_radius < 512,
             "zm_extract: bad parameters (thresh %g, minarea %d, filter %d, radius %g)", (double)params->detect_thresh,
             params->detect_minarea, params->filter, params->aper_radius);
    return 0;
}

// scratch planes; the status word and the counters are cleared
int zm_ex_planes(zm_ctx* ctx, int nx, int ny, int32_t* segm_dev, float* filtered_dev, zm_ex_bufs* b) {
    const int np = nx * ny;
    b->np = np;
    b->nsb = zm_div_up(np, EX_SCAN_SPAN);
    b->filt = filtered_dev;
    b->seg = segm_dev;
    if (!b->filt) ZM_TRY(ctx->get("ex_filt", (size_t)np * 4, (void**)&b->filt));
    if (!b->seg) ZM_TRY(ctx->get("ex_seg", (size_t)np * 4, (void**)&b->seg));
    ZM_TRY(ctx->get("ex_label", (size_t)np * 4, (void**)&b->label));
    ZM_TRY(ctx->get("ex_cnt", (size_t)np * 4, (void**)&b->cnt));
    ZM_TRY(ctx->get("ex_bad32", (size_t)np * 4, (void**)&b->bad32));
    ZM_TRY(ctx->get("ex_small", (size_t)(b->nsb + 4) * 4, (void**)&b->small));
    ZM_HIP(hipMemsetAsync(b->small, 0, 16, ctx->stream));
    return 0;
}

// filter, threshold, labelling, pixels per root
void zm_ex_label(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad, int nx, int ny,
                 const zm_extract_params* params, const zm_ex_bufs* b) {
    const int np = b->np;
    int* d_status = b->small;
    const bool vec = nx % 4 == 0 && (((uintptr_t)img | (uintptr_t)sigma | (uintptr_t)b->filt | (uintptr_t)b->label |
                                      (uintptr_t)b->cnt | (uintptr_t)b->bad32) & 15) == 0 && ((uintptr_t)bad & 3) == 0;
    const dim3 tiles(zm_div_up(nx, EX_TW), zm_div_up(ny, EX_TH)), tile(EX_TW, EX_TH);
    const int nlin = zm_div_up(np, 256);
    hipLaunchKernelGGL(k_ex_filter, dim3(zm_div_up(zm_div_up(nx, 4), 64), zm_div_up(ny, 4)), dim3(64, 4), 0, ctx->stream, img,
                       sigma, bad, nx, ny, params->detect_thresh, params->filter, vec ? 1 : 0, b->filt, b->label, b->cnt,
                       b->bad32);
    hipLaunchKernelGGL(k_ex_local, tiles, tile, 0, ctx->stream, b->label, nx, ny, d_status);
    hipLaunchKernelGGL(k_ex_border, tiles, tile, 0, ctx->stream, b->label, nx, ny, np, d_status);
    hipLaunchKernelGGL(k_ex_flatten, dim3(nlin), dim3(256), 0, ctx->stream, b->label, np, np, d_status);
    hipLaunchKernelGGL(k_ex_count, dim3(nlin), dim3(256), 0, ctx->stream, b->label, np, b->cnt);
}

// pixels per root of another label plane, into the cleared counter plane
int zm_ex_recount(zm_ctx* ctx, const int* label, const zm_ex_bufs* b) {
    ZM_HIP(hipMemsetAsync(b->cnt, 0, (size_t)b->np * 4, ctx->stream));
    hipLaunchKernelGGL(k_ex_count, dim3(zm_div_up(b->np, 256)), dim3(256), 0, ctx->stream, label, b->np, b->cnt);
    return 0;
}

// `label` holds, for every foreground pixel, the smallest linear index of its object, and b->cnt the pixels per root
void zm_ex_count_roots(zm_ctx* ctx, const int* label, int minarea, const zm_ex_bufs* b) {
    hipLaunchKernelGGL(k_ex_scan1, dim3(b->nsb), dim3(256), 0, ctx->stream, label, b->cnt, b->np, minarea, b->small + 4);
    hipLaunchKernelGGL(k_ex_scan2, dim3(1), dim3(1024), 0, ctx->stream, b->small + 4, b->nsb, b->small + 1);
}

// Waits for the stream and reads the head: head[0] the status word, head[1] the number of objects, into the call's
// out_status and out_nfound (cap >= 0: and min(objects, cap) into out_nwritten).  A status word that is set fails the call:
// `what` passed its bound of `bound` steps (bound 0: a loop of either kind).
int zm_ex_head(zm_ctx* ctx, const zm_ex_bufs* b, const zm_ex_outs* o, const char* what, int bound, int head[2], int cap) {
    ZM_HIP(hipMemcpyAsync(head, b->small, 8, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    if (o->status) *o->status = head[0];
    *o->nfound = head[1];
    if (cap >= 0) *o->nwritten = head[1] < cap ? head[1] : cap;
    if (bound) ZM_CHECK(head[0] == 0, "%s: %s passed its bound of %d steps (status %d)", o->who, what, bound, head[0]);
    ZM_CHECK(head[0] == 0, "%s: %s passed its bound (status %d: 1 label chain, 2 deblending)", o->who, what, head[0]);
    return 0;
}

// numbering, segmentation map into `seg`, integer reductions into `obj` (cap rows)
void zm_ex_number(zm_ctx* ctx, const int* label, const float* img, const int32_t* flag, int nx, int ny,
                  const zm_extract_params* params, int cap, int* seg, int* obj, const zm_ex_bufs* b) {
    const int nlin = zm_div_up(b->np, 256);
    if (cap > 0) hipLaunchKernelGGL(k_ex_objinit, dim3(zm_div_up(cap, 256)), dim3(256), 0, ctx->stream, obj, cap);
    hipLaunchKernelGGL(k_ex_scan3, dim3(b->nsb), dim3(256), 0, ctx->stream, label, b->cnt, b->np, params->detect_minarea,
                       b->small + 4, cap, obj);
    hipLaunchKernelGGL(k_ex_relabel, dim3(nlin), dim3(256), 0, ctx->stream, label, b->cnt, img, flag, b->bad32, nx, ny,
                       params->satur_level, cap, seg, obj);
}

// rows 0 .. n - 1 from the segmentation map and the object table
int zm_ex_rows(zm_ctx* ctx, const float* img, const float* sigma, int nx, int ny, const zm_wcs* wcs,
               const zm_extract_params* params, int n, const int* d_seg, const int* d_obj, const zm_ex_bufs* b,
               zm_object* out_rows) {
    const float* d_filt = b->filt;
    const int* d_bad32 = b->bad32;
    char* d_m = nullptr;
    const size_t apbytes = (size_t)n * (4 * sizeof(double) + 2 * sizeof(int32_t));
    ZM_TRY(ctx->get("ex_meas", (size_t)n * sizeof(ex_meas) + apbytes + 64, (void**)&d_m));
    ex_meas* d_meas = (ex_meas*)d_m;
    double* d_x = (double*)(d_m + (((size_t)n * sizeof(ex_meas) + 15) & ~(size_t)15));
    double *d_y = d_x + n, *d_f = d_y + n, *d_e = d_f + n;
    int32_t *d_fl = (int32_t*)(d_e + n), *d_hit = d_fl + n;
    hipLaunchKernelGGL(k_ex_measure, dim3(n), dim3(256), 0, ctx->stream, d_seg, d_filt, img, sigma, nx, params->detect_thresh,
                       d_obj, n, d_meas);
    ZM_HIP(hipGetLastError());
    std::vector<ex_meas> meas(n);
    std::vector<int> oi((size_t)n * EX_OI);
    ZM_HIP(hipMemcpyAsync(meas.data(), d_meas, (size_t)n * sizeof(ex_meas), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(oi.data(), d_obj, (size_t)n * EX_OI * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<double> pos((size_t)n * 4);
    double *hx = pos.data(), *hy = hx + n, *hf = hy + n, *he = hf + n;
    std::vector<int32_t> hfl(n);
    for (int k = 0; k < n; ++k) {
        ex_finish_row(out_rows + k, oi.data() + (size_t)k * EX_OI, meas[k], k + 1, nx, ny, params->aper_radius);
        hx[k] = out_rows[k].x_image - 1.0;
        hy[k] = out_rows[k].y_image - 1.0;
    }
    ZM_HIP(hipMemcpyAsync(d_x, hx, sizeof(double) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
    ZM_TRY(zm_aperture_photometry_dev(ctx, img, sigma, nullptr, nx, ny, n, d_x, d_y, params->aper_radius, d_f, d_e, d_fl));
    hipLaunchKernelGGL(k_ex_apbad, dim3(n), dim3(64), 0, ctx->stream, d_bad32, nx, ny, n, d_x, d_y, params->aper_radius, d_hit);
    ZM_HIP(hipGetLastError());
    ZM_HIP(hipMemcpyAsync(hf, d_f, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(hfl.data(), d_hit, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; ++k) {
        zm_object* r = out_rows + k;
        r->flux_aper = hf[k];
        r->fluxerr_aper = he[k];
        if (hfl[k]) r->flags |= 16;
    }
    if (wcs) {
        std::vector<double> w((size_t)n * 4);
        for (int k = 0; k < n; ++k) { w[k] = out_rows[k].x_image; w[n + k] = out_rows[k].y_image; }
        ZM_TRY(zm_wcs_pix2sky(wcs, n, w.data(), w.data() + n, w.data() + 2 * n, w.data() + 3 * n));
        for (int k = 0; k < n; ++k) { out_rows[k].x_world = w[2 * n + k]; out_rows[k].y_world = w[3 * n + k]; }
    }
    return 0;
}

// The first pass of every form on device planes (checked by the caller): zm_extract_dev (deblend and clean NULL),
// zm_extract_deblend_dev and zm_extract_clean_dev (clean set, deblend or not).  Only the forms that split or merge read the
// head early: they need the objects of the pass before on the host.
int zm_ex_first_pass(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad, const int32_t* flag, int nx, int ny,
                     const zm_wcs* wcs, const zm_extract_params* params, int max_objects, zm_object* out_rows,
                     int32_t* segm_dev, float* filtered_dev, const zm_ex_outs* o, const zm_deblend_params* deblend,
                     const zm_clean_params* clean, int32_t* out_parent, int32_t* out_nmerged) {
    ZM_HIP(hipSetDevice(ctx->device));
    const int np = nx * ny, cap = max_objects;
    zm_ex_bufs b;
    int head[2] = {0, 0};
    if (clean) ctx->cl_npre = 0;
    // planes, labels, roots
    ZM_TRY(zm_ex_planes(ctx, nx, ny, segm_dev, filtered_dev, &b));
    zm_ex_label(ctx, img, sigma, bad, nx, ny, params, &b);
    zm_ex_count_roots(ctx, b.label, params->detect_minarea, &b);
    // split, merge
    int *d_seg1 = nullptr, *d_split = nullptr;
    if (deblend || clean) {
        ZM_HIP(hipGetLastError());
        ZM_TRY(zm_ex_head(ctx, &b, o, "a label chain", np, head, 0));
        if (deblend && head[1] > 0) {
            ZM_TRY(zm_db_split(ctx, img, sigma, flag, nx, ny, params, deblend, head[1], &b, &d_seg1, &d_split));
            if (clean) ZM_TRY(zm_ex_head(ctx, &b, o, "a loop", 0, head));
        }
        if (clean && head[1] > 0)                        // it numbers and measures what it leaves
            return zm_cl_merge(ctx, img, sigma, flag, nx, ny, wcs, params, cap, clean, head[1], &b, d_seg1, d_split, out_rows, o,
                               out_parent, out_nmerged);
    }
    // number
    int* d_obj = nullptr;
    ZM_TRY(ctx->get("ex_obj", (size_t)(cap + 1) * EX_OI * 4, (void**)&d_obj));
    zm_ex_number(ctx, b.label, img, flag, nx, ny, params, cap, b.seg, d_obj, &b);
    ZM_HIP(hipGetLastError());
    if (clean) {                                         // nothing to clean: the empty map
        ZM_HIP(hipStreamSynchronize(ctx->stream));
        return 0;
    }
    // head, rows, parent
    if (deblend) ZM_TRY(zm_ex_head(ctx, &b, o, "a loop", 0, head));
    else ZM_TRY(zm_ex_head(ctx, &b, o, "a label chain", np, head, cap));
    const int n = head[1] < cap ? head[1] : cap;
    *o->nwritten = n;
    if (n == 0) return 0;
    ZM_TRY(zm_ex_rows(ctx, img, sigma, nx, ny, wcs, params, n, b.seg, d_obj, &b, out_rows));
    return deblend ? zm_db_parent(ctx, d_obj, n, d_seg1, d_split, out_rows, out_parent) : 0;
}

extern "C" int zm_extract_dev(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                              const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                              const zm_extract_params* params, int max_objects, zm_object* out_rows,
                              int32_t* segm_dev, float* filtered_dev, int* out_nwritten, int* out_nfound,
                              int* out_status) {
    ZM_TRY(zm_ex_check(ctx, img, sigma, nx, ny, params, max_objects, out_rows, out_nwritten, out_nfound));
    const zm_ex_outs o = {out_nwritten, out_nfound, out_status, "zm_extract"};
    return zm_ex_first_pass(ctx, img, sigma, bad, flag, nx, ny, wcs, params, max_objects, out_rows, segm_dev, filtered_dev, &o,
                            nullptr, nullptr, nullptr, nullptr);
}

// host planes in, host planes out, for zm_extract (deblend == nullptr), zm_extract_deblend and zm_extract_clean (clean set)
int zm_ex_host(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad, const int32_t* flag, int nx, int ny,
               const zm_wcs* wcs, const zm_extract_params* params, int max_objects, zm_object* out_rows, int32_t* out_segm,
               float* out_filtered, int* out_nwritten, int* out_nfound, int* out_status, const zm_deblend_params* deblend,
               int32_t* out_parent, const zm_clean_params* clean, int32_t* out_nmerged) {
    ZM_TRY(zm_ex_check(ctx, img, sigma, nx, ny, params, max_objects, out_rows, out_nwritten, out_nfound));
    if (clean) ZM_TRY(zm_cl_check(clean));
    if (deblend) ZM_TRY(zm_db_check(deblend));
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t np = (size_t)nx * ny;
    float *d_img = nullptr, *d_sig = nullptr, *d_filt = nullptr;
    uint8_t* d_bad = nullptr;
    int32_t *d_flag = nullptr, *d_seg = nullptr;
    ZM_TRY(ctx->get("h_img", np * 4, (void**)&d_img));
    ZM_TRY(ctx->get("h_wgt", np * 4, (void**)&d_sig));
    ZM_HIP(hipMemcpyAsync(d_img, img, np * 4, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_sig, sigma, np * 4, hipMemcpyHostToDevice, ctx->stream));
    if (bad) {
        ZM_TRY(ctx->get("h_bpm", np, (void**)&d_bad));
        ZM_HIP(hipMemcpyAsync(d_bad, bad, np, hipMemcpyHostToDevice, ctx->stream));
    }
    if (flag) {
        ZM_TRY(ctx->get("h_mask", np * 4, (void**)&d_flag));
        ZM_HIP(hipMemcpyAsync(d_flag, flag, np * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    ZM_TRY(ctx->get("ex_seg", np * 4, (void**)&d_seg));
    ZM_TRY(ctx->get("ex_filt", np * 4, (void**)&d_filt));
    int st = 0;
    const zm_ex_outs o = {out_nwritten, out_nfound, &st,
                          clean ? "zm_extract_clean" : deblend ? "zm_extract_deblend" : "zm_extract"};
    const int rc = zm_ex_first_pass(ctx, d_img, d_sig, d_bad, d_flag, nx, ny, wcs, params, max_objects, out_rows, d_seg, d_filt,
                                    &o, deblend, clean, out_parent, out_nmerged);
    if (out_status) *out_status = st;
    if (rc != 0 && st == 0) return rc;                   // with the status word set the planes still come back: they show where
    if (out_segm) ZM_HIP(hipMemcpyAsync(out_segm, d_seg, np * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_filtered) ZM_HIP(hipMemcpyAsync(out_filtered, d_filt, np * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return rc;
}

extern "C" int zm_extract(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                          const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                          const zm_extract_params* params, int max_objects, zm_object* out_rows,
                          int32_t* out_segm, float* out_filtered, int* out_nwritten, int* out_nfound,
                          int* out_status) {
    return zm_ex_host(ctx, img, sigma, bad, flag, nx, ny, wcs, params, max_objects, out_rows, out_segm, out_filtered,
                      out_nwritten, out_nfound, out_status, nullptr, nullptr);
}
