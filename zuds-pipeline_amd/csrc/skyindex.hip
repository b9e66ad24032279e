// Cone searches against a catalogue that stays in HBM, on gfx950: the k nearest rows and all rows within a radius.
//
// Replaces the five cone searches per detection of the reference's xmatch() (zuds/crossmatch.py: Kowalski queries; the
// q3c neighbour tables of nersc/makesources.py:110-190).  The operator is stated in DESIGN.md ("Alert packets").
//
// Geometry: that of associate.hip, through the same functions (sky_cells.h).  A position becomes an fp64 unit vector, two
// points are neighbours when their squared chord is <= (2 sin(r / 2))^2 (inclusive), the separation is
// 2 asin(min(1, chord / 2)).  The cells have the edge of the index's LARGEST radius, so every query with r <= max_radius
// visits the 27 cells around it.
//
// Index (built once, zm_skyindex_create*): a counting sort of the rows by cell.
//   k_si_insert   the 64-bit cell key of a row is claimed in an open-addressing table with a CAS (linear probing, capacity
//                 the power of two >= 2 m, at least 64); the row remembers its slot and counts itself there (atomicAdd)
//   k_si_scan_*   exclusive scan of the counts in slot order: start[slot], start[capacity] = rows
//   k_si_scatter  unit vector and row number of every row to start[slot] + its arrival rank (an integer cursor per slot)
// so the rows of a cell are contiguous (sx, sy, sz, srow), and a cell costs a probe and two words of start[].  The order
// inside a cell differs from run to run; every output below is defined without it.  A row that is not finite is left out.
//
// Queries: one wave per query, four to a workgroup.  The query's cell and probe sequence are wave-uniform (readfirstlane),
// the 64 lanes stride the contiguous rows of a cell.
//   k_si_knn<K>   every lane keeps its K best (squared chord, row) pairs sorted in registers (unrolled insertion, no
//                 scratch); K rounds of a (squared chord, row) minimum across the wave then pop the winner's lane
//   k_si_count    rows within the radius per query -> scan (int32 in, int64 out) -> offsets
//   k_si_fill     the rows of a query to its segment of a work array, in arrival order (ballot ranks within the wave)
//   k_si_sort     one wave per query: every row goes to the slot its rank among the query's rows names, if that slot is
//                 below the capacity - ascending by catalogue row, the same bytes on every run
// No float atomics: counts and cursors are integer atomics.
#include <algorithm>
#include <cmath>

#include "sky_cells.h"

#define SI_SCAN_PER_BLOCK 1024        // elements of one block of the scan (256 threads x 4)
#define SI_KMAX 8
#define SI_NOROW 0x7fffffff           // an empty slot of a lane's list: sorts behind every row

struct zm_skyindex {
    int device = 0, m = 0;
    double max_radius = 0.0;
    as_grid g = {};                   // edge and thr of max_radius
    char* slab = nullptr;             // keys, start, sx, sy, sz, srow
    as_u64* keys = nullptr;
    int* start = nullptr;             // [capacity + 1]
    double *sx = nullptr, *sy = nullptr, *sz = nullptr;
    int* srow = nullptr;
    int64_t stats[4] = {0, 0, 0, 0};  // rows, cells used, capacity, longest probe
};

// stats[0] = the longest probe of one insertion, stats[1] += slots claimed
__global__ __launch_bounds__(256) void k_si_insert(const double* __restrict__ ra, const double* __restrict__ dec, int m,
                                                   as_grid g, as_u64* keys, int* count, int* __restrict__ slot,
                                                   as_u64* stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    as_u64 probes = 0, claimed = 0;
    if (i < m) {
        const double a = ra[i], d = dec[i];
        int mine = -1;
        if (as_finite(a) && as_finite(d)) {
            double x, y, z;
            as_unit(a, d, &x, &y, &z);
            const as_u64 key = as_key(as_cell(x, g.edge), as_cell(y, g.edge), as_cell(z, g.edge));
            as_u64 s = as_hash(key) & g.mask;
            // capacity >= 2 m: a free slot always exists, the bound only keeps a corrupt table from spinning
            for (as_u64 t = 0; t <= g.mask; ++t) {
                ++probes;
                const as_u64 prev = atomicCAS(&keys[s], AS_EMPTY, key);
                if (prev == AS_EMPTY || prev == key) {
                    claimed = prev == AS_EMPTY ? 1 : 0;
                    atomicAdd(&count[s], 1);
                    mine = (int)s;
                    break;
                }
                s = (s + 1) & g.mask;
            }
        }
        slot[i] = mine;
    }
    as_u64 sum = claimed, mx = probes;
#pragma unroll
    for (int of = 32; of >= 1; of >>= 1) {
        sum += __shfl_xor(sum, of);
        const as_u64 o = __shfl_xor(mx, of);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) {
        atomicMax(&stats[0], mx);
        if (sum) atomicAdd(&stats[1], sum);
    }
}

// cursor[] holds the counts of k_si_insert and is counted down: the rank of a row within its cell is its arrival order
__global__ __launch_bounds__(256) void k_si_scatter(const double* __restrict__ ra, const double* __restrict__ dec, int m,
                                                    const int* __restrict__ slot, const int* __restrict__ start, int* cursor,
                                                    double* __restrict__ sx, double* __restrict__ sy, double* __restrict__ sz,
                                                    int* __restrict__ srow) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int s = slot[i];
    if (s < 0) return;
    double x, y, z;
    as_unit(ra[i], dec[i], &x, &y, &z);
    const int pos = start[s] + atomicSub(&cursor[s], 1) - 1;
    sx[pos] = x; sy[pos] = y; sz[pos] = z;
    srow[pos] = i;
}

// ---- exclusive scan, int32 in, T out (per block, the block totals, add) ----------------------------------------------
template <class T>
__device__ __forceinline__ T si_block_scan(T v, T* sh, T* total) {              // exclusive, 256 threads
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int of = 1; of < 256; of <<= 1) {
        const T a = t >= of ? sh[t - of] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const T incl = sh[t];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

template <class T>
__global__ __launch_bounds__(256) void k_si_scan_local(const int* __restrict__ in, long long n, T* __restrict__ out,
                                                       T* __restrict__ bsum) {
    __shared__ T sh[256];
    const long long b0 = (long long)blockIdx.x * SI_SCAN_PER_BLOCK + threadIdx.x * 4;
    T v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = b0 + k < n ? in[b0 + k] : 0;
        s += v[k];
    }
    T total;
    T ex = si_block_scan(s, sh, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (b0 + k < n) out[b0 + k] = ex;
        ex += v[k];
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

template <class T>
__global__ __launch_bounds__(256) void k_si_scan_tops(T* __restrict__ bsum, int nb, T* __restrict__ total_out) {
    __shared__ T sh[256];
    T carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int k = b0 + threadIdx.x;
        const T v = k < nb ? bsum[k] : 0;
        T total;
        const T ex = si_block_scan(v, sh, &total);
        if (k < nb) bsum[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

template <class T>
__global__ __launch_bounds__(256) void k_si_scan_add(T* __restrict__ out, long long n, const T* __restrict__ bsum) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] += bsum[i / SI_SCAN_PER_BLOCK];
}

// ---- queries ---------------------------------------------------------------------------------------------------------
struct si_view {                      // what a query kernel reads of an index
    double edge, thr;                 // the index's cell edge; (2 sin(r / 2))^2 of THIS query radius
    as_u64 mask;
    const as_u64* keys;
    const int* start;
    const double *sx, *sy, *sz;
    const int* srow;
};

// One wave, all 64 lanes in step: f(in, row, d2) once per lane for every 64 rows of the 27 cells around (x, y, z); `in` says
// that the lane holds a row and that its squared chord d2 is <= thr.  The cell coordinates, the probe sequence and the
// bounds of a cell are the same in every lane (readfirstlane puts them into scalar registers), so f may vote (ballot).
template <class F>
__device__ __forceinline__ void si_visit(double x, double y, double z, const si_view& v, int lane, F&& f) {
    const int cx = __builtin_amdgcn_readfirstlane((int)as_cell(x, v.edge)), cy = __builtin_amdgcn_readfirstlane((int)as_cell(y, v.edge)),
              cz = __builtin_amdgcn_readfirstlane((int)as_cell(z, v.edge));
#pragma unroll 1
    for (int c = 0; c < 27; ++c) {
        const as_u64 key = as_key(cx + (c % 3) - 1, cy + ((c / 3) % 3) - 1, cz + (c / 9) - 1);
        as_u64 s = as_hash(key) & v.mask;
        int st = 0, en = 0;
        for (as_u64 t = 0; t <= v.mask; ++t) {
            const as_u64 k = v.keys[s];
            if (k == key) {
                st = v.start[s];
                en = v.start[s + 1];                     // (slot capacity - 1: start[capacity] = rows)
                break;
            }
            if (k == AS_EMPTY) break;
            s = (s + 1) & v.mask;
        }
        st = __builtin_amdgcn_readfirstlane(st);
        en = __builtin_amdgcn_readfirstlane(en);
        for (int e0 = st; e0 < en; e0 += 64) {
            const int e = e0 + lane;
            bool in = false;
            int row = SI_NOROW;
            double d2 = 0.0;
            if (e < en) {
                const double dx = v.sx[e] - x, dy = v.sy[e] - y, dz = v.sz[e] - z;
                d2 = dx * dx + dy * dy + dz * dz;
                in = d2 <= v.thr;
                row = v.srow[e];
            }
            f(in, row, d2);
        }
    }
}

__device__ __forceinline__ bool si_less(double d, int j, double bd, int bj) { return d < bd || (d == bd && j < bj); }

__device__ __forceinline__ int si_wave_sum(int v) {
#pragma unroll
    for (int of = 32; of >= 1; of >>= 1) v += __shfl_xor(v, of);
    return v;
}

template <int K>
__global__ __launch_bounds__(256) void k_si_knn(const double* __restrict__ ra, const double* __restrict__ dec, int n, si_view v,
                                                int* __restrict__ idx, double* __restrict__ sep, int* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (i >= n) return;
    const double inf = __builtin_inf();
    double bd[K];
    int bj[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { bd[t] = inf; bj[t] = SI_NOROW; }
    int cnt = 0;
    const double a = ra[i], d = dec[i];
    if (as_finite(a) && as_finite(d)) {
        double x, y, z;
        as_unit(a, d, &x, &y, &z);
        si_visit(x, y, z, v, lane, [&](bool in, int row, double d2) {
            if (in) {
                ++cnt;
                double cd = d2;                          // carried down the sorted list: the smaller of each pair stays
                int cj = row;
#pragma unroll
                for (int t = 0; t < K; ++t) {
                    const bool lt = si_less(cd, cj, bd[t], bj[t]);
                    const double td = lt ? bd[t] : cd;
                    const int tj = lt ? bj[t] : cj;
                    bd[t] = lt ? cd : bd[t];
                    bj[t] = lt ? cj : bj[t];
                    cd = td;
                    cj = tj;
                }
            }
        });
    }
    cnt = si_wave_sum(cnt);
    double rd = inf;                                     // lane t ends up with the t-th nearest
    int rj = SI_NOROW;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        double md = bd[0];
        int mj = bj[0];
#pragma unroll
        for (int of = 32; of >= 1; of >>= 1) {
            const double od = __shfl_xor(md, of);
            const int oj = __shfl_xor(mj, of);
            const bool lt = si_less(od, oj, md, mj);
            md = lt ? od : md;
            mj = lt ? oj : mj;
        }
        if (mj != SI_NOROW && bj[0] == mj) {             // a row sits in one lane only: that lane pops it
#pragma unroll
            for (int u = 0; u + 1 < K; ++u) { bd[u] = bd[u + 1]; bj[u] = bj[u + 1]; }
            bd[K - 1] = inf;
            bj[K - 1] = SI_NOROW;
        }
        if (lane == t) { rd = md; rj = mj; }
    }
    if (lane < K) {
        const bool hit = rj != SI_NOROW;
        idx[(size_t)i * K + lane] = hit ? rj : -1;
        sep[(size_t)i * K + lane] = hit ? 2.0 * asin(fmin(1.0, 0.5 * sqrt(rd))) * AS_ARCSEC_PER_RAD : __builtin_nan("");
    }
    if (lane == 0) count[i] = cnt;
}

__global__ __launch_bounds__(256) void k_si_count(const double* __restrict__ ra, const double* __restrict__ dec, int n, si_view v,
                                                  int* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (i >= n) return;
    int cnt = 0;
    const double a = ra[i], d = dec[i];
    if (as_finite(a) && as_finite(d)) {
        double x, y, z;
        as_unit(a, d, &x, &y, &z);
        si_visit(x, y, z, v, lane, [&](bool in, int, double) { cnt += in ? 1 : 0; });
    }
    cnt = si_wave_sum(cnt);
    if (lane == 0) count[i] = cnt;
}

// tmp has room for offsets[n] entries: a query writes exactly the count k_si_count found for it
__global__ __launch_bounds__(256) void k_si_fill(const double* __restrict__ ra, const double* __restrict__ dec, int n, si_view v,
                                                 const long long* __restrict__ offsets, int* __restrict__ tmp) {
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (i >= n) return;
    const double a = ra[i], d = dec[i];
    if (!(as_finite(a) && as_finite(d))) return;
    const long long base = offsets[i], room = offsets[i + 1] - base;
    long long w = 0;
    double x, y, z;
    as_unit(a, d, &x, &y, &z);
    si_visit(x, y, z, v, lane, [&](bool in, int row, double) {
        const unsigned long long hits = __ballot(in);
        const long long r = w + __popcll(hits & ((1ull << lane) - 1ull));
        if (in && r < room) tmp[base + r] = row;
        w += __popcll(hits);
    });
}

// one wave per query: every row goes to the slot its rank among the query's rows names (rows are distinct), which undoes
// the arrival order of k_si_fill; nothing is written at or past `capacity`
__global__ __launch_bounds__(256) void k_si_sort(int n, const long long* __restrict__ offsets, const int* __restrict__ tmp,
                                                 long long capacity, int* __restrict__ cat_idx) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const long long o = offsets[i], c = offsets[i + 1] - o;
    if (o >= capacity) return;
    for (long long e = lane; e < c; e += 64) {
        const int val = tmp[o + e];
        long long r = 0;
        for (long long k = 0; k < c; ++k) r += tmp[o + k] < val ? 1 : 0;
        if (o + r < capacity) cat_idx[o + r] = val;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static size_t si_up(size_t b) { return (b + 255) & ~(size_t)255; }

static as_u64 si_capacity(int m) {
    as_u64 c = 64;
    while (c < 2ull * (as_u64)m) c <<= 1;
    return c;
}

static double si_chord(double radius_arcsec) { return 2.0 * sin(0.5 * (radius_arcsec / AS_ARCSEC_PER_RAD)); }

struct si_dev_free {                  // device memory of one call, released on every way out
    void* p = nullptr;
    ~si_dev_free() { if (p) (void)hipFree(p); }
};

template <class T>
static int si_scan(zm_ctx* ctx, const int* in, long long n, T* out, T* bsum, T* total_dev) {
    const int nb = (int)((n + SI_SCAN_PER_BLOCK - 1) / SI_SCAN_PER_BLOCK);
    hipLaunchKernelGGL(k_si_scan_local<T>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, in, n, out, bsum);
    hipLaunchKernelGGL(k_si_scan_tops<T>, dim3(1), dim3(256), 0, ctx->stream, bsum, nb, total_dev);
    hipLaunchKernelGGL(k_si_scan_add<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, out, n, (const T*)bsum);
    ZM_HIP(hipGetLastError());
    return 0;
}

static void si_release(zm_skyindex* ix) {
    if (!ix) return;
    if (ix->slab) {
        (void)hipSetDevice(ix->device);
        (void)hipFree(ix->slab);
    }
    delete ix;
}

extern "C" int zm_skyindex_create_dev(zm_ctx* ctx, int m, const double* ra_dev, const double* dec_dev, double max_radius_arcsec,
                                      zm_skyindex** out_index) {
    ZM_CHECK(ctx && out_index, "zm_skyindex_create_dev: null argument");
    *out_index = nullptr;
    ZM_CHECK(m >= 0 && m <= (1 << 30), "zm_skyindex_create_dev: m must be 0 .. 2^30 (got %d)", m);
    ZM_CHECK(max_radius_arcsec >= 0.25 && max_radius_arcsec <= 3600.0,
             "zm_skyindex_create_dev: max_radius must be 0.25 .. 3600 arcsec (got %g)", max_radius_arcsec);
    ZM_CHECK(m == 0 || (ra_dev && dec_dev), "zm_skyindex_create_dev: null argument");
    const double chord = si_chord(max_radius_arcsec);
    as_grid g;
    g.edge = chord * (1.0 + 1e-6);
    g.thr = chord * chord;
    g.mask = si_capacity(m) - 1;
    ZM_CHECK(1.0 / g.edge + 2.0 < (double)AS_OFF, "zm_skyindex_create_dev: a radius of %g arcsec makes more cells than a key holds",
             max_radius_arcsec);
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t cap = (size_t)g.mask + 1, M = (size_t)m;
    const int nb = (int)((cap + SI_SCAN_PER_BLOCK - 1) / SI_SCAN_PER_BLOCK);
    struct guard { zm_skyindex* p; ~guard() { si_release(p); } } ix{new zm_skyindex};
    ix.p->device = ctx->device;
    ix.p->m = m;
    ix.p->max_radius = max_radius_arcsec;
    ix.p->g = g;
    const size_t o_keys = 0, o_start = o_keys + si_up(cap * 8), o_sx = o_start + si_up((cap + 1) * 4), o_sy = o_sx + si_up(M * 8),
                 o_sz = o_sy + si_up(M * 8), o_row = o_sz + si_up(M * 8), total = o_row + si_up(M * 4) + 256;
    ZM_HIP(hipMalloc((void**)&ix.p->slab, total));
    char* w = ix.p->slab;
    ix.p->keys = (as_u64*)(w + o_keys);
    ix.p->start = (int*)(w + o_start);
    ix.p->sx = (double*)(w + o_sx);
    ix.p->sy = (double*)(w + o_sy);
    ix.p->sz = (double*)(w + o_sz);
    ix.p->srow = (int*)(w + o_row);
    // work arrays of the build: the slot of every row, the count (then cursor) of every slot, the scan's block totals
    const size_t t_slot = 0, t_count = t_slot + si_up(M * 4), t_bsum = t_count + si_up(cap * 4), t_stats = t_bsum + si_up((size_t)nb * 4),
                 t_total = t_stats + 256;
    si_dev_free tmp;
    ZM_HIP(hipMalloc(&tmp.p, t_total));
    char* t = (char*)tmp.p;
    int *slot = (int*)(t + t_slot), *count = (int*)(t + t_count), *bsum = (int*)(t + t_bsum);
    as_u64* stats = (as_u64*)(t + t_stats);
    {
        zm_scope_timer timer(ctx, "skyindex_build");
        ZM_HIP(hipMemsetAsync(ix.p->keys, 0xff, cap * sizeof(as_u64), ctx->stream));
        ZM_HIP(hipMemsetAsync(count, 0, cap * sizeof(int), ctx->stream));
        ZM_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(as_u64), ctx->stream));
        const dim3 grid((unsigned)zm_div_up(std::max(m, 1), 256)), block(256);
        if (m)
            hipLaunchKernelGGL(k_si_insert, grid, block, 0, ctx->stream, ra_dev, dec_dev, m, g, ix.p->keys, count, slot, stats);
        ZM_TRY(si_scan<int>(ctx, count, (long long)cap, ix.p->start, bsum, ix.p->start + cap));
        if (m)
            hipLaunchKernelGGL(k_si_scatter, grid, block, 0, ctx->stream, ra_dev, dec_dev, m, (const int*)slot,
                               (const int*)ix.p->start, count, ix.p->sx, ix.p->sy, ix.p->sz, ix.p->srow);
        ZM_HIP(hipGetLastError());
    }
    as_u64 words[2] = {0, 0};
    int rows = 0;
    ZM_HIP(hipMemcpyAsync(words, stats, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(&rows, ix.p->start + cap, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));           // the work arrays go, and the caller may free ra / dec
    ZM_CHECK(rows >= 0 && rows <= m, "zm_skyindex_create_dev: %d rows indexed of %d", rows, m);
    ix.p->stats[0] = rows;
    ix.p->stats[1] = (int64_t)words[1];
    ix.p->stats[2] = (int64_t)cap;
    ix.p->stats[3] = (int64_t)words[0];
    *out_index = ix.p;
    ix.p = nullptr;
    return 0;
}

extern "C" int zm_skyindex_create(zm_ctx* ctx, int m, const double* ra, const double* dec, double max_radius_arcsec,
                                  zm_skyindex** out_index) {
    ZM_CHECK(ctx && out_index, "zm_skyindex_create: null argument");
    *out_index = nullptr;
    ZM_CHECK(m >= 0 && m <= (1 << 30), "zm_skyindex_create: m must be 0 .. 2^30 (got %d)", m);
    ZM_CHECK(m == 0 || (ra && dec), "zm_skyindex_create: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t M = (size_t)m;
    si_dev_free io;                                      // a catalogue is large and read once: not the context's scratch
    ZM_HIP(hipMalloc(&io.p, 2 * si_up(M * 8) + 256));
    double *d_ra = (double*)io.p, *d_dec = (double*)((char*)io.p + si_up(M * 8));
    if (m) {
        ZM_HIP(hipMemcpyAsync(d_ra, ra, M * 8, hipMemcpyHostToDevice, ctx->stream));
        ZM_HIP(hipMemcpyAsync(d_dec, dec, M * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    return zm_skyindex_create_dev(ctx, m, d_ra, d_dec, max_radius_arcsec, out_index);     // (waits before it returns)
}

extern "C" int zm_skyindex_destroy(zm_skyindex* index) {
    si_release(index);
    return 0;
}

extern "C" int zm_skyindex_stats(const zm_skyindex* index, int64_t* out4) {
    ZM_CHECK(index && out4, "zm_skyindex_stats: null argument");
    for (int k = 0; k < 4; ++k) out4[k] = index->stats[k];
    return 0;
}

// the checks every query shares, and the view of the index at this radius
static int si_query(const char* who, zm_ctx* ctx, const zm_skyindex* ix, int n, double radius_arcsec, si_view* v) {
    ZM_CHECK(ctx && ix, "%s: null argument", who);
    ZM_CHECK(ctx->device == ix->device, "%s: the index lives on device %d, the context on device %d", who, ix->device, ctx->device);
    ZM_CHECK(n >= 0 && n <= (1 << 30), "%s: n must be 0 .. 2^30 (got %d)", who, n);
    ZM_CHECK(radius_arcsec >= 0.25 && radius_arcsec <= 3600.0, "%s: the radius must be 0.25 .. 3600 arcsec (got %g)", who, radius_arcsec);
    ZM_CHECK(radius_arcsec <= ix->max_radius, "%s: a radius of %g arcsec on an index built for at most %g arcsec", who, radius_arcsec,
             ix->max_radius);
    const double chord = si_chord(radius_arcsec);
    v->edge = ix->g.edge;
    v->thr = chord * chord;
    v->mask = ix->g.mask;
    v->keys = ix->keys;
    v->start = ix->start;
    v->sx = ix->sx; v->sy = ix->sy; v->sz = ix->sz;
    v->srow = ix->srow;
    return 0;
}

extern "C" int zm_cone_knn_dev(zm_ctx* ctx, const zm_skyindex* index, int n, const double* ra_dev, const double* dec_dev,
                               double radius_arcsec, int k, int32_t* idx_dev, double* sep_dev, int32_t* count_dev) {
    si_view v;
    ZM_TRY(si_query("zm_cone_knn_dev", ctx, index, n, radius_arcsec, &v));
    ZM_CHECK(k >= 1 && k <= SI_KMAX, "zm_cone_knn_dev: k must be 1 .. %d (got %d)", SI_KMAX, k);
    if (n == 0) return 0;
    ZM_CHECK(ra_dev && dec_dev && idx_dev && sep_dev && count_dev, "zm_cone_knn_dev: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    zm_scope_timer timer(ctx, "cone_knn");
    const dim3 grid((unsigned)zm_div_up(n, 4)), block(256);
#define SI_KNN(K) case K: hipLaunchKernelGGL(k_si_knn<K>, grid, block, 0, ctx->stream, ra_dev, dec_dev, n, v, idx_dev, sep_dev, count_dev); break
    switch (k) {
        SI_KNN(1); SI_KNN(2); SI_KNN(3); SI_KNN(4); SI_KNN(5); SI_KNN(6); SI_KNN(7); SI_KNN(8);
    }
#undef SI_KNN
    ZM_HIP(hipGetLastError());
    return 0;
}

extern "C" int zm_cone_knn(zm_ctx* ctx, const zm_skyindex* index, int n, const double* ra, const double* dec, double radius_arcsec,
                           int k, int32_t* idx, double* sep, int32_t* count) {
    si_view v;
    ZM_TRY(si_query("zm_cone_knn", ctx, index, n, radius_arcsec, &v));
    ZM_CHECK(k >= 1 && k <= SI_KMAX, "zm_cone_knn: k must be 1 .. %d (got %d)", SI_KMAX, k);
    if (n == 0) return 0;
    ZM_CHECK(ra && dec && idx && sep && count, "zm_cone_knn: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)n, NK = N * (size_t)k;
    const size_t o_ra = 0, o_dec = o_ra + si_up(N * 8), o_sep = o_dec + si_up(N * 8), o_idx = o_sep + si_up(NK * 8),
                 o_cnt = o_idx + si_up(NK * 4), total = o_cnt + si_up(N * 4);
    char* d = nullptr;
    ZM_TRY(ctx->get("h_si_io", total, (void**)&d));
    ZM_HIP(hipMemcpyAsync(d + o_ra, ra, N * 8, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d + o_dec, dec, N * 8, hipMemcpyHostToDevice, ctx->stream));
    ZM_TRY(zm_cone_knn_dev(ctx, index, n, (const double*)(d + o_ra), (const double*)(d + o_dec), radius_arcsec, k,
                           (int32_t*)(d + o_idx), (double*)(d + o_sep), (int32_t*)(d + o_cnt)));
    ZM_HIP(hipMemcpyAsync(idx, d + o_idx, NK * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(sep, d + o_sep, NK * 8, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(count, d + o_cnt, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int zm_cone_within_dev(zm_ctx* ctx, const zm_skyindex* index, int n, const double* ra_dev, const double* dec_dev,
                                  double radius_arcsec, int64_t capacity, int64_t* offsets_dev, int32_t* cat_idx_dev,
                                  int64_t* out_npairs) {
    si_view v;
    ZM_TRY(si_query("zm_cone_within_dev", ctx, index, n, radius_arcsec, &v));
    ZM_CHECK(offsets_dev && out_npairs, "zm_cone_within_dev: null argument");
    ZM_CHECK(capacity >= 0, "zm_cone_within_dev: negative capacity");
    ZM_HIP(hipSetDevice(ctx->device));
    *out_npairs = 0;
    if (n == 0) {
        ZM_HIP(hipMemsetAsync(offsets_dev, 0, sizeof(int64_t), ctx->stream));
        return 0;
    }
    ZM_CHECK(ra_dev && dec_dev && (capacity == 0 || cat_idx_dev), "zm_cone_within_dev: null argument");
    const size_t N = (size_t)n;
    const int nb = (int)((N + SI_SCAN_PER_BLOCK - 1) / SI_SCAN_PER_BLOCK);
    const size_t o_cnt = 0, o_bsum = o_cnt + si_up(N * 4), total = o_bsum + si_up((size_t)nb * 8);
    char* w = nullptr;
    ZM_TRY(ctx->get("si_work", total, (void**)&w));
    int* cnt = (int*)(w + o_cnt);
    long long *bsum = (long long*)(w + o_bsum), *offsets = (long long*)offsets_dev;
    long long* th = nullptr;
    ZM_TRY(ctx->get_pinned("si_total_h", sizeof(long long), (void**)&th));
    zm_scope_timer timer(ctx, "cone_within");
    const dim3 grid((unsigned)zm_div_up(n, 4)), block(256);
    hipLaunchKernelGGL(k_si_count, grid, block, 0, ctx->stream, ra_dev, dec_dev, n, v, cnt);
    ZM_TRY(si_scan<long long>(ctx, cnt, (long long)n, offsets, bsum, offsets + n));
    ZM_HIP(hipMemcpyAsync(th, offsets + n, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));           // the one word: it also sizes the work array of the fill
    const long long npairs = *th;
    ZM_CHECK(npairs >= 0, "zm_cone_within_dev: %lld pairs", npairs);
    *out_npairs = (int64_t)npairs;
    if (capacity == 0 || npairs == 0) return 0;
    int* tmp = nullptr;
    ZM_TRY(ctx->get("si_pairs", (size_t)npairs * 4, (void**)&tmp));
    hipLaunchKernelGGL(k_si_fill, grid, block, 0, ctx->stream, ra_dev, dec_dev, n, v, (const long long*)offsets, tmp);
    hipLaunchKernelGGL(k_si_sort, grid, block, 0, ctx->stream, n, (const long long*)offsets, (const int*)tmp, (long long)capacity,
                       cat_idx_dev);
    ZM_HIP(hipGetLastError());
    return 0;
}

extern "C" int zm_cone_within(zm_ctx* ctx, const zm_skyindex* index, int n, const double* ra, const double* dec, double radius_arcsec,
                              int64_t capacity, int64_t* offsets, int32_t* cat_idx, int64_t* out_npairs) {
    si_view v;
    ZM_TRY(si_query("zm_cone_within", ctx, index, n, radius_arcsec, &v));
    ZM_CHECK(offsets && out_npairs, "zm_cone_within: null argument");
    ZM_CHECK(capacity >= 0 && (capacity == 0 || cat_idx), "zm_cone_within: bad capacity or null pair list");
    ZM_CHECK(n == 0 || (ra && dec), "zm_cone_within: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)n, cap = (size_t)capacity;
    const size_t o_ra = 0, o_dec = o_ra + si_up(N * 8), o_off = o_dec + si_up(N * 8), o_idx = o_off + si_up((N + 1) * 8),
                 total = o_idx + si_up(cap * 4) + 256;
    char* d = nullptr;
    ZM_TRY(ctx->get("h_si_io", total, (void**)&d));
    if (n) {
        ZM_HIP(hipMemcpyAsync(d + o_ra, ra, N * 8, hipMemcpyHostToDevice, ctx->stream));
        ZM_HIP(hipMemcpyAsync(d + o_dec, dec, N * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    ZM_TRY(zm_cone_within_dev(ctx, index, n, (const double*)(d + o_ra), (const double*)(d + o_dec), radius_arcsec, capacity,
                              (int64_t*)(d + o_off), (int32_t*)(d + o_idx), out_npairs));
    ZM_HIP(hipMemcpyAsync(offsets, d + o_off, (N + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    const size_t got = std::min((size_t)*out_npairs, cap);
    if (got) ZM_HIP(hipMemcpyAsync(cat_idx, d + o_idx, got * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
