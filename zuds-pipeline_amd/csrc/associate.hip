// Source association on gfx950: a radius join on the sphere and connected components over a night's detections, and
// the nearest-neighbour cross-match that shares its cell table.
//
// Replaces the q3c joins, search_around_sky and DBSCAN(eps = 2, min_samples = 2, metric = 'precomputed') of the
// reference's associate() (nersc/makesources.py:263-456).  The operator is stated in DESIGN.md ("Source association").
//
// Geometry.  Every position becomes an fp64 unit vector; two points are neighbours when their squared chord is
// <= (2 sin(r / 2))^2 (inclusive, as the KD-tree behind search_around_sky and DBSCAN's eps are).  Unit vectors are binned
// into cubic cells whose edge is the chord of r times 1 + 1e-6: two neighbours differ by less than one edge along every
// axis, so a search visits the 27 cells around a point and needs no case for the RA wrap, the poles or declination bands.
//
//   k_as_unit     (ra, dec[, snr]) -> unit vector; a row with a value that is not finite gets NaN and takes part in nothing
//   k_as_insert   open addressing in HBM: the 64-bit cell key is claimed with a CAS (linear probing, capacity the power
//                 of two >= 2 n, at least 64), the point is pushed on the slot's list with an atomic exchange of the head
//                 (next[] per point).  The order of a list differs from run to run; nothing below depends on it.
//   k_as_round    label[i] <- min over i and its neighbours of their labels (atomicMin), the same minimum hooked onto the
//                 old label's entry, then the pointer jumps label[i] <- label[label[i]] down to a fixed entry
//   k_as_roots .. k_as_reduce   noise -> -1, sources numbered by the rank of their smallest member (sklearn's numbering),
//                 CSR of the members in ascending order, best S/N (ties: lowest index), count, sum of rb in member order
//   k_xm          nearest catalogue entry within r (ties: lowest catalogue index), separation in arcsec
//
// No float atomics anywhere: counts and cursors are integer atomics, and the one value that is a sum of reals (sumrb) is
// added up by one thread per source in member order, so it is the same bits on every run.
#include <cmath>

#include "sky_cells.h"

#define AS_SCAN_PER_BLOCK 1024        // elements of one block of the scan (256 threads x 4)

__global__ __launch_bounds__(256) void k_as_unit(const double* __restrict__ ra, const double* __restrict__ dec,
                                                 const double* __restrict__ snr, int n, double* __restrict__ vx,
                                                 double* __restrict__ vy, double* __restrict__ vz) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double a = ra[i], d = dec[i];
    double x = __builtin_nan(""), y = x, z = x;
    if (as_finite(a) && as_finite(d) && (!snr || as_finite(snr[i]))) as_unit(a, d, &x, &y, &z);
    vx[i] = x; vy[i] = y; vz[i] = z;
}

// stats[0] += probes of every insertion (1: the home slot was free or held the key), stats[1] = the longest of them
__global__ __launch_bounds__(256) void k_as_insert(const double* __restrict__ vx, const double* __restrict__ vy,
                                                   const double* __restrict__ vz, int n, as_grid g, as_u64* keys, int* head,
                                                   int* __restrict__ next, as_u64* stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    as_u64 probes = 0;
    if (i < n) {
        const double x = vx[i];
        if (x == x) {
            const as_u64 key = as_key(as_cell(x, g.edge), as_cell(vy[i], g.edge), as_cell(vz[i], g.edge));
            as_u64 s = as_hash(key) & g.mask;
            // capacity >= 2 n: a free slot always exists, the bound only keeps a corrupt table from spinning
            for (as_u64 t = 0; t <= g.mask; ++t) {
                ++probes;
                const as_u64 prev = atomicCAS(&keys[s], AS_EMPTY, key);
                if (prev == AS_EMPTY || prev == key) {
                    next[i] = atomicExch(&head[s], i);
                    break;
                }
                s = (s + 1) & g.mask;
            }
        }
    }
    as_u64 sum = probes, mx = probes;
#pragma unroll
    for (int of = 32; of >= 1; of >>= 1) {
        sum += __shfl_xor(sum, of);
        const as_u64 o = __shfl_xor(mx, of);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && sum) {
        atomicAdd(&stats[0], sum);
        atomicMax(&stats[1], mx);
    }
}

// f(j, d2) for every point j of the table whose squared chord to (x, y, z) is <= thr; the table was built by an earlier
// launch, so plain loads see all of it
template <class F>
__device__ __forceinline__ void as_visit(double x, double y, double z, const as_grid& g, const as_u64* __restrict__ keys,
                                         const int* __restrict__ head, const int* __restrict__ next,
                                         const double* __restrict__ vx, const double* __restrict__ vy,
                                         const double* __restrict__ vz, F&& f) {
    const long long cx = as_cell(x, g.edge), cy = as_cell(y, g.edge), cz = as_cell(z, g.edge);
#pragma unroll 1
    for (int c = 0; c < 27; ++c) {
        const as_u64 key = as_key(cx + (c % 3) - 1, cy + ((c / 3) % 3) - 1, cz + (c / 9) - 1);
        as_u64 s = as_hash(key) & g.mask;
        for (as_u64 t = 0; t <= g.mask; ++t) {
            const as_u64 k = keys[s];
            if (k == key) {
                for (int j = head[s]; j >= 0; j = next[j]) {
                    const double dx = vx[j] - x, dy = vy[j] - y, dz = vz[j] - z;
                    const double d2 = dx * dx + dy * dy + dz * dz;
                    if (d2 <= g.thr) f(j, d2);
                }
                break;
            }
            if (k == AS_EMPTY) break;
            s = (s + 1) & g.mask;
        }
    }
}

// One round of the label propagation.  lab[] only ever decreases, and every value it holds is the index of a member of
// the same component that is <= the entry's own index, so a stale (larger) value read here is still a valid label.
template <bool FIRST>
__global__ __launch_bounds__(256) void k_as_round(const double* __restrict__ vx, const double* __restrict__ vy,
                                                  const double* __restrict__ vz, int n, as_grid g,
                                                  const as_u64* __restrict__ keys, const int* __restrict__ head,
                                                  const int* __restrict__ next, int* lab, int* __restrict__ deg, int* changed) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = vx[i];
    if (!(x == x)) {
        if (FIRST) deg[i] = 0;
        return;
    }
    if (!FIRST && deg[i] == 0) return;                   // no neighbour: noise, nothing to propagate
    const int li = lab[i];
    int m = li, cnt = 0;
    as_visit(x, vy[i], vz[i], g, keys, head, next, vx, vy, vz, [&](int j, double) {
        if (j != i) {
            ++cnt;
            const int lj = lab[j];
            m = lj < m ? lj : m;
        }
    });
    if (FIRST) deg[i] = cnt;
    bool dec = false;
    if (m < li) {
        atomicMin(&lab[i], m);
        atomicMin(&lab[li], m);                          // hook the old label's entry as well: fewer rounds on chains
        dec = true;
    }
    int r = m;
    for (;;) {                                           // pointer jumps: strictly decreasing, so it ends
        const int p = lab[r];
        if (p >= r) break;
        r = p;
    }
    if (r < m) {
        atomicMin(&lab[i], r);
        dec = true;
    }
    if (dec) *changed = 1;
}

__global__ __launch_bounds__(256) void k_as_iota(int* __restrict__ lab, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) lab[i] = i;
}

__global__ __launch_bounds__(256) void k_as_roots(const int* __restrict__ lab, const int* __restrict__ deg, int n,
                                                  int* __restrict__ isroot) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) isroot[i] = (deg[i] > 0 && lab[i] == i) ? 1 : 0;     // (deg is 0 on rows that take part in nothing)
}

// ---- exclusive scan of int32 (three launches: per block, the block totals, add) -----------------------------------
__device__ __forceinline__ int as_block_scan(int v, int* sh, int* total) {      // exclusive, 256 threads
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int of = 1; of < 256; of <<= 1) {
        const int a = t >= of ? sh[t - of] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const int incl = sh[t];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void k_as_scan_local(const int* __restrict__ in, int n, int* __restrict__ out,
                                                       int* __restrict__ bsum) {
    __shared__ int sh[256];
    const int base = blockIdx.x * AS_SCAN_PER_BLOCK + threadIdx.x * 4;
    int v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = base + k < n ? in[base + k] : 0;
        s += v[k];
    }
    int total;
    int ex = as_block_scan(s, sh, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) out[base + k] = ex;
        ex += v[k];
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_as_scan_tops(int* __restrict__ bsum, int nb, int* __restrict__ total_out) {
    __shared__ int sh[256];
    int carry = 0;
    for (int base = 0; base < nb; base += 256) {
        const int k = base + threadIdx.x;
        const int v = k < nb ? bsum[k] : 0;
        int total;
        const int ex = as_block_scan(v, sh, &total);
        if (k < nb) bsum[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(256) void k_as_scan_add(int* __restrict__ out, int n, const int* __restrict__ bsum) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] += bsum[i / AS_SCAN_PER_BLOCK];
}

// ---- compaction ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_as_label(const int* __restrict__ lab, const int* __restrict__ deg,
                                                  const int* __restrict__ rank, int n, int* __restrict__ label, int* count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int s = -1;
    if (deg[i] > 0) {
        s = rank[lab[i]];                                // lab[i]: the smallest member of i's component
        atomicAdd(&count[s], 1);
    }
    label[i] = s;
}

__global__ __launch_bounds__(256) void k_as_fill(const int* __restrict__ label, const int* __restrict__ offsets, int n,
                                                 int* cursor, int* __restrict__ mtmp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = label[i];
    if (s >= 0) mtmp[offsets[s] + atomicAdd(&cursor[s], 1)] = i;
}

// one wave per source: every member goes to the slot its rank among the members names (indices are distinct), which
// undoes the arrival order of k_as_fill
__global__ __launch_bounds__(256) void k_as_sort(const int* __restrict__ nsrc, const int* __restrict__ offsets,
                                                 const int* __restrict__ count, const int* __restrict__ mtmp,
                                                 int* __restrict__ members) {
    const int lane = threadIdx.x & 63;
    const int ns = *nsrc;
    for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < ns; s += gridDim.x * 4) {
        const int o = offsets[s], c = count[s];
        for (int e = lane; e < c; e += 64) {
            const int v = mtmp[o + e];
            int r = 0;
            for (int k = 0; k < c; ++k) r += mtmp[o + k] < v ? 1 : 0;
            members[o + r] = v;
        }
    }
}

// one thread per source, members in ascending order: the fp64 sum of rb in that order and the first member of greatest
// S/N (strict >, so a tie stays with the lowest index: pandas idxmax)
__global__ __launch_bounds__(256) void k_as_reduce(const int* __restrict__ nsrc, const int* __restrict__ offsets,
                                                   const int* __restrict__ members, const double* __restrict__ snr,
                                                   const double* __restrict__ rb, int* __restrict__ best,
                                                   double* __restrict__ sumrb) {
    const int ns = *nsrc;
    for (int s = blockIdx.x * 256 + threadIdx.x; s < ns; s += gridDim.x * 256) {
        const int o = offsets[s], e = offsets[s + 1];
        int b = members[o];
        double bs = snr[b], sum = 0.0;
        for (int k = o; k < e; ++k) {
            const int j = members[k];
            const double v = snr[j];
            if (v > bs) { bs = v; b = j; }
            if (rb) sum += rb[j];
        }
        best[s] = b;
        sumrb[s] = sum;
    }
}

// ---- cross-match --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_xm(const double* __restrict__ ra, const double* __restrict__ dec, int n, as_grid g,
                                            const as_u64* __restrict__ keys, const int* __restrict__ head,
                                            const int* __restrict__ next, const double* __restrict__ vx,
                                            const double* __restrict__ vy, const double* __restrict__ vz,
                                            int* __restrict__ idx, double* __restrict__ sep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double a = ra[i], d = dec[i];
    int bj = -1;
    double bd = 0.0;
    if (as_finite(a) && as_finite(d)) {
        double x, y, z;
        as_unit(a, d, &x, &y, &z);
        as_visit(x, y, z, g, keys, head, next, vx, vy, vz, [&](int j, double d2) {
            if (bj < 0 || d2 < bd || (d2 == bd && j < bj)) { bd = d2; bj = j; }
        });
    }
    idx[i] = bj;
    sep[i] = bj >= 0 ? 2.0 * asin(fmin(1.0, 0.5 * sqrt(bd))) * AS_ARCSEC_PER_RAD : __builtin_nan("");
}

// ---- host ---------------------------------------------------------------------------------------------------------
static size_t as_up(size_t b) { return (b + 255) & ~(size_t)255; }

static as_u64 as_capacity(int n) {
    as_u64 c = 64;
    while (c < 2ull * (as_u64)n) c <<= 1;
    return c;
}

static int as_make_grid(const char* who, double radius_arcsec, int npoints, as_grid* g) {
    ZM_CHECK(radius_arcsec >= 0.25 && radius_arcsec <= 3600.0, "%s: the radius must be 0.25 .. 3600 arcsec (got %g)", who,
             radius_arcsec);
    const double r = radius_arcsec / AS_ARCSEC_PER_RAD;
    const double chord = 2.0 * sin(0.5 * r);
    g->edge = chord * (1.0 + 1e-6);
    g->thr = chord * chord;
    g->mask = as_capacity(npoints) - 1;
    ZM_CHECK(1.0 / g->edge + 2.0 < (double)AS_OFF, "%s: a radius of %g arcsec makes more cells than a key holds", who, radius_arcsec);
    return 0;
}

// what the last call on a context did, for zm_assoc_stats (pinned: the rounds' flag lands in word 0)
struct as_host { int32_t changed, rounds; int64_t capacity; const as_u64* stats; };

static int as_scan(zm_ctx* ctx, const int* in, int n, int* out, int* bsum, int* total_dev) {
    const int nb = zm_div_up(n, AS_SCAN_PER_BLOCK);
    hipLaunchKernelGGL(k_as_scan_local, dim3((unsigned)nb), dim3(256), 0, ctx->stream, in, n, out, bsum);
    hipLaunchKernelGGL(k_as_scan_tops, dim3(1), dim3(256), 0, ctx->stream, bsum, nb, total_dev);
    hipLaunchKernelGGL(k_as_scan_add, dim3((unsigned)zm_div_up(n, 256)), dim3(256), 0, ctx->stream, out, n, bsum);
    ZM_HIP(hipGetLastError());
    return 0;
}

// the cell table of np points whose unit vectors are in v[3]: keys, heads and next[] cleared and filled
static int as_build(zm_ctx* ctx, double* const v[3], int np, const as_grid& g, as_u64* keys, int* head, int* next,
                    as_u64* stats) {
    const size_t cap = (size_t)g.mask + 1;
    ZM_HIP(hipMemsetAsync(keys, 0xff, cap * sizeof(as_u64), ctx->stream));
    ZM_HIP(hipMemsetAsync(head, 0xff, cap * sizeof(int), ctx->stream));
    ZM_HIP(hipMemsetAsync(next, 0xff, (size_t)np * sizeof(int), ctx->stream));
    ZM_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(as_u64), ctx->stream));
    hipLaunchKernelGGL(k_as_insert, dim3((unsigned)zm_div_up(np, 256)), dim3(256), 0, ctx->stream, v[0], v[1], v[2], np, g,
                       keys, head, next, stats);
    ZM_HIP(hipGetLastError());
    return 0;
}

extern "C" int zm_associate_dev(zm_ctx* ctx, int n, const double* ra_dev, const double* dec_dev, const double* snr_dev,
                                const double* rb_dev, double radius_arcsec, int32_t* label_dev, int32_t* nsrc_dev,
                                int32_t* offsets_dev, int32_t* members_dev, int32_t* best_dev, int32_t* count_dev,
                                double* sumrb_dev) {
    ZM_CHECK(ctx && nsrc_dev && offsets_dev, "zm_associate_dev: null argument");
    ZM_CHECK(n >= 0 && n <= (1 << 30), "zm_associate_dev: n must be 0 .. 2^30 (got %d)", n);
    as_grid g;
    ZM_TRY(as_make_grid("zm_associate_dev", radius_arcsec, n, &g));
    ZM_HIP(hipSetDevice(ctx->device));
    as_host* hs = nullptr;
    ZM_TRY(ctx->get_pinned("as_host", sizeof(as_host), (void**)&hs));
    hs->changed = 0; hs->rounds = 0; hs->capacity = 0; hs->stats = nullptr;
    if (n == 0) {
        ZM_HIP(hipMemsetAsync(nsrc_dev, 0, sizeof(int32_t), ctx->stream));
        ZM_HIP(hipMemsetAsync(offsets_dev, 0, sizeof(int32_t), ctx->stream));
        return 0;
    }
    ZM_CHECK(ra_dev && dec_dev && snr_dev && label_dev && members_dev && best_dev && count_dev && sumrb_dev,
             "zm_associate_dev: null argument");
    const size_t cap = (size_t)g.mask + 1, N = (size_t)n;
    const int nb = zm_div_up(n, AS_SCAN_PER_BLOCK);
    // one slab: vectors, table, labels and the compaction's work arrays
    const size_t o_v = 0, o_keys = o_v + as_up(3 * N * 8), o_head = o_keys + as_up(cap * 8), o_next = o_head + as_up(cap * 4),
                 o_lab = o_next + as_up(N * 4), o_deg = o_lab + as_up(N * 4), o_root = o_deg + as_up(N * 4),
                 o_rank = o_root + as_up(N * 4), o_cur = o_rank + as_up(N * 4), o_mtmp = o_cur + as_up(N * 4),
                 o_bsum = o_mtmp + as_up(N * 4), o_words = o_bsum + as_up((size_t)nb * 4), total = o_words + 256;
    char* w = nullptr;
    ZM_TRY(ctx->get("as_work", total, (void**)&w));
    double* v[3] = {(double*)(w + o_v), (double*)(w + o_v) + N, (double*)(w + o_v) + 2 * N};
    as_u64* keys = (as_u64*)(w + o_keys);
    int *head = (int*)(w + o_head), *next = (int*)(w + o_next), *lab = (int*)(w + o_lab), *deg = (int*)(w + o_deg),
        *isroot = (int*)(w + o_root), *rank = (int*)(w + o_rank), *cursor = (int*)(w + o_cur), *mtmp = (int*)(w + o_mtmp),
        *bsum = (int*)(w + o_bsum);
    as_u64* stats = (as_u64*)(w + o_words);              // [0] probes, [1] longest probe
    int* changed = (int*)(w + o_words + 64);
    const dim3 grid((unsigned)zm_div_up(n, 256)), block(256);
    hs->capacity = (int64_t)cap;
    hs->stats = stats;
    {
        zm_scope_timer timer(ctx, "as_build");
        hipLaunchKernelGGL(k_as_unit, grid, block, 0, ctx->stream, ra_dev, dec_dev, snr_dev, n, v[0], v[1], v[2]);
        ZM_TRY(as_build(ctx, v, n, g, keys, head, next, stats));
        hipLaunchKernelGGL(k_as_iota, grid, block, 0, ctx->stream, lab, n);
        ZM_HIP(hipGetLastError());
    }
    // Rounds are separate launches and the loop ends only after a launch in which no label decreased.  Inside one launch a
    // plain load of lab[] may return a value another workgroup has lowered since (the L2 of an XCD is not coherent with the
    // others', a CU's L1 is never refreshed): it is then a larger label of the same component, and with minima that only
    // ever decrease it costs a round, never an answer - provided `changed` is raised on EVERY atomicMin that asks for a
    // decrease (k_as_round does) and the verdict is read at a launch boundary, where every store has landed.  A launch
    // that raised nothing wrote nothing, so all it read was current: the labels are a fixed point.
    {
        zm_scope_timer timer(ctx, "as_rounds");
        for (int round = 0;; ++round) {
            ZM_CHECK(round <= n, "zm_associate_dev: the labels did not settle in %d rounds", round);
            ZM_HIP(hipMemsetAsync(changed, 0, sizeof(int), ctx->stream));
            if (round == 0)
                hipLaunchKernelGGL(k_as_round<true>, grid, block, 0, ctx->stream, v[0], v[1], v[2], n, g, keys, head, next, lab,
                                   deg, changed);
            else
                hipLaunchKernelGGL(k_as_round<false>, grid, block, 0, ctx->stream, v[0], v[1], v[2], n, g, keys, head, next, lab,
                                   deg, changed);
            ZM_HIP(hipGetLastError());
            ZM_HIP(hipMemcpyAsync(&hs->changed, changed, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            ZM_HIP(hipStreamSynchronize(ctx->stream));
            hs->rounds = round + 1;
            if (!hs->changed) break;
        }
    }
    zm_scope_timer timer(ctx, "as_compact");
    hipLaunchKernelGGL(k_as_roots, grid, block, 0, ctx->stream, lab, deg, n, isroot);
    ZM_TRY(as_scan(ctx, isroot, n, rank, bsum, nsrc_dev));
    ZM_HIP(hipMemsetAsync(count_dev, 0, N * sizeof(int32_t), ctx->stream));
    ZM_HIP(hipMemsetAsync(cursor, 0, N * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_as_label, grid, block, 0, ctx->stream, lab, deg, rank, n, label_dev, count_dev);
    ZM_TRY(as_scan(ctx, count_dev, n, offsets_dev, bsum, offsets_dev + n));      // offsets[k >= nsrc] = members in all
    hipLaunchKernelGGL(k_as_fill, grid, block, 0, ctx->stream, label_dev, offsets_dev, n, cursor, mtmp);
    const int smax = n / 2 + 1;                          // a source has two members or more
    hipLaunchKernelGGL(k_as_sort, dim3((unsigned)std::min(zm_div_up(smax, 4), 8192)), block, 0, ctx->stream, nsrc_dev,
                       offsets_dev, count_dev, mtmp, members_dev);
    hipLaunchKernelGGL(k_as_reduce, dim3((unsigned)std::min(zm_div_up(smax, 256), 4096)), block, 0, ctx->stream, nsrc_dev,
                       offsets_dev, members_dev, snr_dev, rb_dev, best_dev, sumrb_dev);
    ZM_HIP(hipGetLastError());
    return 0;
}

extern "C" int zm_associate(zm_ctx* ctx, int n, const double* ra, const double* dec, const double* snr, const double* rb,
                            double radius_arcsec, int32_t* label, int32_t* nsrc, int32_t* offsets, int32_t* members,
                            int32_t* best, int32_t* count, double* sumrb) {
    ZM_CHECK(ctx && nsrc && offsets, "zm_associate: null argument");
    ZM_CHECK(n >= 0 && n <= (1 << 30), "zm_associate: n must be 0 .. 2^30 (got %d)", n);
    if (n == 0) {
        as_grid g;
        ZM_TRY(as_make_grid("zm_associate", radius_arcsec, 0, &g));
        *nsrc = 0;
        offsets[0] = 0;
        return 0;
    }
    ZM_CHECK(ra && dec && snr && label && members && best && count && sumrb, "zm_associate: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    const size_t o_ra = 0, o_dec = o_ra + as_up(N * 8), o_snr = o_dec + as_up(N * 8), o_rb = o_snr + as_up(N * 8),
                 o_sum = o_rb + as_up(N * 8), o_label = o_sum + as_up(N * 8), o_off = o_label + as_up(N * 4),
                 o_mem = o_off + as_up((N + 1) * 4), o_best = o_mem + as_up(N * 4), o_cnt = o_best + as_up(N * 4),
                 o_ns = o_cnt + as_up(N * 4), total = o_ns + 256;
    char* d = nullptr;
    ZM_TRY(ctx->get("h_as_io", total, (void**)&d));
    ZM_HIP(hipMemcpyAsync(d + o_ra, ra, N * 8, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d + o_dec, dec, N * 8, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d + o_snr, snr, N * 8, hipMemcpyHostToDevice, ctx->stream));
    if (rb) ZM_HIP(hipMemcpyAsync(d + o_rb, rb, N * 8, hipMemcpyHostToDevice, ctx->stream));
    int32_t* offsets_dev = (int32_t*)(d + o_off);
    ZM_TRY(zm_associate_dev(ctx, n, (const double*)(d + o_ra), (const double*)(d + o_dec), (const double*)(d + o_snr),
                            rb ? (const double*)(d + o_rb) : nullptr, radius_arcsec, (int32_t*)(d + o_label),
                            (int32_t*)(d + o_ns), offsets_dev, (int32_t*)(d + o_mem), (int32_t*)(d + o_best),
                            (int32_t*)(d + o_cnt), (double*)(d + o_sum)));
    int32_t tail[2] = {0, 0};                            // nsrc and the number of rows that belong to a source
    ZM_HIP(hipMemcpyAsync(&tail[0], d + o_ns, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(&tail[1], offsets_dev + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(label, d + o_label, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    const size_t ns = (size_t)tail[0], nm = (size_t)tail[1];
    ZM_CHECK(ns <= N / 2 && nm <= N, "zm_associate: %zu sources with %zu members of %d rows", ns, nm, n);
    *nsrc = tail[0];
    ZM_HIP(hipMemcpyAsync(offsets, offsets_dev, (ns + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (ns) {
        ZM_HIP(hipMemcpyAsync(members, d + o_mem, nm * 4, hipMemcpyDeviceToHost, ctx->stream));
        ZM_HIP(hipMemcpyAsync(best, d + o_best, ns * 4, hipMemcpyDeviceToHost, ctx->stream));
        ZM_HIP(hipMemcpyAsync(count, d + o_cnt, ns * 4, hipMemcpyDeviceToHost, ctx->stream));
        ZM_HIP(hipMemcpyAsync(sumrb, d + o_sum, ns * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int zm_crossmatch_dev(zm_ctx* ctx, int n, const double* ra_dev, const double* dec_dev, int m,
                                 const double* cat_ra_dev, const double* cat_dec_dev, double radius_arcsec, int32_t* idx_dev,
                                 double* sep_dev) {
    ZM_CHECK(ctx, "zm_crossmatch_dev: null argument");
    ZM_CHECK(n >= 0 && n <= (1 << 30) && m >= 0 && m <= (1 << 30), "zm_crossmatch_dev: n and m must be 0 .. 2^30 (got %d, %d)", n, m);
    as_grid g;
    ZM_TRY(as_make_grid("zm_crossmatch_dev", radius_arcsec, m, &g));
    ZM_HIP(hipSetDevice(ctx->device));
    as_host* hs = nullptr;
    ZM_TRY(ctx->get_pinned("as_host", sizeof(as_host), (void**)&hs));
    hs->changed = 0; hs->rounds = 0; hs->capacity = 0; hs->stats = nullptr;
    if (n == 0) return 0;
    ZM_CHECK(idx_dev && sep_dev, "zm_crossmatch_dev: null argument");
    if (m == 0) {                                        // nothing to match: -1 (all bits set) and a NaN of all bits set
        ZM_HIP(hipMemsetAsync(idx_dev, 0xff, (size_t)n * 4, ctx->stream));
        ZM_HIP(hipMemsetAsync(sep_dev, 0xff, (size_t)n * 8, ctx->stream));
        return 0;
    }
    ZM_CHECK(ra_dev && dec_dev && cat_ra_dev && cat_dec_dev, "zm_crossmatch_dev: null argument");
    const size_t cap = (size_t)g.mask + 1, M = (size_t)m;
    const size_t o_v = 0, o_keys = o_v + as_up(3 * M * 8), o_head = o_keys + as_up(cap * 8), o_next = o_head + as_up(cap * 4),
                 o_words = o_next + as_up(M * 4), total = o_words + 256;
    char* w = nullptr;
    ZM_TRY(ctx->get("as_work", total, (void**)&w));
    double* v[3] = {(double*)(w + o_v), (double*)(w + o_v) + M, (double*)(w + o_v) + 2 * M};
    as_u64* keys = (as_u64*)(w + o_keys);
    int *head = (int*)(w + o_head), *next = (int*)(w + o_next);
    as_u64* stats = (as_u64*)(w + o_words);
    hs->capacity = (int64_t)cap;
    hs->stats = stats;
    zm_scope_timer timer(ctx, "crossmatch");
    hipLaunchKernelGGL(k_as_unit, dim3((unsigned)zm_div_up(m, 256)), dim3(256), 0, ctx->stream, cat_ra_dev, cat_dec_dev,
                       (const double*)nullptr, m, v[0], v[1], v[2]);
    ZM_TRY(as_build(ctx, v, m, g, keys, head, next, stats));
    hipLaunchKernelGGL(k_xm, dim3((unsigned)zm_div_up(n, 256)), dim3(256), 0, ctx->stream, ra_dev, dec_dev, n, g, keys, head,
                       next, v[0], v[1], v[2], idx_dev, sep_dev);
    ZM_HIP(hipGetLastError());
    return 0;
}

extern "C" int zm_crossmatch(zm_ctx* ctx, int n, const double* ra, const double* dec, int m, const double* cat_ra,
                             const double* cat_dec, double radius_arcsec, int32_t* idx, double* sep) {
    ZM_CHECK(ctx, "zm_crossmatch: null argument");
    ZM_CHECK(n >= 0 && n <= (1 << 30) && m >= 0 && m <= (1 << 30), "zm_crossmatch: n and m must be 0 .. 2^30 (got %d, %d)", n, m);
    as_grid g;
    ZM_TRY(as_make_grid("zm_crossmatch", radius_arcsec, m, &g));
    if (n == 0) return 0;
    ZM_CHECK(ra && dec && idx && sep, "zm_crossmatch: null argument");
    if (m == 0) {
        for (int i = 0; i < n; ++i) { idx[i] = -1; sep[i] = __builtin_nan(""); }
        return 0;
    }
    ZM_CHECK(cat_ra && cat_dec, "zm_crossmatch: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)n, M = (size_t)m;
    const size_t o_ra = 0, o_dec = o_ra + as_up(N * 8), o_cra = o_dec + as_up(N * 8), o_cdec = o_cra + as_up(M * 8),
                 o_sep = o_cdec + as_up(M * 8), o_idx = o_sep + as_up(N * 8), total = o_idx + as_up(N * 4);
    char* d = nullptr;
    ZM_TRY(ctx->get("h_as_io", total, (void**)&d));
    ZM_HIP(hipMemcpyAsync(d + o_ra, ra, N * 8, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d + o_dec, dec, N * 8, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d + o_cra, cat_ra, M * 8, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d + o_cdec, cat_dec, M * 8, hipMemcpyHostToDevice, ctx->stream));
    ZM_TRY(zm_crossmatch_dev(ctx, n, (const double*)(d + o_ra), (const double*)(d + o_dec), m, (const double*)(d + o_cra),
                             (const double*)(d + o_cdec), radius_arcsec, (int32_t*)(d + o_idx), (double*)(d + o_sep)));
    ZM_HIP(hipMemcpyAsync(idx, d + o_idx, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(sep, d + o_sep, N * 8, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int zm_assoc_stats(zm_ctx* ctx, int64_t* out4) {
    ZM_CHECK(ctx && out4, "zm_assoc_stats: null argument");
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    auto hp = ctx->pinned.find("as_host");
    if (hp == ctx->pinned.end()) return 0;               // nothing ran on this context yet
    ZM_HIP(hipSetDevice(ctx->device));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    const as_host* hs = (const as_host*)hp->second.first;
    out4[0] = hs->rounds;
    out4[1] = hs->capacity;
    if (!hs->stats) return 0;
    as_u64 words[2] = {0, 0};
    ZM_HIP(hipMemcpy(words, hs->stats, sizeof(words), hipMemcpyDeviceToHost));
    out4[2] = (int64_t)words[0];
    out4[3] = (int64_t)words[1];
    return 0;
}
