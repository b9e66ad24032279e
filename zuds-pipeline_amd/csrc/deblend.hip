// Multi-threshold deblending of the extractor's first-pass objects (DEBLEND_NTHRESH / DEBLEND_MINCONT of
// zuds/astromatic/sextractor.conf).  The operator is a chosen convention, stated in DESIGN.md ("Deblending") and restated
// in numpy in tests/deblend_ref.py: integer sums, comparisons and single correctly rounded float64 operations only, so
// that the new label plane is the same bits on every run and in the restatement.
//
//   k_db_tree    one workgroup of four waves per candidate object (at least 2 x DETECT_MINAREA pixels), over the object's
//                bounding box.  Two forms of one body: where the box has at most DB_CELLS pixels, labels, sums and
//                worklists sit in LDS and are indexed by the pixel's place in the box; larger objects use planes in
//                global memory indexed by the pixel's linear index in the frame - a pixel belongs to one object, so
//                workgroups share those planes and never each other's entries.  Either index grows in raster order, so
//                "the smaller index" means the same pixel in both.  No workgroup waits for another.
//                  levels   one byte per pixel: how many of the nthresh - 1 upper thresholds the filtered value exceeds
//                  tree     top down, level by level: the pixels of the level join an incremental union-find (links by
//                           integer atomicMin towards the smaller index, path halving); the roots of the level above
//                           hand their sums (pixels: int32, flux: int64 fixed point) to the root they now hang under
//                           and say whether they were significant; a root with two significant branches turns them
//                           into seeds and clears the seeds of the others
//                  growth   level by level again: the unlabelled pixels next to a labelled one, kept in a worklist,
//                           take the label of the brightest labelled neighbour as it stood at the start of the round;
//                           a list's members carry its stamp and are not queued again while it is written, so a
//                           round labels its whole list and the lists are the same sets on every run
//                  labels   every pixel of a split object gets the smallest linear index of its sub-object, which is
//                           what the numbering kernels of extract.hip expect of a label plane
//   k_db_parent  per final row: the first-pass NUMBER under its first pixel, and whether that object was split
// Every walk along a label chain and every round loop is bounded by the object's pixel count; a bound that is reached
// sets ZM_EXTRACT_DEBLEND in the status word and the call fails.  Numbering and measurement are the kernels of
// extract.hip on the new label plane.
#include <climits>
#include <cmath>

#include "zm_internal.h"

#define DB_MAXN 64
#ifndef DB_CELLS                     // (developer: ZM_HIPCC_FLAGS=-DDB_CELLS=0 sends every object to the global-memory form)
#define DB_CELLS 1024                // box pixels up to which an object's planes sit in LDS (45 KB: three workgroups per CU)
#endif
#define DB_LDS_CELLS (DB_CELLS > 0 ? DB_CELLS : 1)
#define DB_SIG 4                     // acc: += DB_SIG per significant branch; bit 0: a branch carries seeds
#define DB_ANY 1

struct db_cand { int num, woff; };   // first-pass NUMBER; offset of the object's worklists (pixels of earlier candidates)

struct db_planes {                   // one entry per pixel of the frame, or per pixel of the box (LDS form)
    int *parent, *old, *seed;        // union-find; root at the level above, later the worklist stamps; seed label or -1
    int *rn, *acc, *cst;             // per root: pixels; branch accumulator; bit 0 significant, bit 1 carries seeds
    unsigned long long* rq;          // per root: sum of trunc(f 2^(32 - e))
    unsigned char* level;
    int *wa, *wb, *wl;               // two worklists and the labels a round decides on, per candidate at woff
};

__device__ __forceinline__ int db_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void db_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long db_ld64(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int db_ldb(const unsigned char* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of a; parents only ever decrease, and a pixel that has a parent never becomes a root again, so pointing a at its
// grandparent (atomicMin) is safe beside concurrent links.  -1 when the walk passes its bound.
__device__ __forceinline__ int db_find(int* parent, int a, int bound) {
    for (int it = 0; it <= bound; ++it) {
        const int l = db_ld(parent + a);
        if (l == a) return a;
        const int ll = db_ld(parent + l);
        if (ll != l) atomicMin(parent + a, ll);
        a = l;
    }
    return -1;
}

__device__ __forceinline__ void db_union(int* parent, int a, int b, int bound, int* status) {
    for (int it = 0; it <= bound; ++it) {
        a = db_find(parent, a, bound);
        b = db_find(parent, b, bound);
        if (a < 0 || b < 0) break;
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;                                         // a had a parent already: go on with that one and b
    }
    atomicOr(status, ZM_EXTRACT_DEBLEND);
}

// the walk of one lane over the members of the object: element e of the row-major bounding box belongs to lane e % 256
// p: its linear index in the frame; kp: its index in the planes
#define DB_MEMBERS(p, kp)                                                                 \
    for (int e_ = tid; e_ < total; e_ += 256)                                             \
        if (const int p = (ymin + e_ / bw) * nx + xmin + e_ % bw, kp = LDS ? e_ : p; seg1[p] == num)

// the 8 neighbours q of p inside the frame that belong to the object, in ascending linear index
// (a member lies inside the bounding box, so its place in the box is kp + dy * bw + dx)
#define DB_NEIGHBOURS(p, kp, q, kq)                                                                  \
    for (int d_ = 0; d_ < 9; ++d_)                                                                   \
        if (const int xx_ = p % nx + d_ % 3 - 1, yy_ = p / nx + d_ / 3 - 1;                          \
            d_ != 4 && xx_ >= 0 && xx_ < nx && yy_ >= 0 && yy_ < ny)                                 \
            if (const int q = yy_ * nx + xx_, kq = LDS ? kp + (d_ / 3 - 1) * bw + d_ % 3 - 1 : q; seg1[q] == num)

template <bool LDS>
__global__ __launch_bounds__(256) void k_db_tree(const int* __restrict__ seg1, const float* __restrict__ filt,
                                                 const float* __restrict__ sig, int nx, int ny, float thr,
                                                 const int* __restrict__ obj, const db_cand* __restrict__ cand, int nlev,
                                                 int nroots, double mincont, int minarea, db_planes gw,
                                                 int* __restrict__ label, int* __restrict__ split, int* __restrict__ status) {
    __shared__ double u[DB_MAXN];
    __shared__ int hist[DB_MAXN];
    __shared__ float shp[4];
    __shared__ int shi[4];
    __shared__ unsigned long long qtot;
    __shared__ double s_scale, s_back, s_rhs;
    __shared__ int s_cnt[2], s_split;
    __shared__ unsigned long long l_rq[LDS ? DB_LDS_CELLS : 1];
    __shared__ int l_int[LDS ? 9 * DB_LDS_CELLS : 1];
    __shared__ unsigned char l_level[LDS ? DB_LDS_CELLS : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const db_cand c = cand[blockIdx.x];
    const int num = c.num;
    const int* o = obj + (size_t)(num - 1) * EX_OI;
    const int xmin = o[0], ymin = o[2], npix = o[4], root = o[7];
    const int bw = o[1] - xmin + 1, bh = o[3] - ymin + 1;
    const int total = (bw > 0 && bh > 0) ? bw * bh : 0;
    const int bound = npix + 8;
    db_planes w = gw;
    if (LDS) {
        w.rq = l_rq; w.level = l_level;
        w.parent = l_int; w.old = l_int + DB_CELLS; w.seed = l_int + 2 * DB_CELLS; w.rn = l_int + 3 * DB_CELLS;
        w.acc = l_int + 4 * DB_CELLS; w.cst = l_int + 5 * DB_CELLS;
        w.wa = l_int + 6 * DB_CELLS; w.wb = l_int + 7 * DB_CELLS; w.wl = l_int + 8 * DB_CELLS;
    } else {
        w.wa += c.woff; w.wb += c.woff; w.wl += c.woff;
    }
    const int kroot = !LDS || root < 0 ? root : (root / nx - ymin) * bw + root % nx - xmin;

    // ---- the peak, its threshold, the levels -------------------------------------------------------------------------
    float peak = -INFINITY;
    int pidx = INT_MAX;
    DB_MEMBERS(p, kp) {
        const float vf = filt[p];
        if (vf > peak) { peak = vf; pidx = p; }          // p grows along the walk: the first pixel of a tie stays
    }
#pragma unroll
    for (int of = 32; of >= 1; of >>= 1) {
        const float op = __shfl_xor(peak, of);
        const int oi = __shfl_xor(pidx, of);
        if (op > peak || (op == peak && oi < pidx)) { peak = op; pidx = oi; }
    }
    if (lane == 0) { shp[wave] = peak; shi[wave] = pidx; }
    if (tid < DB_MAXN) hist[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        float pk = shp[0];
        int pi = shi[0];
        for (int k = 1; k < 4; ++k)
            if (shp[k] > pk || (shp[k] == pk && shi[k] < pi)) { pk = shp[k]; pi = shi[k]; }
        const double T = pi != INT_MAX ? (double)(thr * sig[pi]) : 1.0, P = pi != INT_MAX ? (double)pk : 1.0;
        double g = __ddiv_rn(P, T);
        for (int r = 0; r < nroots; ++r) g = __dsqrt_rn(g);
        double ek = 1.0;
        u[0] = __dmul_rn(T, ek);
        for (int k = 1; k < nlev; ++k) {
            ek = __dmul_rn(ek, g);
            u[k] = __dmul_rn(T, ek);
        }
        int ex = 0;
        (void)frexp(P, &ex);
        s_scale = ldexp(1.0, 32 - ex);
        s_back = ldexp(1.0, ex - 32);
        qtot = 0ull;
        s_cnt[0] = s_cnt[1] = 0;
    }
    __syncthreads();
    {
        unsigned long long qs = 0ull;
        const double scale = s_scale;
        DB_MEMBERS(p, kp) {
            const double dv = (double)filt[p];
            int L = 0;
            for (int k = 1; k < nlev; ++k) L += dv > u[k] ? 1 : 0;
            w.level[kp] = (unsigned char)L;
            qs += (unsigned long long)(long long)__dmul_rn(dv, scale);
            db_st(w.parent + kp, kp);
            db_st(w.old + kp, kp);
            db_st(w.seed + kp, -1);
            db_st(w.rn + kp, 0);
            db_st(w.acc + kp, 0);
            db_st(w.cst + kp, 0);
            w.rq[kp] = 0ull;
            atomicAdd(&hist[L], 1);
        }
        if (qs) atomicAdd(&qtot, qs);
    }
    __syncthreads();
    if (tid == 0) s_rhs = __dmul_rn(mincont, __dmul_rn((double)(long long)qtot, s_back));
    __syncthreads();

    // ---- the tree, top down ------------------------------------------------------------------------------------------
    for (int k = nlev - 1; k >= 0; --k) {
        if (hist[k] == 0) continue;                      // the nodes of this level are those of the level above
        int kb = -1;                                     // the next level below that has pixels of its own
        for (int j = k - 1; j >= 0; --j)
            if (hist[j]) { kb = j; break; }
        DB_MEMBERS(p, kp) {
            if (db_ldb(w.level + kp) != k) continue;
            DB_NEIGHBOURS(p, kp, q, kq) {
                if (db_ldb(w.level + kq) >= k) db_union(w.parent, kp, kq, bound, status);
            }
        }
        __syncthreads();
        DB_MEMBERS(p, kp) {
            const int lv = db_ldb(w.level + kp);
            if (lv < k) continue;
            const int r = db_find(w.parent, kp, bound);
            if (r < 0) { atomicOr(status, ZM_EXTRACT_DEBLEND); continue; }
            if (r != kp) atomicMin(w.parent + kp, r);
            if (lv == k) {
                atomicAdd(w.rn + r, 1);
                atomicAdd(w.rq + r, (unsigned long long)(long long)__dmul_rn((double)filt[p], s_scale));
            } else if (db_ld(w.old + kp) == kp) {        // a root of the level above: a branch of r
                const int cs = db_ld(w.cst + kp);
                if (r != kp) {
                    atomicAdd(w.rn + r, db_ld(w.rn + kp));
                    atomicAdd(w.rq + r, db_ld64(w.rq + kp));
                }
                if (cs & 1) atomicAdd(w.acc + r, DB_SIG);
                if (cs & 2) atomicOr(w.acc + r, DB_ANY);
            }
        }
        __syncthreads();
        DB_MEMBERS(p, kp) {
            const int lv = db_ldb(w.level + kp);
            if (lv < k) continue;
            const int r = db_ld(w.parent + kp);
            if (lv > k && db_ld(w.acc + r) / DB_SIG >= 2) {
                const int b = db_ld(w.old + kp), cs = db_ld(w.cst + b);
                if (!(cs & 1)) db_st(w.seed + kp, -1);   // not significant: its earlier splits are dropped
                else if (!(cs & 2)) db_st(w.seed + kp, b);  // significant and unsplit: the branch is a seed
            }
            db_st(w.old + kp, r);
        }
        __syncthreads();
        DB_MEMBERS(p, kp) {
            if (db_ldb(w.level + kp) < k || db_ld(w.parent + kp) != kp) continue;
            const int n = db_ld(w.rn + kp), a = db_ld(w.acc + kp);
            int cs = (a / DB_SIG >= 2 || (a & DB_ANY)) ? 2 : 0;
            if (kb >= 0 && n >= minarea) {               // as a branch of a node of level kb it is a node of level kb + 1
                const double F = __dmul_rn((double)(long long)db_ld64(w.rq + kp), s_back);
                if (__dsub_rn(F, __dmul_rn(u[kb + 1], (double)n)) > s_rhs) cs |= 1;
            }
            db_st(w.cst + kp, cs);
            db_st(w.acc + kp, 0);
        }
        __syncthreads();
    }
    if (tid == 0) s_split = (kroot >= 0 && (db_ld(w.cst + kroot) & 2)) ? 1 : 0;
    __syncthreads();
    if (!s_split) return;

    // ---- leftover pixels ---------------------------------------------------------------------------------------------
    DB_MEMBERS(p, kp) db_st(w.old + kp, 0);
    __syncthreads();
    int *wa = w.wa, *wb = w.wb, *wl = w.wl;
    int stamp = 0, rounds = 0, cur = 0;
    bool spun = false;
    for (int k = nlev - 1; k >= 0 && !spun; --k) {
        if (hist[k] == 0) continue;
        ++stamp;                                         // the members of a worklist carry the stamp of the pass that made it
        DB_MEMBERS(p, kp) {
            if (db_ldb(w.level + kp) < k || db_ld(w.seed + kp) >= 0) continue;
            bool near = false;
            DB_NEIGHBOURS(p, kp, q, kq) near = near || db_ld(w.seed + kq) >= 0;
            if (near) {
                db_st(w.old + kp, stamp);
                wa[atomicAdd(&s_cnt[cur], 1)] = kp;
            }
        }
        __syncthreads();
        int n = s_cnt[cur];
        __syncthreads();                                 // every lane holds n before the slot is written again
        while (n) {
            if (++rounds > bound) { spun = true; break; }
            ++stamp;
            // every member of the list is unlabelled and has a labelled neighbour: each round labels its whole list
            for (int i = tid; i < n; i += 256) {
                const int kp = wa[i], p = LDS ? (ymin + kp / bw) * nx + xmin + kp % bw : kp;
                int bl = -1;
                float bf = 0.f;
                DB_NEIGHBOURS(p, kp, q, kq) {
                    const int sq = db_ld(w.seed + kq);
                    if (sq < 0) continue;
                    const float fq = filt[q];
                    if (bl < 0 || fq > bf) { bf = fq; bl = sq; }   // q grows: the first neighbour of a tie stays
                }
                wl[i] = bl;
            }
            __syncthreads();
            for (int i = tid; i < n; i += 256) {
                const int kp = wa[i], l = wl[i], p = LDS ? (ymin + kp / bw) * nx + xmin + kp % bw : kp;
                if (l < 0) continue;
                db_st(w.seed + kp, l);
                DB_NEIGHBOURS(p, kp, q, kq) {
                    // a member of this round's list (stamp - 1) is being labelled now, whatever its seed reads as
                    if (db_ldb(w.level + kq) < k || db_ld(w.old + kq) == stamp - 1 || db_ld(w.seed + kq) >= 0) continue;
                    if (atomicExch(w.old + kq, stamp) != stamp) wb[atomicAdd(&s_cnt[cur ^ 1], 1)] = kq;
                }
            }
            __syncthreads();
            n = s_cnt[cur ^ 1];
            if (tid == 0) s_cnt[cur] = 0;                // (every lane read this slot before the barrier above)
            cur ^= 1;
            int* t = wa; wa = wb; wb = t;
            __syncthreads();                             // every lane holds the next n before its slot is written again
        }
    }
    if (spun) {
        if (tid == 0) atomicOr(status, ZM_EXTRACT_DEBLEND);
        return;
    }

    // ---- the label plane: the smallest linear index of every sub-object -------------------------------------------
    DB_MEMBERS(p, kp) db_st(w.parent + kp, INT_MAX);
    __syncthreads();
    DB_MEMBERS(p, kp) {
        const int s = db_ld(w.seed + kp);
        if (s < 0) { atomicOr(status, ZM_EXTRACT_DEBLEND); continue; }
        atomicMin(w.parent + s, p);
    }
    __syncthreads();
    DB_MEMBERS(p, kp) {
        const int s = db_ld(w.seed + kp);
        if (s >= 0) label[p] = db_ld(w.parent + s);
    }
    if (tid == 0) split[num - 1] = 1;
}

__global__ __launch_bounds__(256) void k_db_parent(const int* __restrict__ obj, int n, const int* __restrict__ seg1,
                                                   const int* __restrict__ split, int* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int p = obj[(size_t)k * EX_OI + 7];
    const int par = p >= 0 ? seg1[p] : 0;
    out[k] = par;
    out[n + k] = par > 0 ? split[par - 1] : 0;
}

// ---- host -----------------------------------------------------------------------------------------------------------
extern "C" void zm_deblend_params_default(zm_deblend_params* p) {
    if (!p) return;
    p->nthresh = 32;
    p->pad_ = 0;
    p->mincont = 0.005;
}

// The split stage: numbers the first pass in full (n1 > 0 objects: map and table of their own), splits every object that
// can split, writes the new roots into b->label and leaves pixels per root and the number of objects in b->cnt / b->small[1].
int zm_db_split(zm_ctx* ctx, const float* img, const float* sigma, const int32_t* flag, int nx, int ny,
                const zm_extract_params* params, const zm_deblend_params* deblend, int n1, const zm_ex_bufs* b, int** out_seg1,
                int** out_split) {
    const int np = b->np, minarea = params->detect_minarea, N = deblend->nthresh;
    int nroots = 0;
    while ((1 << nroots) < N) ++nroots;
    int *d_seg1 = nullptr, *d_obj1 = nullptr, *d_split = nullptr;
    // the first pass in full: its map and its table, every object of it
    ZM_TRY(ctx->get("db_seg1", (size_t)np * 4, (void**)&d_seg1));
    ZM_TRY(ctx->get("db_obj1", (size_t)(n1 + 1) * EX_OI * 4, (void**)&d_obj1));
    ZM_TRY(ctx->get("db_split", (size_t)n1 * 4, (void**)&d_split));
    zm_ex_number(ctx, b->label, img, flag, nx, ny, params, n1, d_seg1, d_obj1, b);
    ZM_HIP(hipMemsetAsync(d_split, 0, (size_t)n1 * 4, ctx->stream));
    std::vector<int> oi((size_t)n1 * EX_OI);
    ZM_HIP(hipMemcpyAsync(oi.data(), d_obj1, oi.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<db_cand> small, large;               // by the size of the bounding box: planes in LDS / in global memory
    size_t wtotal = 0;
    for (int k = 0; k < n1; ++k) {
        const int* o = oi.data() + (size_t)k * EX_OI;
        if (o[4] < 2 * minarea) continue;            // two seeds take 2 x minarea pixels: it cannot split
        if ((int64_t)(o[1] - o[0] + 1) * (o[3] - o[2] + 1) <= DB_CELLS) {
            small.push_back({k + 1, 0});
        } else {
            large.push_back({k + 1, (int)wtotal});
            wtotal += (size_t)o[4];
        }
    }
    if (!small.empty() || !large.empty()) {
        db_cand* d_cand = nullptr;
        ZM_TRY(ctx->get("db_cand", (small.size() + large.size()) * sizeof(db_cand), (void**)&d_cand));
        db_planes w = {};
        if (!small.empty()) {
            ZM_HIP(hipMemcpyAsync(d_cand, small.data(), small.size() * sizeof(db_cand), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_db_tree<true>, dim3((unsigned)small.size()), dim3(256), 0, ctx->stream, d_seg1, b->filt, sigma,
                               nx, ny, params->detect_thresh, d_obj1, d_cand, N, nroots, deblend->mincont, minarea, w, b->label,
                               d_split, b->small);
        }
        if (!large.empty()) {
            char* d_p = nullptr;
            int* d_work = nullptr;
            db_cand* d_large = d_cand + small.size();
            ZM_TRY(ctx->get("db_planes", (size_t)np * (6 * 4 + 8 + 1) + 64, (void**)&d_p));
            ZM_TRY(ctx->get("db_work", wtotal * 3 * 4, (void**)&d_work));
            w.rq = (unsigned long long*)d_p;
            w.parent = (int*)(w.rq + np);
            w.old = w.parent + np; w.seed = w.old + np; w.rn = w.seed + np; w.acc = w.rn + np; w.cst = w.acc + np;
            w.level = (unsigned char*)(w.cst + np);
            w.wa = d_work; w.wb = d_work + wtotal; w.wl = d_work + 2 * wtotal;
            ZM_HIP(hipMemcpyAsync(d_large, large.data(), large.size() * sizeof(db_cand), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_db_tree<false>, dim3((unsigned)large.size()), dim3(256), 0, ctx->stream, d_seg1, b->filt, sigma,
                               nx, ny, params->detect_thresh, d_obj1, d_large, N, nroots, deblend->mincont, minarea, w,
                               b->label, d_split, b->small);
        }
        ZM_HIP(hipGetLastError());
    }
    ZM_TRY(zm_ex_recount(ctx, b->label, b));
    zm_ex_count_roots(ctx, b->label, minarea, b);
    *out_seg1 = d_seg1;
    *out_split = d_split;
    return 0;
}

// PARENT_NUMBER and FLAGS bit 2 of rows 0 .. n - 1 (k_db_parent)
int zm_db_parent(zm_ctx* ctx, const int* d_obj, int n, const int* d_seg1, const int* d_split, zm_object* out_rows,
                 int32_t* out_parent) {
    int* d_par = nullptr;
    ZM_TRY(ctx->get("db_par", (size_t)n * 2 * 4, (void**)&d_par));
    hipLaunchKernelGGL(k_db_parent, dim3(zm_div_up(n, 256)), dim3(256), 0, ctx->stream, d_obj, n, d_seg1, d_split, d_par);
    ZM_HIP(hipGetLastError());
    std::vector<int> par((size_t)n * 2);
    ZM_HIP(hipMemcpyAsync(par.data(), d_par, par.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; ++k) {
        if (par[n + k]) out_rows[k].flags |= 2;          // a sub-object of a split parent
        if (out_parent) out_parent[k] = par[k];
    }
    return 0;
}

int zm_db_check(const zm_deblend_params* deblend) {
    ZM_CHECK(deblend, "zm_extract_deblend: null deblending parameters");
    const int N = deblend->nthresh;
    ZM_CHECK(N >= 2 && N <= DB_MAXN && (N & (N - 1)) == 0 && deblend->mincont >= 0.0 && deblend->mincont <= 1.0,
             "zm_extract_deblend: bad parameters (nthresh %d: a power of two in 2 .. 64; mincont %g: in [0, 1])", N,
             deblend->mincont);
    return 0;
}

extern "C" int zm_extract_deblend_dev(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                                      const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                                      const zm_extract_params* params, int max_objects, zm_object* out_rows,
                                      int32_t* segm_dev, float* filtered_dev, int* out_nwritten, int* out_nfound,
                                      int* out_status, const zm_deblend_params* deblend, int32_t* out_parent) {
    ZM_TRY(zm_ex_check(ctx, img, sigma, nx, ny, params, max_objects, out_rows, out_nwritten, out_nfound));
    ZM_TRY(zm_db_check(deblend));
    const zm_ex_outs o = {out_nwritten, out_nfound, out_status, "zm_extract_deblend"};
    return zm_ex_first_pass(ctx, img, sigma, bad, flag, nx, ny, wcs, params, max_objects, out_rows, segm_dev, filtered_dev, &o,
                            deblend, nullptr, out_parent, nullptr);
}

extern "C" int zm_extract_deblend(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                                  const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                                  const zm_extract_params* params, int max_objects, zm_object* out_rows,
                                  int32_t* out_segm, float* out_filtered, int* out_nwritten, int* out_nfound,
                                  int* out_status, const zm_deblend_params* deblend, int32_t* out_parent) {
    ZM_CHECK(deblend, "zm_extract_deblend: null deblending parameters");
    return zm_ex_host(ctx, img, sigma, bad, flag, nx, ny, wcs, params, max_objects, out_rows, out_segm, out_filtered,
                      out_nwritten, out_nfound, out_status, deblend, out_parent);
}
