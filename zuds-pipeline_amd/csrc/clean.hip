// The CLEAN pass of the source extraction (CLEAN Y, CLEAN_PARAM of zuds/astromatic/sextractor.conf:25-26), opt-in:
// zm_extract_clean[_dev].  The operator is a chosen convention, stated in DESIGN.md ("CLEAN") and restated in numpy in
// tests/clean_ref.py.
//
// Phases, each a launch of its own on the context's stream (no workgroup ever waits for another one):
//   k_cl_stats    one workgroup per object of the pass before, over its bounding box as k_ex_measure walks it: F (the
//                 same lane-fixed float64 partial sums and fixed-shape reduction), the peak pixel and T, and m, the
//                 minarea-th largest f - t, by rounds of "largest value below the last one, with its multiplicity"
//   (host)        the model of every object, float64, one rounded operation each
//   k_cl_pairs    all pairs, tiled: 256 lanes own one j each, absorbers pass through LDS 256 at a time; distance and
//                 flux order are rejected before any division; every lane keeps its own best (prof, NUMBER): no
//                 cross-lane reduction, no float atomics, the same bits every run
//   k_cl_resolve  every object walks to the root of its chain, bounded by n; integer atomicMin of the merged set's first
//                 index onto the root, integer count of the objects per root.  A walk that reaches its bound sets
//                 ZM_EXTRACT_CLEAN in the status word.
//   k_cl_relabel  label plane -> the merged set's first index, through the map from before CLEAN
//   k_cl_nmerged  NMERGED of the final rows
// The shared stages of extract.hip then number and measure the merged objects.
#include <climits>
#include <cmath>

#include "zm_internal.h"

// every decision is made of single roundings in the order written: no contraction, host or device
#pragma clang fp contract(off)

#define CL_TILE 256

// ---- per-object sums ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cl_wsum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// (value, multiplicity) of the larger value; equal values add up
__device__ __forceinline__ void cl_take(float& v, int& c, float ov, int oc) {
    if (ov > v) { v = ov; c = oc; }
    else if (ov == v) c += oc;
}

// block 256: element e of the row-major bounding box belongs to lane e % 256 (k_ex_measure's walk)
__global__ __launch_bounds__(256) void k_cl_stats(const int* __restrict__ seg, const float* __restrict__ filt,
                                                  const float* __restrict__ sig, int nx, float thr,
                                                  const int* __restrict__ obj, int nobj, int kth,
                                                  double* __restrict__ outF, float* __restrict__ outT,
                                                  float* __restrict__ outM) {
    __shared__ double shs[4];
    __shared__ float shp[4];
    __shared__ int shi[4];
    __shared__ float shv[4];
    __shared__ int shc[4];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (k >= nobj) return;
    const int* o = obj + (size_t)k * EX_OI;
    const int xmin = o[0], xmax = o[1], ymin = o[2], ymax = o[3];
    const int bw = xmax - xmin + 1, bh = ymax - ymin + 1;
    const int total = (bw > 0 && bh > 0) ? bw * bh : 0;
    double s = 0.0;
    float peak = -INFINITY;
    int pidx = INT_MAX;
    for (int e = tid; e < total; e += 256) {
        const int j = e / bw, i = e - j * bw;
        const int p = (ymin + j) * nx + xmin + i;
        if (seg[p] != k + 1) continue;
        const float vf = filt[p];
        s += (double)vf;
        if (vf > peak) { peak = vf; pidx = p; }          // p grows along the walk: the first pixel of a tie stays
    }
    s = cl_wsum(s);
#pragma unroll
    for (int of = 32; of >= 1; of >>= 1) {
        const float op = __shfl_xor(peak, of);
        const int oi = __shfl_xor(pidx, of);
        if (op > peak || (op == peak && oi < pidx)) { peak = op; pidx = oi; }
    }
    if (lane == 0) { shs[wave] = s; shp[wave] = peak; shi[wave] = pidx; }
    __syncthreads();
    if (tid == 0) {
        outF[k] = ((shs[0] + shs[1]) + shs[2]) + shs[3];
        float pk = shp[0];
        int pi = shi[0];
        for (int w = 1; w < 4; ++w)
            if (shp[w] > pk || (shp[w] == pk && shi[w] < pi)) { pk = shp[w]; pi = shi[w]; }
        outT[k] = pi != INT_MAX ? thr * sig[pi] : NAN;
    }
    // the kth largest f - t, ties counted: at most kth rounds, each takes the largest value below the last one
    float last = INFINITY, m = NAN;
    int seen = 0;
    for (int round = 0; round < kth; ++round) {
        float best = -INFINITY;
        int cnt = 0;
        for (int e = tid; e < total; e += 256) {
            const int j = e / bw, i = e - j * bw;
            const int p = (ymin + j) * nx + xmin + i;
            if (seg[p] != k + 1) continue;
            const float d = filt[p] - thr * sig[p];      // two roundings (no contraction in this unit)
            if (d < last) cl_take(best, cnt, d, 1);
        }
#pragma unroll
        for (int of = 32; of >= 1; of >>= 1) {
            const float ov = __shfl_xor(best, of);
            const int oc = __shfl_xor(cnt, of);
            cl_take(best, cnt, ov, oc);
        }
        __syncthreads();                                 // the slots of the round before have been read
        if (lane == 0) { shv[wave] = best; shc[wave] = cnt; }
        __syncthreads();
        best = shv[0]; cnt = shc[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) cl_take(best, cnt, shv[w], shc[w]);
        if (cnt == 0) break;                             // fewer than kth members (the numbering rules it out)
        seen += cnt;
        last = best;
        if (seen >= kth) { m = best; break; }            // uniform over the workgroup: every lane holds the same values
    }
    if (tid == 0) outM[k] = m;
}

// ---- all pairs ------------------------------------------------------------------------------------------------------
struct cl_model {                    // struct of arrays, n entries each (device)
    const double *x, *y, *a, *F, *amp, *alpha, *cxx, *cyy, *cxy;
};

// into[j]: NUMBER of the absorber of j with the largest prof (ties: the smallest NUMBER), 0 for none.  UNIT: beta == 1, the
// default: the profile is a division, and the kernel carries no pow
template <bool UNIT>
__global__ __launch_bounds__(CL_TILE) void k_cl_pairs(cl_model M, const float* __restrict__ mthr, int n, double beta,
                                                      int* __restrict__ into) {
    __shared__ double sx[CL_TILE], sy[CL_TILE], sa[CL_TILE], sF[CL_TILE], samp[CL_TILE], sal[CL_TILE], scxx[CL_TILE],
        scyy[CL_TILE], scxy[CL_TILE];
    const int t = threadIdx.x, j = blockIdx.x * CL_TILE + t;
    const bool live = j < n;
    const double xj = live ? M.x[j] : 0.0, yj = live ? M.y[j] : 0.0, aj = live ? M.a[j] : 0.0, Fj = live ? M.F[j] : 0.0;
    const float mj = live ? mthr[j] : 0.f;
    double bestp = 0.0;
    int besti = 0;
    for (int base = 0; base < n; base += CL_TILE) {
        const int i = base + t;
        __syncthreads();                                 // the tile before has been read
        if (i < n) {
            sx[t] = M.x[i]; sy[t] = M.y[i]; sa[t] = M.a[i]; sF[t] = M.F[i]; samp[t] = M.amp[i]; sal[t] = M.alpha[i];
            scxx[t] = M.cxx[i]; scyy[t] = M.cyy[i]; scxy[t] = M.cxy[i];
        }
        __syncthreads();
        if (!live) continue;
        const int cnt = min(CL_TILE, n - base);
        for (int q = 0; q < cnt; ++q) {                  // every lane reads the same address: LDS broadcasts
            const int ni = base + q;                     // NUMBER - 1
            const double Fi = sF[q];
            if (!(Fi > Fj || (Fi == Fj && ni < j))) continue;
            const double al = sal[q];
            if (!(al > 0.0)) continue;                   // not an absorber (the host writes 0 there)
            const double dx = xj - sx[q], dy = yj - sy[q];
            const double z = 10.0 * (sa[q] + aj);
            if (!(dx * dx + dy * dy < z * z)) continue;
            const double val = 1.0 + al * ((scxx[q] * dx * dx + scyy[q] * dy * dy) + scxy[q] * dx * dy);
            if (!(val > 1.0 && val < 1e10)) continue;
            const double prof = UNIT ? samp[q] / val : samp[q] * pow(val, -beta);
            if (!((float)prof > mj)) continue;
            if (besti == 0 || prof > bestp) { bestp = prof; besti = ni + 1; }   // ni grows: the smallest NUMBER of a tie stays
        }
    }
    if (live) into[j] = besti;
}

// root[j]: NUMBER at the end of j's chain; first index and count of the merged set onto the root
__global__ __launch_bounds__(256) void k_cl_resolve(const int* __restrict__ into, const int* __restrict__ first, int n,
                                                    int* __restrict__ root, int* __restrict__ newfirst,
                                                    int* __restrict__ nmerged, int* __restrict__ status) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int r = j + 1;
    bool done = false;
    for (int it = 0; it <= n; ++it) {
        const int nxt = into[r - 1];
        if (nxt <= 0 || nxt > n) { done = true; break; }
        r = nxt;
    }
    if (!done) { atomicOr(status, ZM_EXTRACT_CLEAN); r = j + 1; }
    root[j] = r;
    atomicMin(newfirst + (r - 1), first[j]);
    atomicAdd(nmerged + (r - 1), 1);
}

__global__ __launch_bounds__(256) void k_cl_fill(int* __restrict__ newfirst, int* __restrict__ nmerged, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    newfirst[j] = INT_MAX;
    nmerged[j] = 0;
}

__global__ __launch_bounds__(256) void k_cl_relabel(const int* __restrict__ seg0, const int* __restrict__ root,
                                                    const int* __restrict__ newfirst, int np, int n,
                                                    int* __restrict__ label) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    const int k = seg0[p];
    if (k <= 0 || k > n) return;
    label[p] = newfirst[root[k - 1] - 1];                // of an untouched object: its own first index, as before
}

// NMERGED of final row k: the count at the root of the object from before CLEAN that holds the row's first pixel
__global__ __launch_bounds__(256) void k_cl_nmerged(const int* __restrict__ obj, int n, const int* __restrict__ seg0,
                                                    const int* __restrict__ root, const int* __restrict__ nmerged, int n0,
                                                    int* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int p = obj[(size_t)k * EX_OI + 7];
    const int pre = p >= 0 ? seg0[p] : 0;
    out[k] = pre > 0 && pre <= n0 ? nmerged[root[pre - 1] - 1] : 0;
}

// ---- host -----------------------------------------------------------------------------------------------------------
extern "C" void zm_clean_params_default(zm_clean_params* p) {
    if (!p) return;
    p->param = 1.0;
}

int zm_cl_check(const zm_clean_params* clean) {
    ZM_CHECK(clean, "zm_extract_clean: null CLEAN parameters");
    ZM_CHECK(std::isfinite(clean->param) && clean->param >= 0.1 && clean->param <= 10.0,
             "zm_extract_clean: bad parameters (param %g: finite, in [0.1, 10])", clean->param);
    return 0;
}

// The model of every object (host, float64, one rounded operation each), then k_cl_pairs and k_cl_resolve.  Leaves
// root / newfirst / nmerged (n ints each) in the scratch slot "cl_ints" and returns their addresses; d_status: a device
// word that takes ZM_EXTRACT_CLEAN.  h_into / h_root: host arrays of n or nullptr.
static int cl_decide(zm_ctx* ctx, int n, const zm_object* rows, const double* F, const float* T, const float* m,
                     const zm_clean_params* clean, int* d_status, int32_t* h_into, int32_t* h_root, int** d_root_out,
                     int** d_newfirst_out, int** d_nmerged_out) {
    const double beta = clean->param;
    std::vector<double> soa((size_t)n * 9);
    std::vector<int> first(n);
    double *x = soa.data(), *y = x + n, *a = y + n, *hF = a + n, *amp = hF + n, *alpha = amp + n, *cxx = alpha + n,
           *cyy = cxx + n, *cxy = cyy + n;
    for (int k = 0; k < n; ++k) {
        const zm_object& r = rows[k];
        const double d = r.x2 * r.y2 - r.xy * r.xy;
        cxx[k] = r.y2 / d;
        cyy[k] = r.x2 / d;
        cxy[k] = -2.0 * r.xy / d;
        const double area = M_PI * r.a_image * r.b_image;
        const double am = F[k] / (2.0 * area);
        const double ratio = am / (double)T[k];
        const double g = beta == 1.0 ? ratio : pow(ratio, 1.0 / beta);
        const double al = (g - 1.0) * area / (double)r.npix;
        const bool ok = std::isfinite(am) && std::isfinite(al) && al > 0.0;
        x[k] = r.x_image; y[k] = r.y_image; a[k] = r.a_image; hF[k] = F[k];
        amp[k] = am;
        alpha[k] = ok ? al : 0.0;                        // 0: not an absorber
        first[k] = r.first;
    }
    char* d_soa = nullptr;
    int* d_ints = nullptr;
    float* d_m = nullptr;
    ZM_TRY(ctx->get("cl_model", (size_t)n * 9 * 8, (void**)&d_soa));
    ZM_TRY(ctx->get("cl_m", (size_t)n * 4, (void**)&d_m));
    ZM_TRY(ctx->get("cl_ints", (size_t)n * 5 * 4, (void**)&d_ints));
    int *d_into = d_ints, *d_first = d_into + n, *d_root = d_first + n, *d_newfirst = d_root + n, *d_nmerged = d_newfirst + n;
    ZM_HIP(hipMemcpyAsync(d_soa, soa.data(), soa.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_m, m, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d_first, first.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    const double* ds = (const double*)d_soa;
    cl_model M = {ds, ds + n, ds + 2 * (size_t)n, ds + 3 * (size_t)n, ds + 4 * (size_t)n, ds + 5 * (size_t)n,
                  ds + 6 * (size_t)n, ds + 7 * (size_t)n, ds + 8 * (size_t)n};
    const int nb = zm_div_up(n, 256);
    hipLaunchKernelGGL(k_cl_fill, dim3(nb), dim3(256), 0, ctx->stream, d_newfirst, d_nmerged, n);
    if (beta == 1.0)
        hipLaunchKernelGGL(k_cl_pairs<true>, dim3(zm_div_up(n, CL_TILE)), dim3(CL_TILE), 0, ctx->stream, M, d_m, n, beta, d_into);
    else
        hipLaunchKernelGGL(k_cl_pairs<false>, dim3(zm_div_up(n, CL_TILE)), dim3(CL_TILE), 0, ctx->stream, M, d_m, n, beta, d_into);
    hipLaunchKernelGGL(k_cl_resolve, dim3(nb), dim3(256), 0, ctx->stream, d_into, d_first, n, d_root, d_newfirst, d_nmerged,
                       d_status);
    ZM_HIP(hipGetLastError());
    if (h_into) ZM_HIP(hipMemcpyAsync(h_into, d_into, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (h_root) ZM_HIP(hipMemcpyAsync(h_root, d_root, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));           // soa, first and the caller's m are free again
    *d_root_out = d_root;
    *d_newfirst_out = d_newfirst;
    *d_nmerged_out = d_nmerged;
    return 0;
}

extern "C" int zm_clean_decide(zm_ctx* ctx, int n, const zm_object* rows, const double* fdflux, const float* dthresh,
                               const float* mthresh, int minarea, const zm_clean_params* clean, int32_t* out_into,
                               int32_t* out_root) {
    ZM_CHECK(ctx && rows && fdflux && dthresh && mthresh, "zm_clean_decide: null argument");
    ZM_TRY(zm_cl_check(clean));
    ZM_CHECK(n >= 1 && n <= (1 << 24) && minarea >= 1, "zm_clean_decide: bad sizes (n %d: 1 .. 2^24; minarea %d)", n, minarea);
    for (int k = 0; k < n; ++k)
        ZM_CHECK(rows[k].number == k + 1 && rows[k].npix >= minarea && rows[k].first >= 0,
                 "zm_clean_decide: row %d has number %d, npix %d, first %d (number = index + 1, npix >= minarea %d, first >= 0)",
                 k, rows[k].number, rows[k].npix, rows[k].first, minarea);
    ZM_HIP(hipSetDevice(ctx->device));
    int *d_status = nullptr, *d_root, *d_newfirst, *d_nmerged;
    ZM_TRY(ctx->get("cl_status", 16, (void**)&d_status));
    ZM_HIP(hipMemsetAsync(d_status, 0, 16, ctx->stream));
    ZM_TRY(cl_decide(ctx, n, rows, fdflux, dthresh, mthresh, clean, d_status, out_into, out_root, &d_root, &d_newfirst,
                     &d_nmerged));
    int st = 0;
    ZM_HIP(hipMemcpyAsync(&st, d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    ZM_CHECK(st == 0, "zm_clean_decide: a chain of absorptions passed its bound of %d steps (status %d)", n, st);
    return 0;
}

extern "C" int zm_extract_clean_stats(zm_ctx* ctx, int max_n, double* fdflux, float* dthresh, float* mthresh, int* out_n) {
    ZM_CHECK(ctx && out_n && max_n >= 0, "zm_extract_clean_stats: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    const int n0 = ctx->cl_npre;
    *out_n = n0;
    const int n = n0 < max_n ? n0 : max_n;
    if (n == 0) return 0;
    char* d = nullptr;
    ZM_TRY(ctx->get("cl_stats", (size_t)n0 * 16, (void**)&d));      // (the slot of the last call: it is not grown here)
    if (fdflux) ZM_HIP(hipMemcpyAsync(fdflux, d, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (dthresh) ZM_HIP(hipMemcpyAsync(dthresh, d + (size_t)n0 * 8, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (mthresh) ZM_HIP(hipMemcpyAsync(mthresh, d + (size_t)n0 * 12, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// The CLEAN stage of zm_ex_first_pass (extract.hip): b->label holds the n0 > 0 objects of the pass before (d_seg1, d_split:
// what zm_db_split left, or nullptr where nothing was deblended).  Numbers and measures that pass in full, decides, and
// where anything is absorbed numbers and measures again; rows, PARENT_NUMBER, NMERGED and the call's counts are final.
int zm_cl_merge(zm_ctx* ctx, const float* img, const float* sigma, const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                const zm_extract_params* params, int cap, const zm_clean_params* clean, int n0, const zm_ex_bufs* b,
                int* d_seg1, int* d_split, zm_object* out_rows, const zm_ex_outs* o, int32_t* out_parent, int32_t* out_nmerged) {
    const int np = b->np, minarea = params->detect_minarea;
    int head[2] = {0, 0};
    // the pass before in full: its map, its table and its rows
    int *d_seg0 = nullptr, *d_obj0 = nullptr;
    char* d_stats = nullptr;
    ZM_TRY(ctx->get("cl_seg0", (size_t)np * 4, (void**)&d_seg0));
    ZM_TRY(ctx->get("cl_obj0", (size_t)(n0 + 1) * EX_OI * 4, (void**)&d_obj0));
    ZM_TRY(ctx->get("cl_stats", (size_t)n0 * 16, (void**)&d_stats));
    double* d_F = (double*)d_stats;
    float *d_T = (float*)(d_stats + (size_t)n0 * 8), *d_M = d_T + n0;
    zm_ex_number(ctx, b->label, img, flag, nx, ny, params, n0, d_seg0, d_obj0, b);
    hipLaunchKernelGGL(k_cl_stats, dim3(n0), dim3(256), 0, ctx->stream, d_seg0, b->filt, sigma, nx, params->detect_thresh, d_obj0,
                       n0, minarea, d_F, d_T, d_M);
    ZM_HIP(hipGetLastError());
    std::vector<zm_object> pre(n0);
    ZM_TRY(zm_ex_rows(ctx, img, sigma, nx, ny, wcs, params, n0, d_seg0, d_obj0, b, pre.data()));
    ctx->cl_npre = n0;
    std::vector<double> hF(n0);
    std::vector<float> hT((size_t)n0 * 2);
    ZM_HIP(hipMemcpyAsync(hF.data(), d_F, (size_t)n0 * 8, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipMemcpyAsync(hT.data(), d_T, (size_t)n0 * 8, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> root(n0);
    int *d_root, *d_newfirst, *d_nmerged;
    ZM_TRY(cl_decide(ctx, n0, pre.data(), hF.data(), hT.data(), hT.data() + n0, clean, b->small, nullptr, root.data(), &d_root,
                     &d_newfirst, &d_nmerged));
    ZM_TRY(zm_ex_head(ctx, b, o, "a chain of absorptions", n0, head));    // (the count is still n0)
    int nabsorbed = 0;
    for (int k = 0; k < n0; ++k) nabsorbed += root[k] != k + 1;
    if (!d_seg1) {                                       // PARENT_NUMBER: the NUMBER of the pass before; nothing was split
        d_seg1 = d_seg0;
        ZM_TRY(ctx->get("db_split", (size_t)n0 * 4, (void**)&d_split));
        ZM_HIP(hipMemsetAsync(d_split, 0, (size_t)n0 * 4, ctx->stream));
    }
    int* d_obj = nullptr;
    int n = 0;
    if (nabsorbed == 0) {
        // nothing is absorbed: the label plane is untouched, map and rows are those of the pass before
        *o->nfound = n0;
        n = n0 < cap ? n0 : cap;
        *o->nwritten = n;
        ZM_HIP(hipMemcpyAsync(b->seg, d_seg0, (size_t)np * 4, hipMemcpyDeviceToDevice, ctx->stream));
        if (n > 0) memcpy(out_rows, pre.data(), (size_t)n * sizeof(zm_object));
        d_obj = d_obj0;
    } else {
        hipLaunchKernelGGL(k_cl_relabel, dim3(zm_div_up(np, 256)), dim3(256), 0, ctx->stream, d_seg0, d_root, d_newfirst, np, n0,
                           b->label);
        ZM_TRY(zm_ex_recount(ctx, b->label, b));
        zm_ex_count_roots(ctx, b->label, minarea, b);
        ZM_TRY(ctx->get("ex_obj", (size_t)(cap + 1) * EX_OI * 4, (void**)&d_obj));
        zm_ex_number(ctx, b->label, img, flag, nx, ny, params, cap, b->seg, d_obj, b);
        ZM_HIP(hipGetLastError());
        // (no kernel since the last read takes the status word: this one cannot fail on it)
        ZM_TRY(zm_ex_head(ctx, b, o, "a chain of absorptions", n0, head, cap));
        n = *o->nwritten;
        if (n > 0) ZM_TRY(zm_ex_rows(ctx, img, sigma, nx, ny, wcs, params, n, b->seg, d_obj, b, out_rows));
    }
    if (n == 0) {
        ZM_HIP(hipStreamSynchronize(ctx->stream));
        return 0;
    }
    ZM_TRY(zm_db_parent(ctx, d_obj, n, d_seg1, d_split, out_rows, out_parent));
    if (out_nmerged) {
        int* d_nm = nullptr;
        ZM_TRY(ctx->get("cl_nm", (size_t)n * 4, (void**)&d_nm));
        hipLaunchKernelGGL(k_cl_nmerged, dim3(zm_div_up(n, 256)), dim3(256), 0, ctx->stream, d_obj, n, d_seg0, d_root, d_nmerged,
                           n0, d_nm);
        ZM_HIP(hipGetLastError());
        ZM_HIP(hipMemcpyAsync(out_nmerged, d_nm, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        ZM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

extern "C" int zm_extract_clean_dev(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                                    const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                                    const zm_extract_params* params, int max_objects, zm_object* out_rows,
                                    int32_t* segm_dev, float* filtered_dev, int* out_nwritten, int* out_nfound,
                                    int* out_status, const zm_deblend_params* deblend, const zm_clean_params* clean,
                                    int32_t* out_parent, int32_t* out_nmerged) {
    ZM_TRY(zm_ex_check(ctx, img, sigma, nx, ny, params, max_objects, out_rows, out_nwritten, out_nfound));
    ZM_TRY(zm_cl_check(clean));
    if (deblend) ZM_TRY(zm_db_check(deblend));
    const zm_ex_outs o = {out_nwritten, out_nfound, out_status, "zm_extract_clean"};
    return zm_ex_first_pass(ctx, img, sigma, bad, flag, nx, ny, wcs, params, max_objects, out_rows, segm_dev, filtered_dev, &o,
                            deblend, clean, out_parent, out_nmerged);
}

extern "C" int zm_extract_clean(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                                const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                                const zm_extract_params* params, int max_objects, zm_object* out_rows,
                                int32_t* out_segm, float* out_filtered, int* out_nwritten, int* out_nfound,
                                int* out_status, const zm_deblend_params* deblend, const zm_clean_params* clean,
                                int32_t* out_parent, int32_t* out_nmerged) {
    ZM_TRY(zm_cl_check(clean));
    return zm_ex_host(ctx, img, sigma, bad, flag, nx, ny, wcs, params, max_objects, out_rows, out_segm, out_filtered,
                      out_nwritten, out_nfound, out_status, deblend, out_parent, clean, out_nmerged);
}
