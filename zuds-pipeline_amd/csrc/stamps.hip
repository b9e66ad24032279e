// Detection thumbnails on gfx950: S x S stamps of one or more planes on a target grid, resampling only the output tiles
// the stamps touch.
//
// Replaces the two whole-frame SWarp runs + Cutout2D per subtraction of the reference's thumbnail step
// (scripts/dosub.py:133-150 -> zuds/thumbnails.py:54-94,133-146: sub.aligned_to(ref), sci.aligned_to(ref), then at most
// 50 cutouts of 63 x 63 pixels each) and the norms of make_triplet_for_braai (zuds/filterobjects.py:36-54).
// The operator is stated in DESIGN.md ("Detection thumbnails").
//
// Why tiles: k_resample (resample.hip) interpolates its positions in float32 relative to the input box of the 64 x 32
// output tile a pixel belongs to, so a stamp pixel has the bits of zm_resample_dev only when it is computed as part of
// that tile: same lattice nodes, same header (rs_build_header), same tap table, same tap order.  The work items of
// k_stamp_resample are therefore (stamp, plane, tile) triples - the tiles of the grid's partition that the stamp
// intersects - and the per-pixel body below restates the one of k_resample<KIND, 0> operation for operation
// (tests/test_stamps_gpu.py compares the two bit for bit; k_resample itself is untouched).
//
//   k_stamp_fill      per (stamp, plane): a plane already on the grid is gathered (values untouched, 0 outside the grid);
//                     of a resampled plane only the pixels outside the grid are written (0)
//   k_stamp_resample  per item: header, the tile's input box staged from the RAW plane through prep_pixel (no weights, no
//                     background: what k_prep writes for zm_resample_dev(img, NULL, NULL, ...)), then the tile pixels that
//                     lie inside the stamp.  A box beyond the LDS tile (use_lds == 0) gathers from global memory, as there.
//   k_stamp_norm      per (stamp, plane): L2 norm of the block, squares summed in float64 in a lane-fixed order
//
// Every in-grid stamp pixel belongs to exactly one tile, every other one to k_stamp_fill: each output word is written
// once, no atomics, no workgroup waits for another.
#include "resample_dev.h"

struct st_plane {                    // one source plane (device memory)
    const float* img;
    const double2* lat;              // lattice of (grid -> plane); NULL when on_grid
    int nx, ny, lds_cap, on_grid;
    float fscale;
    int vec_ok;                      // rows of `img` can be read as aligned float4
};
struct st_item { int stamp, plane, tile, pad_; };

__global__ __launch_bounds__(256) void k_stamp_fill(const st_plane* __restrict__ planes, int nplanes,
                                                    const int* __restrict__ x0s, const int* __restrict__ y0s, int S,
                                                    int onx, int ony, float* __restrict__ out) {
    const int k = blockIdx.x / nplanes, p = blockIdx.x - k * nplanes;
    const st_plane P = planes[p];
    const int x0 = x0s[k], y0 = y0s[k];
    float* o = out + (size_t)blockIdx.x * S * S;
    for (int e = threadIdx.x; e < S * S; e += 256) {
        const int j = e / S, i = e - j * S;
        const long long gx = (long long)x0 + i, gy = (long long)y0 + j;
        const bool in = gx >= 0 && gx < onx && gy >= 0 && gy < ony;
        if (P.on_grid)
            o[e] = in ? P.img[(size_t)gy * onx + gx] : 0.f;
        else if (!in)
            o[e] = 0.f;
    }
}

#define ST_PF 4                      // staged pixel quads per thread: 4 x 256 x 4 = 4096 pixels >= RS_PFCAP, the largest LDS box
static_assert(ST_PF * 256 * 4 >= RS_PFCAP, "the staging slots must cover the largest box k_resample stages");

template <int KIND>
__global__ __launch_bounds__(256) void k_stamp_resample(const st_plane* __restrict__ planes, int nplanes,
                                                        const st_item* __restrict__ items,
                                                        const int* __restrict__ x0s, const int* __restrict__ y0s, int S,
                                                        int lnx, int lny, int onx, int ony, int ntx,
                                                        const float* __restrict__ taptab, float* __restrict__ out) {
    extern __shared__ float4 smem4[];
    rs_hdr* H = reinterpret_cast<rs_hdr*>(smem4);
    constexpr int TABF = (KIND == ZM_RESAMPLE_LANCZOS3) ? LZ_FLOATS : 0;
    const float* ltab = reinterpret_cast<const float*>(smem4) + HDR_FLOATS;
    float2* tile = reinterpret_cast<float2*>(smem4) + (HDR_FLOATS + TABF) / 2;
    constexpr int NT = taps_traits<KIND>::N;
    constexpr int OFF = taps_traits<KIND>::OFF;
    constexpr int CI = -OFF;
    const int tid = threadIdx.x;
    const st_item it = items[blockIdx.x];
    const st_plane P = planes[it.plane];
    const float* __restrict__ img = P.img;
    const int nx = P.nx, ny = P.ny;
    const float fscale = P.fscale;
    const int sx0 = x0s[it.stamp], sy0 = y0s[it.stamp];
    float* __restrict__ o = out + ((size_t)it.stamp * nplanes + it.plane) * S * S;

    if (KIND == ZM_RESAMPLE_LANCZOS3) {
        for (int e = tid; e < LZ_FLOATS / 4; e += 256)
            smem4[HDR_FLOATS / 4 + e] = reinterpret_cast<const float4*>(taptab)[e];
    }
    if (tid < 64) rs_build_header<KIND>(P.lat, lnx, lny, it.tile, ntx, nx, ny, P.lds_cap, H);
    __syncthreads();
    const bool use_lds = H->use_lds, touches = H->touches;
    const int bx0 = H->h.bx0, by0 = H->h.by0, bw = H->h.bw, bh = H->h.bh;
    if (use_lds) {
        // the box starts on a multiple of 4 pixels and is a multiple of 4 wide: one pixel quad per thread and slot,
        // the loads of all slots first; pixels off the frame enter as k_resample's fill {0, BIGVAR}
        const int bw4 = bw >> 2, n4 = bw4 * bh;
        float v[ST_PF][4];
        bool in[ST_PF][4];
#pragma unroll
        for (int k = 0; k < ST_PF; ++k) {
            const int e = tid + 256 * k;
            const int r = e / bw4, c4 = e - r * bw4;
            const int gy = by0 + r, gx = bx0 + 4 * c4;
            const bool row = e < n4 && gy >= 0 && gy < ny;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                in[k][c] = row && gx + c >= 0 && gx + c < nx;
                v[k][c] = 0.f;
            }
            if (P.vec_ok && row && gx >= 0 && gx + 3 < nx) {
                const float4 a = *reinterpret_cast<const float4*>(img + (size_t)gy * nx + gx);
                v[k][0] = a.x; v[k][1] = a.y; v[k][2] = a.z; v[k][3] = a.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (in[k][c]) v[k][c] = img[(size_t)gy * nx + gx + c];
            }
        }
#pragma unroll
        for (int k = 0; k < ST_PF; ++k) {
            const int e = tid + 256 * k;
            if (e < n4) {
                float2 p[4];
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    p[c] = in[k][c] ? prep_pixel(v[k][c], 1.f, false, 0.f, 1.0f, 1e-30f) : make_float2(0.f, ZM_BIGVAR);
                float4* d4 = reinterpret_cast<float4*>(tile + 4 * e);          // rows are bw = 4 bw4 wide: linear
                d4[0] = make_float4(p[0].x, p[0].y, p[1].x, p[1].y);
                d4[1] = make_float4(p[2].x, p[2].y, p[3].x, p[3].y);
            }
        }
    }
    __syncthreads();

    const int tyi = it.tile / ntx, txi = it.tile - tyi * ntx;
    const int ox0 = txi * TW, oy0 = tyi * RTH;
    const int tx = tid & 63, tyb = tid >> 6;
    const int ox = ox0 + tx;
    // (from here to the store: the body of k_resample<KIND, 0> without a pair plane, operation for operation)
    float xr[3], yr[3];
    {
        const int cell = tx >> 4;
        const float fx = (float)(tx & 15) * (1.f / LSTEP);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float x0 = H->h.nrel[r][cell][0], x1 = H->h.nrel[r][cell + 1][0];
            const float y0 = H->h.nrel[r][cell][1], y1 = H->h.nrel[r][cell + 1][1];
            xr[r] = x0 + fx * (x1 - x0);
            yr[r] = y0 + fx * (y1 - y0);
        }
    }
#pragma unroll 1
    for (int q = 0; q < RTH / 4; ++q) {
        const int ty = tyb + 4 * q;
        const int oy = oy0 + ty;
        if (ox >= onx || oy >= ony) continue;
        const int si = ox - sx0, sj = oy - sy0;               // position in the stamp
        if (si < 0 || si >= S || sj < 0 || sj >= S) continue;
        const int cr = q >> 2;
        const float fy = (float)(ty & 15) * (1.f / LSTEP);
        const float xa = cr ? xr[1] : xr[0], xb = cr ? xr[2] : xr[1];
        const float ya = cr ? yr[1] : yr[0], yb = cr ? yr[2] : yr[1];
        const float px = xa + fy * (xb - xa), py = ya + fy * (yb - ya);
        int ixr, iyr;
        float dx, dy;
        bool ddx, ddy;
        split_pos(px, &ixr, &dx, &ddx);
        split_pos(py, &iyr, &dy, &ddy);
        const int ix = bx0 + ixr + OFF, iy = by0 + iyr + OFF;
        const bool inbx = ddx ? (ix + CI >= 0 && ix + CI < nx) : (ix >= 0 && ix + NT <= nx);
        const bool inby = ddy ? (iy + CI >= 0 && iy + CI < ny) : (iy >= 0 && iy + NT <= ny);
        const bool inb = touches && inbx && inby;
        float res = 0.f;
        if (inb) {
            zm_v2f tw[NT];
            float acc = 0.f, vacc = 0.f;
            if (KIND == ZM_RESAMPLE_LANCZOS3) {
                zm_v2f txp[3], typ[3];
                zm_lz3_lookup(ltab, ddx ? 0.5f : dx, txp);
                zm_lz3_lookup(ltab, ddy ? 0.5f : dy, typ);
                if (ddx || ddy) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const zm_v2f dl = (zm_v2f){j == 1 ? 1.f : 0.f, 0.f};
                        txp[j] = ddx ? dl : txp[j];
                        typ[j] = ddy ? dl : typ[j];
                    }
                }
#pragma unroll
                for (int k = 0; k < NT; ++k)
                    tw[k] = (zm_v2f){(k & 1) ? txp[k >> 1].y : txp[k >> 1].x,
                                     (k & 1) ? typ[k >> 1].y : typ[k >> 1].x};
            } else {
                tw[0] = (zm_v2f){1.f - dx, 1.f - dy};
                tw[1] = (zm_v2f){dx, dy};
            }
            if (use_lds) {
                const float2* p = tile + (iyr + OFF) * bw + (ixr + OFF);
                zm_v2f av = (zm_v2f){0.f, 0.f};
#pragma unroll
                for (int r = 0; r < NT; ++r) {
                    float2 s[NT];
                    lds_row<NT>::read(p, s);
                    zm_v2f rv2 = (zm_v2f){0.f, 0.f};
#pragma unroll
                    for (int c = 0; c < NT; ++c)
                        rv2 = __builtin_elementwise_fma((zm_v2f){tw[c].x, tw[c].x}, (zm_v2f){s[c].x, s[c].y}, rv2);
                    av = __builtin_elementwise_fma((zm_v2f){tw[r].y, tw[r].y}, rv2, av);
                    p += bw;
                }
                acc = av.x;
                vacc = av.y;
            } else {
                const float* p = img + (size_t)iy * nx + ix;
#pragma unroll
                for (int r = 0; r < NT; ++r) {
                    float ra = 0.f, rv = 0.f;
                    // (zero taps of a delta axis may lie off the frame: not read)
                    if (tw[r].y != 0.f) {
#pragma unroll
                        for (int c = 0; c < NT; ++c) {
                            if (tw[c].x != 0.f) {
                                const float2 s = prep_pixel(p[c], 1.f, false, 0.f, 1.0f, 1e-30f);
                                ra = fmaf(tw[c].x, s.x, ra);
                                rv = fmaf(tw[c].x, s.y, rv);
                            }
                        }
                    }
                    acc = fmaf(tw[r].y, ra, acc);
                    vacc = fmaf(tw[r].y, rv, vacc);
                    p += nx;
                }
            }
            if (vacc > 0.f && vacc < ZM_BADVAR_TEST) res = acc * fscale;
        }
        o[(size_t)sj * S + si] = res;
    }
}

// the order of tests/extract_ref.py's sums: element e belongs to lane e % 256, waves by xor-tree, then ((w0 + w1) + w2) + w3
__global__ __launch_bounds__(256) void k_stamp_norm(const float* __restrict__ out, int S, double* __restrict__ norm) {
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* o = out + (size_t)blockIdx.x * S * S;
    double s = 0.0;
    for (int e = tid; e < S * S; e += 256) {
        const double v = (double)o[e];
        s += v * v;                                       // (the square of a float is exact in float64)
    }
#pragma unroll
    for (int of = 32; of >= 1; of >>= 1) s += __shfl_xor(s, of);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    if (tid == 0) norm[blockIdx.x] = sqrt(((sh[0] + sh[1]) + sh[2]) + sh[3]);
}

// ---- host ----------------------------------------------------------------------------------------------------------
extern "C" int zm_stamp_origin(const zm_wcs* wgrid, int n, const double* ra, const double* dec, int size,
                               int32_t* x0, int32_t* y0, int32_t* status) {
    ZM_CHECK(wgrid && x0 && y0 && status && (n == 0 || (ra && dec)), "zm_stamp_origin: null argument");
    ZM_CHECK(n >= 0, "zm_stamp_origin: n must not be negative (got %d)", n);
    ZM_CHECK(size >= 1 && size <= ZM_STAMP_MAX, "zm_stamp_origin: size must be 1 .. %d (got %d)", ZM_STAMP_MAX, size);
    if (n == 0) return 0;
    std::vector<double> xy((size_t)2 * n);
    ZM_TRY(zm_wcs_sky2pix(wgrid, n, ra, dec, xy.data(), xy.data() + n));
    const int onx = wgrid->naxis[0], ony = wgrid->naxis[1];
    for (int k = 0; k < n; ++k) {
        const double x = xy[k] - 1.0, y = xy[n + k] - 1.0;
        x0[k] = y0[k] = 0;
        if (!(std::isfinite(x) && std::isfinite(y)) || fabs(x) > 1e9 || fabs(y) > 1e9) {
            status[k] = std::isfinite(x) && std::isfinite(y) ? ZM_STAMP_NO_OVERLAP : ZM_STAMP_NOT_FINITE;
            continue;
        }
        // astropy.nddata.utils.overlap_slices: first pixel = ceil(position - size / 2)
        const long long a = (long long)ceil(x - 0.5 * size), b = (long long)ceil(y - 0.5 * size);
        x0[k] = (int32_t)a;
        y0[k] = (int32_t)b;
        status[k] = (a + size <= 0 || a >= onx || b + size <= 0 || b >= ony) ? ZM_STAMP_NO_OVERLAP : 0;
    }
    return 0;
}

static int stamps_check(const char* who, zm_ctx* ctx, int nplanes, const zm_stamp_plane* planes, const zm_wcs* wgrid,
                        int kernel, int n, const int32_t* x0, const int32_t* y0, int size, const float* out) {
    ZM_CHECK(ctx && planes && wgrid, "%s: null argument", who);
    ZM_CHECK(n >= 0, "%s: n must not be negative (got %d)", who, n);
    ZM_CHECK(n == 0 || (x0 && y0 && out), "%s: null argument", who);
    ZM_CHECK(nplanes >= 1 && nplanes <= ZM_STAMP_PLANES_MAX, "%s: 1 .. %d planes (got %d)", who, ZM_STAMP_PLANES_MAX, nplanes);
    ZM_CHECK(size >= 1 && size <= ZM_STAMP_MAX, "%s: size must be 1 .. %d (got %d)", who, ZM_STAMP_MAX, size);
    ZM_CHECK(kernel == ZM_RESAMPLE_LANCZOS3 || kernel == ZM_RESAMPLE_BILINEAR, "%s: LANCZOS3 or BILINEAR (got %d)", who, kernel);
    ZM_CHECK(ctx->edge == ZM_EDGE_ZERO && ctx->mask_resample == ZM_MASKRES_OR, "%s: default conventions only", who);
    ZM_TRY(zm_check_wcs(wgrid, "stamp grid"));
    for (int p = 0; p < nplanes; ++p) {
        ZM_CHECK(planes[p].img != nullptr, "%s: plane %d has no image", who, p);
        ZM_TRY(zm_check_wcs(&planes[p].wcs, "stamp plane"));
        ZM_CHECK(!planes[p].on_grid || (planes[p].wcs.naxis[0] == wgrid->naxis[0] && planes[p].wcs.naxis[1] == wgrid->naxis[1]),
                 "%s: plane %d is marked on_grid but is %d x %d, the grid %d x %d", who, p, planes[p].wcs.naxis[0],
                 planes[p].wcs.naxis[1], wgrid->naxis[0], wgrid->naxis[1]);
    }
    return 0;
}

extern "C" int zm_stamps_dev(zm_ctx* ctx, int nplanes, const zm_stamp_plane* planes, const zm_wcs* wgrid, int kernel,
                             int n, const int32_t* x0, const int32_t* y0, int size, float* out, double* out_norm) {
    ZM_TRY(stamps_check("zm_stamps_dev", ctx, nplanes, planes, wgrid, kernel, n, x0, y0, size, out));
    if (n == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    const int onx = wgrid->naxis[0], ony = wgrid->naxis[1], S = size;
    const int lnx = (onx - 1) / ZM_LATTICE_STEP + 2, lny = (ony - 1) / ZM_LATTICE_STEP + 2;
    const int ntx = zm_div_up(onx, TW), nty = zm_div_up(ony, RTH);
    // lattices and plane descriptors
    int nres = 0;
    for (int p = 0; p < nplanes; ++p) nres += planes[p].on_grid ? 0 : 1;
    double2* lat = nullptr;
    if (nres) ZM_TRY(ctx->get("stamp_lattice", sizeof(double2) * (size_t)lnx * lny * nres, (void**)&lat));
    std::vector<st_plane> hp(nplanes);
    int lds_max = 0;
    for (int p = 0, r = 0; p < nplanes; ++p) {
        st_plane& d = hp[p];
        memset(&d, 0, sizeof(d));
        d.img = planes[p].img;
        d.nx = planes[p].wcs.naxis[0];
        d.ny = planes[p].wcs.naxis[1];
        d.on_grid = planes[p].on_grid ? 1 : 0;
        d.vec_ok = (d.nx % 4 == 0) && (((uintptr_t)d.img & 15) == 0);
        if (d.on_grid) continue;
        zm_map_params mp;
        zm_make_map(wgrid, &planes[p].wcs, &mp);
        d.lds_cap = std::min(zm_resample_lds_plan(&mp, onx, ony, kernel), RS_PFCAP);   // as zm_launch_resample clamps it
        d.fscale = (float)planes[p].fscale;
        d.lat = lat + (size_t)lnx * lny * r++;
        ZM_TRY(zm_launch_lattice(ctx, &mp, lnx, lny, const_cast<double2*>(d.lat)));
        lds_max = std::max(lds_max, d.lds_cap);
    }
    // items: the tiles of the grid's 64 x 32 partition each stamp intersects, per resampled plane
    std::vector<st_item> items;
    for (int k = 0; k < n; ++k) {
        const long long xa = std::max<long long>(x0[k], 0), xb = std::min<long long>((long long)x0[k] + S - 1, onx - 1);
        const long long ya = std::max<long long>(y0[k], 0), yb = std::min<long long>((long long)y0[k] + S - 1, ony - 1);
        if (xa > xb || ya > yb) continue;
        for (int p = 0; p < nplanes; ++p) {
            if (hp[p].on_grid) continue;
            for (int ty = (int)(ya / RTH); ty <= (int)(yb / RTH) && ty < nty; ++ty)
                for (int tx = (int)(xa / TW); tx <= (int)(xb / TW) && tx < ntx; ++tx)
                    items.push_back(st_item{k, p, ty * ntx + tx, 0});
        }
    }
    // one staging buffer {planes, x0, y0, items}: pinned, guarded by an event so that a later call cannot overwrite a copy
    // still in flight
    const size_t o_x = ((sizeof(st_plane) * nplanes + 15) & ~(size_t)15), o_y = o_x + (((size_t)n * 4 + 15) & ~(size_t)15);
    const size_t o_it = o_y + (((size_t)n * 4 + 15) & ~(size_t)15), total = o_it + sizeof(st_item) * std::max<size_t>(items.size(), 1);
    hipEvent_t* ev = nullptr;
    ZM_TRY(zm_get_sync_events(ctx, 12, &ev));
    ZM_HIP(hipEventSynchronize(ev[11]));
    char *pin = nullptr, *dev = nullptr;
    ZM_TRY(ctx->get_pinned("stamp_args_h", total, (void**)&pin));
    ZM_TRY(ctx->get("stamp_args", total, (void**)&dev));
    memcpy(pin, hp.data(), sizeof(st_plane) * nplanes);
    memcpy(pin + o_x, x0, (size_t)n * 4);
    memcpy(pin + o_y, y0, (size_t)n * 4);
    if (!items.empty()) memcpy(pin + o_it, items.data(), sizeof(st_item) * items.size());
    ZM_HIP(hipMemcpyAsync(dev, pin, total, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipEventRecord(ev[11], ctx->stream));
    const st_plane* d_pl = (const st_plane*)dev;
    const int *d_x0 = (const int*)(dev + o_x), *d_y0 = (const int*)(dev + o_y);
    const st_item* d_it = (const st_item*)(dev + o_it);
    {
        zm_scope_timer t(ctx, "stamps");
        hipLaunchKernelGGL(k_stamp_fill, dim3((unsigned)n * nplanes), dim3(256), 0, ctx->stream, d_pl, nplanes, d_x0, d_y0, S,
                           onx, ony, out);
        ZM_HIP(hipGetLastError());
        if (!items.empty()) {
            size_t shmem = (size_t)HDR_FLOATS * 4 + (size_t)lds_max * sizeof(float2);
            if (kernel == ZM_RESAMPLE_LANCZOS3) {
                const float* taptab = nullptr;
                ZM_TRY(zm_get_lanczos_table(ctx, &taptab));
                shmem += sizeof(float) * LZ_FLOATS;
                hipLaunchKernelGGL(k_stamp_resample<ZM_RESAMPLE_LANCZOS3>, dim3((unsigned)items.size()), dim3(256), shmem,
                                   ctx->stream, d_pl, nplanes, d_it, d_x0, d_y0, S, lnx, lny, onx, ony, ntx, taptab, out);
            } else {
                hipLaunchKernelGGL(k_stamp_resample<ZM_RESAMPLE_BILINEAR>, dim3((unsigned)items.size()), dim3(256), shmem,
                                   ctx->stream, d_pl, nplanes, d_it, d_x0, d_y0, S, lnx, lny, onx, ony, ntx, nullptr, out);
            }
            ZM_HIP(hipGetLastError());
        }
        if (out_norm) {
            hipLaunchKernelGGL(k_stamp_norm, dim3((unsigned)n * nplanes), dim3(256), 0, ctx->stream, out, S, out_norm);
            ZM_HIP(hipGetLastError());
        }
    }
    return 0;
}

extern "C" int zm_stamps(zm_ctx* ctx, int nplanes, const zm_stamp_plane* planes, const zm_wcs* wgrid, int kernel,
                         int n, const int32_t* x0, const int32_t* y0, int size, float* out, double* out_norm) {
    ZM_TRY(stamps_check("zm_stamps", ctx, nplanes, planes, wgrid, kernel, n, x0, y0, size, out));
    if (n == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    std::vector<zm_stamp_plane> dp(planes, planes + nplanes);
    size_t total = 0;
    std::vector<size_t> off(nplanes);
    for (int p = 0; p < nplanes; ++p) {
        off[p] = total;
        total += ((size_t)planes[p].wcs.naxis[0] * planes[p].wcs.naxis[1] * 4 + 255) & ~(size_t)255;
    }
    const size_t ob = (size_t)n * nplanes * size * size * 4, nb = (size_t)n * nplanes * 8;
    char *base = nullptr, *d_out = nullptr;
    ZM_TRY(ctx->get("h_stamp_planes", total, (void**)&base));
    ZM_TRY(ctx->get("h_stamp_out", ((ob + 15) & ~(size_t)15) + nb, (void**)&d_out));
    double* d_norm = (double*)(d_out + ((ob + 15) & ~(size_t)15));
    for (int p = 0; p < nplanes; ++p) {
        const size_t bytes = (size_t)planes[p].wcs.naxis[0] * planes[p].wcs.naxis[1] * 4;
        ZM_HIP(hipMemcpyAsync(base + off[p], planes[p].img, bytes, hipMemcpyHostToDevice, ctx->stream));
        dp[p].img = (const float*)(base + off[p]);
    }
    ZM_TRY(zm_stamps_dev(ctx, nplanes, dp.data(), wgrid, kernel, n, x0, y0, size, (float*)d_out, out_norm ? d_norm : nullptr));
    ZM_HIP(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    if (out_norm) ZM_HIP(hipMemcpyAsync(out_norm, d_norm, nb, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
