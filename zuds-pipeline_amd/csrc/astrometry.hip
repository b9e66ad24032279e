// Astrometric refit on gfx950: a frame's detections against a star catalogue -> the PV terms of its TPV header.
//
// Stands where the reference shells out to SCAMP (zuds/scamp.py:16-113, astromatic/default.scamp).  The operator is
// this project's own and is stated in DESIGN.md ("Astrometric refit"); it takes SCAMP's parameters where default.scamp
// sets them and does not claim SCAMP's digits.
//
//   k_am_prep     per detection: its position in the plane of the initial header (arcsec) and its rank key (NaN on a
//                 row with a value that is not finite: such a row takes part in nothing)
//   k_am_select   the match_nmax rows of greatest key per frame (rank by counting; ties: the lowest row), each written
//                 to the slot its rank names, so the list has one order on every run
//   k_am_bbox     the box around a frame's selected detections
//   k_am_vote     grid (chunk of 256 stars, frame): every lane projects one star about the frame's CRVAL; a chunk with
//                 no star inside the box grown by P leaves at once.  Otherwise the offsets of every (star, detection)
//                 pair within P on both axes are counted in an LDS histogram (ds_add_u32) and its non-zero bins are
//                 added to the frame's histogram in HBM (integer atomics)
//   k_am_peak     per frame: 3 x 3 box sums, the peak (ties: the lowest bin), the runner-up outside its 5 x 5
//                 neighbourhood and the integer moments of the nine bins under the peak
//   k_am_sky      per detection: (ra, dec) under the frame's current solution, for zm_crossmatch_dev
//   k_am_fit      one workgroup per frame, every clip iteration of one round: weighted normal equations in fp64 (each
//                 thread its rows in row order, then a fixed tree over lanes and waves), Cholesky and the two solves,
//                 residuals, the next keep set, the comparison with the round before
//
// No float atomics: every sum of reals has one order, so two runs give the same bits.  Nothing is shared between
// workgroups inside a launch except the histogram's integer adds; the round loop is on the host and reads one word per
// frame at the launch boundary.
#include <algorithm>
#include <cmath>
#include <vector>

#include "zm_internal.h"
#include "wcs_math.h"

#define AM_T 256
#define AM_LDS_TOTAL (160 * 1024)     // LDS of a gfx950 compute unit
#define AM_D2R 0.017453292519943295
#define AM_MAXC 10                    // coefficients per axis at degree 3
#define AM_PENDING (-1)               // status of a frame whose rounds are not over

struct am_frame {
    zm_wcs w;                         // the current solution, always in TPV form
    double fr[9];                     // east, north, pole at CRVAL
    double s, pixscale;               // normalisation of (u, v) in degrees; arcsec per pixel
    double box[4];                    // min xi, max xi, min eta, max eta of the selected detections (arcsec)
    double rms[2], chi2;
    int32_t off, n, status, nmatch, nused, rounds, pad_[2];
};

struct am_cfg {
    double P, q, radius, clip2;       // clip2 = 2 clip_nsigma^2
    int32_t nb, nmax, max_clip, dchunk;
};

__device__ __forceinline__ bool am_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// gnomonic projection about the frame's CRVAL in degrees; false behind the tangent plane or on a value that is not finite
__device__ __forceinline__ bool am_project(const double* fr, double ra, double dec, double* xi, double* eta) {
    if (!(am_finite(ra) && am_finite(dec))) return false;
    const double a = ra * AM_D2R, d = dec * AM_D2R;
    const double cd = cos(d), x = cd * cos(a), y = cd * sin(a), z = sin(d);
    const double c = x * fr[6] + y * fr[7] + z * fr[8];
    if (!(c > 0.0)) return false;
    *xi = (x * fr[0] + y * fr[1] + z * fr[2]) / c / AM_D2R;
    *eta = (x * fr[3] + y * fr[4] + z * fr[5]) / c / AM_D2R;
    return true;
}

// ---- vote -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AM_T) void k_am_prep(const am_frame* __restrict__ frames, const double* __restrict__ x,
                                                  const double* __restrict__ y, const double* __restrict__ sd,
                                                  const double* __restrict__ snr, double* __restrict__ key,
                                                  double* __restrict__ px, double* __restrict__ py) {
    const am_frame& F = frames[blockIdx.y];
    const int i = blockIdx.x * AM_T + threadIdx.x;
    if (i >= F.n) return;
    const int g = F.off + i;
    const double xx = x[g], yy = y[g], k = snr[g];
    double a = __builtin_nan(""), b = a, kk = a;
    if (am_finite(xx) && am_finite(yy) && am_finite(sd[g]) && am_finite(k)) {
        zm_pix2plane(&F.w, xx, yy, &a, &b);
        a *= 3600.0;
        b *= 3600.0;
        kk = k;
    }
    key[g] = kk; px[g] = a; py[g] = b;
}

__global__ __launch_bounds__(AM_T) void k_am_select(const am_frame* __restrict__ frames, const double* __restrict__ key,
                                                    const double* __restrict__ px, const double* __restrict__ py, int nmax,
                                                    double2* __restrict__ sel, int* nsel) {
    __shared__ double tile[AM_T];
    const am_frame& F = frames[blockIdx.y];
    const int n = F.n, off = F.off;
    if ((int)blockIdx.x * AM_T >= n) return;
    const int i = blockIdx.x * AM_T + threadIdx.x;
    const double ki = i < n ? key[off + i] : __builtin_nan("");
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += AM_T) {
        __syncthreads();
        tile[threadIdx.x] = j0 + (int)threadIdx.x < n ? key[off + j0 + threadIdx.x] : __builtin_nan("");
        __syncthreads();
        const int cnt = min(AM_T, n - j0);
        for (int t = 0; t < cnt; ++t) {
            const double kj = tile[t];                    // a NaN compares false both ways: it outranks nothing
            rank += (kj > ki || (kj == ki && j0 + t < i)) ? 1 : 0;
        }
    }
    if (ki == ki && rank < nmax) {
        sel[(size_t)blockIdx.y * nmax + rank] = make_double2(px[off + i], py[off + i]);
        atomicAdd(&nsel[blockIdx.y], 1);
    }
}

__global__ __launch_bounds__(AM_T) void k_am_bbox(am_frame* frames, const double2* __restrict__ sel, const int* __restrict__ nsel,
                                                  int nmax) {
    __shared__ double sh[4][AM_T];
    const int f = blockIdx.x, t = threadIdx.x, ns = nsel[f];
    double lo0 = 1e300, hi0 = -1e300, lo1 = 1e300, hi1 = -1e300;
    for (int k = t; k < ns; k += AM_T) {
        const double2 p = sel[(size_t)f * nmax + k];
        lo0 = fmin(lo0, p.x); hi0 = fmax(hi0, p.x);
        lo1 = fmin(lo1, p.y); hi1 = fmax(hi1, p.y);
    }
    sh[0][t] = lo0; sh[1][t] = hi0; sh[2][t] = lo1; sh[3][t] = hi1;
    __syncthreads();
    for (int of = AM_T / 2; of >= 1; of >>= 1) {
        if (t < of) {
            sh[0][t] = fmin(sh[0][t], sh[0][t + of]); sh[1][t] = fmax(sh[1][t], sh[1][t + of]);
            sh[2][t] = fmin(sh[2][t], sh[2][t + of]); sh[3][t] = fmax(sh[3][t], sh[3][t + of]);
        }
        __syncthreads();
    }
    if (t < 4) frames[f].box[t] = sh[t][0];
}

__global__ __launch_bounds__(AM_T) void k_am_vote(const am_frame* __restrict__ frames, const double2* __restrict__ sel,
                                                  const int* __restrict__ nsel, int m, const double* __restrict__ ref_ra,
                                                  const double* __restrict__ ref_dec, am_cfg c, unsigned* hist) {
    extern __shared__ __align__(16) unsigned am_lds[];
    const int f = blockIdx.y, t = threadIdx.x, ns = nsel[f];
    const am_frame& F = frames[f];
    const int nbins = c.nb * c.nb;
    unsigned* lh = am_lds;
    double2* ld = (double2*)(am_lds + ((nbins + 3) & ~3));
    const int j = blockIdx.x * AM_T + t;
    double xs = 0.0, ys = 0.0;
    bool inside = false;
    if (j < m && ns > 0 && am_project(F.fr, ref_ra[j], ref_dec[j], &xs, &ys)) {
        xs *= 3600.0;
        ys *= 3600.0;
        inside = xs >= F.box[0] - c.P && xs <= F.box[1] + c.P && ys >= F.box[2] - c.P && ys <= F.box[3] + c.P;
    }
    if (!__syncthreads_or(inside ? 1 : 0)) return;
    for (int k = t; k < nbins; k += AM_T) lh[k] = 0u;
    for (int k0 = 0; k0 < ns; k0 += c.dchunk) {
        const int cnt = min(c.dchunk, ns - k0);
        __syncthreads();
        for (int k = t; k < cnt; k += AM_T) ld[k] = sel[(size_t)f * c.nmax + k0 + k];
        __syncthreads();
        if (inside) {
            for (int k = 0; k < cnt; ++k) {
                const double2 p = ld[k];
                const double dx = xs - p.x, dy = ys - p.y;
                if (fabs(dx) <= c.P && fabs(dy) <= c.P) {
                    int bx = (int)floor((dx + c.P) / c.q + 0.5), by = (int)floor((dy + c.P) / c.q + 0.5);
                    bx = min(max(bx, 0), c.nb - 1);
                    by = min(max(by, 0), c.nb - 1);
                    atomicAdd(&lh[by * c.nb + bx], 1u);
                }
            }
        }
    }
    __syncthreads();
    unsigned* gh = hist + (size_t)f * nbins;
    for (int k = t; k < nbins; k += AM_T) {
        const unsigned v = lh[k];
        if (v) atomicAdd(&gh[k], v);
    }
}

__device__ __forceinline__ unsigned long long am_box_sum(const unsigned* __restrict__ h, int nb, int r, int c) {
    unsigned long long s = 0;
    for (int dr = -1; dr <= 1; ++dr)
        for (int dc = -1; dc <= 1; ++dc) {
            const int rr = r + dr, cc = c + dc;
            if (rr >= 0 && rr < nb && cc >= 0 && cc < nb) s += h[rr * nb + cc];
        }
    return s;
}

__device__ __forceinline__ unsigned long long am_block_max(unsigned long long v, unsigned long long* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int of = AM_T / 2; of >= 1; of >>= 1) {
        if (t < of) sh[t] = sh[t] > sh[t + of] ? sh[t] : sh[t + of];
        __syncthreads();
    }
    return sh[0];
}

// vote[f] = {peak, runner-up, sum of count * column, sum of count * row} over the nine bins under the peak
__global__ __launch_bounds__(AM_T) void k_am_peak(const unsigned* __restrict__ hist, int nb, long long* __restrict__ vote) {
    __shared__ unsigned long long sh[AM_T];
    const int f = blockIdx.x, t = threadIdx.x, nbins = nb * nb;
    const unsigned* h = hist + (size_t)f * nbins;
    unsigned long long best = 0;
    for (int k = t; k < nbins; k += AM_T) {
        const unsigned long long s = am_box_sum(h, nb, k / nb, k % nb);
        const unsigned long long key = (s << 32) | (unsigned long long)(0xffffffffu - (unsigned)k);   // ties: the lowest bin
        best = key > best ? key : best;
    }
    best = am_block_max(best, sh);
    const long long peak = (long long)(best >> 32);
    const int pk = (int)(0xffffffffu - (unsigned)(best & 0xffffffffu)), pr = pk / nb, pc = pk % nb;
    unsigned long long run = 0;
    for (int k = t; k < nbins; k += AM_T) {
        const int r = k / nb, cc = k % nb;
        if (abs(r - pr) <= 2 && abs(cc - pc) <= 2) continue;
        const unsigned long long s = am_box_sum(h, nb, r, cc);
        run = s > run ? s : run;
    }
    run = am_block_max(run, sh);
    if (t == 0) {
        long long sx = 0, sy = 0;
        for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
                const int rr = pr + dr, cc = pc + dc;
                if (rr >= 0 && rr < nb && cc >= 0 && cc < nb) {
                    const long long v = h[rr * nb + cc];
                    sx += v * cc;
                    sy += v * rr;
                }
            }
        vote[4 * f] = peak; vote[4 * f + 1] = (long long)run; vote[4 * f + 2] = sx; vote[4 * f + 3] = sy;
    }
}

// ---- rounds ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AM_T) void k_am_sky(const am_frame* __restrict__ frames, const int* __restrict__ state,
                                                 const double* __restrict__ x, const double* __restrict__ y,
                                                 const double* __restrict__ key, double* __restrict__ ra,
                                                 double* __restrict__ dec) {
    const am_frame& F = frames[blockIdx.y];
    const int i = blockIdx.x * AM_T + threadIdx.x;
    if (i >= F.n) return;
    const int g = F.off + i;
    double a = __builtin_nan(""), d = a;
    if (state[blockIdx.y] == 0 && key[g] == key[g]) {
        double xi, eta;
        zm_pix2plane(&F.w, x[g], y[g], &xi, &eta);
        const double xr = xi * AM_D2R, er = eta * AM_D2R;
        const double vx = xr * F.fr[0] + er * F.fr[3] + F.fr[6], vy = xr * F.fr[1] + er * F.fr[4] + F.fr[7],
                     vz = xr * F.fr[2] + er * F.fr[5] + F.fr[8];
        a = atan2(vy, vx) / AM_D2R;
        if (a < 0.0) a += 360.0;
        d = atan2(vz, sqrt(vx * vx + vy * vy)) / AM_D2R;
    }
    ra[g] = a; dec[g] = d;
}

// the sum of v over the workgroup in one fixed tree (lanes: xor butterfly, commutative at every step, so every lane
// holds the same bits; waves: (0 + 1) + (2 + 3)), returned to every thread
__device__ __forceinline__ double am_wave_sum(double v) {
#pragma unroll
    for (int of = 32; of >= 1; of >>= 1) v += __shfl_xor(v, of);
    return v;
}

__device__ __forceinline__ double am_block_sum(double v, double* sh4) {
    v = am_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}

template <int NC>
__device__ __forceinline__ void am_basis(double a, double b, double* phi) {
    phi[0] = 1.0; phi[1] = a; phi[2] = b;
    if (NC >= 6) { phi[3] = a * a; phi[4] = a * b; phi[5] = b * b; }
    if (NC >= 10) { phi[6] = phi[3] * a; phi[7] = phi[3] * b; phi[8] = a * phi[5]; phi[9] = phi[5] * b; }
}

// One round of one frame.  Row scratch (ra .. rchi, keep) is private to the thread that owns the row (rows are dealt by
// index modulo the workgroup), so it needs no barrier of its own.
template <int NC>
__global__ __launch_bounds__(AM_T) void k_am_fit(am_frame* frames, int* state, const double* __restrict__ x,
                                                 const double* __restrict__ y, const double* __restrict__ sd,
                                                 const double* __restrict__ ref_ra, const double* __restrict__ ref_dec,
                                                 const double* __restrict__ ref_sig, const int* __restrict__ mnew,
                                                 int* __restrict__ match, unsigned char* __restrict__ used,
                                                 unsigned char* __restrict__ keep, double* __restrict__ ra_, double* __restrict__ rb_,
                                                 double* __restrict__ rw_, double* __restrict__ rxi, double* __restrict__ reta,
                                                 double* __restrict__ rchi, am_cfg c, int round) {
    constexpr int NA = NC * (NC + 1) / 2 + 2 * NC;
    __shared__ double red[4][NA];
    __shared__ double A[NC * NC], rhs[2][NC], coef[2][NC], sh4[4];
    __shared__ int flag;
    const int f = blockIdx.x, t = threadIdx.x;
    if (state[f] != 0) return;
    am_frame& F = frames[f];
    const int n = F.n, off = F.off;
    const double s = F.s, ps = F.pixscale;
    int diff = round == 1 ? 1 : 0, nm = 0;
    for (int i = t; i < n; i += AM_T) {
        const int g = off + i, j = mnew[g];
        if (match[g] != j) diff = 1;
        match[g] = j;
        unsigned char k = 0;
        if (j >= 0) {
            const double dx = x[g] - F.w.crpix[0], dy = y[g] - F.w.crpix[1];
            const double u = F.w.cd[0] * dx + F.w.cd[1] * dy, v = F.w.cd[2] * dx + F.w.cd[3] * dy;
            double xi = 0.0, eta = 0.0;
            am_project(F.fr, ref_ra[j], ref_dec[j], &xi, &eta);
            const double e = sd[g] * ps, sr = ref_sig[j];
            ra_[g] = u / s; rb_[g] = v / s; rw_[g] = 1.0 / (e * e + sr * sr); rxi[g] = xi; reta[g] = eta;
            k = 1;
            ++nm;
        }
        keep[g] = k;
    }
    int nmatch = 0;
    {
        const double tot = am_block_sum((double)nm, sh4);    // counts below 2^53 are exact in fp64
        nmatch = (int)tot;
    }
    int status = AM_PENDING, nused = 0, fits = 0;
    double chi2 = 0.0, rms0 = 0.0, rms1 = 0.0;
    for (;;) {
        int nk = 0;
        for (int i = t; i < n; i += AM_T) nk += keep[off + i];
        nk = (int)am_block_sum((double)nk, sh4);
        nused = nk;
        if (nk < 2 * NC) { status = ZM_ASTROM_TOO_FEW; break; }
        double acc[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) acc[k] = 0.0;
        for (int i = t; i < n; i += AM_T) {
            const int g = off + i;
            if (!keep[g]) continue;
            double phi[NC];
            am_basis<NC>(ra_[g], rb_[g], phi);
            const double w = rw_[g], wx = w * rxi[g], we = w * reta[g];
            int k = 0;
#pragma unroll
            for (int a = 0; a < NC; ++a) {
                const double wa = w * phi[a];
#pragma unroll
                for (int b = a; b < NC; ++b) acc[k++] += wa * phi[b];
            }
#pragma unroll
            for (int a = 0; a < NC; ++a) {
                acc[k + a] += wx * phi[a];
                acc[k + NC + a] += we * phi[a];
            }
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) acc[k] = am_wave_sum(acc[k]);
        __syncthreads();
        if ((t & 63) == 0) {
#pragma unroll
            for (int k = 0; k < NA; ++k) red[t >> 6][k] = acc[k];
        }
        __syncthreads();
        if (t == 0) {
            int k = 0;
            for (int a = 0; a < NC; ++a)
                for (int b = a; b < NC; ++b, ++k) A[a * NC + b] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
            for (int a = 0; a < 2 * NC; ++a, ++k) rhs[a / NC][a % NC] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
            // A = U^T U in place (upper triangle), then the two solves
            int ok = 1;
            for (int a = 0; a < NC && ok; ++a) {
                double d = A[a * NC + a];
                for (int p = 0; p < a; ++p) d -= A[p * NC + a] * A[p * NC + a];
                if (!(d > 0.0)) { ok = 0; break; }
                d = sqrt(d);
                A[a * NC + a] = d;
                for (int b = a + 1; b < NC; ++b) {
                    double v = A[a * NC + b];
                    for (int p = 0; p < a; ++p) v -= A[p * NC + a] * A[p * NC + b];
                    A[a * NC + b] = v / d;
                }
            }
            if (ok) {
                for (int ax = 0; ax < 2; ++ax) {
                    double z[NC];
                    for (int a = 0; a < NC; ++a) {
                        double v = rhs[ax][a];
                        for (int p = 0; p < a; ++p) v -= A[p * NC + a] * coef[ax][p];
                        coef[ax][a] = v / A[a * NC + a];
                    }
                    for (int a = NC - 1; a >= 0; --a) {
                        double v = coef[ax][a];
                        for (int p = a + 1; p < NC; ++p) v -= A[a * NC + p] * z[p];
                        z[a] = v / A[a * NC + a];
                    }
                    for (int a = 0; a < NC; ++a) coef[ax][a] = z[a];
                }
            }
            flag = ok;
        }
        __syncthreads();
        if (!flag) { status = ZM_ASTROM_SINGULAR; break; }
        ++fits;
        double sc = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = t; i < n; i += AM_T) {
            const int g = off + i;
            if (match[g] < 0) continue;
            double phi[NC];
            am_basis<NC>(ra_[g], rb_[g], phi);
            double m1 = 0.0, m2 = 0.0;
#pragma unroll
            for (int a = 0; a < NC; ++a) { m1 += coef[0][a] * phi[a]; m2 += coef[1][a] * phi[a]; }
            const double r1 = 3600.0 * (m1 - rxi[g]), r2 = 3600.0 * (m2 - reta[g]);
            const double chi = rw_[g] * (r1 * r1 + r2 * r2);
            rchi[g] = chi;
            if (keep[g]) { sc += chi; s1 += r1 * r1; s2 += r2 * r2; }
        }
        chi2 = am_block_sum(sc, sh4);
        rms0 = sqrt(am_block_sum(s1, sh4) / (double)nk);
        rms1 = sqrt(am_block_sum(s2, sh4) / (double)nk);
        status = ZM_ASTROM_OK;
        if (fits >= c.max_clip) break;
        const double fsc = fmax(1.0, chi2 / (2.0 * (double)(nk - NC))), bound = c.clip2 * fsc;
        int ch = 0;
        for (int i = t; i < n; i += AM_T) {
            const int g = off + i;
            if (match[g] < 0) continue;
            ch |= ((rchi[g] <= bound) ? 1 : 0) != (int)keep[g];
        }
        if (!__syncthreads_or(ch)) break;
        for (int i = t; i < n; i += AM_T) {
            const int g = off + i;
            if (match[g] >= 0) keep[g] = rchi[g] <= bound ? 1 : 0;
        }
    }
    for (int i = t; i < n; i += AM_T) {
        const int g = off + i;
        if (used[g] != keep[g]) diff = 1;
        used[g] = keep[g];
    }
    const int changed = __syncthreads_or(diff);
    if (t == 0) {
        F.nmatch = nmatch; F.nused = nused; F.rounds = round;
        if (status == ZM_ASTROM_OK) {
            const int T[AM_MAXC] = {0, 1, 2, 4, 5, 6, 7, 8, 9, 10}, SW[AM_MAXC] = {0, 2, 1, 5, 4, 3, 9, 8, 7, 6},
                      DG[AM_MAXC] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 3};
            const double sp[4] = {1.0, s, s * s, s * s * s};
            for (int k = 0; k < ZM_NPV; ++k) F.w.pv1[k] = F.w.pv2[k] = 0.0;
            for (int a = 0; a < NC; ++a) {
                F.w.pv1[T[a]] = coef[0][a] / sp[DG[a]];
                F.w.pv2[T[SW[a]]] = coef[1][a] / sp[DG[a]];
            }
            F.w.flags |= 1;
            F.rms[0] = rms0; F.rms[1] = rms1; F.chi2 = chi2;
            if (changed) {
                F.status = AM_PENDING;
            } else {
                F.status = ZM_ASTROM_OK;
                state[f] = 1;
            }
        } else {
            F.rms[0] = F.rms[1] = F.chi2 = 0.0;
            F.status = status;
            state[f] = 1;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
static size_t am_up(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" void zm_astrom_params_default(zm_astrom_params* p) {
    if (!p) return;
    p->position_maxerr = 60.0;
    p->match_resol = 0.0;
    p->crossid_radius = 2.0;
    p->clip_nsigma = 3.0;
    p->degree = 3;
    p->match = 1;
    p->match_nmax = 1024;
    p->max_rounds = 8;
    p->max_clip = 10;
    p->pad_ = 0;
}

static int am_check(const char* who, int nframes, const zm_wcs* wcs0, const int32_t* offsets, int m,
                    const zm_astrom_params* p, const zm_astrom_result* results, am_cfg* c) {
    ZM_CHECK(nframes >= 0 && nframes <= 65535, "%s: nframes must be 0 .. 65535 (got %d)", who, nframes);
    ZM_CHECK(m >= 0 && m <= (1 << 30), "%s: m must be 0 .. 2^30 (got %d)", who, m);
    ZM_CHECK(p, "%s: null params", who);
    ZM_CHECK(p->degree >= 1 && p->degree <= 3, "%s: degree must be 1, 2 or 3 (got %d)", who, p->degree);
    ZM_CHECK(p->crossid_radius > 0.0 && p->position_maxerr > 0.0 && p->clip_nsigma > 0.0,
             "%s: crossid_radius, position_maxerr and clip_nsigma must be positive", who);
    ZM_CHECK(p->match_nmax >= 1 && p->match_nmax <= (1 << 20) && p->max_rounds >= 1 && p->max_clip >= 1,
             "%s: match_nmax must be 1 .. 2^20, max_rounds and max_clip at least 1", who);
    const double q = p->match_resol == 0.0 ? 0.5 * p->crossid_radius : p->match_resol;
    ZM_CHECK(q > 0.0, "%s: the vote's bin (match_resol) must be positive (got %g)", who, q);
    ZM_CHECK(p->position_maxerr / q <= 100.0, "%s: position_maxerr / match_resol must not exceed 100 (got %g)", who,
             p->position_maxerr / q);
    if (nframes > 0) {
        ZM_CHECK(wcs0 && offsets && results, "%s: null argument", who);
        ZM_CHECK(offsets[0] >= 0, "%s: offsets[0] must not be negative (got %d)", who, offsets[0]);
        for (int f = 0; f < nframes; ++f) {
            ZM_CHECK(offsets[f + 1] >= offsets[f], "%s: offsets must ascend (offsets[%d] = %d after %d)", who, f + 1,
                     offsets[f + 1], offsets[f]);
            const double det = wcs0[f].cd[0] * wcs0[f].cd[3] - wcs0[f].cd[1] * wcs0[f].cd[2];
            ZM_CHECK(det != 0.0 && det == det && wcs0[f].naxis[0] > 0 && wcs0[f].naxis[1] > 0,
                     "%s: frame %d needs an invertible CD matrix and positive NAXIS", who, f);
        }
        ZM_CHECK(offsets[nframes] <= (1 << 30), "%s: more than 2^30 detections", who);
    }
    c->P = p->position_maxerr;
    c->q = q;
    c->radius = p->crossid_radius;
    c->clip2 = 2.0 * p->clip_nsigma * p->clip_nsigma;
    c->nb = (int)floor(2.0 * c->P / q + 0.5) + 1;
    c->nmax = p->match_nmax;
    c->max_clip = p->max_clip;
    c->dchunk = 0;                                       // set once the device is known (am_vote_lds)
    return 0;
}

// LDS of the vote: the histogram, then as many of the frame's detections as fit beside it (all of them up to 121 x 121 bins
// at the default match_nmax; in pieces of c->dchunk above).  What the kernel keeps in LDS of its own - the word of the
// workgroup OR - is asked of the runtime, not assumed.
static int am_vote_lds(const char* who, am_cfg* c, size_t* lds) {
    hipFuncAttributes fa;
    ZM_HIP(hipFuncGetAttributes(&fa, (const void*)k_am_vote));
    const size_t histb = (((size_t)c->nb * c->nb + 3) & ~(size_t)3) * 4;
    const long long room = (long long)AM_LDS_TOTAL - (long long)fa.sharedSizeBytes - (long long)histb;
    ZM_CHECK(room >= 64 * (long long)sizeof(double2), "%s: a vote of %d x %d bins leaves no room in LDS", who, c->nb, c->nb);
    c->dchunk = (int)std::min<long long>(c->nmax, room / (long long)sizeof(double2));
    *lds = histb + (size_t)c->dchunk * sizeof(double2);
    ZM_HIP(hipFuncSetAttribute((const void*)k_am_vote, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds));
    return 0;
}

template <int NC>
static void am_launch_fit(zm_ctx* ctx, int nframes, am_frame* frames, int* state, const double* x, const double* y,
                          const double* sd, const double* ref_ra, const double* ref_dec, const double* ref_sig, const int* mnew,
                          int* match, unsigned char* used, unsigned char* keep, double* const row[6], const am_cfg& c, int round) {
    hipLaunchKernelGGL(k_am_fit<NC>, dim3((unsigned)nframes), dim3(AM_T), 0, ctx->stream, frames, state, x, y, sd, ref_ra,
                       ref_dec, ref_sig, mnew, match, used, keep, row[0], row[1], row[2], row[3], row[4], row[5], c, round);
}

extern "C" int zm_astrom_solve_dev(zm_ctx* ctx, int nframes, const zm_wcs* wcs0, const int32_t* offsets, const double* x_dev,
                                   const double* y_dev, const double* sd_dev, const double* snr_dev, int m,
                                   const double* ref_ra_dev, const double* ref_dec_dev, const double* ref_sig_dev,
                                   const zm_astrom_params* params, zm_astrom_result* results, int32_t* match_dev,
                                   uint8_t* used_dev) {
    ZM_CHECK(ctx, "zm_astrom_solve_dev: null argument");
    am_cfg c;
    ZM_TRY(am_check("zm_astrom_solve_dev", nframes, wcs0, offsets, m, params, results, &c));
    if (nframes == 0) return 0;
    const int base = offsets[0], N = offsets[nframes] - base;
    ZM_CHECK(N == 0 || (x_dev && y_dev && sd_dev && snr_dev && match_dev && used_dev), "zm_astrom_solve_dev: null argument");
    ZM_CHECK(m == 0 || (ref_ra_dev && ref_dec_dev && ref_sig_dev), "zm_astrom_solve_dev: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    const int NC = params->degree == 1 ? 3 : params->degree == 2 ? 6 : 10;
    // the arrays are indexed from offsets[0] on
    const double *x = x_dev + base, *y = y_dev + base, *sd = sd_dev + base, *snr = snr_dev + base;
    int32_t* match = match_dev + base;
    uint8_t* used = used_dev + base;

    am_frame* hf = nullptr;                              // pinned: uploaded twice, downloaded once
    ZM_TRY(ctx->get_pinned("am_frames", (size_t)nframes * sizeof(am_frame), (void**)&hf));
    long long* hvote = nullptr;
    ZM_TRY(ctx->get_pinned("am_vote", (size_t)nframes * 4 * sizeof(long long), (void**)&hvote));
    int* hstate = nullptr;
    ZM_TRY(ctx->get_pinned("am_state", (size_t)nframes * sizeof(int), (void**)&hstate));
    int maxn = 0;
    for (int f = 0; f < nframes; ++f) {
        am_frame& F = hf[f];
        memset(&F, 0, sizeof(F));
        F.w = wcs0[f];
        if (!(F.w.flags & 1)) {                          // TAN: TPV with the identity polynomial
            for (int k = 0; k < ZM_NPV; ++k) F.w.pv1[k] = F.w.pv2[k] = 0.0;
            F.w.pv1[1] = F.w.pv2[1] = 1.0;
        }
        F.w.flags = 1;
        zm_wcs_frame(&F.w, F.fr);
        const double cx[2] = {0.5 - F.w.crpix[0], F.w.naxis[0] + 0.5 - F.w.crpix[0]},
                     cy[2] = {0.5 - F.w.crpix[1], F.w.naxis[1] + 0.5 - F.w.crpix[1]};
        double s = 0.0;
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                s = std::max(s, fabs(F.w.cd[0] * cx[a] + F.w.cd[1] * cy[b]));
                s = std::max(s, fabs(F.w.cd[2] * cx[a] + F.w.cd[3] * cy[b]));
            }
        F.s = s;
        F.pixscale = 3600.0 * sqrt(fabs(F.w.cd[0] * F.w.cd[3] - F.w.cd[1] * F.w.cd[2]));
        F.off = offsets[f] - base;
        F.n = offsets[f + 1] - offsets[f];
        F.status = AM_PENDING;
        maxn = std::max(maxn, F.n);
        hstate[f] = 0;
        hvote[4 * f] = hvote[4 * f + 1] = hvote[4 * f + 2] = hvote[4 * f + 3] = 0;
    }
    const size_t NN = (size_t)N, nbins = (size_t)c.nb * c.nb;
    const size_t histb = params->match ? (size_t)nframes * nbins * 4 : 0;
    ZM_CHECK(histb <= ((size_t)1 << 32), "zm_astrom_solve_dev: %d frames of %d x %d bins need more than 4 GiB", nframes, c.nb, c.nb);
    const size_t o_fr = 0, o_state = o_fr + am_up((size_t)nframes * sizeof(am_frame)), o_nsel = o_state + am_up((size_t)nframes * 4),
                 o_vote = o_nsel + am_up((size_t)nframes * 4), o_sel = o_vote + am_up((size_t)nframes * 32),
                 o_hist = o_sel + am_up(params->match ? (size_t)nframes * c.nmax * 16 : 0), o_key = o_hist + am_up(histb),
                 o_row = o_key + am_up(NN * 8), o_ra = o_row + 6 * am_up(NN * 8), o_dec = o_ra + am_up(NN * 8),
                 o_sep = o_dec + am_up(NN * 8), o_mnew = o_sep + am_up(NN * 8), o_keep = o_mnew + am_up(NN * 4),
                 total = o_keep + am_up(NN);
    char* w = nullptr;
    ZM_TRY(ctx->get("am_work", total, (void**)&w));
    am_frame* frames = (am_frame*)(w + o_fr);
    int *state = (int*)(w + o_state), *nsel = (int*)(w + o_nsel), *mnew = (int*)(w + o_mnew);
    long long* vote = (long long*)(w + o_vote);
    double2* sel = (double2*)(w + o_sel);
    unsigned* hist = (unsigned*)(w + o_hist);
    double *key = (double*)(w + o_key), *ra = (double*)(w + o_ra), *dec = (double*)(w + o_dec), *sep = (double*)(w + o_sep);
    double* row[6];
    for (int k = 0; k < 6; ++k) row[k] = (double*)(w + o_row + (size_t)k * am_up(NN * 8));
    unsigned char* keep = (unsigned char*)(w + o_keep);
    const dim3 rows((unsigned)std::max(1, zm_div_up(maxn, AM_T)), (unsigned)nframes), block(AM_T);

    ZM_HIP(hipMemcpyAsync(frames, hf, (size_t)nframes * sizeof(am_frame), hipMemcpyHostToDevice, ctx->stream));
    if (N) {
        ZM_HIP(hipMemsetAsync(match, 0xff, NN * 4, ctx->stream));
        ZM_HIP(hipMemsetAsync(used, 0, NN, ctx->stream));
        ZM_HIP(hipMemsetAsync(keep, 0, NN, ctx->stream));
    }
    hipLaunchKernelGGL(k_am_prep, rows, block, 0, ctx->stream, frames, x, y, sd, snr, key, (double*)row[0], (double*)row[1]);
    ZM_HIP(hipGetLastError());
    if (params->match) {
        zm_scope_timer timer(ctx, "astrom_vote");
        size_t lds = 0;
        ZM_TRY(am_vote_lds("zm_astrom_solve_dev", &c, &lds));
        ZM_HIP(hipMemsetAsync(hist, 0, histb, ctx->stream));
        ZM_HIP(hipMemsetAsync(nsel, 0, (size_t)nframes * 4, ctx->stream));
        hipLaunchKernelGGL(k_am_select, rows, block, 0, ctx->stream, frames, key, (const double*)row[0], (const double*)row[1],
                           c.nmax, sel, nsel);
        hipLaunchKernelGGL(k_am_bbox, dim3((unsigned)nframes), block, 0, ctx->stream, frames, sel, nsel, c.nmax);
        if (m > 0)
            hipLaunchKernelGGL(k_am_vote, dim3((unsigned)zm_div_up(m, AM_T), (unsigned)nframes), block, lds, ctx->stream, frames,
                               sel, nsel, m, ref_ra_dev, ref_dec_dev, c, hist);
        hipLaunchKernelGGL(k_am_peak, dim3((unsigned)nframes), block, 0, ctx->stream, hist, c.nb, vote);
        ZM_HIP(hipGetLastError());
        ZM_HIP(hipMemcpyAsync(hvote, vote, (size_t)nframes * 32, hipMemcpyDeviceToHost, ctx->stream));
        ZM_HIP(hipStreamSynchronize(ctx->stream));
    }
    std::vector<double> shift(2 * (size_t)nframes, 0.0);
    for (int f = 0; f < nframes; ++f) {
        if (!params->match) continue;
        const long long peak = hvote[4 * f], run = hvote[4 * f + 1];
        if (peak < 2 * NC || run * 2 >= peak) {
            hf[f].status = ZM_ASTROM_AMBIGUOUS;
            hstate[f] = 1;
            continue;
        }
        // count-weighted centroid of the nine bin centres, from integers: bin b is centred on b q - P
        shift[2 * f] = (double)hvote[4 * f + 2] * c.q / (double)peak - c.P;
        shift[2 * f + 1] = (double)hvote[4 * f + 3] * c.q / (double)peak - c.P;
        hf[f].w.pv1[0] += shift[2 * f] / 3600.0;
        hf[f].w.pv2[0] += shift[2 * f + 1] / 3600.0;
    }
    if (params->match) ZM_HIP(hipMemcpyAsync(frames, hf, (size_t)nframes * sizeof(am_frame), hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(state, hstate, (size_t)nframes * 4, hipMemcpyHostToDevice, ctx->stream));
    {
        zm_scope_timer timer(ctx, "astrom_rounds");
        for (int round = 1; round <= params->max_rounds; ++round) {
            bool any = false;
            for (int f = 0; f < nframes; ++f) any = any || hstate[f] == 0;
            if (!any) break;
            hipLaunchKernelGGL(k_am_sky, rows, block, 0, ctx->stream, frames, state, x, y, key, ra, dec);
            ZM_HIP(hipGetLastError());
            ZM_TRY(zm_crossmatch_dev(ctx, N, ra, dec, m, ref_ra_dev, ref_dec_dev, c.radius, mnew, sep));
            if (NC == 3)
                am_launch_fit<3>(ctx, nframes, frames, state, x, y, sd, ref_ra_dev, ref_dec_dev, ref_sig_dev, mnew, match, used, keep, row, c, round);
            else if (NC == 6)
                am_launch_fit<6>(ctx, nframes, frames, state, x, y, sd, ref_ra_dev, ref_dec_dev, ref_sig_dev, mnew, match, used, keep, row, c, round);
            else
                am_launch_fit<10>(ctx, nframes, frames, state, x, y, sd, ref_ra_dev, ref_dec_dev, ref_sig_dev, mnew, match, used, keep, row, c, round);
            ZM_HIP(hipGetLastError());
            ZM_HIP(hipMemcpyAsync(hstate, state, (size_t)nframes * 4, hipMemcpyDeviceToHost, ctx->stream));
            ZM_HIP(hipStreamSynchronize(ctx->stream));
        }
    }
    ZM_HIP(hipMemcpyAsync(hf, frames, (size_t)nframes * sizeof(am_frame), hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    for (int f = 0; f < nframes; ++f) {
        const am_frame& F = hf[f];
        zm_astrom_result& R = results[f];
        memset(&R, 0, sizeof(R));
        R.status = F.status == AM_PENDING ? ZM_ASTROM_NOT_CONVERGED : F.status;
        const bool solved = R.status == ZM_ASTROM_OK || R.status == ZM_ASTROM_NOT_CONVERGED;
        R.wcs = solved ? F.w : wcs0[f];
        R.wcs.naxis[0] = wcs0[f].naxis[0];
        R.wcs.naxis[1] = wcs0[f].naxis[1];
        R.wcs.pad_ = wcs0[f].pad_;
        R.shift[0] = shift[2 * f];
        R.shift[1] = shift[2 * f + 1];
        R.vote_peak = (int32_t)hvote[4 * f];
        R.vote_runner_up = (int32_t)hvote[4 * f + 1];
        R.nmatch = F.nmatch; R.nused = F.nused; R.rounds = F.rounds;
        R.rms[0] = solved ? F.rms[0] : 0.0;
        R.rms[1] = solved ? F.rms[1] : 0.0;
        R.chi2 = solved ? F.chi2 : 0.0;
    }
    return 0;
}

extern "C" int zm_astrom_solve(zm_ctx* ctx, int nframes, const zm_wcs* wcs0, const int32_t* offsets, const double* x,
                               const double* y, const double* sd, const double* snr, int m, const double* ref_ra,
                               const double* ref_dec, const double* ref_sig, const zm_astrom_params* params,
                               zm_astrom_result* results, int32_t* match, uint8_t* used) {
    ZM_CHECK(ctx, "zm_astrom_solve: null argument");
    am_cfg c;
    ZM_TRY(am_check("zm_astrom_solve", nframes, wcs0, offsets, m, params, results, &c));
    if (nframes == 0) return 0;
    const int base = offsets[0], N = offsets[nframes] - base;
    ZM_CHECK(N == 0 || (x && y && sd && snr && match && used), "zm_astrom_solve: null argument");
    ZM_CHECK(m == 0 || (ref_ra && ref_dec && ref_sig), "zm_astrom_solve: null argument");
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t NN = (size_t)N, M = (size_t)m;
    const size_t o_x = 0, o_y = o_x + am_up(NN * 8), o_sd = o_y + am_up(NN * 8), o_snr = o_sd + am_up(NN * 8),
                 o_ra = o_snr + am_up(NN * 8), o_dec = o_ra + am_up(M * 8), o_sig = o_dec + am_up(M * 8),
                 o_match = o_sig + am_up(M * 8), o_used = o_match + am_up(NN * 4), total = o_used + am_up(NN) + 256;
    char* d = nullptr;
    ZM_TRY(ctx->get("h_am_io", total, (void**)&d));
    if (N) {
        ZM_HIP(hipMemcpyAsync(d + o_x, x + base, NN * 8, hipMemcpyHostToDevice, ctx->stream));
        ZM_HIP(hipMemcpyAsync(d + o_y, y + base, NN * 8, hipMemcpyHostToDevice, ctx->stream));
        ZM_HIP(hipMemcpyAsync(d + o_sd, sd + base, NN * 8, hipMemcpyHostToDevice, ctx->stream));
        ZM_HIP(hipMemcpyAsync(d + o_snr, snr + base, NN * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    if (m) {
        ZM_HIP(hipMemcpyAsync(d + o_ra, ref_ra, M * 8, hipMemcpyHostToDevice, ctx->stream));
        ZM_HIP(hipMemcpyAsync(d + o_dec, ref_dec, M * 8, hipMemcpyHostToDevice, ctx->stream));
        ZM_HIP(hipMemcpyAsync(d + o_sig, ref_sig, M * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    std::vector<int32_t> rel((size_t)nframes + 1);
    for (int f = 0; f <= nframes; ++f) rel[f] = offsets[f] - base;
    ZM_TRY(zm_astrom_solve_dev(ctx, nframes, wcs0, rel.data(), (const double*)(d + o_x), (const double*)(d + o_y),
                               (const double*)(d + o_sd), (const double*)(d + o_snr), m, (const double*)(d + o_ra),
                               (const double*)(d + o_dec), (const double*)(d + o_sig), params, results,
                               (int32_t*)(d + o_match), (uint8_t*)(d + o_used)));
    if (N) {
        ZM_HIP(hipMemcpyAsync(match + base, d + o_match, NN * 4, hipMemcpyDeviceToHost, ctx->stream));
        ZM_HIP(hipMemcpyAsync(used + base, d + o_used, NN, hipMemcpyDeviceToHost, ctx->stream));
    }
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
