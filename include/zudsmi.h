/*
 * zudsmi.h - C-ABI of libzudsmi.so, the MI355X (gfx950) engine behind the
 * ZUDS coadd / subtraction object API.
 *
 * The reference pipeline has no FFI on this path: it builds command strings
 * and runs `subprocess.check_call` on SWarp, SExtractor and hotpants,
 * exchanging FITS files.  Every entry point below replaces one of those
 * process boundaries (cited per function, paths relative to the reference
 * tree).  INTEGRATION.md shows the ctypes stubs a maintainer adds on the
 * reference side.
 *
 * Conventions
 *  - all functions return 0 on success, non-zero on failure; the message is
 *    available per thread from zm_last_error();
 *  - images are C-contiguous, native-endian, row-major [ny][nx]; pixel (1,1)
 *    of FITS is element [0][0];
 *  - pointers passed to the host entry points are borrowed for the call;
 *    outputs are caller-allocated;
 *  - a zm_ctx owns one HIP stream and all device scratch; one ctx per
 *    process/GPU, not thread-safe;
 *  - `*_dev` entry points take device pointers (hipMalloc / torch storage)
 *    and only enqueue work on the ctx stream.
 */
#ifndef ZUDSMI_H
#define ZUDSMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zm_ctx zm_ctx;

#define ZM_NPV 40

/* TAN (flags = 0) or TPV (flags & 1) WCS; FITS 1-based pixel convention.
 * Replaces astropy.wcs.WCS(header) (zuds/fitsfile.py:233-238) and the
 * `.head` files handed to SWarp (zuds/swarp.py:114-133). */
typedef struct zm_wcs {
    double crpix[2];
    double crval[2];      /* degrees */
    double cd[4];         /* CD1_1 CD1_2 CD2_1 CD2_2, degrees / pixel */
    double pv1[ZM_NPV];   /* PV1_k; only read when flags & 1 */
    double pv2[ZM_NPV];
    int32_t naxis[2];     /* NAXIS1 (x), NAXIS2 (y) */
    int32_t flags;        /* bit 0: TPV distortion present */
    int32_t pad_;
} zm_wcs;

enum { ZM_RESAMPLE_NEAREST = 0, ZM_RESAMPLE_BILINEAR = 1, ZM_RESAMPLE_LANCZOS3 = 3 };
enum { ZM_COMBINE_WEIGHTED = 0, ZM_COMBINE_MEDIAN = 1, ZM_COMBINE_CLIPPED = 2,
       ZM_COMBINE_AVERAGE = 3 };
enum { ZM_MASK_AND = 0, ZM_MASK_OR = 1 };

/* ---- context ---------------------------------------------------------- */
int zm_ctx_create(int device, zm_ctx** out);
int zm_ctx_destroy(zm_ctx* ctx);
/* A context bound to the caller's hipStream_t from the start: it never creates a stream of its own (its second stream
 * is made on first use).  For processes that run many contexts side by side on one GPU (scripts/donightly.py:21-40
 * runs one process per job; here: one context per chain). */
int zm_ctx_create_on_stream(int device, void* hip_stream, zm_ctx** out);
/* Use an external hipStream_t (e.g. torch's current stream); NULL = own stream.  Binding the stream already bound is
 * free; a change orders the new stream behind the work enqueued on the old one with an event (the context's scratch
 * is shared) - the host never waits (round 6; rounds 1 - 5 synchronised the old stream here). */
int zm_ctx_set_stream(zm_ctx* ctx, void* hip_stream);
int zm_ctx_synchronize(zm_ctx* ctx);
/* Several contexts (one host thread each) may subtract on one GPU at the same time - the
 * reference runs 64 independent `hotpants` processes per node (nersc/controller.py:101,
 * scripts/donightly.py:21-40).  The kernel-fit solver of a context that has the GPU to itself
 * (nctx = 1, the default) keeps ~230 workgroups resident behind in-kernel barriers - the short
 * form; declaring nctx >= 2 (1 .. 64) switches the context to the one-workgroup-per-region
 * form, which claims nothing (k_chol_tp).  Results do not depend on the share: same bits. */
int zm_ctx_set_share(zm_ctx* ctx, int nctx);
const char* zm_last_error(void);
const char* zm_version(void);
/* What the context last did / how the library was built, by name (-> *out; unknown name: error):
 *   "fused_form"  the fused resample -> coadd kernel the last coadd of this context launched: 0 none yet,
 *                 1 k_coadd_fused_dma, 2 k_coadd_fused_own (bench.py labels its roofline with it)
 *   "dev_build"   1 when the library was compiled with -DZM_DEV (developer switches are read), else 0
 * No counterpart in the reference (its tools report through their logs, zuds/astromatic/makecoadd/default.swarp:111). */
int zm_ctx_query(zm_ctx* ctx, const char* what, int64_t* out);

/* SWarp's own edge and mask conventions as options of every resample / coadd call of this context (defaults: the
 * conventions of DESIGN.md section 2; both options are for pixel-for-pixel comparisons with real SWarp products and
 * make a stack take the materialised path - INTEGRATION.md says when to pick them):
 *   edge           ZM_EDGE_ZERO      an output pixel with a non-zero tap off the input frame gets value 0 / weight 0
 *                  ZM_EDGE_TRUNCATE  SWarp's truncated kernel: a pixel whose position lies on the frame is computed
 *                                    from the taps that are on it (zuds/astromatic/makecoadd/default.swarp:42-67)
 *   mask_resample  ZM_MASKRES_OR             OR of the mask words under the non-zero taps
 *                  ZM_MASKRES_LANCZOS_ROUND  the mask interpolated like an image and rounded, as SWarp does with
 *                                            mask.swarp (zuds/astromatic/makecoadd/mask.swarp:25, zuds/swarp.py:141-152) */
#define ZM_EDGE_ZERO 0
#define ZM_EDGE_TRUNCATE 1
#define ZM_MASKRES_OR 0
#define ZM_MASKRES_LANCZOS_ROUND 1
int zm_ctx_set_conventions(zm_ctx* ctx, int edge, int mask_resample);

/* ---- WCS helpers (host, fp64) ------------------------------------------ */
/* Output grid of a coadd: SWarp CENTER_TYPE ALL / PIXELSCALE_TYPE MEDIAN /
 * IMAGE_SIZE 0 (zuds/astromatic/makecoadd/default.swarp:40-49). */
int zm_autogrid(int nframes, const zm_wcs* wcs, zm_wcs* out);
/* pixel -> sky and sky -> pixel for n points (degrees, 1-based pixels). */
int zm_wcs_pix2sky(const zm_wcs* w, int n, const double* x, const double* y,
                   double* ra, double* dec);
int zm_wcs_sky2pix(const zm_wcs* w, int n, const double* ra, const double* dec,
                   double* x, double* y);
/* input-frame pixel of output pixels (the inverse map SWarp evaluates). */
int zm_wcs_map(const zm_wcs* wout, const zm_wcs* win, int n, const double* xo,
               const double* yo, double* xi, double* yi);
/* FLXSCALE x fixed pixel-area ratio (FSCALASTRO_TYPE FIXED, default.swarp:58). */
int zm_flux_scale(const zm_wcs* win, const zm_wcs* wout, double flxscale,
                  double* out);

/* ---- resample one image onto another grid ------------------------------ */
/* Replaces the SWarp run of run_align (zuds/swarp.py:157-204; HasWCS.aligned_to
 * zuds/fitsfile.py:290-314): Lanczos-3 by default, no background subtraction,
 * `wgt` NULL = WEIGHT_TYPE NONE.  out_wgt == 0 marks no-data pixels (bit 16,
 * zuds/mask.py:26-33).  mask/out_mask may be NULL. */
int zm_resample(zm_ctx* ctx, const float* img, const float* wgt,
                const int32_t* mask, const zm_wcs* win, const zm_wcs* wout,
                int kernel, double fscale, float* out_img, float* out_wgt,
                int32_t* out_mask);

/* ---- mesh background ----------------------------------------------------- */
/* Replaces `sex ... -CHECKIMAGE_TYPE BACKGROUND,BACKGROUND_RMS,-BACKGROUND`
 * (zuds/sextractor.py:110-150; used by zuds/hotpants.py:28 and
 * zuds/image.py:206) and SWarp's SUBTRACT_BACK (default.swarp:77-88).
 * wgt NULL = no weighting; any of out_bkg/out_rms/out_sub may be NULL.
 * out_stats[0..1] = global (backmean, backsig) = medians of the mesh maps. */
int zm_background(zm_ctx* ctx, const float* img, const float* wgt, int nx,
                  int ny, int mesh, int filtersize, float* out_bkg,
                  float* out_rms, float* out_sub, double* out_stats);

/* ---- coadd ---------------------------------------------------------------- */
/* Mask planes are integer bit masks (zuds/mask.py:26-72).  ZTF mask files are BITPIX 16: such a plane is
 * handed over as it is (mask_type = ZM_MASKTYPE_I16, `mask` points at int16_t) and is read as int16 by the
 * kernels - half the bytes over PCIe and from HBM; its values mean what numpy's astype(int32) would make
 * of them (sign extension).  mask_type = 0 (a zero-initialised struct): int32_t, as before. */
#define ZM_MASKTYPE_I32 0
#define ZM_MASKTYPE_I16 1
typedef struct zm_frame {
    const float* img;       /* [ny][nx] */
    const float* wgt;       /* inverse variance, NULL = WEIGHT_TYPE NONE */
    const void* mask;       /* int32_t (or int16_t, see mask_type) [ny][nx]; NULL = no mask */
    zm_wcs wcs;
    double flxscale;        /* FLXSCALE = 10^(-0.4 (MAGZP - 25)), zuds/swarp.py:31 */
    int32_t mask_type;      /* ZM_MASKTYPE_* */
    int32_t pad_;
} zm_frame;

typedef struct zm_coadd_params {
    int32_t combine;          /* ZM_COMBINE_*  (COMBINE_TYPE, default CLIPPED) */
    int32_t mask_combine;     /* ZM_MASK_*     (mask.swarp:25 AND; swarp.py:141 OR) */
    int32_t resample;         /* ZM_RESAMPLE_* (RESAMPLING_TYPE LANCZOS3) */
    int32_t subtract_back;    /* SUBTRACT_BACK Y */
    int32_t back_size;        /* -BACK_SIZE 128 (zuds/swarp.py:69) */
    int32_t back_filtersize;  /* BACK_FILTERSIZE 3 */
    int32_t rescale_weights;  /* RESCALE_WEIGHTS Y */
    int32_t pad_;
    double clip_sigma;        /* CLIP_SIGMA 4.0 */
    double clip_ampfrac;      /* CLIP_AMPFRAC 0.3 */
    double weight_thresh;     /* WEIGHT_THRESH 1e-30 */
} zm_coadd_params;

void zm_coadd_params_default(zm_coadd_params* p);

/* Replaces both SWarp runs of _coadd_from_images (zuds/coadd.py:126-163):
 * science coadd (prepare_swarp_sci, zuds/swarp.py:20-80) and mask coadd
 * (prepare_swarp_mask, zuds/swarp.py:83-104) on the grid `wout`.
 * out_mask may be NULL when no frame carries a mask; out_mask_wgt (may be NULL)
 * is the coverage map of the mask coadd (mskoutweightname, zuds/coadd.py:146-147)
 * from which the caller sets bit 16 (zuds/mask.py:26-33). */
int zm_coadd(zm_ctx* ctx, int nframes, const zm_frame* frames,
             const zm_wcs* wout, const zm_coadd_params* params, float* out_img,
             float* out_wgt, int32_t* out_mask, float* out_mask_wgt);

/* ---- subtraction ------------------------------------------------------------ */
typedef struct zm_hp_params {
    /* flags emitted by prepare_hotpants (zuds/hotpants.py:77-93) */
    double tu, tl, iu, il;    /* -tu -tl -iu -il valid data range */
    double r;                 /* -r   kernel half width (2.5 SEEING) */
    double rss;               /* -rss substamp half width (6 SEEING) */
    double fin;               /* -fin noise fill value (BIG_RMS) */
    double fi;                /* diff fill value, hotpants default 1e-30 */
    int32_t nsx, nsy;         /* -nsx -nsy stamps per region */
    int32_t nrx, nry;         /* -nrx -nry regions */
    int32_t ko, bgo;          /* -ko -bgo spatial orders (reference: 4, 0) */
    int32_t nss;              /* substamps per stamp (hotpants default 3) */
    int32_t normalize;        /* 0: -n i (reference), 1: -n t */
    double ft;                /* -ft  substamp threshold in sigma (20) */
    double ks;                /* -ks  stamp rejection sigma (2.0) */
    int32_t ngauss;           /* 3 */
    int32_t deg[4];           /* 6 4 2 */
    int32_t pad_[3];
    double sigma[4];          /* 0.7 1.5 3.0 */
    /* Round 4: lower data limits taken on the device.  When limits_dev is not NULL it points at the six doubles
     * zm_median_mad2_async_dev left in device memory ({median, 1.4826 MAD, count} of the science frame, then of
     * the template), and the subtraction uses il = median_a - limits_nsigma * sigma_a, tl = median_b -
     * limits_nsigma * sigma_b (zuds/hotpants.py:65-72: nsigma = 10) instead of the `il` / `tl` fields above:
     * the two quick_background_estimate calls and the fit are enqueued back to back, without the host reading
     * the estimates in between.  Device entry points only (zm_subtract_dev); NULL (zm_hp_params_default): the
     * fields above. */
    const double* limits_dev;
    double limits_nsigma;
    /* Round 4: the step behind hotpants folded into the call.  The reference sets bit 17 of the subtraction's mask
     * where hotpants left its fill value (zuds/subtraction.py:167-177: `submask[sub.data == 1e-30] |= 2**17`); when
     * flag_mask_dev is not NULL (device entry points only) the call enqueues exactly that - mask |= flag_bit where
     * out_diff == 1e-30f - behind the convolution, before it waits for the fit summary, instead of the caller
     * launching zm_mask_flag_dev after the call has returned (a launch with the GPU idle).  NULL: nothing. */
    int32_t* flag_mask_dev;
    int32_t flag_bit;
    /* Round 6: 1 = zm_subtract_dev returns when the LAST REJECTION ROUND has been seen by the host - the convolution,
     * the bit-17 pass and the copy of the fit summary are enqueued behind it, not waited for.  out_info then carries
     * status = ZM_HP_PENDING (niter, ncoeff, retries are final); zm_subtract_info(ctx, &info) waits for the rest and
     * fills it in.  The caller's next launches on the stream (the next coadd, the next job's alignment) are enqueued
     * while the convolution runs.  A barrier time-out of the solver makes the call fall back to the synchronous
     * form (the fit is repeated, as ever).  0 (zm_hp_params_default): wait, as rounds 1 - 5 did.  Device entry
     * point only; zm_subtract ignores it. */
    int32_t async_info;
} zm_hp_params;

void zm_hp_params_default(zm_hp_params* p);

typedef struct zm_hp_info {
    int32_t nstamps_total, nstamps_used;
    int32_t niter, ncoeff;
    double kernel_sum;        /* mean kernel sum over regions */
    double chi2;              /* mean figure of merit of the used stamps */
    int32_t nmasked;          /* output pixels filled with `fi` */
    int32_t status;           /* 0, or ZM_HP_* bits */
    int32_t nunsolved;        /* regions without a usable fit (filled with `fi`) */
    int32_t retries;          /* fits repeated after a solver barrier timed out (see below) */
} zm_hp_info;
/* status bits.  The reference sees a failed hotpants as a non-zero exit (CalledProcessError,
 * zuds/subtraction.py:162); here: ZM_HP_UNSOLVED = a region of the fit had no usable stamps or a
 * normal matrix that is not positive definite - a property of the data, the call still returns 0
 * and the region carries the fill value.  ZM_HP_TIMEOUT is reserved (never set): a barrier of the
 * many-workgroup factorisation that times out makes the fit repeat on the one-workgroup form, which
 * has no barrier that could time out - `retries` counts such repeats. */
#define ZM_HP_UNSOLVED 1
#define ZM_HP_TIMEOUT 2
#define ZM_HP_PENDING 4       /* zm_hp_params.async_info: the summary is still on its way - zm_subtract_info */

/* Replaces the hotpants run of Subtraction.from_images
 * (zuds/subtraction.py:144-162; flags zuds/hotpants.py:77-93): convolve the
 * template (-c t), D = I - (T (x) K + bg), noise = sqrt(sI^2 + sT^2 (x) K^2),
 * masked pixels filled with fi / fin (zuds/subtraction.py:170-171).
 * sci/ref and their rms maps are on the same grid; bpm is the boolean
 * bad-pixel map (zuds/subtraction.py:141-142), may be NULL. */
int zm_subtract(zm_ctx* ctx, const float* sci, const float* sci_rms,
                const float* ref, const float* ref_rms, const uint8_t* bpm,
                int nx, int ny, const zm_hp_params* params, float* out_diff,
                float* out_rms, zm_hp_info* out_info);

/* ---- robust statistics ---------------------------------------------------- */
/* Replaces quick_background_estimate (zuds/utils.py:32-53): median and
 * 1.4826 MAD of the pixels whose mask is 0 (mask NULL = all). */
int zm_median_mad(zm_ctx* ctx, const float* img, const int32_t* mask, int64_t n,
                  double* out_median, double* out_mad_sigma);
int zm_median_mad_dev(zm_ctx* ctx, const float* img, const int32_t* mask,
                      int64_t n, double* out_median, double* out_mad_sigma);
/* The two estimates prepare_hotpants needs (science and aligned reference,
 * zuds/hotpants.py:65-67) in one set of launches: out4 = {median_a, mad_a,
 * median_b, mad_b}.  Both images have n pixels. */
int zm_median_mad2_dev(zm_ctx* ctx, const float* img_a, const int32_t* mask_a,
                       const float* img_b, const int32_t* mask_b, int64_t n,
                       double* out4);
/* The same two estimates left on the device (round 4): out6_dev receives {median_a, sigma_a, count_a, median_b,
 * sigma_b, count_b} as doubles when the stream reaches that point; nothing is copied back, nothing is waited
 * for.  A frame without a single valid pixel has count 0 (the host entry points raise; here the caller looks
 * at the counts when it reads the estimates).  Consumer: zm_hp_params.limits_dev. */
int zm_median_mad2_async_dev(zm_ctx* ctx, const float* img_a, const int32_t* mask_a,
                             const float* img_b, const int32_t* mask_b, int64_t n, double* out6_dev);

/* ---- forced aperture photometry ------------------------------------------- */
/* Replaces photutils.aperture_photometry(method='exact') + the bounding-box flag
 * OR of raw_aperture_photometry / aperture_photometry (zuds/photometry.py:61-113,
 * 116-249): x, y are 0-based pixel positions, radius in pixels (APERTURE_RADIUS = 3,
 * zuds/constants.py:14); flux = sum(img frac), err = sqrt(sum(rms^2 frac)),
 * flags = OR of mask over the aperture bounding box.  rms / mask may be NULL. */
int zm_aperture_photometry(zm_ctx* ctx, const float* img, const float* rms,
                           const int32_t* mask, int nx, int ny, int npos,
                           const double* x, const double* y, double radius,
                           double* out_flux, double* out_err, int32_t* out_flags);
int zm_aperture_photometry_dev(zm_ctx* ctx, const float* img, const float* rms,
                               const int32_t* mask, int nx, int ny, int npos,
                               const double* x, const double* y, double radius,
                               double* out_flux, double* out_err, int32_t* out_flags);

/* ---- photometric calibration (csrc/photcal.hip; DESIGN.md "Photometric calibration") ---- */
/* zm_growth: curves of growth with a local sky, one wave per star.  x, y: 0-based positions; radii: naper (1 .. 8)
 * ascending aperture radii in pixels, HOST memory in both forms; the sky annulus is the pixels whose centres lie at
 * r_in <= d < r_out (r_out <= ZM_GROWTH_ROUT_MAX), clipped to the frame; a pixel is usable when it is finite and
 * (mask & bad_bits) == 0.  Sky: exact median of the usable float32 values (even count: mean of the two middle values in
 * double), sky_sigma = 1.4826 x the exact median of |v - sky|; values with |v - sky| > kappa x sky_sigma are dropped
 * and the two are taken again, until nothing is dropped or maxiter times.  nsky: the survivors; none: sky and
 * sky_sigma NaN, every flux and err NaN.  Sums run over the bounding box of the largest radius, clipped as
 * zm_aperture_photometry clips it: flux[s * naper + k] = sum((img - sky) frac_k) in fp64, err = sqrt(sum(rms^2
 * frac_k)), or sqrt(sum(frac_k)) x sky_sigma when rms is NULL.  An rms value that is not finite (NaN or +-inf) makes NaN
 * every err whose circle its pixel touches.  A pixel "touches" radius r when its nearest point to
 * the centre lies nearer than r; a pixel that does not touch contributes nothing, one whose farthest corner lies
 * within r counts whole.  flags: ZM_GROWTH_* below.  A position that is not finite: every output NaN, nsky 0, flags
 * ZM_GROWTH_BADPOS.  saturate <= 0: no saturation test.  nstar == 0: returns at once, writes nothing.
 * The host form stages the planes as zm_aperture_photometry does; the _dev form only enqueues on the stream. */
#define ZM_GROWTH_NAPER_MAX 8
#define ZM_GROWTH_ROUT_MAX 20.0
#define ZM_GROWTH_BAD 1         /* a pixel with mask & bad_bits touches the largest aperture */
#define ZM_GROWTH_SATURATED 2   /* a pixel >= saturate touches the largest aperture */
#define ZM_GROWTH_NONFINITE 4   /* a non-finite pixel touches the largest aperture; every flux whose circle it touches is NaN */
#define ZM_GROWTH_BOXCLIP 8     /* the box of the largest aperture was clipped by the frame */
#define ZM_GROWTH_ANNCLIP 16    /* the annulus was clipped by the frame */
#define ZM_GROWTH_FEWSKY 32     /* nsky < nsky_min (the fluxes are still reported) */
#define ZM_GROWTH_BADPOS 64     /* the position is not finite */
int zm_growth(zm_ctx* ctx, const float* img, const float* rms, const int32_t* mask, int32_t bad_bits,
              float saturate, int nx, int ny, int nstar, const double* x, const double* y, int naper,
              const double* radii, double r_in, double r_out, double kappa, int maxiter, int nsky_min,
              double* out_flux, double* out_err, double* out_sky, double* out_sky_sigma, int32_t* out_nsky,
              int32_t* out_flags);
int zm_growth_dev(zm_ctx* ctx, const float* img, const float* rms, const int32_t* mask, int32_t bad_bits,
                  float saturate, int nx, int ny, int nstar, const double* x, const double* y, int naper,
                  const double* radii, double r_in, double r_out, double kappa, int maxiter, int nsky_min,
                  double* out_flux, double* out_err, double* out_sky, double* out_sky_sigma, int32_t* out_nsky,
                  int32_t* out_flags);
/* zm_clipped_median: a clipped median per column, one workgroup per column.  values: n rows of ncol doubles, row
 * stride `stride` elements (>= ncol); an entry that is not finite is not used.  The same iteration as the sky of
 * zm_growth (median, 1.4826 x MAD, strict drop; maxiter 0: the plain median and MAD).  out[4 * c ..] = {median, sigma,
 * n_used, n_valid}; n_valid 0 (or nothing left): median and sigma NaN.  n <= ZM_CLIPMED_NMAX: the column lies in LDS. */
#define ZM_CLIPMED_NMAX 16384
int zm_clipped_median(zm_ctx* ctx, const double* values, int n, int ncol, int64_t stride, double kappa, int maxiter,
                      double* out);
int zm_clipped_median_dev(zm_ctx* ctx, const double* values, int n, int ncol, int64_t stride, double kappa,
                          int maxiter, double* out);
/* zm_maglim_dev: the noise in an aperture over a lattice, for the limiting magnitude.  Centres (0-based) at
 * step / 2 + i step in x and y, kept where the centre lies at least radius + 1 pixels from every edge of the frame
 * (the frame spans -0.5 .. n - 0.5); sigma_ap = sqrt(sum(rms^2 frac)).  A point is used when no pixel of its aperture
 * box has mask & bad_bits and every rms value in the box is finite and positive.  out3_dev (device) = {median sigma_ap
 * of the used points (NaN: none), number used, number of lattice points}.  More than ZM_CLIPMED_NMAX lattice points:
 * an error, take a coarser step.  mask may be NULL. */
int zm_maglim_dev(zm_ctx* ctx, const float* rms, const int32_t* mask, int32_t bad_bits, int nx, int ny,
                  double radius, int step, double* out3_dev);

/* ---- device-pointer entry points (bench, multi-GPU, pipelines) ----------- */
/* Same arithmetic as above on device-resident buffers; enqueue only. */
typedef struct zm_dframe {
    const float* img;       /* device */
    const float* wgt;       /* device or NULL */
    const void* mask;       /* device int32_t / int16_t plane (mask_type) or NULL */
    zm_wcs wcs;
    double flxscale;
    int32_t mask_type;      /* ZM_MASKTYPE_* */
    int32_t pad_;
} zm_dframe;

/* Resample + combine nframes device frames; outputs are device planes.
 * If `partial` != 0 the outputs are the partial sums S1 = sum(w v) (out_img)
 * and S0 = sum(w) (out_wgt) of a WEIGHTED coadd, ready for an RCCL
 * all-reduce across ranks followed by zm_coadd_finalize_dev. */
int zm_coadd_dev(zm_ctx* ctx, int nframes, const zm_dframe* frames,
                 const zm_wcs* wout, const zm_coadd_params* params,
                 int partial, float* out_img, float* out_wgt, int32_t* out_mask,
                 float* out_mask_wgt);
int zm_coadd_finalize_dev(zm_ctx* ctx, float* s1_to_img, const float* s0,
                          int64_t npix);
/* Mask coadd across ranks: zm_coadd_dev(partial = 1) leaves -1 ("no frame of this rank
 * covers the pixel") in out_mask instead of finalising it.  zm_mask_accum_dev folds
 * another partial mask in (AND / OR over the covering frames, -1 = identity; first != 0
 * initialises acc from m), zm_mask_finalize_dev turns the marker into 0 and writes the
 * coverage plane (cov may be NULL) - the mask SWarp run of zuds/swarp.py:83-104 sharded
 * by frame.  -1 is the marker and nothing else: a real mask value of -1 (all 32 bits set), in m or
 * as the OR of covering frames, cannot be told from "not covered" and is folded as such. */
int zm_mask_accum_dev(zm_ctx* ctx, int32_t* acc, const int32_t* m, int64_t npix,
                      int kind, int first);
int zm_mask_finalize_dev(zm_ctx* ctx, int32_t* acc, float* cov, int64_t npix);
/* ---- multi-GPU: the exchange step of a frame-sharded coadd on RCCL (one process per GPU) ----
 * The reference has no collective: it shards by job (zuds/mpi.py:36-64, nersc/controller.py:101);
 * BASELINE config 4 shards the FRAMES of one stack, and these calls are the reduce that adds.
 * librccl is opened on first use.  zm_comm_unique_id on rank 0, the 128 bytes handed to every rank
 * by the launcher (MPI broadcast, torch.distributed, a file), zm_comm_init on every rank.
 * zm_coadd_reduce_dev: sum-reduce of S1 / S0, the two planes of ONE buffer of 2 npix floats as
 * zm_coadd_dev(partial = 1) fills them when out_wgt == out_img + npix; then zm_coadd_finalize_dev.
 * zm_mask_reduce_dev: the partial masks (-1 marker) of all ranks folded with AND / OR by row
 * bands, every rank ends with the finalised mask (cov may be NULL).  All enqueue on the stream.
 * A communicator holds at most ZM_COMM_MAX_RANKS (64) ranks: zm_comm_init refuses more. */
#define ZM_COMM_ID_BYTES 128
typedef struct zm_comm zm_comm;
int zm_comm_unique_id(void* id128);
int zm_comm_init(zm_ctx* ctx, int nranks, int rank, const void* id128, zm_comm** out);
int zm_comm_destroy(zm_comm* comm);
int zm_coadd_reduce_dev(zm_ctx* ctx, zm_comm* comm, float* s1s0, int64_t npix);
int zm_mask_reduce_dev(zm_ctx* ctx, zm_comm* comm, int32_t* mask, int nx, int ny, int kind,
                       float* cov);
/* Host arithmetic of the banded schedule, callable without a GPU (tests replay it for every rank):
 * zm_comm_band_bounds: rows [bounds[g], bounds[g + 1]) belong to rank g, g < world - the split of
 * np.array_split / zuds/mpi.py:36-64 (bounds: world + 1 entries).
 * zm_comm_mask_plan: what zm_mask_reduce_dev sends / receives / gathers for one rank, in elements. */
#define ZM_COMM_MAX_RANKS 64
typedef struct {
    int32_t world, rank;
    int64_t band_px;                          /* slot size: rows of the largest band x nx */
    int64_t my_px;                            /* this rank's band */
    int64_t send_off[ZM_COMM_MAX_RANKS];      /* band g of this rank's plane (offset, count) -> rank g */
    int64_t send_cnt[ZM_COMM_MAX_RANKS];
    int64_t recv_off[ZM_COMM_MAX_RANKS];      /* slot of rank g in the receive buffer, my_px elements each */
    int64_t recv_cnt[ZM_COMM_MAX_RANKS];
    int64_t gather_off[ZM_COMM_MAX_RANKS];    /* folded band of rank g in the all-gather buffer */
} zm_mask_plan;
int zm_comm_band_bounds(int nrows, int world, int32_t* bounds);
int zm_comm_mask_plan(int nx, int ny, int world, int rank, zm_mask_plan* plan);
/* Resample the frames to `wout` into a resident stack [nframes][ony][onx][2]
 * of (value, weight) pairs (the CLIPPED multi-GPU exchange operates on it).
 * out_mask_partial (may be NULL): the mask coadd of these frames with the -1 marker
 * left in, as zm_coadd_dev(partial = 1) leaves it. */
int zm_resample_stack_dev(zm_ctx* ctx, int nframes, const zm_dframe* frames,
                          const zm_wcs* wout, const zm_coadd_params* params,
                          float* stack, int32_t* out_mask_partial);
/* Combine a resident stack; rows [row0, row0+nrows) of every frame. */
int zm_combine_stack_dev(zm_ctx* ctx, int nframes, const float* stack,
                         int64_t frame_stride_px, int64_t npix,
                         const zm_coadd_params* params, float* out_img,
                         float* out_wgt);
int zm_subtract_dev(zm_ctx* ctx, const float* sci, const float* sci_rms,
                    const float* ref, const float* ref_rms, const uint8_t* bpm,
                    int nx, int ny, const zm_hp_params* params, float* out_diff,
                    float* out_rms, zm_hp_info* out_info_host);
/* The summary of the subtraction this context last ran with zm_hp_params.async_info = 1: waits for its convolution
 * and the copy of the summary, then fills out_info as the synchronous call would have.  An error when nothing is
 * pending.  (What `hotpants` prints at its end and Subtraction.from_images keeps in the header:
 * zuds/subtraction.py:144-177.) */
int zm_subtract_info(zm_ctx* ctx, zm_hp_info* out_info);
/* Many subtractions, one call (round 4; the reference runs one hotpants process per job, 64 per node:
 * nersc/controller.py:101, scripts/donightly.py:21-40 -> zuds/subtraction.py:144-162).  Every job is what
 * zm_subtract_dev takes - planes of nx x ny pixels in device memory, its own flags (`params`: the data limits
 * and fill values may differ from job to job; everything that shapes the fit - half widths, basis, orders,
 * regions, stamps, thresholds - has to agree, else the call returns non-zero) - and gets the same bits.  The
 * kernel fit of all jobs runs as ONE chain of launches with the job as a grid dimension (a job that has
 * converged rides along as empty workgroups), on the one-workgroup-per-region factorisation; validity masks,
 * stamp search and the final convolution are enqueued job after job.  out_info_host: njobs entries.  A
 * configuration the batched kernels do not cover (more than 15 spatial kernel terms, more than 960 unknowns or
 * 256 stamps per region) runs job by job through zm_subtract_dev.  1 <= njobs <= ZM_SUB_BATCH_MAX. */
#define ZM_SUB_BATCH_MAX 64
typedef struct zm_sub_job {
    const float* sci;          /* background-subtracted science frame (+ pedestal) */
    const float* sci_rms;
    const float* ref;          /* template on the science grid */
    const float* ref_rms;
    const uint8_t* bpm;        /* boolean bad-pixel map or NULL */
    const zm_hp_params* params;
    float* out_diff;
    float* out_rms;
} zm_sub_job;
int zm_subtract_batch_dev(zm_ctx* ctx, int njobs, const zm_sub_job* jobs, int nx, int ny,
                          zm_hp_info* out_info_host);
/* The same on host planes (every pointer of a job in host memory; `params->limits_dev` must be NULL): staged to
 * the device, subtracted as one batch, products copied back - zm_subtract for many frames of one configuration. */
int zm_subtract_batch(zm_ctx* ctx, int njobs, const zm_sub_job* jobs, int nx, int ny,
                      zm_hp_info* out_info);
int zm_background_dev(zm_ctx* ctx, const float* img, const float* wgt, int nx,
                      int ny, int mesh, int filtersize, float* out_bkg,
                      float* out_rms, float* out_sub, double* out_stats_host);
int zm_resample_dev(zm_ctx* ctx, const float* img, const float* wgt,
                    const int32_t* mask, const zm_wcs* win, const zm_wcs* wout,
                    int kernel, double fscale, float* out_img, float* out_wgt,
                    int32_t* out_mask);

/* Two images that share a geometry through one resampling launch (device pointers): what the reference does in two
 * SWarp runs when it aligns a reference image and that image's rms map to a science grid (zuds/subtraction.py:109 ->
 * zuds/fitsfile.py:290-314, zuds/hotpants.py:51).  img_a (optionally with its int32 mask: OR under the footprint,
 * into out_mask) and img_b; no weights (WEIGHT_TYPE NONE); out_b is scaled by fscale_b.  Values equal those of two
 * zm_resample_dev calls bit for bit; uncovered pixels are 0 in both outputs; no weight planes. */
int zm_align_pair_dev(zm_ctx* ctx, const float* img_a, const float* img_b, const int32_t* mask,
                      const zm_wcs* win, const zm_wcs* wout, int kernel, double fscale_a, double fscale_b,
                      float* out_a, float* out_b, int32_t* out_mask);
/* zm_resample / zm_resample_dev for a BITPIX 16 mask plane (run_align on a ZTF mask, zuds/swarp.py:157-204):
 * the int16 plane crosses PCIe as it is and is widened on the device; out_mask stays int32 (bit 16 / 17 of
 * the products, zuds/mask.py:26-33, zuds/subtraction.py:170-171). */
int zm_resample_i16(zm_ctx* ctx, const float* img, const float* wgt,
                    const int16_t* mask, const zm_wcs* win, const zm_wcs* wout,
                    int kernel, double fscale, float* out_img, float* out_wgt,
                    int32_t* out_mask);
int zm_resample_i16_dev(zm_ctx* ctx, const float* img, const float* wgt,
                        const int16_t* mask, const zm_wcs* win, const zm_wcs* wout,
                        int kernel, double fscale, float* out_img, float* out_wgt,
                        int32_t* out_mask);
/* out[i] = (int32_t) in[i] (sign extension), n elements, device planes. */
int zm_mask_widen_dev(zm_ctx* ctx, const int16_t* in, int64_t n, int32_t* out);

/* ---- per-pixel bookkeeping on device planes ---------------------------------- */
/* rms = 1/sqrt(w), big_rms where bad or w <= 0 (zuds/image.py:173-208; the reference's numpy gives inf for a
 * zero weight on a pixel its mask does not flag - the object layer restores that, subtraction.py). */
int zm_rms_from_weight_dev(zm_ctx* ctx, const float* wgt, const uint8_t* bad,
                           int64_t n, float big_rms, float* out);
/* w = 1/rms^2, 0 where bad or img >= satur (0.9 SATURATE; zuds/image.py:136-171). */
int zm_weight_from_rms_dev(zm_ctx* ctx, const float* rms, const uint8_t* bad,
                           const float* img, float satur, int64_t n, float* out);
/* The false weight map of a background run without weights (zuds/sextractor.py:80-96: 1, 0 where the mask has a
 * bad bit, 0 in a `border`-pixel frame for raw science images) and / or the boolean bad-pixel map of the mask
 * (zuds/mask.py:42-72); mask_type ZM_MASKTYPE_I32 / _I16.  What `rms_image` / `weight_image` of a frame without
 * .rms.fits / .weight.fits need in front of zm_background_dev and zm_weight_from_rms_dev (zuds/image.py:136-208). */
int zm_false_weight_dev(zm_ctx* ctx, const void* mask, int mask_type, int32_t badsum, int border,
                        int nx, int ny, float* out_wgt, uint8_t* out_bpm);
/* out_or = a | b (b may be NULL); out_bpm = (out_or & badsum) != 0
 * (zuds/subtraction.py:135-142, zuds/mask.py:42-72). */
int zm_mask_bad_dev(zm_ctx* ctx, const int32_t* a, const int32_t* b,
                    int32_t badsum, int64_t n, int32_t* out_or, uint8_t* out_bpm);
/* mask |= bit where img == value: bit 16 from weight == 0 (zuds/mask.py:26-33),
 * bit 17 from diff == 1e-30 (zuds/subtraction.py:170-171). */
int zm_mask_flag_dev(zm_ctx* ctx, int32_t* mask, const float* img, float value,
                     int32_t bit, int64_t n);
/* img += v: the 150-count pedestal (zuds/coadd.py:205-206, zuds/hotpants.py:29). */
int zm_add_scalar_dev(zm_ctx* ctx, float* img, float v, int64_t n);
/* Measurement aid ("an achieved-copy ceiling with a float4 copy kernel"): dst = src,
 * nbytes a multiple of 16, 16-byte aligned device pointers, on the context's stream.  bench.py times it
 * and reports the roofline kernel against the rate it reaches as well as against the nominal 8 TB/s. */
int zm_copy_probe_dev(zm_ctx* ctx, const void* src, void* dst, int64_t nbytes);

/* ---- seeing estimate and detection cuts from pixels -------------------------- */
/* Pixel-only stand-ins for the parts of estimate_seeing (zuds/seeing.py:10-118) and
 * filter_sexcat (zuds/filterobjects.py:57-195) that the reference feeds from SExtractor
 * catalogs and Gaia queries.
 * zm_find_stars: isolated local maxima (strict over the (2 isolation + 1)^2 box, ties to the
 *   first pixel in raster order) with thresh_lo < peak < thresh_hi, no bad (bad[] != 0) or
 *   NaN pixel in the box, at least `border` pixels from the edges.  Unordered; *out_n is the
 *   number found (may exceed max_out: only max_out are returned).
 * zm_star_fwhm: FWHM (pixels) and centroid of each star from adaptive Gaussian-weighted
 *   second moments in a (2 half + 1)^2 window; NaN when the iteration fails.
 * zm_negpix_test: out_bad[k] = 1 when the 11 x 11 cutout around (X_IMAGE, Y_IMAGE) (1-based)
 *   holds a pixel below median - 5 sigma with a 3 x 3 neighbour above median + 5 sigma. */
int zm_find_stars(zm_ctx* ctx, const float* img, const uint8_t* bad, int nx, int ny,
                  float thresh_lo, float thresh_hi, int isolation, int border,
                  int max_out, int* out_x, int* out_y, float* out_peak, int* out_n);
int zm_star_fwhm(zm_ctx* ctx, const float* img, int nx, int ny, int nstar,
                 const int* x, const int* y, int half, double* out_fwhm,
                 double* out_cx, double* out_cy);
int zm_negpix_test(zm_ctx* ctx, const float* img, int nx, int ny, int npos,
                   const double* x, const double* y, double median, double sigma,
                   int32_t* out_bad);
/* The two star measurements on planes that are already in HBM (img / bad: device pointers; positions, widths
 * and lists: host arrays): the seeing of a coadd is estimated before it leaves the device. */
int zm_find_stars_dev(zm_ctx* ctx, const float* img, const uint8_t* bad, int nx, int ny,
                      float thresh_lo, float thresh_hi, int isolation, int border,
                      int max_out, int* out_x, int* out_y, float* out_peak, int* out_n);
int zm_star_fwhm_dev(zm_ctx* ctx, const float* img, int nx, int ny, int nstar,
                     const int* x, const int* y, int half, double* out_fwhm,
                     double* out_cx, double* out_cy);
/* The three pixel cuts of filter_sexcat (zuds/filterobjects.py:83-195) on planes that are already in HBM (d_img,
 * d_rms, d_mask: device pointers; everything else: host arrays).  x, y: X_IMAGE / Y_IMAGE, 1-based, handed to the
 * r = 6 aperture unchanged as the reference does.  Per candidate: out_bpmcut = exact-overlap aperture sum of
 * (mask & bad_bits) != 0, out_rmscut = aperture sum of d_rms / (pi 36), out_negpix = the dipole test of
 * zm_negpix_test.  out_stats = {medcut, immed, imsig}: 1.1 x the median of d_rms over (mask & bad_bits) == 0, the
 * median of d_img over all pixels, 1.48 x its MAD; taken on the device and read by the cuts from device memory.
 * A position that is not finite gives zero sums and negpix 0.  npos == 0 returns at once and writes nothing.
 * Fails when no pixel is good or the image has no spread (imsig = 0). */
int zm_candidate_cuts_dev(zm_ctx* ctx, const float* d_img, const float* d_rms, const int32_t* d_mask,
                          int32_t bad_bits, int nx, int ny, int npos, const double* x, const double* y,
                          double* out_bpmcut, double* out_rmscut, int32_t* out_negpix, double* out_stats);

/* ---- source extraction: detection catalog and segmentation map -------------- */
/* Replaces the SExtractor run of PipelineFITSCatalog.from_image (zuds/catalog.py:96-130) with the
 * settings of zuds/astromatic/sextractor.conf.  The arithmetic is a chosen convention (DESIGN.md,
 * "Source extraction"; restated in tests/extract_ref.py):
 *   a pixel is bad if bad != 0, img or sigma is not finite, or sigma <= 0;
 *   filter       3 x 3 [1 2 1; 2 4 2; 1 2 1] / 16 (default.conv), bad and outside pixels enter as 0,
 *                float32 sums in row-major tap order (filter = 0: the image itself);
 *   foreground   not bad and filtered > (float)detect_thresh * sigma;
 *   objects      8-connected components of at least detect_minarea pixels, numbered 1 .. n in raster
 *                order of their first pixel; no deblending, no cleaning;
 *   measurements isophotal, float64 sums in a fixed order; apertures with zm_aperture_photometry_dev. */
typedef struct zm_extract_params {
    float detect_thresh;     /* DETECT_THRESH, in units of sigma (1.5) */
    float satur_level;       /* SATUR_LEVEL (50000) */
    int32_t detect_minarea;  /* DETECT_MINAREA (5) */
    int32_t filter;          /* 1: default.conv (FILTER Y), 0: none (FILTER N) */
    double aper_radius;      /* PHOT_APERTURES / 2 (3 px) */
} zm_extract_params;
void zm_extract_params_default(zm_extract_params* p);

#define ZM_EXTRACT_CHAIN 1       /* status bit: a label chain passed its bound (results are not to be used) */

/* One row of the object table.  Pixel coordinates are 1-based (SExtractor's *_IMAGE). */
typedef struct zm_object {
    int32_t number;          /* NUMBER */
    int32_t npix;            /* ISOAREA_IMAGE */
    int32_t xmin, xmax, ymin, ymax;   /* XMIN_IMAGE .. YMAX_IMAGE */
    int32_t flags;           /* FLAGS: 2 deblended (with deblending only), 4 saturated, 8 on the frame border, 16 aperture incomplete */
    int32_t flags_weight;    /* FLAGS_WEIGHT: 1 = a bad pixel touches the object */
    int32_t imaflags_iso;    /* IMAFLAGS_ISO: OR of the flag plane over the object */
    int32_t first;           /* 0-based linear index of the object's first pixel in raster order */
    int32_t nthresh;         /* pixels at or above the level FWHM_IMAGE is measured at */
    int32_t pad_;
    double x_image, y_image; /* barycentre of the filtered values */
    double x2, y2, xy;       /* central second moments */
    double a_image, b_image, theta_image, elongation;
    double fwhm_image;
    double flux_iso, flux_max;   /* unfiltered values */
    double peak;             /* largest filtered value */
    double flux_aper, fluxerr_aper;
    double x_world, y_world; /* NaN without a WCS */
} zm_object;

/* img, sigma, bad (uint8, may be NULL), flag (int32, may be NULL): device planes of nx x ny pixels.
 * out_rows: host array of max_objects rows (may be NULL when max_objects is 0).  segm_dev (int32) and
 * filtered_dev (float32): optional device planes.  More objects than max_objects is not an error: the
 * first max_objects in NUMBER order are written (*out_nwritten), the segmentation map holds all of them
 * and *out_nfound is the total.  *out_status (may be NULL): 0, or ZM_EXTRACT_* bits. */
int zm_extract_dev(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                   const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                   const zm_extract_params* params, int max_objects, zm_object* out_rows,
                   int32_t* segm_dev, float* filtered_dev, int* out_nwritten, int* out_nfound,
                   int* out_status);
/* The same with host planes (out_segm / out_filtered: host arrays or NULL). */
int zm_extract(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
               const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
               const zm_extract_params* params, int max_objects, zm_object* out_rows,
               int32_t* out_segm, float* out_filtered, int* out_nwritten, int* out_nfound,
               int* out_status);

/* ---- source extraction with multi-threshold deblending (opt-in) -------------- */
/* DEBLEND_NTHRESH / DEBLEND_MINCONT of sextractor.conf.  zm_extract and its results are what they were; these entry
 * points run the same first pass and then split every object whose tree of nthresh exponentially spaced levels has at
 * least two significant branches ("Deblending"; restated in tests/deblend_ref.py).  Objects, split or not, are
 * renumbered 1 .. n in raster order of their first pixel and measured on their own pixels; the sub-objects of a split
 * parent carry FLAGS bit 2.  Where nothing splits, rows and map equal those of zm_extract bit for bit.  The CLEAN pass
 * that folds shreds back is a step of its own (zm_extract_clean, below). */
typedef struct zm_deblend_params {
    int32_t nthresh;         /* DEBLEND_NTHRESH (32): a power of two in 2 .. 64 */
    int32_t pad_;
    double mincont;          /* DEBLEND_MINCONT (0.005): in [0, 1] */
} zm_deblend_params;
void zm_deblend_params_default(zm_deblend_params* p);

#define ZM_EXTRACT_DEBLEND 2     /* status bit: a loop of the deblending kernel reached its bound (results are not to be used) */

/* The arguments of zm_extract_dev, then the deblending parameters and out_parent (host array of max_objects int32, or
 * NULL): the first-pass NUMBER of the object each row was part of. */
int zm_extract_deblend_dev(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                           const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                           const zm_extract_params* params, int max_objects, zm_object* out_rows,
                           int32_t* segm_dev, float* filtered_dev, int* out_nwritten, int* out_nfound,
                           int* out_status, const zm_deblend_params* deblend, int32_t* out_parent);
/* The same with host planes. */
int zm_extract_deblend(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                       const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                       const zm_extract_params* params, int max_objects, zm_object* out_rows,
                       int32_t* out_segm, float* out_filtered, int* out_nwritten, int* out_nfound,
                       int* out_status, const zm_deblend_params* deblend, int32_t* out_parent);

/* ---- source extraction with the CLEAN pass (opt-in) --------------------------- */
/* CLEAN Y / CLEAN_PARAM of sextractor.conf.  The entry points above and their results are what they were.  These run the
 * same passes (deblend == NULL: no deblending), then let every object be absorbed by the neighbour whose Moffat-like wing
 * amp (1 + alpha q)^-param, as high as the detection threshold at the neighbour's isophotal area, exceeds what the object
 * holds above its local threshold on its detect_minarea-th brightest pixel ("CLEAN"; restated in
 * tests/clean_ref.py).  One round on the quantities from before any merge; an absorbed object still absorbs; every object
 * ends at the root of its chain.  Merged objects are renumbered 1 .. n in raster order of their first pixel and measured
 * on the union of their pixels.  Where nothing is absorbed, rows and map equal those of the call without CLEAN bit for
 * bit.  FLAGS bit 2 and out_parent follow the rule of zm_extract_deblend on the final rows: a parent that was split keeps
 * bit 2 even where CLEAN folds all its pieces back. */
typedef struct zm_clean_params {
    double param;            /* CLEAN_PARAM (1.0): the wing's exponent, finite, in [0.1, 10] */
} zm_clean_params;
void zm_clean_params_default(zm_clean_params* p);

#define ZM_EXTRACT_CLEAN 4       /* status bit: a chain of absorptions passed its bound (results are not to be used) */

/* The arguments of zm_extract_deblend_dev (deblend and out_parent may be NULL), then the CLEAN parameters and out_nmerged
 * (host array of max_objects int32, or NULL): the objects from before CLEAN that a row holds, 1 = untouched.  CLEAN sees
 * every object of the pass before, whatever max_objects is: max_objects truncates the final table alone. */
int zm_extract_clean_dev(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                         const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                         const zm_extract_params* params, int max_objects, zm_object* out_rows,
                         int32_t* segm_dev, float* filtered_dev, int* out_nwritten, int* out_nfound,
                         int* out_status, const zm_deblend_params* deblend, const zm_clean_params* clean,
                         int32_t* out_parent, int32_t* out_nmerged);
/* The same with host planes. */
int zm_extract_clean(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                     const int32_t* flag, int nx, int ny, const zm_wcs* wcs,
                     const zm_extract_params* params, int max_objects, zm_object* out_rows,
                     int32_t* out_segm, float* out_filtered, int* out_nwritten, int* out_nfound,
                     int* out_status, const zm_deblend_params* deblend, const zm_clean_params* clean,
                     int32_t* out_parent, int32_t* out_nmerged);
/* The per-object sums (k_cl_stats) of the last zm_extract_clean[_dev] call on this context, for the first
 * min(max_n, *out_n) objects from before CLEAN: F (float64 sum of the filtered values), T (threshold at the peak pixel)
 * and m (the detect_minarea-th largest excess over the local threshold).  Host arrays; any of them may be NULL. */
int zm_extract_clean_stats(zm_ctx* ctx, int max_n, double* fdflux, float* dthresh, float* mthresh, int* out_n);
/* The decision alone, on host arrays of n objects: rows (number == index + 1; x_image, y_image, a_image, b_image, x2, y2,
 * xy, npix and first are read), fdflux = F, dthresh = T, mthresh = m, minarea = DETECT_MINAREA (every npix is at least
 * that).  out_into[j]: the NUMBER of the object that absorbs j, 0 for none; out_root[j]: the NUMBER at the end of j's
 * chain (its own where it is not absorbed).  Either may be NULL. */
int zm_clean_decide(zm_ctx* ctx, int n, const zm_object* rows, const double* fdflux, const float* dthresh,
                    const float* mthresh, int minarea, const zm_clean_params* clean, int32_t* out_into,
                    int32_t* out_root);

/* ---- source extraction, second pass: the Kron and windowed columns of sextractor.param ---- */
/* Opt-in: zm_extract and its table are what they were.  Measures, for rows zm_extract wrote, the columns of
 * zuds/astromatic/sextractor.param that the isophotal table lacks ("The wide table"; restated in
 * tests/measure_ref.py).  All sums are float64 over the unfiltered image and the noise plane; bad pixels (the rule of
 * zm_extract) and pixels outside the frame are skipped; pixels of other objects are not masked (MASK_TYPE NONE).
 *   Kron      r1 = sum sqrt(r2) v / sum v over the ellipse r2 <= 36 of the isophotal moments; KRON_RADIUS =
 *             max(kron_fact r1, kron_min_radius); flux sums over r2 <= KRON_RADIUS^2, pixel centres, no sub-pixel weights
 *   windowed  w = (exact circle overlap, radius 4 sigma_win) x exp(-r^2 / (2 sigma_win^2)); the centre moves by twice
 *             the weighted first moment until the step is below 1e-4 px, 16 times at the most
 *   errors    errx2 = sum sigma^2 dx^2 / (sum f)^2 over the member pixels (f: the filtered value), likewise y2, xy */
typedef struct zm_measure_params {
    double kron_fact;        /* PHOT_AUTOPARAMS, first value (2.5) */
    double kron_min_radius;  /* PHOT_AUTOPARAMS, second value (3.5) */
    int32_t filter;          /* MUST equal zm_extract_params.filter of the run that made the rows: the error sums
                              * recompute that run's filtered values f from the planes; another value gives
                              * errx2 / erry2 / errxy (and ERR*_WORLD) of a detection image that was never used */
    int32_t pad_;
} zm_measure_params;
void zm_measure_params_default(zm_measure_params* p);

#define ZM_AUTO_SKIPPED 1        /* flags_auto: more than 10 % of the Kron ellipse's pixels in the frame were skipped */
#define ZM_AUTO_OFFFRAME 2       /* ... the Kron ellipse leaves the frame */
#define ZM_AUTO_MINRADIUS 4      /* ... r1 = 0: the minimum radius for lack of positive sums */
#define ZM_WIN_FALLBACK 1        /* flags_win: the window's weighted sum was not positive: isophotal values */
#define ZM_WIN_NOTCONVERGED 2    /* ... the step after the 16th iteration was still 1e-4 px or longer */

/* One row of the second pass; row k belongs to rows[k] of the call.  *_image positions are 1-based. */
typedef struct zm_object_ext {
    int32_t number;          /* NUMBER of the row this one extends */
    int32_t npix_auto;       /* pixels summed in FLUX_AUTO */
    int32_t nskip_auto;      /* bad pixels inside the frame that the Kron ellipse skipped */
    int32_t flags_auto;      /* FLAGS_AUTO: ZM_AUTO_* */
    int32_t flags_win;       /* FLAGS_WIN: ZM_WIN_* */
    int32_t niter_win;       /* centring passes taken */
    double kron_radius;      /* KRON_RADIUS, in units of the isophotal ellipse */
    double flux_auto, fluxerr_auto, mag_auto, magerr_auto;
    double sigma_win;
    double xwin_image, ywin_image;
    double x2win, y2win, xywin;              /* window moments (before the 1/12 rule) */
    double errx2win, erry2win, errxywin;     /* their error moments */
    double awin_image, bwin_image, thetawin_image;
    double errawin_image, errbwin_image, errthetawin_image;
    double errx2, erry2, errxy;              /* isophotal position error moments */
    double xwin_world, ywin_world;           /* NaN without a WCS, as the three below */
    double erra_world, errb_world, errtheta_world;   /* degrees; the angle in the local tangent plane */
} zm_object_ext;

/* img, sigma, bad (uint8, may be NULL), segm_dev (int32: the map zm_extract_dev wrote): device planes of nx x ny
 * pixels.  rows / out: host arrays of n rows.  n = 0 returns success and writes nothing.  The call waits. */
int zm_extract_measure_dev(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                           const int32_t* segm_dev, int nx, int ny, const zm_wcs* wcs,
                           const zm_measure_params* params, int n, const zm_object* rows, zm_object_ext* out);
/* The same with host planes. */
int zm_extract_measure(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                       const int32_t* segm, int nx, int ny, const zm_wcs* wcs,
                       const zm_measure_params* params, int n, const zm_object* rows, zm_object_ext* out);

/* ---- second pass with MASK_TYPE BLANK / CORRECT (opt-in) ---------------------- */
/* MASK_TYPE of sextractor.conf.  zm_extract_measure[_dev] and its results are what they were.  These measure the same
 * columns, and the aperture of the first pass again, with the pixels of other objects and the object's own bad pixels
 * taken out ("MASK_TYPE"; restated in tests/mask_ref.py).  For the object with NUMBER n a pixel inside the
 * frame is unusable when it is bad (the rule of zm_extract) or when segm is neither 0 nor n.  CORRECT: an unusable pixel
 * takes value and sigma of its mirror about the centre, (floor(2 cx - i + 0.5), floor(2 cy - j + 0.5)), where that lies
 * inside the frame and is usable for n (counted as replaced); otherwise, and always under BLANK, it adds nothing to any
 * sum (counted as lost).  Weights that depend on position are taken at the pixel itself.  The centre is the isophotal
 * barycentre for the Kron sums and the aperture, the current centre of every pass for the window.  An object without an
 * unusable pixel in its footprints gets the zm_object_ext row of zm_extract_measure bit for bit. */
#define ZM_MASK_BLANK 1
#define ZM_MASK_CORRECT 2
typedef struct zm_mask_params {
    int32_t type;            /* ZM_MASK_BLANK or ZM_MASK_CORRECT */
    int32_t pad_;
    double aper_radius;      /* radius of the aperture, pixels: zm_extract_params.aper_radius of the first pass, in (0, 512) */
} zm_mask_params;
void zm_mask_params_default(zm_mask_params* p);      /* CORRECT, 3.0 */

#define ZM_AUTO_CROWDED 8        /* flags_auto (masked pass only): 10 (nrepl + nlost) > npix + nlost */

/* One row of the masked pass beside its zm_object_ext.  In the ext row npix_auto counts the pixels summed, replaced ones
 * included, and nskip_auto the lost ones; ZM_AUTO_SKIPPED, _OFFFRAME and _MINRADIUS keep their formulas. */
typedef struct zm_object_mask {
    int32_t number;
    int32_t nrepl_auto;      /* Kron ellipse: pixels replaced by their mirror */
    int32_t nlost_auto;      /* ... pixels left out (= nskip_auto) */
    int32_t nap;             /* aperture: pixels inside the frame that overlap the circle */
    int32_t nrepl_aper;      /* ... of these replaced */
    int32_t nlost_aper;      /* ... of these left out */
    int32_t nrepl_win;       /* window, final pass, pixels that overlap its circle: replaced */
    int32_t nlost_win;       /* ... left out */
    int32_t crowded;         /* 1: ZM_AUTO_CROWDED is set or 10 (nrepl_aper + nlost_aper) > nap */
    int32_t pad_;
    double flux_aper;        /* sum of overlap x value over the aperture, lost pixels left out (the first pass sums bad
                              * pixels' values and only flags them) */
    double fluxerr_aper;     /* sqrt(sum of overlap x sigma^2) */
} zm_object_mask;

/* The arguments of zm_extract_measure_dev, then the mask parameters and out_mask (host array of n rows).  A type other
 * than BLANK or CORRECT or a radius outside (0, 512) is an error.  n = 0 returns success and writes nothing. */
int zm_extract_measure_masked_dev(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                                  const int32_t* segm_dev, int nx, int ny, const zm_wcs* wcs,
                                  const zm_measure_params* params, int n, const zm_object* rows, zm_object_ext* out,
                                  const zm_mask_params* mask, zm_object_mask* out_mask);
/* The same with host planes. */
int zm_extract_measure_masked(zm_ctx* ctx, const float* img, const float* sigma, const uint8_t* bad,
                              const int32_t* segm, int nx, int ny, const zm_wcs* wcs,
                              const zm_measure_params* params, int n, const zm_object* rows, zm_object_ext* out,
                              const zm_mask_params* mask, zm_object_mask* out_mask);

/* ---- detection thumbnails: stamps of several planes on one grid --------------- */
/* Replaces the thumbnail step of the subtraction driver (scripts/dosub.py:133-150 -> zuds/thumbnails.py:54-94,133-146):
 * two whole-frame SWarp runs (sub.aligned_to(ref), sci.aligned_to(ref)) and a Cutout2D per detection and image, and the
 * norms of make_triplet_for_braai (zuds/filterobjects.py:36-54).  Only the output tiles the stamps touch are resampled.
 * The operator ("Detection thumbnails"):
 *   origin   (x, y) = 0-based position of (ra, dec) on `wgrid`; the stamp covers x0 .. x0 + size - 1 with
 *            x0 = ceil(x - size / 2), likewise y0 (the rule of astropy's overlap_slices / Cutout2D, restated);
 *   pixels   of a plane on another grid: exactly the float32 zm_resample_dev(ctx, img, NULL, NULL, &plane.wcs, wgrid,
 *            kernel, fscale, ...) writes to out_img at that grid pixel; of a plane with on_grid = 1: the plane's value,
 *            untouched; 0 outside the grid (Cutout2D mode='partial', fill_value=0);
 *   norm     L2 norm of the size x size block, squares summed in float64 in a fixed order (two runs: same bytes).
 * kernel: ZM_RESAMPLE_LANCZOS3 or ZM_RESAMPLE_BILINEAR; default conventions only (zm_ctx_set_conventions). */
#define ZM_STAMP_MAX 256            /* largest stamp size */
#define ZM_STAMP_PLANES_MAX 8       /* planes per call */
#define ZM_STAMP_NOT_FINITE 1       /* status of zm_stamp_origin: the position is not finite */
#define ZM_STAMP_NO_OVERLAP 2       /* ... the stamp does not overlap the grid (Cutout2D: NoOverlapError) */
typedef struct zm_stamp_plane {
    const float* img;      /* [naxis2][naxis1] of `wcs`; device pointer for *_dev */
    zm_wcs wcs;
    double fscale;         /* as zm_resample; ignored when on_grid */
    int32_t on_grid;       /* 1: plane is on the target grid already (gather) */
    int32_t pad_;
} zm_stamp_plane;
/* host, float64: the origin rule; status[k] != 0 (ZM_STAMP_*): x0[k] / y0[k] are not to be used */
int zm_stamp_origin(const zm_wcs* wgrid, int n, const double* ra, const double* dec,
                    int size, int32_t* x0, int32_t* y0, int32_t* status);
/* out [n][nplanes][size][size] float32, out_norm [n][nplanes] float64 (may be NULL): device memory; x0 / y0: host
 * arrays.  Enqueued on the context's stream, nothing waited for.  n = 0: nothing happens.  A stamp that lies off the
 * grid altogether is all 0. */
int zm_stamps_dev(zm_ctx* ctx, int nplanes, const zm_stamp_plane* planes, const zm_wcs* wgrid,
                  int kernel, int n, const int32_t* x0, const int32_t* y0, int size,
                  float* out, double* out_norm);
/* the same arguments on host planes and host outputs: planes are copied in, the call waits */
int zm_stamps(zm_ctx* ctx, int nplanes, const zm_stamp_plane* planes, const zm_wcs* wgrid,
              int kernel, int n, const int32_t* x0, const int32_t* y0, int size,
              float* out, double* out_norm);

/* ---- real / bogus score: the braai network behind the candidate cuts ----------- */
/* Replaces ml_model.predict(make_triplet_for_braai(...)) of the candidate filter (zuds/filterobjects.py:196-240):
 * forward inference, exact fp32 with fp32 accumulation in a fixed order, of a sequential model made of
 *   Conv2D        3 x 3, 'valid', stride 1, bias, relu or linear;
 *   MaxPooling2D  square, stride = size, 'valid' (an odd remainder is dropped, as Keras does);
 *   Flatten       channels-last order (h, w, c);
 *   Dense         relu, sigmoid or linear;
 * at most 64 channels per convolution, 4096 units per Dense layer; the first layer is a Conv2D, the last a Dense of
 * one unit.  Anything else is refused by zm_rb_model_create with a message (zm_last_error).  Dropout is identity at
 * inference: leave it out of the list.
 * Input: the stamp blocks as zm_stamps_dev writes them, [n][nplanes][S][S] float32 and [n][nplanes] float64 norms;
 * channel c of the network is plane plane_of_channel[c] divided by (float)norm, as the first convolution reads it.
 * A triplet of which a used norm is zero or not finite scores NaN, by an explicit test (NaN < cut is false: such a
 * row keeps its GOODCUT, as in the reference, whose cutout / norm is a plane of NaN).
 * The score of a triplet has the same bits alone, first, last or anywhere in a batch; two runs give the same bytes.
 * Batches are worked through in chunks of at most ZM_RB_CHUNK triplets; the activations between launches live in two
 * scratch slots of the context that never grow beyond ZM_RB_CHUNK x (largest activation of the even launches +
 * largest of the odd ones) floats: 128 x (61 x 61 x 16 + 29 x 29 x 16) x 4 bytes = 37 MB for braai's VGG6. */
#define ZM_RB_CHUNK 128
enum { ZM_RB_CONV2D = 1, ZM_RB_MAXPOOL = 2, ZM_RB_FLATTEN = 3, ZM_RB_DENSE = 4 };
enum { ZM_RB_LINEAR = 0, ZM_RB_RELU = 1, ZM_RB_SIGMOID = 2 };
enum { ZM_RB_VALID = 0, ZM_RB_SAME = 1 };
typedef struct zm_rb_layer {
    int32_t type;          /* ZM_RB_CONV2D ... */
    int32_t activation;    /* ZM_RB_LINEAR ... (Conv2D, Dense) */
    int32_t cin, cout;     /* Conv2D: channels in / out; Dense: inputs / units; else 0 */
    int32_t pool;          /* MaxPooling2D: window size; else 0 */
    int32_t ksize;         /* Conv2D: kernel size (3) */
    int32_t stride;        /* Conv2D: 1; MaxPooling2D: = pool */
    int32_t padding;       /* ZM_RB_VALID */
    int64_t w_off, b_off;  /* first float of the kernel / of the bias in the blob; Keras layouts: Conv2D kernels
                              [kh][kw][cin][cout], Dense kernels [in][out] */
} zm_rb_layer;
typedef struct zm_rb_model zm_rb_model;
/* validates the shape chain and every limit, re-lays the weights for the kernels and uploads them once (the call waits) */
int zm_rb_model_create(zm_ctx* ctx, int in_size, int in_channels, int nlayers, const zm_rb_layer* layers,
                       const float* weights, int64_t nweights, zm_rb_model** out);
int zm_rb_model_destroy(zm_rb_model* model);
/* blocks_dev, norms_dev, rb_dev [n] float32: device memory; plane_of_channel: host array of in_channels entries (3 for
 * braai: the planes that hold new, ref, sub).  Enqueued on the context's stream, nothing waited for.  n = 0: nothing
 * happens. */
int zm_rb_score_dev(zm_ctx* ctx, const zm_rb_model* model, int n, const float* blocks_dev, const double* norms_dev,
                    int nplanes, const int32_t* plane_of_channel, float* rb_dev);
/* the same on host arrays: copied in, the call waits */
int zm_rb_score(zm_ctx* ctx, const zm_rb_model* model, int n, const float* blocks, const double* norms,
                int nplanes, const int32_t* plane_of_channel, float* rb);

/* ---- source association: a night's detections into sources ------------------- */
/* The join and the clustering of the reference's associate() (nersc/makesources.py:263-456) and the nearest-neighbour
 * match behind its q3c joins (csrc/associate.hip; DESIGN.md, "Source association").
 * Positions are degrees.  Two rows are neighbours when the chord between their fp64 unit vectors is <= 2 sin(r / 2)
 * (inclusive); radius_arcsec must lie in 0.25 .. 3600.  A row whose ra, dec or snr is not finite takes part in nothing.
 *
 * zm_associate_dev: connected components of the neighbour graph of n rows, as DBSCAN(eps = r, min_samples = 2) labels them:
 *   label[n]        -1 for a row without a neighbour, else its source: sources are numbered by the rank of their
 *                   smallest row index;
 *   nsrc            one word: the number of sources;
 *   offsets, members   CSR of the rows of every source, ascending within a source.  offsets has n + 1 entries: entries
 *                   nsrc .. n all hold the number of rows that belong to a source;
 *   best[nsrc]      the row of greatest snr (ties: the lowest index);
 *   count[nsrc]     rows of the source (entries nsrc .. n - 1 are zeroed);
 *   sumrb[nsrc]     fp64 sum of rb over the members in ascending order (0 when rb is NULL): the same bits on every run.
 * Every array is device memory with room for n entries (offsets: n + 1); rb_dev may be NULL.  Enqueued on the context's
 * stream; the call waits for the verdict of every propagation round (a device word per round), not for the compaction
 * behind the last one.  n = 0: nsrc = 0 and offsets[0] = 0 are enqueued, nothing else is touched. */
int zm_associate_dev(zm_ctx* ctx, int n, const double* ra_dev, const double* dec_dev, const double* snr_dev,
                     const double* rb_dev, double radius_arcsec, int32_t* label_dev, int32_t* nsrc_dev,
                     int32_t* offsets_dev, int32_t* members_dev, int32_t* best_dev, int32_t* count_dev, double* sumrb_dev);
/* the same on host arrays of the same sizes: copied in, the call waits; only the first nsrc (offsets: nsrc + 1, members:
 * offsets[nsrc]) entries of the per-source arrays are written */
int zm_associate(zm_ctx* ctx, int n, const double* ra, const double* dec, const double* snr, const double* rb,
                 double radius_arcsec, int32_t* label, int32_t* nsrc, int32_t* offsets, int32_t* members, int32_t* best,
                 int32_t* count, double* sumrb);
/* For each of n positions the nearest of m catalogue positions within the radius (ties: the lowest catalogue index):
 * idx[n] (-1: none) and sep[n] in arcsec (NaN: none).  A position that is not finite matches nothing, a catalogue row that
 * is not finite is matched by nothing.  Device memory, enqueued on the context's stream, nothing waited for.  n = 0:
 * nothing happens; m = 0: every idx is -1. */
int zm_crossmatch_dev(zm_ctx* ctx, int n, const double* ra_dev, const double* dec_dev, int m, const double* cat_ra_dev,
                      const double* cat_dec_dev, double radius_arcsec, int32_t* idx_dev, double* sep_dev);
/* the same on host arrays: copied in, the call waits */
int zm_crossmatch(zm_ctx* ctx, int n, const double* ra, const double* dec, int m, const double* cat_ra,
                  const double* cat_dec, double radius_arcsec, int32_t* idx, double* sep);
/* What the last of the four calls above did on this context (waits for the stream): out4 = propagation rounds (0 for a
 * cross-match), slots of the cell table, probes summed over every insertion, the longest probe of one insertion. */
int zm_assoc_stats(zm_ctx* ctx, int64_t* out4);

/* ---- light curves: footprint join and batched forced photometry --------------- */
/* The per-subtraction loop of the reference's scripts/dophot.py - q3c_poly_query(Source.ra, Source.dec,
 * wcs.calc_footprint()) and raw_aperture_photometry at the positions it returns - for many images at once
 * (csrc/lightcurve.hip; DESIGN.md, "Light curves").
 *
 * Footprint of an image: the spherical quadrilateral whose vertices are the sky positions of the centres of its four
 * corner pixels ((1, 1), (1, NAXIS2), (NAXIS1, NAXIS2), (NAXIS1, 1): WCS.calc_footprint, center = True), joined by great
 * circles.  A source is inside when its unit vector is on the inner side of all four edge planes (boundary inclusive) and
 * in the hemisphere of the vertex sum; the inner side follows from the polygon's own orientation (det(CD) of either sign).
 * A polygon that is degenerate or not convex is an error.  A source whose ra or dec is not finite joins nothing.
 *
 * zm_footprint_join_dev: wcs[nimg] is host memory, ra / dec[nsrc] (degrees) device memory.
 *   offsets[nimg + 1]   int64, device: the pairs of image i are entries offsets[i] .. offsets[i + 1] - 1 of src_idx;
 *                       always complete, offsets[nimg] is the number of pairs whatever the capacity;
 *   src_idx[capacity]   int32, device: source indices, ascending within an image; the same bytes on every run;
 *   *out_npairs         host: the number of pairs.  When it exceeds `capacity`, only the first `capacity` entries of src_idx
 *                       were written and nothing past them (the zm_find_stars contract): call again with room for all.
 * The call waits for that one word.  nimg <= 65535, nsrc <= 2^30. */
int zm_footprint_join_dev(zm_ctx* ctx, int nimg, const zm_wcs* wcs, int nsrc, const double* ra_dev, const double* dec_dev,
                          int64_t capacity, int64_t* offsets_dev, int32_t* src_idx_dev, int64_t* out_npairs);
/* the same on host arrays: copied in, the call waits; min(*out_npairs, capacity) entries of src_idx are written */
int zm_footprint_join(zm_ctx* ctx, int nimg, const zm_wcs* wcs, int nsrc, const double* ra, const double* dec,
                      int64_t capacity, int64_t* offsets, int32_t* src_idx, int64_t* out_npairs);

typedef struct zm_lc_image {
    const float* img;       /* device, ny x nx */
    const float* rms;       /* device or NULL */
    const int32_t* mask;    /* device or NULL */
    zm_wcs wcs;
    int32_t nx, ny;
} zm_lc_image;

/* Forced photometry of every pair of a join in one launch, one wave per pair: the source goes through its image's WCS on
 * the device (TPV inverse included), then the aperture is summed exactly as zm_aperture_photometry_dev sums it - flux, err
 * and flags are the bits that call returns at (x, y).  images[nimg] is host memory (its pointers device memory; sizes may
 * differ from image to image); offsets / src_idx are a join's (npairs <= offsets[nimg]: a clipped list is fine), ra / dec
 * [nsrc] the positions it was made from.  Per pair, device memory: x, y (0-based pixels), flux, err (fp64), flags (int32).
 * A src_idx entry outside 0 .. nsrc - 1 gives NaN positions and zero sums.  Enqueued on the context's stream, nothing waited
 * for (the image table is copied from pinned memory the next call leaves alone until that copy is done). */
int zm_forced_photometry_batch_dev(zm_ctx* ctx, int nimg, const zm_lc_image* images, const int64_t* offsets_dev,
                                   const int32_t* src_idx_dev, int64_t npairs, int nsrc, const double* ra_dev,
                                   const double* dec_dev, double radius, double* x_dev, double* y_dev, double* flux_dev,
                                   double* err_dev, int32_t* flags_dev);

/* ---- PSF photometry: star model and batched fits (csrc/psf.hip; DESIGN.md "PSF photometry") ---- */
/* Taps: Lanczos-3, separable, fp64: offsets k = -2 .. 3 from the floor sample, t_k ~ sinc(d - k) sinc((d - k) / 3), each
 * 6-vector scaled to unit sum; at d == 0 exactly the vector is a delta and its footprint on that axis the single sample.
 *
 * zm_psf_build: the model of an image from nstar stars - x, y (0-based centroids), sky (local sky) and norm (flux in the
 * reference aperture above that sky: zm_growth's outputs).  The model is (2 half + 1)^2 doubles at the image's own
 * sampling, row j + half, column i + half for the offset (i, j) from the centre; 1 <= half <= ZM_PSF_HALF_MAX.
 * Cutout entry (j, i) of star s: the Lanczos-3 interpolation of (img - sky_s) / norm_s at (x + i, y + j).  An entry is NaN
 * when any tap of its footprint lies outside the frame, on a pixel that is not finite, or on one with mask & bad_bits; a
 * whole row is NaN when x, y, sky or norm is not finite or norm <= 0.  Model: the clipped median over the stars of
 * every entry (zm_clipped_median_dev with kappa / maxiter: NaN entries are not used); then 0 where i^2 + j^2 >
 * norm_radius^2 (squares compared), where n_used < min_stars_pixel, or where no star gave a value; then scaled to unit
 * sum (fp64, fixed order).  A sum that is not positive and finite: every entry NaN.  out_n_used[(2 half + 1)^2]: the
 * stars that entered the median of every entry, exact.  out_cutouts: NULL, or nstar rows of cutout_stride (>= (2 half +
 * 1)^2) doubles.  nstar <= ZM_CLIPMED_NMAX, more is an error; nstar == 0: returns at once, writes nothing.
 * The host form stages the planes as zm_aperture_photometry does; the _dev form (every array device memory) only
 * enqueues on the stream. */
#define ZM_PSF_HALF_MAX 15
int zm_psf_build(zm_ctx* ctx, const float* img, const int32_t* mask, int32_t bad_bits, int nx, int ny, int nstar,
                 const double* x, const double* y, const double* sky, const double* norm, int half, double norm_radius,
                 double kappa, int maxiter, int min_stars_pixel, double* out_model, int32_t* out_n_used,
                 double* out_cutouts, int64_t cutout_stride);
int zm_psf_build_dev(zm_ctx* ctx, const float* img, const int32_t* mask, int32_t bad_bits, int nx, int ny, int nstar,
                     const double* x, const double* y, const double* sky, const double* norm, int half,
                     double norm_radius, double kappa, int maxiter, int min_stars_pixel, double* out_model,
                     int32_t* out_n_used, double* out_cutouts, int64_t cutout_stride);
/* zm_psf_photometry: a linear fit of the model at npos given 0-based positions, one wave per position.  ix = floor(x +
 * 0.5), fx = x - ix in [-0.5, 0.5), the same in y.  Pixels: (ix + i, iy + j) with (i - fx)^2 + (j - fy)^2 <= R^2 (centre
 * rule, squares compared as plain IEEE operations), clipped to the frame; R = fit_radius, and R + 3.5 <= half is
 * required (an error otherwise).  Profile: P_ij = the model interpolated at (i - fx, j - fy) with the taps above (the model
 * is 0 outside its grid).  A pixel is used when its value is finite, (mask & bad_bits) == 0 and, with an rms plane, its rms
 * is finite and positive; weight w = 1 / rms^2, or 1 when rms is NULL.  fit_sky == 0: flux = sum(w P d) / sum(w P^2), err =
 * 1 / sqrt(sum(w P^2)), sky = 0.  fit_sky != 0: the 2 x 2 weighted least squares for {flux, sky}, err from the inverse
 * normal matrix (solved about the weighted mean of P).  rms NULL: err is scaled by sqrt(chi2 / (npix - nparam)), NaN when
 * npix <= nparam.  chi2 = sum(w (d - flux P - sky)^2), npix = pixels used (exact), cover = sum(P) over the used pixels /
 * sum(P) over the pixels of the circle inside the frame.  flags: ZM_PSF_* below, exact.  With ZM_PSF_SINGULAR or
 * ZM_PSF_BADPOS every float output is NaN.  All sums are fp64 in a fixed order: the same bits on every run.
 * ZM_PSF_SINGULAR is exact where a circle holds fewer usable pixels than parameters; on a circle that is only nearly rank
 * deficient (two parameters on a few pixels of nearly equal profile, as R = 1 with a sky term) the decision is this
 * kernel's Sxx > 0 and is not pinned: another solver may call such a fit singular, or return very different numbers.
 * npos == 0: returns at once, writes nothing.  Host form: planes staged as zm_aperture_photometry does; _dev: enqueues. */
#define ZM_PSF_BAD 1          /* a pixel of the circle was left out for its mask */
#define ZM_PSF_NONFINITE 2    /* a pixel of the circle was left out because its value is not finite */
#define ZM_PSF_BADRMS 4       /* a pixel of the circle was left out for its rms (not finite, or not positive) */
#define ZM_PSF_CLIPPED 8      /* the frame cut the circle */
#define ZM_PSF_LOWCOVER 16    /* cover < 0.5 */
#define ZM_PSF_SINGULAR 32    /* fewer pixels left than parameters, or the determinant is not positive */
#define ZM_PSF_BADPOS 64      /* the position is not finite (npix 0) */
int zm_psf_photometry(zm_ctx* ctx, const float* img, const float* rms, const int32_t* mask, int32_t bad_bits, int nx,
                      int ny, int npos, const double* x, const double* y, const double* model, int half,
                      double fit_radius, int fit_sky, double* out_flux, double* out_err, double* out_chi2,
                      double* out_sky, double* out_cover, int32_t* out_npix, int32_t* out_flags);
int zm_psf_photometry_dev(zm_ctx* ctx, const float* img, const float* rms, const int32_t* mask, int32_t bad_bits, int nx,
                          int ny, int npos, const double* x, const double* y, const double* model, int half,
                          double fit_radius, int fit_sky, double* out_flux, double* out_err, double* out_chi2,
                          double* out_sky, double* out_cover, int32_t* out_npix, int32_t* out_flags);

typedef struct zm_psf_image {   /* zm_lc_image, then the model of the image */
    const float* img;       /* device, ny x nx */
    const float* rms;       /* device or NULL */
    const int32_t* mask;    /* device or NULL */
    zm_wcs wcs;
    int32_t nx, ny;
    const double* model;    /* device, (2 half + 1)^2 */
    int32_t half;
    int32_t pad_;
} zm_psf_image;

/* The fits of every pair of a join in one launch, one wave per pair: zm_forced_photometry_batch_dev with
 * zm_psf_photometry_dev in place of the aperture sum.  At the positions it returns (x, y) every other output is bit for bit
 * what zm_psf_photometry_dev returns there with the image's planes and model.  rms / mask may be NULL per image; sizes
 * and half may differ from image to image (fit_radius + 3.5 <= half of every image).  A src_idx entry outside 0 .. nsrc - 1
 * gives NaN positions and ZM_PSF_BADPOS.  Enqueued on the context's stream, nothing waited for. */
int zm_psf_photometry_batch_dev(zm_ctx* ctx, int nimg, const zm_psf_image* images, const int64_t* offsets_dev,
                                const int32_t* src_idx_dev, int64_t npairs, int nsrc, const double* ra_dev,
                                const double* dec_dev, int32_t bad_bits, double fit_radius, int fit_sky, double* x_dev,
                                double* y_dev, double* flux_dev, double* err_dev, double* chi2_dev, double* sky_dev,
                                double* cover_dev, int32_t* npix_dev, int32_t* flags_dev);

/* ---- fake sources: PSF-model point sources added to resident planes (csrc/inject.hip; DESIGN.md "Fake sources") ---- */
/* zm_inject_dev adds n fakes to img (ny x nx float32, device) and, optionally, their Poisson variance to rms.  The fake list
 * x, y (0-based pixels), flux (data units) is HOST memory, as the stamp origins of zm_stamps_dev are; model is the device
 * array of a PSF model as zm_psf_photometry_dev takes it, (2 half + 1)^2 doubles, 1 <= half <= ZM_PSF_HALF_MAX.
 *
 * Geometry: that of zm_psf_photometry.  ix = floor(x + 0.5), fx = x - ix in [-0.5, 0.5), the same in y.  The profile at
 * pixel (ix + i, iy + j) is P_ij, the model interpolated at (i - fx, j - fy) with the six Lanczos-3 taps at offsets -2 .. 3
 * scaled to unit sum (a fractional part of 0 is a delta); the model is 0 outside its samples.  The walk over the 6 x 6 taps
 * is that of the fit, in its order: rows outer, ty[a] * (sum_b tx[b] * m), no contraction.  The box of a fake is |i|, |j| <=
 * half + 3, clipped to the frame.
 * Image: every box pixel inside the frame with v = flux * P_ij != 0 becomes (float)((double)img + v).  Pixels with v == 0
 * are not written (a fake of flux 0 writes nothing); a pixel that is not written keeps its bytes, NaN payloads and -0.0
 * included.  A pixel holding NaN or inf is written by the same formula and stays non-finite.
 * Rms: with rms != NULL and gain > 0 the same pixels with v > 0 whose rms is finite and positive become
 * (float)sqrt((double)rms * rms + v / gain); every other rms pixel keeps its bytes.  No noise realisation is drawn.
 * Overlaps: the result is that of adding the fakes one at a time in index order, each addition rounded to float32 as
 * above, the same bytes on every run, without float atomics: zm_inject_layers gives every fake layer = 1 + max(layer of
 * every EARLIER fake whose box shares a pixel with its own, 0); two boxes share a pixel iff |ix_a - ix_b| <= 2 (half + 3)
 * and the same in y; a fake whose x or y is not finite has layer 0 and shares nothing.  zm_inject_dev makes one launch per
 * layer, in order, on the context's stream: within a layer no two fakes share a pixel, and of every overlapping pair the
 * earlier index lies in an earlier layer.  Fakes kept 2 (half + 3) + 1 pixels apart make one layer.
 * out_sum[s] (device, or NULL): flux * sum(P_ij) over the pixels written, fp64, reduced in a fixed order: the flux really
 * deposited.  out_flags[s] (device): ZM_INJ_* below, exact.
 * n == 0 returns at once.  half outside 1 .. ZM_PSF_HALF_MAX, a negative or non-finite gain or core_radius, or NULL where
 * a pointer is required: an error, zm_last_error names the function.  zm_inject_dev only enqueues (one copy of the fake list
 * and the per-layer work list, then the launches); zm_inject takes every array from the host - the planes staged as
 * zm_psf_photometry stages them, written back in place - and waits.  zm_inject_layers is host only and touches no GPU. */
#define ZM_INJ_CLIPPED 1      /* a box pixel lies off the frame */
#define ZM_INJ_OUTSIDE 2      /* no box pixel lies inside (always with ZM_INJ_CLIPPED): nothing written, out_sum 0 */
#define ZM_INJ_BAD 4          /* mask given: a box pixel inside the frame with (i - fx)^2 + (j - fy)^2 <= core_radius^2 has mask & bad_bits */
#define ZM_INJ_NONFINITE 8    /* a written pixel held a value that is not finite */
#define ZM_INJ_BADPOS 16      /* x, y or flux is not finite: nothing written, out_sum NaN */
int zm_inject_dev(zm_ctx* ctx, float* img, float* rms, const int32_t* mask, int32_t bad_bits, int nx, int ny, int n,
                  const double* x, const double* y, const double* flux, const double* model, int half, double gain,
                  double core_radius, double* out_sum, int32_t* out_flags);
int zm_inject(zm_ctx* ctx, float* img, float* rms, const int32_t* mask, int32_t bad_bits, int nx, int ny, int n,
              const double* x, const double* y, const double* flux, const double* model, int half, double gain,
              double core_radius, double* out_sum, int32_t* out_flags);
int zm_inject_layers(int n, const double* x, const double* y, int half, int32_t* out_layer, int* out_nlayers);

/* ---- alert packets: cone searches against a catalogue that stays in HBM -------- */
/* The cone searches of the reference's xmatch() (zuds/crossmatch.py: the three nearest PS1 and LegacySurvey rows within
 * 30 arcsec, every ZTF alert, milliquas and TNS row within 1.5 arcsec) against local tables (csrc/skyindex.hip; DESIGN.md,
 * "Alert packets").  The geometry is that of the association section, through the same arithmetic: fp64 unit vectors, two
 * points are neighbours when their chord is <= 2 sin(r / 2) (inclusive), separations are 2 asin(min(1, chord / 2)) in arcsec.
 * A query that is not finite matches nothing, a catalogue row that is not finite is matched by nothing.
 *
 * zm_skyindex_create: the index of m catalogue rows (host arrays, degrees; m = 0 .. 2^30) for queries of at most
 * max_radius_arcsec (0.25 .. 3600): the rows sorted by cubic cell of edge chord(max_radius) (1 + 1e-6), unit vectors and
 * row numbers of a cell contiguous.  It lives in device memory of the context's device until zm_skyindex_destroy and is
 * never rebuilt: any number of queries, on any context of that device, read it.  The call waits; ra / dec are not kept. */
typedef struct zm_skyindex zm_skyindex;
int zm_skyindex_create(zm_ctx* ctx, int m, const double* ra, const double* dec, double max_radius_arcsec, zm_skyindex** out_index);
/* the same on device arrays; the call waits as well (its work arrays are released before it returns) */
int zm_skyindex_create_dev(zm_ctx* ctx, int m, const double* ra_dev, const double* dec_dev, double max_radius_arcsec,
                           zm_skyindex** out_index);
/* frees the index (NULL: nothing happens); waits for the device, so queries still in flight finish first */
int zm_skyindex_destroy(zm_skyindex* index);
/* out4 = rows indexed (the finite ones), cells in use, slots of the cell table, the longest probe of one insertion */
int zm_skyindex_stats(const zm_skyindex* index, int64_t* out4);
/* For each of n positions the k nearest catalogue rows within the radius, k = 1 .. 8:
 *   idx[n * k]    rows of query i at i * k .., ascending by (squared chord, catalogue row); -1 in the slots not filled;
 *   sep[n * k]    their separations in arcsec; NaN in the slots not filled;
 *   count[n]      rows within the radius, which may exceed k.
 * k = 1 gives the idx and sep bits of zm_crossmatch_dev.  radius_arcsec above the index's max_radius is an error
 * (zm_last_error names both).  Device memory, enqueued on the context's stream, nothing waited for.  n = 0: nothing
 * happens; an index of no rows: every idx is -1 and every count 0.  The result does not depend on the order of the rows
 * inside a cell: it is the same bytes on every run. */
int zm_cone_knn_dev(zm_ctx* ctx, const zm_skyindex* index, int n, const double* ra_dev, const double* dec_dev,
                    double radius_arcsec, int k, int32_t* idx_dev, double* sep_dev, int32_t* count_dev);
/* the same on host arrays: copied in, the call waits */
int zm_cone_knn(zm_ctx* ctx, const zm_skyindex* index, int n, const double* ra, const double* dec, double radius_arcsec, int k,
                int32_t* idx, double* sep, int32_t* count);
/* Every catalogue row within the radius of each of n positions, as zm_footprint_join_dev returns its pairs:
 *   offsets[n + 1]      int64, device: the rows of query i are entries offsets[i] .. offsets[i + 1] - 1 of cat_idx;
 *                       always complete, offsets[n] is the number of pairs whatever the capacity;
 *   cat_idx[capacity]   int32, device: catalogue rows, ascending within a query; the same bytes on every run;
 *   *out_npairs         host: the number of pairs.  When it exceeds `capacity`, only the first `capacity` entries of cat_idx
 *                       were written and nothing past them: call again with room for all.
 * The call waits for that one word (offsets are complete then; cat_idx is enqueued behind it). */
int zm_cone_within_dev(zm_ctx* ctx, const zm_skyindex* index, int n, const double* ra_dev, const double* dec_dev,
                       double radius_arcsec, int64_t capacity, int64_t* offsets_dev, int32_t* cat_idx_dev, int64_t* out_npairs);
/* the same on host arrays: copied in, the call waits; min(*out_npairs, capacity) entries of cat_idx are written */
int zm_cone_within(zm_ctx* ctx, const zm_skyindex* index, int n, const double* ra, const double* dec, double radius_arcsec,
                   int64_t capacity, int64_t* offsets, int32_t* cat_idx, int64_t* out_npairs);

/* ---- astrometric refit: detections against a star catalogue -> the PV terms of a TPV header ---- */
/* Stands where the reference runs SCAMP (zuds/scamp.py:16-113, astromatic/default.scamp); the operator is stated in
 * DESIGN.md, "Astrometric refit" (csrc/astrometry.hip): a vote for the gross offset (MATCH Y, POSITION_MAXERR), then rounds
 * of cross-identification (zm_crossmatch_dev at CROSSID_RADIUS) and a clipped weighted polynomial fit per axis.  CRPIX, CRVAL
 * and CD never change: the solution lives in PVi_0 .. PVi_10 (no radial terms).  SCAMP's own digits are not claimed. */
typedef struct zm_astrom_params {
    double position_maxerr;   /* P, arcsec: half width of the vote's window                          (60)  */
    double match_resol;       /* q, arcsec: the vote's bin; 0 = crossid_radius / 2                   (0)   */
    double crossid_radius;    /* arcsec, inclusive                                                   (2)   */
    double clip_nsigma;       /* a row stays while chi2 <= 2 clip_nsigma^2 max(1, reduced chi2)      (3)   */
    int32_t degree;           /* 1, 2 or 3: 3, 6 or 10 coefficients per axis                         (3)   */
    int32_t match;            /* 0 skips the vote                                                    (1)   */
    int32_t match_nmax;       /* detections of greatest snr that vote                                (1024)*/
    int32_t max_rounds;       /* cross-id + fit rounds                                               (8)   */
    int32_t max_clip;         /* fits per round                                                      (10)  */
    int32_t pad_;
} zm_astrom_params;
void zm_astrom_params_default(zm_astrom_params* p);

enum { ZM_ASTROM_OK = 0, ZM_ASTROM_TOO_FEW = 1, ZM_ASTROM_AMBIGUOUS = 2, ZM_ASTROM_SINGULAR = 3,
       ZM_ASTROM_NOT_CONVERGED = 4 };

typedef struct zm_astrom_result {
    zm_wcs wcs;               /* the solution (TPV); the input header unless status is OK or NOT_CONVERGED */
    double shift[2];          /* the vote's offset (xi, eta), arcsec, star - detection                      */
    double rms[2];            /* unweighted rms residual of the rows used, per axis, arcsec (ASTRRMS1 / 2)  */
    double chi2;              /* sum of chi2 over the rows used                                             */
    int32_t status;
    int32_t vote_peak, vote_runner_up;
    int32_t nmatch, nused, rounds;
} zm_astrom_result;

/* nframes frames against one catalogue of m stars.  Rows of all frames are concatenated: frame f owns rows
 * offsets[f] .. offsets[f + 1] - 1 of x, y (FITS 1-based pixels), sd (position sigma, pixels), snr (rank key), match
 * (index of the star a row is identified with, or -1) and used (1: the row was in the last fit).  ref_ra, ref_dec are
 * degrees, ref_sig arcsec.  A row with a value that is not finite takes part in nothing.  Detection, star, match and used
 * arrays are device memory; wcs0, offsets and results are host memory.  The call waits for one word per frame after the
 * vote and after every round; two calls on the same input give the same bits.  nframes <= 65535. */
int zm_astrom_solve_dev(zm_ctx* ctx, int nframes, const zm_wcs* wcs0, const int32_t* offsets, const double* x_dev,
                        const double* y_dev, const double* sd_dev, const double* snr_dev, int m, const double* ref_ra_dev,
                        const double* ref_dec_dev, const double* ref_sig_dev, const zm_astrom_params* params,
                        zm_astrom_result* results, int32_t* match_dev, uint8_t* used_dev);
/* the same on host arrays: copied in, the call waits; the same bits as the device form */
int zm_astrom_solve(zm_ctx* ctx, int nframes, const zm_wcs* wcs0, const int32_t* offsets, const double* x, const double* y,
                    const double* sd, const double* snr, int m, const double* ref_ra, const double* ref_dec,
                    const double* ref_sig, const zm_astrom_params* params, zm_astrom_result* results, int32_t* match,
                    uint8_t* used);

/* ---- FITS data blocks on the device ------------------------------------------ */
/* Replaces the host-side decode / encode astropy does inside FITSFile.load_data / save
 * (zuds/fitsfile.py:69-94,146-206): raw_dev holds the big-endian data block of a primary
 * HDU as it lies on disk (n pixels of BITPIX 8 / 16 / 32 / 64 / -32 / -64; stored values are
 * uint8, int16, int32, int64, float32, float64); the decoded plane is float32 (out_kind 0), int32 (1),
 * uint8 (2) or int16 (3: a BITPIX 16 mask kept at 16 bits for zm_dframe.mask_type = ZM_MASKTYPE_I16)
 * with physical = bzero + bscale * stored.  "Unscaled" below: bscale == 1 and bzero == 0.
 *
 * The contract (restated by tests/fits_ref.py, pinned by tests/test_fits_decode_gpu.py):
 *  - float32 out, unscaled BITPIX -32: the 32 bits of the file, byte-swapped.  NaN payload and
 *    sign, -0.0 and subnormals are unchanged.
 *  - float32 out, unscaled integer BITPIX (64 included): the integer converted directly, one
 *    rounding to nearest even, never through fp64 (numpy's int64 -> float32).
 *  - float32 out, anything else: fl(stored) * bscale rounded to fp64, + bzero rounded to fp64,
 *    rounded once to float32; two fp64 operations, never a fused multiply-add.  (fl(stored) is
 *    exact but for BITPIX 64 beyond 2^53.)  Bit for bit what fits.read(...) followed by
 *    .astype(float32) gives; the one exception is BITPIX 64 with BSCALE 1 and an integer BZERO,
 *    where the host reader adds in int64 and rounds once.  A NaN that comes out of the
 *    arithmetic or out of float64 -> float32 is a NaN of no particular payload.
 *  - int32 / uint8 / int16 out: the same fp64 value, truncated toward zero and SATURATED at the
 *    ends of the output type (+-inf included); NaN gives 0.  Unscaled integer blocks, and
 *    BSCALE 1 with an integer BZERO of magnitude <= 2^63 (the unsigned 16 / 32 / 64 bit and
 *    signed-byte conventions), stay in exact integer arithmetic - stored + BZERO without
 *    rounding, also where that sum leaves int64 - and saturate in the same way: an unsigned-16
 *    file read as int16 gives 32767 for 40000, not -25536.
 *  - BLANK is not implemented (nor is it by the host reader).
 * Encode: float32 -> BITPIX -32 (in_kind 0), int32 -> 32 (1), uint8 -> 8 (2),
 * int32 -> BITPIX 16 (3): the bits of the plane, byte-swapped; in_kind 3 writes the low 16 bits,
 * so values must lie within -32768 .. 32767 (the caller's duty). */
int zm_fits_decode_dev(zm_ctx* ctx, const void* raw_dev, int bitpix, double bscale,
                       double bzero, int64_t n, int out_kind, void* out_dev);
int zm_fits_encode_dev(zm_ctx* ctx, const void* in_dev, int in_kind, int64_t n,
                       void* raw_dev);

/* ---- timing hooks (bench.py reads per-kernel HIP-event times) ------------- */
/* Enable recording of HIP events around the dominant kernels on the ctx
 * stream; zm_timing_read returns accumulated milliseconds and launch counts. */
int zm_timing_enable(zm_ctx* ctx, int on);
/* Time only the scope `only` (e.g. "resample"); NULL = every scope.  The two event records
 * around a launch cost a few microseconds of dispatch latency each, so a throughput
 * measurement times just the kernel it needs. */
int zm_timing_filter(zm_ctx* ctx, const char* only);
int zm_timing_reset(zm_ctx* ctx);
int zm_timing_read(zm_ctx* ctx, const char* kernel_name, double* total_ms,
                   int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* ZUDSMI_H */
