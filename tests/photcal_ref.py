"""A float64 numpy restatement of the photometric calibration (``zuds-pipeline_amd/photcal.py``, ``csrc/photcal.hip``),
independent of the library.

The aperture fractions come from ``tests/aperture_ref.py`` (a quadrature that shares no formula with the kernel's closed
form; ``sums_bounds`` there gives the rounding bound of a sum).  The median, the MAD, the clipping, the star selection
and the ``APCOR`` / ``MAGZP`` / ``MAGLIM`` arithmetic are written out plainly here.

Definitions the kernel and this file share (include/zudsmi.h):
  * annulus: pixel centres with ``r_in^2 <= dx^2 + dy^2 < r_out^2`` (the centre rule, compared as squares);
  * a pixel touches radius r when its nearest point to the centre is nearer than r (``near^2 < r^2``); a pixel that does
    not touch contributes nothing, one whose farthest corner is within r counts whole;
  * clipping: median, 1.4826 x median |v - median|, drop where ``|v - median| > kappa sigma`` (strict), again until
    nothing is dropped or ``maxiter`` times; the statistics are always those of the survivors.

CARD_TOL, the tolerance of a header card between the product and this file on the same planes.  Both select the same
pixels and the same stars (the scenes' conditions, asserted in tests/test_photcal_ref.py), so what is left is rounding.
tests/measure_photcal_tolerance.py prints two propagated rounding errors on the end-to-end frame: that of this file's
float64 sums (1.4e-13 mag) and the largest difference of a card between this file's run and a run of the same pipeline
in numpy.longdouble (3.1e-15 mag), and takes 4 x the larger, rounded up to a power of two: 2^-40 mag.  What the GPU
admits in an aperture sum is no part of it; tests/test_photcal_ref.py holds the constant to that script.
"""
import math

import numpy as np

import aperture_ref as ar

CARD_TOL = 2.0 ** -40
FLUX_RTOL, FLUX_ATOL = 1e-10, 1e-9          # tests/test_photometry_gpu.py
BAD, SATURATED, NONFINITE, BOXCLIP, ANNCLIP, FEWSKY, BADPOS = 1, 2, 4, 8, 16, 32, 64
APERTURE_RADIUS = 3.0


# ---- clipped statistics -----------------------------------------------------------------------------------------------
def _median(s):
    m = s.size
    return float(s[m // 2]) if m & 1 else 0.5 * (float(s[m // 2 - 1]) + float(s[m // 2]))


def clip_stats(values, kappa, maxiter):
    """Clipped median / sigma of the finite entries of ``values`` (float32 or float64; the arithmetic is float64).
    Returns a dict: ``median``, ``sigma``, ``n_used``, ``n_valid``, ``keep`` (bool per input entry), ``rounds`` (rounds in
    which something was dropped) and ``margin``: the smallest ``| |v - median| - threshold | / threshold`` met in any
    round (inf when no threshold was applied or it was 0 with nothing at it)."""
    v = np.asarray(values).astype(np.float64).ravel()
    keep = np.isfinite(v)
    n_valid = int(keep.sum())
    med = sig = float('nan')
    rounds, margin = 0, float('inf')
    for it in range(maxiter + 1):
        s = np.sort(v[keep])
        if s.size == 0:
            med = sig = float('nan')
            break
        med = _median(s)
        sig = 1.4826 * _median(np.sort(np.abs(s - med)))
        if it >= maxiter:
            break
        thr = kappa * sig
        dev = np.abs(v - med)
        if thr > 0:
            margin = min(margin, float(np.min(np.abs(dev[keep] - thr)) / thr))
        drop = keep & (dev > thr)
        if not drop.any():
            break
        keep = keep & ~drop
        rounds += 1
    return dict(median=med, sigma=sig, n_used=int(keep.sum()), n_valid=n_valid, keep=keep, rounds=rounds, margin=margin)


def clipped_median(values, kappa=3.0, maxiter=5):
    """``[median, sigma, n_used, n_valid]`` per column of a (n, ncol) array, with the statistics dicts."""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim == 1:
        v = v[:, None]
    st = [clip_stats(v[:, c], kappa, maxiter) for c in range(v.shape[1])]
    return np.array([[s['median'], s['sigma'], s['n_used'], s['n_valid']] for s in st]).reshape(-1, 4), st


# ---- curves of growth -------------------------------------------------------------------------------------------------
def annulus_pixels(x, y, r_in, r_out, nx, ny):
    """(i, j) of the annulus pixels inside the frame, and whether any lies outside."""
    i = np.arange(math.ceil(x - r_out), math.floor(x + r_out) + 1, dtype=np.float64)
    j = np.arange(math.ceil(y - r_out), math.floor(y + r_out) + 1, dtype=np.float64)
    ii, jj = np.meshgrid(i, j)
    dx, dy = ii - x, jj - y
    d2 = dx * dx + dy * dy
    sel = (d2 >= r_in * r_in) & (d2 < r_out * r_out)
    inside = (ii >= 0) & (jj >= 0) & (ii < nx) & (jj < ny)
    return ii[sel & inside].astype(np.int64), jj[sel & inside].astype(np.int64), bool((sel & ~inside).any())


def growth(img, x, y, radii, rms=None, mask=None, bad_bits=0, saturate=None, r_in=12.0, r_out=18.0, kappa=3.0,
           maxiter=5, nsky_min=50):
    """The outputs of ``zm_growth`` (flux, err, sky, sky_sigma, nsky, flags) plus ``flux_bound`` / ``var_bound``
    (``aperture_ref.sums_bounds`` of every sum: the allowance for the closed form's fractions plus the roundings of the
    sum), ``round_bound`` (the roundings alone), ``sky_stats`` (the dicts of ``clip_stats``) and ``sky_pixels``."""
    img = np.asarray(img, dtype=np.float32)
    ny, nx = img.shape
    x, y = np.atleast_1d(np.asarray(x, np.float64)), np.atleast_1d(np.asarray(y, np.float64))
    radii = [float(r) for r in radii]
    n, na = x.size, len(radii)
    m32 = None if mask is None else np.asarray(mask).astype(np.int64)
    out = dict(flux=np.full((n, na), np.nan), err=np.full((n, na), np.nan), sky=np.full(n, np.nan),
               sky_sigma=np.full(n, np.nan), nsky=np.zeros(n, np.int32), flags=np.zeros(n, np.int32),
               flux_bound=np.zeros((n, na)), var_bound=np.zeros((n, na)), round_bound=np.zeros((n, na)),
               sky_stats=[None] * n, sky_pixels=[None] * n)
    old = np.seterr(invalid='ignore', over='ignore')
    for s in range(n):
        xc, yc = float(x[s]), float(y[s])
        if not (math.isfinite(xc) and math.isfinite(yc)):
            out['flags'][s] = BADPOS
            continue
        fl = 0
        ai, aj, annclip = annulus_pixels(xc, yc, r_in, r_out, nx, ny)
        vals = img[aj, ai]
        usable = np.isfinite(vals)
        if m32 is not None:
            usable &= (m32[aj, ai] & bad_bits) == 0
        st = clip_stats(vals[usable], kappa, maxiter)
        sky, sig, nsky = st['median'], st['sigma'], st['n_used']
        out['sky'][s], out['sky_sigma'][s], out['nsky'][s] = sky, sig, nsky
        out['sky_stats'][s], out['sky_pixels'][s] = st, (ai[usable], aj[usable])
        rmax = radii[-1]
        b = [math.floor(xc - rmax + 0.5), math.ceil(xc + rmax + 0.5), math.floor(yc - rmax + 0.5), math.ceil(yc + rmax + 0.5)]
        if b[0] < 0 or b[2] < 0 or b[1] > nx or b[3] > ny:
            fl |= BOXCLIP
        i0, i1, j0, j1 = max(b[0], 0), min(b[1], nx), max(b[2], 0), min(b[3], ny)
        if i1 > i0 and j1 > j0:
            ii, jj = np.meshgrid(np.arange(i0, i1), np.arange(j0, j1))
            ii, jj = ii.ravel(), jj.ravel()
            x0, x1, y0, y1 = ar.pixel_edges(ii, jj, xc, yc)
            qx, qy = np.clip(0.0, x0, x1), np.clip(0.0, y0, y1)
            near2 = qx * qx + qy * qy
            d = img[jj, ii].astype(np.float64)
            fin = np.isfinite(d)
            tmax = near2 < rmax * rmax
            if m32 is not None and ((m32[jj, ii] & bad_bits) != 0)[tmax].any():
                fl |= BAD
            if saturate is not None and saturate > 0 and (img[jj, ii] >= np.float32(saturate))[tmax].any():
                fl |= SATURATED
            if (~fin)[tmax].any():
                fl |= NONFINITE
            var = None if rms is None else np.asarray(rms, np.float32)[jj, ii].astype(np.float64) ** 2
            for k, r in enumerate(radii):
                t = near2 < r * r
                if nsky == 0:
                    continue
                frac = ar.edges_fraction(x0[t], x1[t], y0[t], y1[t], r)
                lim = ar.edges_limit(x0[t], x1[t], y0[t], y1[t], r)
                dv = d[t] - sky
                f = fin[t]
                terms = np.zeros(5)
                terms[0], terms[1], terms[4] = (np.abs(dv) * lim)[f].sum(), np.abs(dv * frac)[f].sum(), t.sum()
                w = np.ones(int(t.sum())) if var is None else var[t]
                wf = np.isfinite(w)
                terms[2], terms[3] = (w * lim)[wf].sum(), (w * frac)[wf].sum()
                fb, vb = ar.sums_bounds(terms)
                out['flux_bound'][s, k], out['var_bound'][s, k] = fb, vb
                out['round_bound'][s, k] = terms[4] * ar.EPS * terms[1]           # the float64 sum's own roundings
                out['flux'][s, k] = math.fsum(dv * frac) if f.all() else np.nan
                v = math.fsum(w * frac) if wf.all() else np.nan
                out['err'][s, k] = math.sqrt(v) if var is not None else math.sqrt(v) * sig
        elif nsky:
            out['flux'][s, :] = 0.0
            out['err'][s, :] = 0.0
        if annclip:
            fl |= ANNCLIP
        if nsky < nsky_min:
            fl |= FEWSKY
        out['flags'][s] = fl
    np.seterr(**old)
    return out


def growth_tolerances(ref):
    """(flux tolerance, err tolerance) per entry: rtol 1e-10 / atol 1e-9, or ``sums_bounds`` where that is larger (for
    the error: the bound of the variance carried through the square root)."""
    ftol = np.maximum(FLUX_ATOL + FLUX_RTOL * np.abs(ref['flux']), ref['flux_bound'])
    with np.errstate(invalid='ignore', divide='ignore'):
        scale = np.where(ref['err'] > 0, ref['err'], np.inf)
        sig = ref['sky_sigma'][:, None]
        etol = np.maximum(FLUX_ATOL + FLUX_RTOL * np.abs(ref['err']), ref['var_bound'] * np.where(np.isfinite(sig), np.maximum(sig * sig, 1.0), 1.0) / scale)
    return ftol, etol


# ---- limiting magnitude -----------------------------------------------------------------------------------------------
def lattice(n, step, radius):
    h, margin = 0.5 * step, radius + 1.0
    return [h + i * step for i in range(0, n) if h + i * step + 0.5 >= margin and n - 0.5 - (h + i * step) >= margin]


def maglim_sigma(rms, mask, bad_bits, radius, step):
    """(median sigma_ap of the used points or NaN, number used, number of lattice points, sigma of every point, bound)."""
    rms = np.asarray(rms, dtype=np.float32)
    ny, nx = rms.shape
    xs, ys = lattice(nx, step, radius), lattice(ny, step, radius)
    px = np.array([xc for yc in ys for xc in xs])
    py = np.array([yc for yc in ys for xc in xs])
    sig, bound = np.full(px.size, np.nan), np.zeros(px.size)
    v, _, _, terms = ar.aperture_sums(rms.astype(np.float64) ** 2, None, None, px, py, radius, with_terms=True) if px.size \
        else (np.zeros(0), 0, 0, np.zeros((5, 0)))
    fb, _ = ar.sums_bounds(terms)
    i0, i1, j0, j1, ok = ar.boxes(px, py, radius, nx, ny)
    for k in range(px.size):
        box = (slice(j0[k], j1[k]), slice(i0[k], i1[k]))
        r = rms[box]
        good = bool(np.all(np.isfinite(r) & (r > 0)))
        if mask is not None and ((np.asarray(mask)[box].astype(np.int64) & bad_bits) != 0).any():
            good = False
        if good:
            sig[k] = math.sqrt(max(v[k], 0.0))
            bound[k] = fb[k] / (2.0 * sig[k])
    st = clip_stats(sig, 3.0, 0)
    return st['median'], st['n_valid'], px.size, sig, bound


# ---- the operator -----------------------------------------------------------------------------------------------------
def card_slots(apertures):
    free = iter(k for k in range(1, 2 * len(apertures) + 2) if k != 4)
    return [4 if d == 2.0 * APERTURE_RADIUS else next(free) for d in apertures]


def measure(data, sub, positions, centroid, rms=None, mask=None, bad_bits=0, saturate=None, mag=None, magzp=None,
            pixel_scale=None, apertures=(2.0, 3.0, 4.0, 6.0, 10.0, 14.0), ref_diameter=20.0, annulus=(24.0, 36.0),
            sn_min=50.0, crossid_radius=2.0, clip_sigma=3.0, clip_iter=5, nsky_min=50, min_stars=5, maglim_nsigma=5.0,
            maglim_step=32):
    """The cards of ``measure_photometry`` on numpy planes.

    ``positions``: (px, py), the projected 0-based positions of every catalogue star (``mag`` beside them), or the
    integer peaks of the image's own stars (``mag`` None).  ``centroid(sub, ix, iy) -> (cx, cy)``: the centroid that
    stands in for ``zm_star_fwhm`` (``oracle.detect.star_fwhm``, which tests/test_seeing_gpu.py pins the kernel to).
    Returns a dict: ``cards`` {key: value}, ``index`` (rows measured), ``used``, ``x``, ``y``, ``growth``, ``sn``,
    ``shift`` (arcsec, with a catalogue), and the statistics dicts ``apcor_stats`` / ``zp_stats``."""
    data = np.asarray(data, dtype=np.float32)
    ny, nx = data.shape
    px, py = (np.asarray(v, dtype=np.float64) for v in positions)
    r_in, r_out = 0.5 * annulus[0], 0.5 * annulus[1]
    radii = [0.5 * d for d in apertures] + [0.5 * ref_diameter]
    shift = None
    if mag is None:
        cand = np.arange(px.size)
        cx, cy = centroid(sub, px.astype(np.int64), py.astype(np.int64))
        keep = np.isfinite(cx) & np.isfinite(cy)
    else:
        with np.errstate(invalid='ignore'):
            inside = (px >= r_out) & (px <= nx - 1 - r_out) & (py >= r_out) & (py <= ny - 1 - r_out)
        cand = np.flatnonzero(inside)
        cx, cy = centroid(sub, np.rint(px[cand]).astype(np.int64), np.rint(py[cand]).astype(np.int64))
        with np.errstate(invalid='ignore'):
            shift = np.hypot(cx - px[cand], cy - py[cand]) * pixel_scale
            keep = np.isfinite(cx) & np.isfinite(cy) & (shift <= crossid_radius)
        fin = np.isfinite(px) & np.isfinite(py)
        for k, c in enumerate(cand):
            d2 = (px - px[c]) ** 2 + (py - py[c]) ** 2
            d2[c] = np.inf
            if (d2[fin] < r_out * r_out).any():
                keep[k] = False
    x, y, index = cx[keep], cy[keep], cand[keep]
    g = growth(data, x, y, radii, rms=rms, mask=mask, bad_bits=bad_bits, saturate=saturate, r_in=r_in, r_out=r_out,
               kappa=clip_sigma, maxiter=clip_iter, nsky_min=nsky_min)
    flux, err = g['flux'], g['err']
    with np.errstate(invalid='ignore', divide='ignore'):
        sn = flux[:, -1] / err[:, -1]
        used = (g['flags'] == 0) & np.all(flux > 0, axis=1) & (sn >= sn_min)
    out = dict(index=index, used=used, x=x, y=y, growth=g, sn=sn, shift=None if shift is None else shift[keep],
               shift_all=shift, cards={}, radii=radii)
    if used.sum() < min_stars:
        out['too_few'] = True
        return out
    slots = card_slots(apertures)
    k4 = slots.index(4)
    dm = -2.5 * np.log10(flux[used, -1:] / flux[used, :-1])
    cm, cst = clipped_median(dm, clip_sigma, clip_iter)
    cards = out['cards']
    for k, slot in enumerate(slots):
        cards[f'APCOR{slot}'] = cm[k, 0]
        cards[f'APCORUN{slot}'] = 1.2533 * cm[k, 1] / math.sqrt(cm[k, 2])
    out['apcor_stats'], out['dm'] = cst, dm
    zp = magzp
    if mag is not None:
        zpi = np.asarray(mag, np.float64)[index[used]] + 2.5 * np.log10(flux[used, k4]) - cards['APCOR4']
        zm, zst = clipped_median(zpi, clip_sigma, clip_iter)
        zp = float(zm[0, 0])
        cards['MAGZP'] = zp
        cards['MAGZPUNC'] = math.hypot(1.2533 * zm[0, 1] / math.sqrt(zm[0, 2]), cards['APCORUN4'])
        cards['MAGZPRMS'], cards['NMATCHES'] = zm[0, 1], int(zm[0, 2])
        out['zp_stats'], out['zp_stars'] = zst[0], zpi
    if rms is not None and zp is not None:
        step = maglim_step
        while len(lattice(nx, step, APERTURE_RADIUS)) * len(lattice(ny, step, APERTURE_RADIUS)) > 16384:
            step *= 2
        med, nu, npts, _, _ = maglim_sigma(rms, mask, bad_bits, APERTURE_RADIUS, step)
        if np.isfinite(med):
            cards['MAGLIM'] = zp + cards['APCOR4'] - 2.5 * math.log10(maglim_nsigma * med)
        out['maglim_sigma'] = med
    cards['ZMPHOTCA'] = True
    return out


def analytic_apcor(r_k, r_ref, fwhm):
    """``-2.5 log10((1 - exp(-r_ref^2 / 2 s^2)) / (1 - exp(-r_k^2 / 2 s^2)))`` of a circular Gaussian."""
    s2 = (fwhm / 2.3548200450309493) ** 2
    return -2.5 * math.log10((1.0 - math.exp(-r_ref * r_ref / (2 * s2))) / (1.0 - math.exp(-r_k * r_k / (2 * s2))))
