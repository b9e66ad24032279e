"""Photometric calibration from the pixels: ``APCORk``, ``MAGZP`` and ``MAGLIM`` ("Photometric calibration").

The reference never measures these cards: it inherits them from IPAC's headers on single exposures, and
``Subtraction.from_images`` copies ``MAGZP`` and ``APCOR4`` from the science image when they are there.  Coadds made
here have no IPAC header, so forced photometry, light curves and alerts on them have no magnitude scale.  This module
measures the three quantities on the image itself and writes the cards the rest of the code already reads
(``zp = MAGZP + APCOR4``, ``diffmaglim`` from ``MAGLIM``).  It is this project's own operator, as ``calibrate_astrometry``
is: IPAC's PSF-fit ``MAGZP``, colour terms and spatially varying zero points are not claimed.

The hot path is ``csrc/photcal.hip``: ``zm_growth`` (curves of growth with a clipped local sky, one wave per star, every
radius in one pass), ``zm_clipped_median`` (clipped median / MAD per column, the column in LDS) and ``zm_maglim_dev``
(aperture noise over a lattice and its median).
"""
import ctypes as C
import math
import warnings

import numpy as np

from . import _lib
from . import fits as _fits
from ._lib import as_f32, as_i32, check, ptr
from .constants import APER_KEY, APERTURE_RADIUS, BAD_SUM

__all__ = ['growth_curves', 'growth_curves_dev', 'clipped_median', 'clipped_median_dev', 'limiting_magnitude',
           'read_photrefcat', 'measure', 'measure_photometry', 'measure_planes', 'calibrate_photometry', 'photcal_settings', 'write_maglim']

PHOTREF_COLUMNS = ('X_WORLD', 'Y_WORLD', 'MAG')
HALF = 10                       # centroid window of zm_star_fwhm: 21 x 21, as seeing.py
NSIGMA = 30.0                   # detection threshold of the image's own stars, in background sigmas (seeing.py)
CAP = 65536
DEFAULTS = dict(photref=None, apertures=(2.0, 3.0, 4.0, 6.0, 10.0, 14.0), ref_diameter=20.0, annulus=(24.0, 36.0),
                sn_min=50.0, crossid_radius=2.0, clip_sigma=3.0, clip_iter=5, nsky_min=50, min_stars=5, nmax=1000,
                maglim_nsigma=5.0, maglim_step=32)
_KEYS = {'PHOTREF_NAME': 'photref', 'APERTURES': 'apertures', 'REF_DIAMETER': 'ref_diameter', 'ANNULUS': 'annulus',
         'SN_MIN': 'sn_min', 'CROSSID_RADIUS': 'crossid_radius', 'CLIP_SIGMA': 'clip_sigma', 'CLIP_ITER': 'clip_iter',
         'NSKY_MIN': 'nsky_min', 'MIN_STARS': 'min_stars', 'NMAX': 'nmax', 'MAGLIM_NSIGMA': 'maglim_nsigma',
         'MAGLIM_STEP': 'maglim_step'}


def _engine(engine):
    from .engine import get_engine
    return engine or get_engine()


# ---- settings ---------------------------------------------------------------------------------------------------------
def _floats(v, what):
    tok = str(v).replace('(', '').replace(')', '').split(',') if not isinstance(v, (list, tuple, np.ndarray)) else list(v)
    try:
        return tuple(float(t) for t in tok)
    except (TypeError, ValueError):
        raise ValueError(f'photcal_kws: {what} takes numbers (got {v!r})')


def _check_settings(st):
    aps = st['apertures']
    if not 1 <= len(aps) <= _lib.GROWTH_NAPER_MAX - 1:
        raise ValueError(f'photcal_kws: APERTURES takes 1 to {_lib.GROWTH_NAPER_MAX - 1} diameters (got {len(aps)})')
    if any(b <= a for a, b in zip(aps, aps[1:])) or aps[0] <= 0:
        raise ValueError(f'photcal_kws: APERTURES must be positive and ascend (got {aps})')
    if 2.0 * APERTURE_RADIUS not in aps:
        raise ValueError(f'photcal_kws: APERTURES must contain {2.0 * APERTURE_RADIUS:g}, the diameter of {APER_KEY} '
                         f'(got {aps})')
    if not st['ref_diameter'] > aps[-1]:
        raise ValueError(f'photcal_kws: REF_DIAMETER {st["ref_diameter"]:g} must exceed the largest of APERTURES')
    a0, a1 = st['annulus']
    if not 0 <= a0 < a1:
        raise ValueError(f'photcal_kws: ANNULUS {a0:g},{a1:g}: two ascending diameters')
    if 0.5 * a1 > _lib.GROWTH_ROUT_MAX:
        raise ValueError(f'photcal_kws: ANNULUS outer diameter {a1:g} beyond {2 * _lib.GROWTH_ROUT_MAX:g} px')
    for k in ('sn_min', 'crossid_radius', 'clip_sigma', 'maglim_nsigma'):
        if not st[k] > 0:
            raise ValueError(f'photcal_kws: {k.upper()} must be positive (got {st[k]!r})')
    for k in ('clip_iter', 'nsky_min'):
        if st[k] < 0:
            raise ValueError(f'photcal_kws: {k.upper()} must not be negative (got {st[k]!r})')
    for k in ('min_stars', 'nmax', 'maglim_step'):
        if st[k] < 1:
            raise ValueError(f'photcal_kws: {k.upper()} must be at least 1 (got {st[k]!r})')
    if st['nmax'] > _lib.CLIPMED_NMAX:
        raise ValueError(f'photcal_kws: NMAX {st["nmax"]} beyond {_lib.CLIPMED_NMAX}')
    return st


def photcal_settings(photcal_kws=None, **overrides):
    """``photcal_kws`` (``-KEY value`` pairs in the manner of ``scamp_kws``) -> a dict of settings with every default
    filled in.  An unknown key raises ``ValueError``.  ``overrides``: settings by their lower-case names."""
    st = dict(DEFAULTS)
    for k, v in (photcal_kws or {}).items():
        key = str(k).upper().lstrip('-')
        if key not in _KEYS:
            raise ValueError(f'photcal_kws: -{key} {v} is not a key of the photometric calibration '
                             f'(known: {", ".join(_KEYS)})')
        st[_KEYS[key]] = v
    for k, v in overrides.items():
        if k not in DEFAULTS:
            raise ValueError(f'photcal: unknown setting {k!r} (known: {", ".join(DEFAULTS)})')
        st[k] = v
    st['apertures'] = _floats(st['apertures'], 'APERTURES')
    st['annulus'] = _floats(st['annulus'], 'ANNULUS')
    if len(st['annulus']) != 2:
        raise ValueError(f'photcal_kws: ANNULUS takes two diameters (got {st["annulus"]})')
    for k in ('ref_diameter', 'sn_min', 'crossid_radius', 'clip_sigma', 'maglim_nsigma'):
        st[k] = float(st[k])
    for k in ('clip_iter', 'nsky_min', 'min_stars', 'nmax', 'maglim_step'):
        st[k] = int(st[k])
    st['photref'] = None if st['photref'] is None else str(st['photref'])
    return _check_settings(st)


def card_names(apertures):
    """The ``APCORk`` slot of every aperture: the one of diameter ``2 APERTURE_RADIUS`` is slot 4 (``APCOR4``, the card
    every consumer reads), the others take 1, 2, 3, 5, 6, ... in order.  With the default list that is ZTF's own
    numbering, ``APCOR1 .. APCOR6``."""
    free = iter(k for k in range(1, 2 * len(apertures) + 2) if k != 4)
    return [4 if d == 2.0 * APERTURE_RADIUS else next(free) for d in apertures]


# ---- the star catalogue -----------------------------------------------------------------------------------------------
def read_photrefcat(path):
    """``(ra, dec, mag, magerr)`` of a star catalogue in the FITS_LDAC layout ``scamp.write_astrefcat`` writes:
    ``X_WORLD``, ``Y_WORLD`` (degrees) and ``MAG``; ``MAGERR`` is optional and defaults to 0."""
    tab = _fits.read_ldac(str(path))[0]
    names = tab.dtype.names or ()
    missing = [c for c in PHOTREF_COLUMNS if c not in names]
    if missing:
        raise ValueError(f'{path}: not a photometric reference catalogue (no {", ".join(missing)})')
    f64 = lambda k: np.array(tab[k], dtype=np.float64)
    return f64('X_WORLD'), f64('Y_WORLD'), f64('MAG'), f64('MAGERR') if 'MAGERR' in names else np.zeros(len(tab))


# ---- the three launches -----------------------------------------------------------------------------------------------
def _radii(radii):
    r = np.ascontiguousarray(np.atleast_1d(radii), dtype=np.float64)
    if r.ndim != 1 or not 1 <= r.size <= _lib.GROWTH_NAPER_MAX:
        raise ValueError(f'growth_curves: 1 to {_lib.GROWTH_NAPER_MAX} radii (got {r.size})')
    return r


def growth_curves(data, x, y, radii, rms=None, mask=None, saturate=None, annulus=(12.0, 18.0), bad_bits=BAD_SUM,
                  kappa=3.0, maxiter=5, nsky_min=50, engine=None):
    """Curves of growth at 0-based pixel positions (``zm_growth``): ``radii`` ascending in pixels (at most 8),
    ``annulus`` the inner and outer sky radii.  Returns a dict: ``flux`` and ``err`` of shape (n, len(radii)), ``sky``,
    ``sky_sigma``, ``nsky`` and ``flags`` (bits: 1 bad pixel, 2 saturated, 4 non-finite pixel in the largest aperture;
    8 aperture box, 16 annulus clipped by the frame; 32 fewer than ``nsky_min`` sky pixels; 64 position not finite)."""
    eng = _engine(engine)
    img, rms, mask = as_f32(data), as_f32(rms), as_i32(mask)
    if img.ndim != 2:
        raise ValueError('growth_curves: data must be a 2-D image')
    for a, nm in ((rms, 'rms'), (mask, 'mask')):
        if a is not None and a.shape != img.shape:
            raise ValueError(f'growth_curves: {nm} has shape {a.shape}, the image {img.shape}')
    ny, nx = img.shape
    x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
    y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError('growth_curves: x and y must be 1-D and of one length')
    r = _radii(radii)
    n, na = x.size, r.size
    out = dict(flux=np.zeros((n, na)), err=np.zeros((n, na)), sky=np.zeros(n), sky_sigma=np.zeros(n),
               nsky=np.zeros(n, np.int32), flags=np.zeros(n, np.int32))
    check(eng.L.zm_growth(eng.ctx, ptr(img), ptr(rms), ptr(mask), int(bad_bits), float(saturate or 0.0), nx, ny, n,
                          ptr(x), ptr(y), na, ptr(r), float(annulus[0]), float(annulus[1]), float(kappa), int(maxiter),
                          int(nsky_min), ptr(out['flux']), ptr(out['err']), ptr(out['sky']), ptr(out['sky_sigma']),
                          ptr(out['nsky']), ptr(out['flags'])), 'zm_growth')
    return out


def growth_curves_dev(img, x, y, radii, rms=None, mask=None, saturate=None, annulus=(12.0, 18.0), bad_bits=BAD_SUM,
                      kappa=3.0, maxiter=5, nsky_min=50, engine=None):
    """``growth_curves`` on planes that lie in HBM (``zm_growth_dev``): ``img`` / ``rms`` float32 and ``mask`` int32
    torch tensors, ``x`` / ``y`` float64 tensors on the same device.  Only enqueues; the results are device tensors.
    The caller has the engine's stream current."""
    import torch
    eng = _engine(engine)
    if img.dtype != torch.float32 or img.dim() != 2 or not img.is_contiguous():
        raise ValueError('growth_curves_dev: img must be a contiguous 2-D float32 tensor')
    for a, nm, dt in ((rms, 'rms', torch.float32), (mask, 'mask', torch.int32)):
        if a is not None and (a.dtype != dt or a.shape != img.shape or not a.is_contiguous() or a.device != img.device):
            raise ValueError(f'growth_curves_dev: {nm} must be a contiguous {dt} tensor of the image\'s shape and device')
    for a, nm in ((x, 'x'), (y, 'y')):
        if a.dtype != torch.float64 or a.dim() != 1 or not a.is_contiguous() or a.device != img.device:
            raise ValueError(f'growth_curves_dev: {nm} must be a contiguous 1-D float64 tensor on the image\'s device')
    if x.numel() != y.numel():
        raise ValueError('growth_curves_dev: x and y differ in length')
    ny, nx = img.shape
    r = _radii(radii)
    n, na = x.numel(), r.size
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=img.device)
    out = dict(flux=new((n, na), torch.float64), err=new((n, na), torch.float64), sky=new(n, torch.float64),
               sky_sigma=new(n, torch.float64), nsky=new(n, torch.int32), flags=new(n, torch.int32))
    dp = lambda t: None if t is None else t.data_ptr()
    check(eng.L.zm_growth_dev(eng.ctx, dp(img), dp(rms), dp(mask), int(bad_bits), float(saturate or 0.0), nx, ny, n,
                              dp(x), dp(y), na, ptr(r), float(annulus[0]), float(annulus[1]), float(kappa),
                              int(maxiter), int(nsky_min), dp(out['flux']), dp(out['err']), dp(out['sky']),
                              dp(out['sky_sigma']), dp(out['nsky']), dp(out['flags'])), 'zm_growth_dev')
    return out


def clipped_median(values, kappa=3.0, maxiter=5, engine=None):
    """Clipped median per column (``zm_clipped_median``): ``values`` of shape (n,) or (n, ncol), float64; an entry that
    is not finite is not used.  Median, then ``1.4826 MAD``, then entries with ``|v - median| > kappa sigma`` are
    dropped, up to ``maxiter`` times (0: the plain median and MAD).  Returns ``[median, sigma, n_used, n_valid]``, one
    row per column (a single row for 1-D input)."""
    eng = _engine(engine)
    v = np.asarray(values, dtype=np.float64)
    one = v.ndim == 1
    if one:
        v = v[:, None]
    if v.ndim != 2:
        raise ValueError('clipped_median: values must be 1-D or 2-D')
    if v.strides[1] != 8 or v.strides[0] < 8 * v.shape[1] or v.strides[0] % 8:
        v = np.ascontiguousarray(v)
    n, ncol = v.shape
    out = np.zeros((ncol, 4))
    check(eng.L.zm_clipped_median(eng.ctx, ptr(v), n, ncol, v.strides[0] // 8 if n else ncol, float(kappa),
                                  int(maxiter), ptr(out)), 'zm_clipped_median')
    return out[0] if one else out


def clipped_median_dev(values, kappa=3.0, maxiter=5, engine=None):
    """``clipped_median`` on a float64 torch tensor of shape (n, ncol) in HBM, rows ``values.stride(0)`` apart
    (``zm_clipped_median_dev``).  Only enqueues; returns a (ncol, 4) device tensor."""
    import torch
    eng = _engine(engine)
    if values.dtype != torch.float64 or values.dim() != 2 or \
            (values.numel() and values.shape[1] > 1 and values.stride(1) != 1):
        raise ValueError('clipped_median_dev: values must be a 2-D float64 tensor whose columns are adjacent')
    n, ncol = values.shape
    stride = values.stride(0) if n > 1 else ncol
    if stride < ncol:
        raise ValueError('clipped_median_dev: rows overlap')
    out = torch.empty((ncol, 4), dtype=torch.float64, device=values.device)
    check(eng.L.zm_clipped_median_dev(eng.ctx, values.data_ptr(), n, ncol, stride, float(kappa), int(maxiter),
                                      out.data_ptr()), 'zm_clipped_median_dev')
    return out


def lattice(n, step, radius):
    """(first centre, count) of the limiting magnitude's lattice along an axis of ``n`` pixels: centres at
    ``step / 2 + i step`` that lie at least ``radius + 1`` pixels from both edges (the frame spans -0.5 .. n - 0.5)."""
    h, margin = 0.5 * step, radius + 1.0
    i0 = max(int(math.ceil((margin - 0.5 - h) / step)), 0)
    i1 = int(math.floor((n - 0.5 - margin - h) / step))
    return h + i0 * step, max(i1 - i0 + 1, 0)


def limiting_magnitude(image_or_planes, zp, nsigma=5.0, radius=APERTURE_RADIUS, step=32, bad_bits=BAD_SUM, engine=None):
    """The ``nsigma`` limiting magnitude in an aperture of ``radius`` pixels: ``zp - 2.5 log10(nsigma x median
    sigma_ap)``, ``sigma_ap = sqrt(sum(rms^2 frac))`` over a lattice of apertures every ``step`` pixels
    (``zm_maglim_dev``).  ``image_or_planes``: an image object (its ``rms_image`` and ``mask_image``) or ``(rms, mask)``
    as numpy arrays or as torch tensors in HBM; ``mask`` may be None.  ``zp``: the zero point of fluxes in that aperture
    (``MAGZP + APCOR4``).  A lattice of more than 16384 points takes twice the step, as often as needed.  Returns a dict:
    ``maglim`` (NaN when no lattice point is usable), ``sigma_ap``, ``nused``, ``npoints``, ``step``.

    This call blocks: it waits for the engine's stream and copies the three doubles back (there is no enqueue-only
    form; the card is made once per image).  ``DeviceSubtraction.maglim()`` calls it on its chain's stream."""
    import torch
    eng = _engine(engine)
    if isinstance(image_or_planes, (tuple, list)):
        rms, mask = image_or_planes
    else:
        rms = image_or_planes.rms_image.data
        m = getattr(image_or_planes, 'mask_image', None)
        mask = None if m is None else m.data
    if not torch.is_tensor(rms):
        rms = torch.from_numpy(as_f32(rms)).to(f'cuda:{eng.device}')
        mask = None if mask is None else torch.from_numpy(as_i32(mask)).to(rms.device)
        torch.cuda.synchronize(rms.device)
    if rms.dtype != torch.float32 or rms.dim() != 2 or not rms.is_contiguous():
        raise ValueError('limiting_magnitude: rms must be a contiguous 2-D float32 plane')
    if mask is not None and (mask.dtype != torch.int32 or mask.shape != rms.shape or not mask.is_contiguous()):
        raise ValueError('limiting_magnitude: mask must be a contiguous int32 plane of the shape of rms')
    ny, nx = rms.shape
    step = int(step)
    if step < 1:
        raise ValueError('limiting_magnitude: step must be at least 1')
    while lattice(nx, step, radius)[1] * lattice(ny, step, radius)[1] > _lib.CLIPMED_NMAX:
        step *= 2
    out = torch.empty(3, dtype=torch.float64, device=rms.device)
    check(eng.L.zm_maglim_dev(eng.ctx, rms.data_ptr(), None if mask is None else mask.data_ptr(), int(bad_bits), nx, ny,
                              float(radius), step, out.data_ptr()), 'zm_maglim_dev')
    eng.synchronize()
    med, nused, npts = out.cpu().tolist()
    with np.errstate(invalid='ignore', divide='ignore'):
        maglim = float(zp - 2.5 * np.log10(nsigma * med))
    return dict(maglim=maglim, sigma_ap=med, nused=int(nused), npoints=int(npts), step=step)


# ---- the operator -----------------------------------------------------------------------------------------------------
def _own_stars(eng, sub, bad8, bmean, bsig, saturate, r_out, nmax):
    """The image's own stars: the ``zm_find_stars`` route of ``seeing.py`` with isolation ``ceil(r_out)``, peaks below
    half of SATURATE, the brightest ``nmax``.  Integer pixel positions."""
    ny, nx = sub.shape
    iso = int(math.ceil(r_out))
    lo = float(NSIGMA * max(bsig, 1e-6))
    hi = float(0.5 * saturate - bmean) if saturate else 3.0e38
    xs, ys, pk = np.empty(CAP, np.int32), np.empty(CAP, np.int32), np.empty(CAP, np.float32)
    n = C.c_int(0)
    while True:
        check(eng.L.zm_find_stars(eng.ctx, ptr(sub), ptr(bad8), nx, ny, lo, hi, iso, iso, CAP, ptr(xs), ptr(ys), ptr(pk),
                                  C.byref(n)), 'zm_find_stars')
        if n.value <= CAP:
            break
        lo *= 2.0
    m = n.value
    order = np.lexsort((xs[:m], ys[:m], -pk[:m].astype(np.float64)))[:nmax]
    return np.ascontiguousarray(xs[:m][order]), np.ascontiguousarray(ys[:m][order])


def _centroids(eng, sub, sx, sy):
    ny, nx = sub.shape
    k = len(sx)
    fw, cx, cy = np.empty(k), np.empty(k), np.empty(k)
    if k:
        check(eng.L.zm_star_fwhm(eng.ctx, ptr(sub), nx, ny, k, ptr(sx), ptr(sy), HALF, ptr(fw), ptr(cx), ptr(cy)),
              'zm_star_fwhm')
    return cx, cy


def measure_planes(data, wcs=None, mask=None, rms=None, saturate=None, magzp=None, stars=None, engine=None,
                   bad_bits=BAD_SUM, **settings):
    """``measure_photometry`` on numpy planes.  ``wcs`` is needed with a catalogue; ``magzp``: the header's ``MAGZP``,
    for ``MAGLIM`` when none is fitted.  Returns the dict ``measure_photometry`` documents."""
    st = photcal_settings(None, **settings)
    eng = _engine(engine)
    data = as_f32(data)
    mask = as_i32(mask)
    rms = as_f32(rms)
    ny, nx = data.shape
    aps = st['apertures']
    radii = np.array([0.5 * d for d in aps] + [0.5 * st['ref_diameter']])
    r_in, r_out = 0.5 * st['annulus'][0], 0.5 * st['annulus'][1]
    bad = None if mask is None else (mask & int(bad_bits)) != 0
    wgt = None if bad is None else np.where(bad, 0.0, 1.0).astype(np.float32)
    _, _, sub, (bmean, bsig) = eng.background(data, wgt, want=('sub',))
    cat = None
    if stars is None:
        bad8 = None if bad is None else np.ascontiguousarray(bad).astype(np.uint8)
        sx, sy = _own_stars(eng, sub, bad8, bmean, bsig, saturate, r_out, st['nmax'])
        cx, cy = _centroids(eng, sub, sx, sy)
        keep = np.isfinite(cx) & np.isfinite(cy)
        x, y, index, peaks = cx[keep], cy[keep], np.flatnonzero(keep), (sx[keep], sy[keep])
    else:
        if wcs is None:
            raise ValueError('photcal: a star catalogue needs the image\'s WCS')
        if isinstance(stars, (str, bytes)) or hasattr(stars, '__fspath__'):
            stars = read_photrefcat(stars)
        ra, dec, mag = (np.asarray(v, dtype=np.float64).ravel() for v in stars[:3])
        cat = dict(ra=ra, dec=dec, mag=mag)
        px, py = wcs.all_world2pix(ra, dec, 0)
        px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
        with np.errstate(invalid='ignore'):
            inside = (px >= r_out) & (px <= nx - 1 - r_out) & (py >= r_out) & (py <= ny - 1 - r_out)
        cand = np.flatnonzero(inside)
        sx = np.ascontiguousarray(np.rint(px[cand]), dtype=np.int32)
        sy = np.ascontiguousarray(np.rint(py[cand]), dtype=np.int32)
        cx, cy = _centroids(eng, sub, sx, sy)
        scale = 3600.0 * float(np.sqrt(abs(np.linalg.det(np.asarray(wcs.cd, dtype=np.float64).reshape(2, 2)))))
        with np.errstate(invalid='ignore'):
            shift = np.hypot(cx - px[cand], cy - py[cand]) * scale
            keep = np.isfinite(cx) & np.isfinite(cy) & (shift <= st['crossid_radius'])
        # a neighbour in the catalogue (kept or not) within r_out of the projected position
        fin = np.flatnonzero(np.isfinite(px) & np.isfinite(py))
        for k, c in enumerate(cand):
            if keep[k]:
                d2 = (px[fin] - px[c]) ** 2 + (py[fin] - py[c]) ** 2
                d2[fin == c] = np.inf
                if d2.size and d2.min() < r_out * r_out:
                    keep[k] = False
        x, y, index, peaks = cx[keep], cy[keep], cand[keep], (sx[keep], sy[keep])
    g = growth_curves(data, x, y, radii, rms=rms, mask=mask, saturate=saturate, annulus=(r_in, r_out), bad_bits=bad_bits,
                      kappa=st['clip_sigma'], maxiter=st['clip_iter'], nsky_min=st['nsky_min'], engine=eng)
    flux, err = g['flux'], g['err']
    with np.errstate(invalid='ignore', divide='ignore'):
        sn = flux[:, -1] / err[:, -1]
        used = (g['flags'] == 0) & np.all(flux > 0, axis=1) & (sn >= st['sn_min'])
    nused = int(used.sum())
    if nused < st['min_stars']:
        raise RuntimeError(f'Unable to calibrate the photometry: {nused} usable star(s) of {x.size} measured, '
                           f'MIN_STARS is {st["min_stars"]}')
    slots = card_names(aps)
    k4 = slots.index(4)
    dm = -2.5 * np.log10(flux[used, -1:] / flux[used, :-1])            # (nused, len(aps))
    cm = clipped_median(dm, st['clip_sigma'], st['clip_iter'], engine=eng)
    cards = []
    apcor = {}
    for k, (d, slot) in enumerate(zip(aps, slots)):
        apcor[slot] = float(cm[k, 0])
        cards.append((f'APCOR{slot}', float(cm[k, 0]), f'Aperture correction, D = {d:g} to {st["ref_diameter"]:g} px (mag)'))
        cards.append((f'APCORUN{slot}', float(1.2533 * cm[k, 1] / math.sqrt(cm[k, 2])), f'Uncertainty of APCOR{slot} (mag)'))
    out = dict(x=x, y=y, index=index, peaks=peaks, used=used, growth=g, sn=sn, apcor=apcor, apcor_stats=cm, settings=st, radii=radii)
    zp = magzp
    if cat is not None:
        zpi = cat['mag'][index[used]] + 2.5 * np.log10(flux[used, k4]) - apcor[4]
        zm = clipped_median(zpi, st['clip_sigma'], st['clip_iter'], engine=eng)
        zp = float(zm[0])
        # MAGZP carries the error of APCOR4 it was shifted by: on background-limited stars that term is the larger one
        # (the reference aperture holds 11 x the pixels of aperture 4), so the two are added in quadrature
        unc = math.hypot(1.2533 * zm[1] / math.sqrt(zm[2]), 1.2533 * cm[k4, 1] / math.sqrt(cm[k4, 2]))
        cards += [('MAGZP', zp, f'Zero point in the D = {st["ref_diameter"]:g} px aperture (mag)'),
                  ('MAGZPUNC', float(unc), 'Uncertainty of MAGZP, that of APCOR4 included (mag)'),
                  ('MAGZPRMS', float(zm[1]), 'Clipped 1.4826 MAD of the zero points of the stars (mag)'),
                  ('NMATCHES', int(zm[2]), 'Catalogue stars used in MAGZP')]
        out.update(zp_stars=zpi, zp_stats=zm)
    if rms is not None and zp is not None:
        ml = limiting_magnitude((rms, mask), zp + apcor[4], nsigma=st['maglim_nsigma'], radius=APERTURE_RADIUS,
                                step=st['maglim_step'], bad_bits=bad_bits, engine=eng)
        out['maglim'] = ml
        if np.isfinite(ml['maglim']):
            cards.append(('MAGLIM', ml['maglim'], f'{st["maglim_nsigma"]:g}-sigma limiting magnitude, r = '
                                                  f'{APERTURE_RADIUS:g} px aperture'))
        else:
            warnings.warn('photcal: no usable aperture on the noise map, MAGLIM is not written')
    cards.append(('ZMPHOTCA', True, 'Photometric cards measured from the pixels'))
    out['cards'] = cards
    return out


def _has_noise_map(image):
    return hasattr(image, '_rmsimg') or hasattr(image, '_weightimg')


def measure_photometry(image, stars=None, engine=None, **settings):
    """Measure the photometric cards of ``image`` (an image object with a mask; nothing is written).

    ``stars``: None - the image's own isolated, unsaturated stars, which give ``APCORk`` (and ``MAGLIM`` when the header
    has a ``MAGZP``) - or a catalogue, ``(ra, dec, mag)`` or the path of a FITS_LDAC file (``read_photrefcat``), which
    gives ``MAGZP`` as well.  ``settings``: the lower-case names of ``photcal_kws``.

    Returns a dict: ``cards`` [(key, value, comment)], ``x`` / ``y`` (the 0-based positions measured), ``peaks`` (the
    pixels their centroids started from), ``index`` (their catalogue rows, or their rank among the image's stars), ``used`` (which of them entered the medians), ``growth``
    (what ``growth_curves`` returned), ``sn``, ``apcor`` {slot: value}, ``apcor_stats``, and with a catalogue
    ``zp_stars`` / ``zp_stats``; ``maglim`` (the dict of ``limiting_magnitude``) when there is a noise map and a zero
    point.  Raises ``RuntimeError`` when fewer than ``MIN_STARS`` stars are usable."""
    m = getattr(image, 'mask_image', None)
    sat = image.header.get('SATURATE')
    magzp = image.header.get('MAGZP')
    return measure_planes(image.data, wcs=image.wcs if stars is not None else None, mask=None if m is None else m.data,
                          rms=image.rms_image.data if _has_noise_map(image) else None,
                          saturate=float(sat) if sat else None, magzp=None if magzp is None else float(magzp),
                          stars=stars, engine=engine, **settings)


measure = measure_photometry


def calibrate_photometry(image_or_images, photcal_kws=None, inplace=False):
    """Measure ``APCORk``, ``MAGZP`` (with ``PHOTREF_NAME``) and ``MAGLIM`` of the input images and write the cards into
    their headers, in the manner of ``calibrate_astrometry``.  ``inplace``: the cards go into the headers of the images
    themselves, which are saved when they are mapped to a file; otherwise into transaction copies, and the caller's
    objects and files stay as they are.  Returns one result dict of ``measure_photometry`` per image; its ``image`` is
    the object that carries the cards."""
    from .scamp import transaction_copies
    images = np.atleast_1d(image_or_images).tolist()
    st = photcal_settings(photcal_kws)
    stars = None if st['photref'] is None else read_photrefcat(st['photref'])
    targets = images if inplace else transaction_copies(images)
    results = []
    for target in targets:
        res = measure_photometry(target, stars=stars, **{k: v for k, v in st.items() if k != 'photref'})
        if target.header_comments is None:
            target.header_comments = {}
        for key, value, comment in res['cards']:
            target.header[key] = value
            target.header_comments[key] = comment
        if inplace and target.ismapped:
            target.save()
        res['image'] = target
        results.append(res)
    return results


def write_maglim(image, nsigma=5.0, step=32, engine=None):
    """``MAGLIM`` of an image from its own rms plane and the zero point its header carries (``MAGZP + APCOR4``: what a
    subtraction copies from its science image), written into the header and saved when the image is mapped.  Returns the
    dict of ``limiting_magnitude``, or None - with a warning, and no card - when the header has no zero point or no
    aperture on the noise map is usable."""
    h = image.header
    if 'MAGZP' not in h or APER_KEY not in h:
        warnings.warn(f'"{image.basename}" has no MAGZP / {APER_KEY} card: MAGLIM is not written')
        return None
    ml = limiting_magnitude(image, float(h['MAGZP']) + float(h[APER_KEY]), nsigma=nsigma, radius=APERTURE_RADIUS,
                            step=step, engine=engine)
    if not np.isfinite(ml['maglim']):
        warnings.warn(f'"{image.basename}": no usable aperture on the noise map, MAGLIM is not written')
        return None
    if image.header_comments is None:
        image.header_comments = {}
    h['MAGLIM'] = ml['maglim']
    image.header_comments['MAGLIM'] = f'{nsigma:g}-sigma limiting magnitude, r = {APERTURE_RADIUS:g} px aperture'
    if image.ismapped:
        image.save()
    return ml
