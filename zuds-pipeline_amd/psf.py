"""PSF-fit forced photometry: the star model of an image and linear fits of it ("PSF photometry").

The light curves of ``lightcurve.py`` are sums in an r = 3 px aperture.  On background-limited sources a PSF-weighted fit
is the better estimator, and it measures a source that has a flagged pixel in its aperture.  This module builds the model
of an image from its own stars (or a catalogue's) and fits it at given positions.  It is this project's own operator, as
``photcal.py`` is - the reference has no PSF photometry - and opt-in everywhere: with every keyword at its default no
product and no table changes.

The hot path is ``csrc/psf.hip``: ``zm_psf_build`` (Lanczos-3 cutouts of the stars, one wave per star; the clipped median
of every entry by ``zm_clipped_median``; support, floor and unit sum), ``zm_psf_photometry`` (one wave per position, the
model in LDS) and ``zm_psf_photometry_batch_dev`` (one launch for all pairs of a footprint join).

The zero point of a PSF flux is ``MAGZP + PSFCOR``, as ``MAGZP + APCOR4`` is the aperture's.
"""
import math

import numpy as np

from . import _lib
from . import fits as _fits
from ._lib import as_f32, as_i32, check, ptr
from .constants import BAD_SUM

__all__ = ['psf_settings', 'PSFModel', 'build_psf', 'build_psf_planes', 'psf_build', 'psf_build_dev', 'psf_photometry',
           'psf_photometry_dev', 'psf_photometry_batch', 'PSF_FLAGS']

PSF_FLAGS = dict(BAD=_lib.PSF_BAD, NONFINITE=_lib.PSF_NONFINITE, BADRMS=_lib.PSF_BADRMS, CLIPPED=_lib.PSF_CLIPPED,
                 LOWCOVER=_lib.PSF_LOWCOVER, SINGULAR=_lib.PSF_SINGULAR, BADPOS=_lib.PSF_BADPOS)
DEFAULTS = dict(psf_half=12, norm_radius=10.0, fit_radius=6.0, fit_sky=0, sn_min=50.0, nmax=1000, min_stars=10,
                min_stars_pixel=3, clip_sigma=3.0, clip_iter=5, annulus=(24.0, 36.0), crossid_radius=2.0, psfref=None)
_KEYS = {'PSF_HALF': 'psf_half', 'NORM_RADIUS': 'norm_radius', 'FIT_RADIUS': 'fit_radius', 'FIT_SKY': 'fit_sky',
         'SN_MIN': 'sn_min', 'NMAX': 'nmax', 'MIN_STARS': 'min_stars', 'MIN_STARS_PIXEL': 'min_stars_pixel',
         'CLIP_SIGMA': 'clip_sigma', 'CLIP_ITER': 'clip_iter', 'ANNULUS': 'annulus', 'CROSSID_RADIUS': 'crossid_radius',
         'PSFREF_NAME': 'psfref'}
CARD_COMMENTS = {'PSFCOR': 'PSF-fit correction to the reference aperture (mag)', 'PSFCORUN': 'Uncertainty of PSFCOR (mag)',
                 'PSFNSTAR': 'Stars used in PSFCOR', 'PSFHALF': 'Half width of the PSF model (px)',
                 'PSFFITR': 'Radius of a PSF fit (px)', 'PSFFWHM': 'FWHM of the PSF model (px)',
                 'ZMPSF': 'PSF model measured from the pixels'}


def _engine(engine):
    from .engine import get_engine
    return engine or get_engine()


# ---- settings ---------------------------------------------------------------------------------------------------------
def psf_settings(psf_kws=None, **overrides):
    """``psf_kws`` (``-KEY value`` pairs in the manner of ``photcal_kws``) -> a dict of settings with every default
    filled in.  An unknown key raises ``ValueError``.  ``overrides``: settings by their lower-case names."""
    st = dict(DEFAULTS)
    for k, v in (psf_kws or {}).items():
        key = str(k).upper().lstrip('-')
        if key not in _KEYS:
            raise ValueError(f'psf_kws: -{key} {v} is not a key of the PSF photometry (known: {", ".join(_KEYS)})')
        st[_KEYS[key]] = v
    for k, v in overrides.items():
        if k not in DEFAULTS:
            raise ValueError(f'psf: unknown setting {k!r} (known: {", ".join(DEFAULTS)})')
        st[k] = v
    ann = st['annulus']
    if not isinstance(ann, (list, tuple, np.ndarray)):
        ann = str(ann).replace('(', '').replace(')', '').split(',')
    try:
        st['annulus'] = tuple(float(t) for t in ann)
    except (TypeError, ValueError):
        raise ValueError(f'psf_kws: ANNULUS takes numbers (got {ann!r})')
    if len(st['annulus']) != 2 or not 0 <= st['annulus'][0] < st['annulus'][1]:
        raise ValueError(f'psf_kws: ANNULUS takes two ascending diameters (got {st["annulus"]})')
    for k in ('norm_radius', 'fit_radius', 'sn_min', 'clip_sigma', 'crossid_radius'):
        st[k] = float(st[k])
        if not st[k] > 0:
            raise ValueError(f'psf_kws: {k.upper()} must be positive (got {st[k]!r})')
    for k in ('psf_half', 'nmax', 'min_stars', 'min_stars_pixel', 'clip_iter'):
        st[k] = int(st[k])
    st['fit_sky'] = int(bool(int(st['fit_sky'])))
    if not 1 <= st['psf_half'] <= _lib.PSF_HALF_MAX:
        raise ValueError(f'psf_kws: PSF_HALF {st["psf_half"]} outside 1 .. {_lib.PSF_HALF_MAX}')
    if not st['fit_radius'] + 3.5 <= st['psf_half']:
        raise ValueError(f'psf_kws: FIT_RADIUS {st["fit_radius"]:g} + 3.5 exceeds PSF_HALF {st["psf_half"]}')
    if st['clip_iter'] < 0 or st['min_stars_pixel'] < 0:
        raise ValueError('psf_kws: CLIP_ITER and MIN_STARS_PIXEL must not be negative')
    if st['min_stars'] < 1 or not 1 <= st['nmax'] <= _lib.CLIPMED_NMAX:
        raise ValueError(f'psf_kws: MIN_STARS must be at least 1 and NMAX 1 .. {_lib.CLIPMED_NMAX}')
    st['psfref'] = None if st['psfref'] is None else str(st['psfref'])
    return st


# ---- the model --------------------------------------------------------------------------------------------------------
class PSFModel:
    """The model of one image: ``data`` ((2 half + 1)^2 float64, unit sum, constant across the frame), ``half``,
    ``n_used`` (stars per entry; None for a model read from a file) and ``cards`` {key: value}."""

    def __init__(self, data, n_used=None, cards=None):
        data = np.ascontiguousarray(data, dtype=np.float64)
        if data.ndim != 2 or data.shape[0] != data.shape[1] or not data.shape[0] & 1:
            raise ValueError(f'PSFModel: the model must be square with an odd side (got {data.shape})')
        self.data = data
        self.half = (data.shape[0] - 1) // 2
        if not 1 <= self.half <= _lib.PSF_HALF_MAX:
            raise ValueError(f'PSFModel: half {self.half} outside 1 .. {_lib.PSF_HALF_MAX}')
        self.n_used = None if n_used is None else np.ascontiguousarray(n_used, dtype=np.int32)
        self.cards = dict(cards or {})

    @property
    def fit_radius(self):
        return float(self.cards.get('PSFFITR', DEFAULTS['fit_radius']))

    def save(self, path):
        """``*.psf.fits``: BITPIX -64, the cards in the header.  It reads back to the same bits."""
        _fits.write(str(path), self.data, self.cards, {k: CARD_COMMENTS.get(k, '') for k in self.cards})
        return str(path)

    @classmethod
    def from_file(cls, path):
        data, header, _ = _fits.read(str(path))
        if data is None or data.dtype != np.float64:
            raise ValueError(f'{path}: not a PSF model (BITPIX -64 expected)')
        return cls(data, cards={k: header[k] for k in CARD_COMMENTS if k in header})


def psf_build(data, x, y, sky, norm, half=12, norm_radius=10.0, mask=None, bad_bits=BAD_SUM, clip_sigma=3.0, clip_iter=5,
              min_stars_pixel=3, want_cutouts=False, engine=None):
    """``zm_psf_build`` on numpy planes: (model [w, w], n_used [w, w] int32[, cutouts [n, w, w]]), w = 2 half + 1.  With
    no star nothing is computed: the model comes back NaN and n_used 0."""
    eng = _engine(engine)
    img, mask = as_f32(data), as_i32(mask)
    if img.ndim != 2 or (mask is not None and mask.shape != img.shape):
        raise ValueError('psf_build: data must be a 2-D image and mask of its shape')
    ny, nx = img.shape
    x, y, sky, norm = (np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64) for v in (x, y, sky, norm))
    n = x.size
    if not (y.size == n and sky.size == n and norm.size == n):
        raise ValueError('psf_build: x, y, sky and norm must be of one length')
    w = 2 * int(half) + 1
    model, n_used = np.full((w, w), np.nan), np.zeros((w, w), np.int32)
    cut = np.full((n, w, w), np.nan) if want_cutouts else None
    check(eng.L.zm_psf_build(eng.ctx, ptr(img), ptr(mask), int(bad_bits), nx, ny, n, ptr(x), ptr(y), ptr(sky), ptr(norm),
                             int(half), float(norm_radius), float(clip_sigma), int(clip_iter), int(min_stars_pixel),
                             ptr(model), ptr(n_used), ptr(cut) if n else None, w * w), 'zm_psf_build')
    return (model, n_used, cut) if want_cutouts else (model, n_used)


def psf_build_dev(img, x, y, sky, norm, half=12, norm_radius=10.0, mask=None, bad_bits=BAD_SUM, clip_sigma=3.0,
                  clip_iter=5, min_stars_pixel=3, want_cutouts=False, engine=None):
    """``psf_build`` on planes and star arrays that lie in HBM (``zm_psf_build_dev``): ``img`` float32, ``mask`` int32,
    the star arrays float64 torch tensors.  Only enqueues; the results are device tensors."""
    import torch
    eng = _engine(engine)
    if img.dtype != torch.float32 or img.dim() != 2 or not img.is_contiguous():
        raise ValueError('psf_build_dev: img must be a contiguous 2-D float32 tensor')
    if mask is not None and (mask.dtype != torch.int32 or mask.shape != img.shape or not mask.is_contiguous()):
        raise ValueError('psf_build_dev: mask must be a contiguous int32 tensor of the image\'s shape')
    n = x.numel()
    for a in (x, y, sky, norm):
        if a.dtype != torch.float64 or a.dim() != 1 or not a.is_contiguous() or a.numel() != n or a.device != img.device:
            raise ValueError('psf_build_dev: x, y, sky, norm must be contiguous float64 vectors of one length on the image\'s device')
    ny, nx = img.shape
    w = 2 * int(half) + 1
    model = torch.full((w, w), float('nan'), dtype=torch.float64, device=img.device)
    n_used = torch.zeros((w, w), dtype=torch.int32, device=img.device)
    cut = torch.full((n, w, w), float('nan'), dtype=torch.float64, device=img.device) if want_cutouts else None
    dp = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    check(eng.L.zm_psf_build_dev(eng.ctx, img.data_ptr(), dp(mask), int(bad_bits), nx, ny, n, dp(x), dp(y), dp(sky), dp(norm),
                                 int(half), float(norm_radius), float(clip_sigma), int(clip_iter), int(min_stars_pixel),
                                 model.data_ptr(), n_used.data_ptr(), dp(cut), w * w), 'zm_psf_build_dev')
    return (model, n_used, cut) if want_cutouts else (model, n_used)


# ---- the fit ----------------------------------------------------------------------------------------------------------
def _model_of(psf):
    data = psf.data if isinstance(psf, PSFModel) else np.ascontiguousarray(psf, dtype=np.float64)
    if data.ndim != 2 or data.shape[0] != data.shape[1] or not data.shape[0] & 1:
        raise ValueError(f'psf: the model must be square with an odd side (got {data.shape})')
    return data, (data.shape[0] - 1) // 2


def _planes(image_or_planes):
    if isinstance(image_or_planes, (tuple, list)):
        img, rms, mask = (tuple(image_or_planes) + (None, None))[:3]
        return img, rms, mask
    if isinstance(image_or_planes, np.ndarray):
        return image_or_planes, None, None
    im = image_or_planes
    m = getattr(im, 'mask_image', None)
    has_rms = hasattr(im, '_rmsimg') or hasattr(im, '_weightimg')
    return im.data, im.rms_image.data if has_rms else None, None if m is None else m.data


def psf_photometry(image_or_planes, x, y, psf, fit_radius=None, fit_sky=0, bad_bits=BAD_SUM, engine=None):
    """Fits of the model ``psf`` (a ``PSFModel`` or its array) at 0-based pixel positions (``zm_psf_photometry``).
    ``image_or_planes``: an image object (its ``rms_image`` and ``mask_image``) or ``(img, rms, mask)`` numpy planes, rms
    and mask optional.  ``fit_radius``: pixels, the model's ``PSFFITR`` card or 6 by default; ``fit_radius + 3.5`` must not
    exceed the model's half width.  Returns a dict of arrays: ``flux``, ``fluxerr``, ``chi2``, ``sky``, ``cover``,
    ``npix`` and ``flags`` (``PSF_FLAGS``)."""
    eng = _engine(engine)
    img, rms, mask = _planes(image_or_planes)
    img, rms, mask = as_f32(img), as_f32(rms), as_i32(mask)
    if img.ndim != 2:
        raise ValueError('psf_photometry: the image must be 2-D')
    for a, nm in ((rms, 'rms'), (mask, 'mask')):
        if a is not None and a.shape != img.shape:
            raise ValueError(f'psf_photometry: {nm} has shape {a.shape}, the image {img.shape}')
    model, half = _model_of(psf)
    if fit_radius is None:
        fit_radius = psf.fit_radius if isinstance(psf, PSFModel) else DEFAULTS['fit_radius']
    ny, nx = img.shape
    x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
    y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError('psf_photometry: x and y must be 1-D and of one length')
    n = x.size
    out = dict(flux=np.zeros(n), fluxerr=np.zeros(n), chi2=np.zeros(n), sky=np.zeros(n), cover=np.zeros(n),
               npix=np.zeros(n, np.int32), flags=np.zeros(n, np.int32))
    check(eng.L.zm_psf_photometry(eng.ctx, ptr(img), ptr(rms), ptr(mask), int(bad_bits), nx, ny, n, ptr(x), ptr(y),
                                  ptr(model), half, float(fit_radius), int(bool(fit_sky)), ptr(out['flux']),
                                  ptr(out['fluxerr']), ptr(out['chi2']), ptr(out['sky']), ptr(out['cover']),
                                  ptr(out['npix']), ptr(out['flags'])), 'zm_psf_photometry')
    return out


def psf_photometry_dev(img, x, y, model, fit_radius=6.0, fit_sky=0, rms=None, mask=None, bad_bits=BAD_SUM, engine=None):
    """``psf_photometry`` on planes that lie in HBM (``zm_psf_photometry_dev``): ``img`` / ``rms`` float32, ``mask`` int32,
    ``x`` / ``y`` float64 vectors and ``model`` a (2 half + 1)^2 float64 tensor on the same device.  Only enqueues; the
    results are device tensors.  The caller has the engine's stream current."""
    import torch
    eng = _engine(engine)
    if img.dtype != torch.float32 or img.dim() != 2 or not img.is_contiguous():
        raise ValueError('psf_photometry_dev: img must be a contiguous 2-D float32 tensor')
    for a, nm, dt in ((rms, 'rms', torch.float32), (mask, 'mask', torch.int32)):
        if a is not None and (a.dtype != dt or a.shape != img.shape or not a.is_contiguous() or a.device != img.device):
            raise ValueError(f'psf_photometry_dev: {nm} must be a contiguous {dt} tensor of the image\'s shape and device')
    for a, nm in ((x, 'x'), (y, 'y')):
        if a.dtype != torch.float64 or a.dim() != 1 or not a.is_contiguous() or a.device != img.device:
            raise ValueError(f'psf_photometry_dev: {nm} must be a contiguous 1-D float64 tensor on the image\'s device')
    if x.numel() != y.numel():
        raise ValueError('psf_photometry_dev: x and y differ in length')
    if model.dtype != torch.float64 or model.dim() != 2 or model.shape[0] != model.shape[1] or not model.shape[0] & 1 \
            or not model.is_contiguous() or model.device != img.device:
        raise ValueError('psf_photometry_dev: model must be a contiguous square float64 tensor with an odd side')
    half = (model.shape[0] - 1) // 2
    ny, nx = img.shape
    n = x.numel()
    new = lambda dt: torch.empty(n, dtype=dt, device=img.device)
    out = dict(flux=new(torch.float64), fluxerr=new(torch.float64), chi2=new(torch.float64), sky=new(torch.float64),
               cover=new(torch.float64), npix=new(torch.int32), flags=new(torch.int32))
    dp = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    check(eng.L.zm_psf_photometry_dev(eng.ctx, img.data_ptr(), dp(rms), dp(mask), int(bad_bits), nx, ny, n, dp(x), dp(y),
                                      model.data_ptr(), half, float(fit_radius), int(bool(fit_sky)), dp(out['flux']),
                                      dp(out['fluxerr']), dp(out['chi2']), dp(out['sky']), dp(out['cover']),
                                      dp(out['npix']), dp(out['flags'])) if n else 0, 'zm_psf_photometry_dev')
    return out


def psf_photometry_batch(images, ra, dec, done=None, engine=None, fit_radius=None, fit_sky=0, bad_bits=BAD_SUM):
    """PSF fits of every (image, source) pair whose source lies inside the image's footprint: one join and one launch
    (``zm_footprint_join_dev``, ``zm_psf_photometry_batch_dev``).  ``images``: as ``forced_photometry_batch`` takes them,
    each with its model under ``psf`` (a ``PSFModel`` or an array; an image object: its ``psf_model``).  Returns the table
    of ``forced_photometry_batch`` plus ``chi2``, ``npix``, ``cover`` and ``sky``."""
    from .lightcurve import forced_photometry_batch
    return forced_photometry_batch(images, ra, dec, done=done, engine=engine, method='psf', fit_radius=fit_radius,
                                   fit_sky=fit_sky, bad_bits=bad_bits)


# ---- the operator -----------------------------------------------------------------------------------------------------
def build_psf_planes(data, wcs=None, mask=None, rms=None, saturate=None, stars=None, engine=None, bad_bits=BAD_SUM,
                     **settings):
    """``build_psf`` on numpy planes.  ``wcs`` is needed with a catalogue.  Returns the dict ``build_psf`` documents."""
    from . import photcal
    st = psf_settings(None, **settings)
    eng = _engine(engine)
    data, mask, rms = as_f32(data), as_i32(mask), as_f32(rms)
    # photcal's route to the stars: the image's own or a catalogue's, centroids, local sky and the flux in the reference
    # aperture (zm_growth), flags 0 and S/N >= SN_MIN there
    try:
        pc = photcal.measure_planes(data, wcs=wcs, mask=mask, rms=rms, saturate=saturate, stars=stars, engine=eng,
                                    bad_bits=bad_bits, ref_diameter=2.0 * st['norm_radius'], annulus=st['annulus'],
                                    apertures=(2.0 * photcal.APERTURE_RADIUS,), sn_min=st['sn_min'],
                                    crossid_radius=st['crossid_radius'], clip_sigma=st['clip_sigma'],
                                    clip_iter=st['clip_iter'], nmax=st['nmax'], min_stars=1)
        used = pc['used']
    except _lib.ZMError:                               # a failed library call is not "too few stars"
        raise
    except RuntimeError:                               # photcal's own: not one usable star
        pc, used = None, np.zeros(0, bool)
    nused = int(used.sum())
    if nused < st['min_stars']:
        raise RuntimeError(f'Unable to build the PSF model: {nused} usable star(s), MIN_STARS is {st["min_stars"]}')
    g = pc['growth']
    x, y = pc['x'][used], pc['y'][used]
    sky, norm = g['sky'][used], g['flux'][used, -1]
    half = st['psf_half']
    model, n_used = psf_build(data, x, y, sky, norm, half=half, norm_radius=st['norm_radius'], mask=mask, bad_bits=bad_bits,
                              clip_sigma=st['clip_sigma'], clip_iter=st['clip_iter'],
                              min_stars_pixel=st['min_stars_pixel'], engine=eng)
    if not np.all(np.isfinite(model)):
        raise RuntimeError('Unable to build the PSF model: its sum is not positive')
    # the cards: the model's own stars fitted with the finished model, under the sky setting it will be used with
    fit = psf_photometry((data, rms, mask), x, y, model, fit_radius=st['fit_radius'], fit_sky=st['fit_sky'],
                         bad_bits=bad_bits, engine=eng)
    fpsf = fit['flux']
    if not st['fit_sky']:
        # without a sky term the local sky of each star is taken out: the fit is linear, so fit(d - sky) = fit(d) - sky fit(1)
        # (only stars whose fit left no pixel out enter PSFCOR, so the two fits run over the same pixels)
        one = psf_photometry((np.ones_like(data), rms, mask), x, y, model, fit_radius=st['fit_radius'], fit_sky=0,
                             bad_bits=bad_bits, engine=eng)
        fpsf = fpsf - sky * one['flux']
    with np.errstate(invalid='ignore', divide='ignore'):
        ok = (fit['flags'] == 0) & (fpsf > 0)
        dm = -2.5 * np.log10(norm / fpsf)
    cm = photcal.clipped_median(np.where(ok, dm, np.nan), st['clip_sigma'], st['clip_iter'], engine=eng)
    fw, cx, cy = np.empty(1), np.empty(1), np.empty(1)
    plane = np.ascontiguousarray(model, dtype=np.float32)
    c = np.array([half], np.int32)
    check(eng.L.zm_star_fwhm(eng.ctx, ptr(plane), plane.shape[1], plane.shape[0], 1, ptr(c), ptr(c), min(photcal.HALF, half),
                             ptr(fw), ptr(cx), ptr(cy)), 'zm_star_fwhm')
    nstar = int(cm[2])
    cards = {'PSFCOR': float(cm[0]), 'PSFCORUN': float(1.2533 * cm[1] / math.sqrt(nstar)) if nstar else float('nan'),
             'PSFNSTAR': nstar, 'PSFHALF': half, 'PSFFITR': st['fit_radius'], 'PSFFWHM': float(fw[0]), 'ZMPSF': True}
    psf = PSFModel(model, n_used, cards)
    return dict(psf=psf, cards=[(k, v, CARD_COMMENTS[k]) for k, v in cards.items()], x=x, y=y, sky=sky, norm=norm,
                index=pc['index'][used], fit=fit, flux_psf=fpsf, dm=dm, used=ok, cor_stats=cm, settings=st, photcal=pc)


def build_psf(image, stars=None, engine=None, **settings):
    """Build the PSF model of ``image`` (an image object with a mask; nothing is written).

    ``stars``: None - the image's own isolated, unsaturated stars, or the catalogue ``psfref`` (``PSFREF_NAME``) names - or a
    catalogue, ``(ra, dec, mag)`` or the path of a FITS_LDAC file (``photcal.read_photrefcat``).  Stars are chosen by photcal's route: ``zm_growth`` flags 0 and S/N in
    the reference aperture (radius ``NORM_RADIUS``) >= ``SN_MIN``.  ``settings``: the lower-case names of ``psf_kws``.

    Returns a dict: ``psf`` (the ``PSFModel``, its ``cards`` filled: ``PSFCOR``, ``PSFCORUN``, ``PSFNSTAR``, ``PSFHALF``,
    ``PSFFITR``, ``PSFFWHM``, ``ZMPSF``), ``cards`` [(key, value, comment)], ``x`` / ``y`` / ``sky`` / ``norm`` of the stars
    that made the model, ``index`` (their catalogue rows or ranks), ``fit`` (their own fits), ``flux_psf``, ``dm``, ``used``
    (which of them entered ``PSFCOR``) and ``cor_stats``.  Raises ``RuntimeError`` with fewer than ``MIN_STARS`` stars."""
    m = getattr(image, 'mask_image', None)
    sat = image.header.get('SATURATE')
    has_rms = hasattr(image, '_rmsimg') or hasattr(image, '_weightimg')
    if stars is None and settings.get('psfref'):
        stars = settings['psfref']                     # PSFREF_NAME
    if isinstance(stars, (str, bytes)) or hasattr(stars, '__fspath__'):
        from .photcal import read_photrefcat
        stars = read_photrefcat(stars)
    return build_psf_planes(image.data, wcs=image.wcs if stars is not None else None, mask=None if m is None else m.data,
                            rms=image.rms_image.data if has_rms else None, saturate=float(sat) if sat else None,
                            stars=stars, engine=engine, **settings)
