"""Fake sources: PSF-model point sources injected into resident planes, recovered through the subtraction and the
candidate cuts, and the detection efficiency they measure ("Fake sources").

``MAGLIM`` (``photcal.limiting_magnitude``) comes from the rms plane alone.  This module asks the pipeline itself: fakes of
known magnitude are added to a copy of the science frame with the image's own PSF model at their sub-pixel phase
(``zm_inject_dev``, ``csrc/inject.hip``), the copy goes through ``DeviceSubtraction.run`` and ``candidates``, and the
fraction that comes back with ``GOODCUT == 1`` per magnitude bin is the efficiency; ``m50`` is where it falls through 0.5.
It is this project's own operator - the reference left fakes to offline work - and opt-in everywhere: with every keyword at
its default no product and no table changes.

The zero point of a fake is ``MAGZP + PSFCOR``, that of a PSF flux (``psf.py``).  No noise realisation is drawn for a fake
(its Poisson variance is added to the rms plane when a gain is given) and fakes are not placed on host galaxies.
"""
import csv
import math

import numpy as np

from . import _lib
from ._lib import as_i32, check, ptr
from .constants import BAD_SUM
from .psf import DEFAULTS as PSF_DEFAULTS
from .psf import PSFModel, _model_of, _planes

__all__ = ['fake_settings', 'draw_fakes', 'inject', 'inject_dev', 'inject_layers', 'match_fakes', 'efficiency',
           'recover_dev', 'write_fakes_csv', 'read_fakes_csv', 'INJ_FLAGS', 'FAKE_DTYPE']

INJ_FLAGS = dict(CLIPPED=_lib.INJ_CLIPPED, OUTSIDE=_lib.INJ_OUTSIDE, BAD=_lib.INJ_BAD, NONFINITE=_lib.INJ_NONFINITE,
                 BADPOS=_lib.INJ_BADPOS)
FAKE_DTYPE = np.dtype([('id', np.int32), ('x', np.float64), ('y', np.float64), ('ra', np.float64), ('dec', np.float64),
                       ('mag', np.float64), ('flux', np.float64)])
BOX_PAD = 3                                             # the box of a fake reaches PSF_HALF + 3 px from its centre pixel
_KEYS = {'N': 'n', 'MAG_MIN': 'mag_min', 'MAG_MAX': 'mag_max', 'SEED': 'seed', 'MIN_SEP': 'min_sep', 'BORDER': 'border',
         'MATCH_RADIUS': 'match_radius', 'GAIN': 'gain', 'CORE_RADIUS': 'core_radius'}
CARD_COMMENTS = {'FAKEN': 'Fake sources injected', 'FAKESEED': 'Seed of the fake sources',
                 'FAKEM50': 'Magnitude of 50 % detection efficiency', 'FAKEM80': 'Magnitude of 80 % detection efficiency'}


def _engine(engine):
    from .engine import get_engine
    return engine or get_engine()


# ---- settings ---------------------------------------------------------------------------------------------------------
def fake_settings(fake_kws=None, header=None, psf=None, **overrides):
    """``fake_kws`` (``-KEY value`` pairs in the manner of ``psf_kws``) -> a dict of settings with every default filled in.
    An unknown key raises ``ValueError``.  ``overrides``: settings by their lower-case names.  ``header`` gives the
    defaults that come from the image - ``MAG_MIN`` / ``MAG_MAX`` = ``MAGLIM - 2.5`` / ``MAGLIM + 1.0`` and ``GAIN`` -
    and ``psf`` (a ``PSFModel``) those that come from the model: ``MIN_SEP`` = ``2 (PSF_HALF + 3) + 1`` px, which keeps
    the boxes of the fakes apart (one layer), ``BORDER`` = ``PSF_HALF + 3`` px and ``CORE_RADIUS`` = its ``FIT_RADIUS``.
    Without ``MAGLIM`` in the header ``MAG_MIN`` and ``MAG_MAX`` are required."""
    header = header or {}
    half = psf.half if isinstance(psf, PSFModel) else PSF_DEFAULTS['psf_half']
    st = dict(n=200, mag_min=None, mag_max=None, seed=0, min_sep=2.0 * (half + BOX_PAD) + 1.0, border=float(half + BOX_PAD),
              match_radius=2.0, gain=header.get('GAIN', 0.0) or 0.0,
              core_radius=psf.fit_radius if isinstance(psf, PSFModel) else PSF_DEFAULTS['fit_radius'])
    for k, v in (fake_kws or {}).items():
        key = str(k).upper().lstrip('-')
        if key not in _KEYS:
            raise ValueError(f'fake_kws: -{key} {v} is not a key of the fake sources (known: {", ".join(_KEYS)})')
        st[_KEYS[key]] = v
    for k, v in overrides.items():
        if k not in st:
            raise ValueError(f'fakes: unknown setting {k!r} (known: {", ".join(st)})')
        st[k] = v
    if 'MAGLIM' in header:
        if st['mag_min'] is None:
            st['mag_min'] = float(header['MAGLIM']) - 2.5
        if st['mag_max'] is None:
            st['mag_max'] = float(header['MAGLIM']) + 1.0
    if st['mag_min'] is None or st['mag_max'] is None:
        raise ValueError('fake_kws: MAG_MIN and MAG_MAX are required when the header has no MAGLIM')
    st['n'], st['seed'] = int(st['n']), int(st['seed'])
    for k in ('mag_min', 'mag_max', 'min_sep', 'border', 'match_radius', 'gain', 'core_radius'):
        st[k] = float(st[k])
        if not math.isfinite(st[k]):
            raise ValueError(f'fake_kws: {k.upper()} must be finite (got {st[k]!r})')
    if st['n'] < 0 or st['seed'] < 0:
        raise ValueError('fake_kws: N and SEED must not be negative')
    if not st['mag_min'] <= st['mag_max']:
        raise ValueError(f'fake_kws: MAG_MIN {st["mag_min"]:g} exceeds MAG_MAX {st["mag_max"]:g}')
    for k in ('min_sep', 'border', 'gain', 'core_radius'):
        if st[k] < 0:
            raise ValueError(f'fake_kws: {k.upper()} must not be negative (got {st[k]!r})')
    if not st['match_radius'] > 0:
        raise ValueError(f'fake_kws: MATCH_RADIUS must be positive (got {st["match_radius"]!r})')
    return st


# ---- the draw ---------------------------------------------------------------------------------------------------------
def draw_fakes(shape, wcs, zp, settings, avoid_xy=None, clean=None, max_tries=None):
    """``N`` fakes on a frame of ``shape`` (ny, nx): magnitudes uniform in ``MAG_MIN .. MAG_MAX``, 0-based positions by
    rejection with ``numpy.random.default_rng(SEED)`` - ``BORDER`` px from the edge, ``MIN_SEP`` px from each other and
    from every position of ``avoid_xy`` (x, y) along x or along y (the distance of boxes: two positions are too close when
    they are nearer than ``MIN_SEP`` on both axes), and only on pixels where the bool plane ``clean`` holds, when given.
    ``zp`` = ``MAGZP + PSFCOR``: ``flux = 10 ** (-0.4 (mag - zp))``.  ``wcs`` gives ``ra`` / ``dec`` (NaN without one).
    Returns a structured array (``FAKE_DTYPE``: id, x, y, ra, dec, mag, flux); the same seed gives the same bytes.
    Raises ``RuntimeError`` when the frame has no room for ``N``."""
    st = settings
    ny, nx = (int(v) for v in shape)
    n, border, sep = st['n'], st['border'], st['min_sep']
    rng = np.random.default_rng(st['seed'])
    out = np.zeros(n, FAKE_DTYPE)
    out['id'] = np.arange(n)
    out['mag'] = rng.uniform(st['mag_min'], st['mag_max'], n)
    lo_x, hi_x, lo_y, hi_y = border, nx - 1.0 - border, border, ny - 1.0 - border
    if n and not (lo_x < hi_x and lo_y < hi_y):
        raise RuntimeError(f'draw_fakes: a frame of {nx} x {ny} has no room inside a border of {border:g} px')
    # a grid of cells of MIN_SEP: a position is compared with what lies in the 3 x 3 cells around it
    cell = max(sep, 1.0)
    grid = {}

    def near(x, y):
        cx, cy = int(x // cell), int(y // cell)
        for a in (cy - 1, cy, cy + 1):
            for b in (cx - 1, cx, cx + 1):
                for (px, py) in grid.get((b, a), ()):
                    if abs(px - x) < sep and abs(py - y) < sep:
                        return True
        return False

    def put(x, y):
        grid.setdefault((int(x // cell), int(y // cell)), []).append((x, y))

    if avoid_xy is not None:
        for x, y in zip(np.atleast_1d(np.asarray(avoid_xy[0], np.float64)), np.atleast_1d(np.asarray(avoid_xy[1], np.float64))):
            if np.isfinite(x) and np.isfinite(y):
                put(float(x), float(y))
    if clean is not None:
        clean = np.asarray(clean, dtype=bool)
        if clean.shape != (ny, nx):
            raise ValueError(f'draw_fakes: clean has shape {clean.shape}, the frame {(ny, nx)}')
    k, tries = 0, 0
    max_tries = int(max_tries) if max_tries is not None else 200 * n + 1000
    while k < n:
        if tries >= max_tries:
            raise RuntimeError(f'draw_fakes: the frame has no room for {n} fakes {sep:g} px apart ({k} placed in {tries} tries)')
        tries += 1
        x, y = float(rng.uniform(lo_x, hi_x)), float(rng.uniform(lo_y, hi_y))
        if clean is not None and not clean[int(math.floor(y + 0.5)), int(math.floor(x + 0.5))]:
            continue
        if near(x, y):
            continue
        put(x, y)
        out['x'][k], out['y'][k] = x, y
        k += 1
    out['flux'] = 10.0 ** (-0.4 * (out['mag'] - float(zp)))
    if wcs is not None and n:
        out['ra'], out['dec'] = wcs.all_pix2world(out['x'], out['y'], 0)
    else:
        out['ra'] = out['dec'] = np.nan
    return out


# ---- injection --------------------------------------------------------------------------------------------------------
def inject_layers(x, y, half):
    """The layer of every fake (``zm_inject_layers``; host only): 1 + the largest layer among the earlier fakes whose box
    shares a pixel with its own, 0 for a position that is not finite.  Returns (layer int32 [n], number of layers)."""
    import ctypes as C
    x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
    y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError('inject_layers: x and y must be 1-D and of one length')
    layer = np.zeros(x.size, np.int32)
    nl = C.c_int(0)
    check(_lib.lib().zm_inject_layers(x.size, ptr(x), ptr(y), int(half), ptr(layer), C.byref(nl)), 'zm_inject_layers')
    return layer, int(nl.value)


def _fake_columns(fakes, flux=None):
    if isinstance(fakes, np.ndarray) and fakes.dtype.names:
        x, y, flux = fakes['x'], fakes['y'], fakes['flux']
    else:
        x, y, flux = fakes
    x, y, flux = (np.ascontiguousarray(np.atleast_1d(v), dtype=np.float64) for v in (x, y, flux))
    if not (x.ndim == 1 and x.shape == y.shape == flux.shape):
        raise ValueError('fakes: x, y and flux must be 1-D and of one length')
    return x, y, flux


def inject(image_or_planes, fakes, psf, gain=None, core_radius=None, bad_bits=BAD_SUM, engine=None):
    """``zm_inject`` on numpy planes.  ``image_or_planes``: an image object (its ``rms_image`` and ``mask_image``) or
    ``(img, rms, mask)``, rms and mask optional; ``fakes``: the table of ``draw_fakes`` or ``(x, y, flux)``; ``psf``: a
    ``PSFModel`` or its array.  ``gain``: electrons per data unit for the rms rule (None: the image's ``GAIN`` card, else 0:
    the rms plane is left alone).  The input is not modified.  Returns a dict: ``img``, ``rms`` (new planes; rms None when
    none was given), ``flux_in`` (the flux really deposited, ``out_sum``) and ``inj_flags`` (``INJ_FLAGS``)."""
    eng = _engine(engine)
    img, rms, mask = _planes(image_or_planes)
    if gain is None:
        hdr = getattr(image_or_planes, 'header', None) or {}
        gain = float(hdr.get('GAIN', 0.0) or 0.0)
    img = np.array(img, dtype=np.float32, order='C')              # copies: the planes are written in place
    rms = None if rms is None else np.array(rms, dtype=np.float32, order='C')
    mask = as_i32(mask)
    if img.ndim != 2:
        raise ValueError('inject: the image must be 2-D')
    for a, nm in ((rms, 'rms'), (mask, 'mask')):
        if a is not None and a.shape != img.shape:
            raise ValueError(f'inject: {nm} has shape {a.shape}, the image {img.shape}')
    model, half = _model_of(psf)
    if core_radius is None:
        core_radius = psf.fit_radius if isinstance(psf, PSFModel) else PSF_DEFAULTS['fit_radius']
    x, y, flux = _fake_columns(fakes)
    n = x.size
    ny, nx = img.shape
    out_sum, out_flags = np.zeros(n), np.zeros(n, np.int32)
    check(eng.L.zm_inject(eng.ctx, ptr(img), ptr(rms), ptr(mask), int(bad_bits), nx, ny, n, ptr(x), ptr(y), ptr(flux),
                          ptr(model), half, float(gain), float(core_radius), ptr(out_sum), ptr(out_flags)), 'zm_inject')
    return dict(img=img, rms=rms, flux_in=out_sum, inj_flags=out_flags)


def inject_dev(img, x, y, flux, model, rms=None, mask=None, gain=0.0, core_radius=6.0, bad_bits=BAD_SUM, engine=None):
    """``zm_inject_dev``: the fakes added IN PLACE to ``img`` (float32) and, with ``gain`` > 0, their variance to ``rms``
    (float32) - torch tensors in HBM; ``mask`` int32 or None; ``model`` a (2 half + 1)^2 float64 tensor on the same device.
    ``x``, ``y``, ``flux``: host arrays (the fake list is host memory, as the stamp origins of ``zm_stamps_dev`` are).
    Only enqueues, on the engine's stream, which the caller has current.  Returns ``(flux_in, inj_flags)`` as device
    tensors (float64, int32)."""
    import torch
    eng = _engine(engine)
    if img.dtype != torch.float32 or img.dim() != 2 or not img.is_contiguous():
        raise ValueError('inject_dev: img must be a contiguous 2-D float32 tensor')
    for a, nm, dt in ((rms, 'rms', torch.float32), (mask, 'mask', torch.int32)):
        if a is not None and (a.dtype != dt or a.shape != img.shape or not a.is_contiguous() or a.device != img.device):
            raise ValueError(f'inject_dev: {nm} must be a contiguous {dt} tensor of the image\'s shape and device')
    if model.dtype != torch.float64 or model.dim() != 2 or model.shape[0] != model.shape[1] or not model.shape[0] & 1 \
            or not model.is_contiguous() or model.device != img.device:
        raise ValueError('inject_dev: model must be a contiguous square float64 tensor with an odd side')
    half = (model.shape[0] - 1) // 2
    x, y, flux = _fake_columns((x, y, flux))
    n = x.size
    ny, nx = img.shape
    out_sum = torch.zeros(n, dtype=torch.float64, device=img.device)
    out_flags = torch.zeros(n, dtype=torch.int32, device=img.device)
    if n:
        check(eng.L.zm_inject_dev(eng.ctx, img.data_ptr(), None if rms is None else rms.data_ptr(),
                                  None if mask is None else mask.data_ptr(), int(bad_bits), nx, ny, n, ptr(x), ptr(y),
                                  ptr(flux), model.data_ptr(), half, float(gain), float(core_radius), out_sum.data_ptr(),
                                  out_flags.data_ptr()), 'zm_inject_dev')
    return out_sum, out_flags


# ---- recovery ---------------------------------------------------------------------------------------------------------
MATCH_COLUMNS = [('detected', np.bool_), ('recovered', np.bool_), ('det_number', np.int32), ('sep_px', np.float64),
                 ('flux_aper', np.float64), ('fluxerr_aper', np.float64)]


def _append_columns(table, columns):
    """A structured array with ``columns`` [(name, dtype, values)] added behind those of ``table``."""
    out = np.zeros(len(table), np.dtype(table.dtype.descr + [(n, np.dtype(dt).str) for n, dt, _ in columns]))
    for name in table.dtype.names:
        out[name] = table[name]
    for name, _, values in columns:
        out[name] = values
    return out


def match_fakes(fakes, cat, wcs, radius_px, engine=None):
    """The fakes against a candidate table (``DeviceSubtraction.candidates``): ``source.crossmatch`` (``zm_crossmatch``) of
    their ``ra`` / ``dec`` against the table's ``X_WORLD`` / ``Y_WORLD``, once against all rows (``detected``) and once
    against the ``GOODCUT == 1`` rows (``recovered``).  ``radius_px`` is taken to the sky with the pixel scale of ``wcs``
    (the root of the area of a pixel at the reference point) and ``sep_px`` comes back through it.  Returns the table with
    ``detected``, ``recovered``, ``det_number`` (``NUMBER`` of the recovered row, else of the detected one, else -1),
    ``sep_px``, ``flux_aper`` and ``fluxerr_aper`` of that row (NaN without a match)."""
    from .source import crossmatch
    eng = _engine(engine)
    n = len(fakes)
    scale = 3600.0 * math.sqrt(abs(float(np.linalg.det(np.asarray(wcs.cd, dtype=np.float64).reshape(2, 2)))))
    cols = dict(detected=np.zeros(n, bool), recovered=np.zeros(n, bool), det_number=np.full(n, -1, np.int32),
                sep_px=np.full(n, np.nan), flux_aper=np.full(n, np.nan), fluxerr_aper=np.full(n, np.nan))
    if n and cat is not None and len(cat):
        ra, dec = np.asarray(fakes['ra'], np.float64), np.asarray(fakes['dec'], np.float64)
        for key, rows in (('detected', np.arange(len(cat))), ('recovered', np.flatnonzero(cat['GOODCUT'] == 1))):
            if not rows.size:
                continue
            idx, sep = crossmatch(ra, dec, np.asarray(cat['X_WORLD'][rows], np.float64),
                                  np.asarray(cat['Y_WORLD'][rows], np.float64), float(radius_px) * scale, engine=eng)
            hit = idx >= 0
            cols[key] = hit
            row = cat[rows[idx[hit]]]
            cols['det_number'][hit] = row['NUMBER']
            cols['sep_px'][hit] = sep[hit] / scale
            cols['flux_aper'][hit] = row['FLUX_APER']
            cols['fluxerr_aper'][hit] = row['FLUXERR_APER']
    return _append_columns(fakes, [(nm, dt, cols[nm]) for nm, dt in MATCH_COLUMNS])


def wilson(nrec, n, z=1.0):
    """The Wilson score interval of ``nrec`` out of ``n`` at ``z`` sigma: (lo, hi); NaN where ``n`` is 0."""
    nrec, n = np.asarray(nrec, np.float64), np.asarray(n, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        p = nrec / n
        den = 1.0 + z * z / n
        mid = (p + z * z / (2.0 * n)) / den
        hw = z * np.sqrt(p * (1.0 - p) / n + z * z / (4.0 * n * n)) / den
    return mid - hw, mid + hw


def _crossing(centres, eff, level):
    """The first faintward crossing of ``eff`` through ``level``: between neighbouring non-empty bins with
    ``eff >= level`` then ``eff < level``, linear between their centres.  NaN when there is none."""
    ok = np.isfinite(eff)
    c, e = centres[ok], eff[ok]
    for k in range(len(c) - 1):
        if e[k] >= level > e[k + 1]:
            return float(c[k] + (e[k] - level) / (e[k] - e[k + 1]) * (c[k + 1] - c[k]))
    return float('nan')


def efficiency(table, edges=None, step=0.25):
    """The detection efficiency of a matched table (``match_fakes``) per magnitude bin.  ``edges``: the bin edges, or bins
    of ``step`` mag from ``floor(min mag / step) step`` on.  Fakes with ``inj_flags & (OUTSIDE | BADPOS)`` - nothing of
    them reached the frame - are left out (``nskipped``).  Returns a dict: ``edges``, ``centres``, ``n``, ``nrec``, ``eff``
    (NaN in an empty bin), ``lo`` / ``hi`` (the Wilson interval at z = 1), ``m50`` / ``m80`` (the first faintward crossing
    of the efficiency through 0.5 / 0.8, linear between bin centres; NaN when there is none), ``nused`` and ``nskipped``."""
    mag = np.asarray(table['mag'], np.float64)
    rec = np.asarray(table['recovered'], bool)
    use = np.isfinite(mag)
    if 'inj_flags' in table.dtype.names:
        use &= (np.asarray(table['inj_flags']) & (_lib.INJ_OUTSIDE | _lib.INJ_BADPOS)) == 0
    nskipped = int((~use).sum())
    mag, rec = mag[use], rec[use]
    if edges is None:
        step = float(step)
        if not step > 0:
            raise ValueError(f'efficiency: step must be positive (got {step!r})')
        if mag.size:
            k0, k1 = math.floor(mag.min() / step), math.floor(mag.max() / step) + 1
            edges = step * np.arange(k0, k1 + 1)
        else:
            edges = np.array([0.0, step])
    edges = np.asarray(edges, np.float64)
    if edges.ndim != 1 or edges.size < 2 or not np.all(np.diff(edges) > 0):
        raise ValueError('efficiency: edges must ascend')
    which = np.searchsorted(edges, mag, side='right') - 1          # [edge_k, edge_k+1)
    inside = (which >= 0) & (which < edges.size - 1)
    nb = edges.size - 1
    n = np.bincount(which[inside], minlength=nb).astype(np.int64)
    nrec = np.bincount(which[inside], weights=rec[inside].astype(np.float64), minlength=nb).astype(np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        eff = np.where(n > 0, nrec / np.maximum(n, 1), np.nan)
    lo, hi = wilson(nrec, n)
    lo, hi = np.where(n > 0, lo, np.nan), np.where(n > 0, hi, np.nan)
    centres = 0.5 * (edges[:-1] + edges[1:])
    return dict(edges=edges, centres=centres, n=n, nrec=nrec, eff=eff, lo=lo, hi=hi, m50=_crossing(centres, eff, 0.5),
                m80=_crossing(centres, eff, 0.8), nused=int(use.sum()), nskipped=nskipped)


def recover_dev(chain, sci, sci_rms, sci_mask, sci_wgt, ref, ref_rms, ref_mask, seeing, fakes, psf, run_kws=None,
                candidate_kws=None, gain=0.0, core_radius=None, match_radius=2.0, wcs=None):
    """One recovery pass on the device: ``sci`` and ``sci_rms`` are cloned, the fakes are added to the clones
    (``inject_dev`` with the model ``psf``), the clones go through ``chain.run(...)`` (``run_kws``: its keywords) and
    ``chain.candidates(seeing, ...)`` (``candidate_kws``), and the fakes are matched against the table (``match_fakes``).
    ``wcs``: the science grid's WCS object for the match (``candidate_kws['wcs']`` by default).  With ``rb_model`` among
    ``candidate_kws`` the stamps the network scores are cut from the planes of THIS run: ``sci`` there is always the clone
    that holds the fakes (one the caller names is replaced: it could only be the frame without them, whose 'new' cutout
    would not show the source the 'sub' cutout shows), ``ref`` the reference handed in here unless named.  The caller's
    tensors are not modified.  AFTERWARDS THE CHAIN'S RESIDENT PLANES (``diff``, ``noise``, ``submask``) HOLD THE FAKE RUN, not the
    real one: take what is needed of the real run first.  Returns ``(table, cat, nfound)``: the fakes with ``flux_in``,
    ``inj_flags`` and the columns of ``match_fakes``, and the candidate table of the fake run."""
    import torch
    ckw = dict(candidate_kws or {})
    if wcs is None:
        wcs = ckw.get('wcs')
    if wcs is None:
        raise ValueError('recover_dev: the match needs the science WCS (wcs= or candidate_kws["wcs"])')
    ckw.setdefault('wcs', wcs)
    model, half = _model_of(psf)
    if core_radius is None:
        core_radius = psf.fit_radius if isinstance(psf, PSFModel) else PSF_DEFAULTS['fit_radius']
    eng = chain.engine
    eng.set_stream(chain.stream.cuda_stream)
    chain.stream.wait_stream(torch.cuda.current_stream(chain.device))     # the caller's planes are complete
    with torch.cuda.stream(chain.stream):
        img, rms = sci.clone(), sci_rms.clone()
        dmodel = torch.from_numpy(model).to(chain.device)
        flux_in, flags = inject_dev(img, fakes['x'], fakes['y'], fakes['flux'], dmodel, rms=rms, mask=sci_mask, gain=gain,
                                    core_radius=core_radius, bad_bits=chain.BAD_SUM, engine=eng)
        flux_in, flags = flux_in.cpu(), flags.cpu()
    if ckw.get('rb_model') is not None:
        ckw['sci'] = img
        ckw.setdefault('ref', ref)
    chain.run(img, rms, sci_mask, sci_wgt, ref, ref_rms, ref_mask, seeing=float(seeing), **(run_kws or {}))
    cat, nfound = chain.candidates(float(seeing), **ckw)
    chain.stream.synchronize()
    table = _append_columns(fakes, [('flux_in', np.float64, flux_in.numpy()), ('inj_flags', np.int32, flags.numpy())])
    return match_fakes(table, cat, wcs, match_radius, engine=eng), cat, int(nfound)


# ---- files ------------------------------------------------------------------------------------------------------------
def write_fakes_csv(path, table):
    """The table as CSV: a header row of its column names; floats by ``repr`` (they read back to the same bits), bools as
    0 / 1."""
    names = table.dtype.names
    with open(str(path), 'w', newline='') as fh:
        w = csv.writer(fh)
        w.writerow(names)
        for row in table:
            w.writerow([int(v) if table.dtype[nm].kind in 'biu' else repr(float(v)) for nm, v in zip(names, row)])
    return str(path)


_CSV_TYPES = dict({n: FAKE_DTYPE[n] for n in FAKE_DTYPE.names}, flux_in=np.dtype(np.float64), inj_flags=np.dtype(np.int32),
                  **{n: np.dtype(dt) for n, dt in MATCH_COLUMNS})


def read_fakes_csv(path):
    """What ``write_fakes_csv`` wrote, as the structured array it was (columns it does not know come back float64)."""
    with open(str(path), newline='') as fh:
        rows = list(csv.reader(fh))
    if not rows:
        raise ValueError(f'{path}: not a table of fakes (no header row)')
    names = rows[0]
    dt = np.dtype([(n, _CSV_TYPES.get(n, np.dtype(np.float64))) for n in names])
    out = np.zeros(len(rows) - 1, dt)
    for k, row in enumerate(rows[1:]):
        for n, v in zip(names, row):
            out[n][k] = int(v) if dt[n].kind in 'biu' else float(v)
    return out
