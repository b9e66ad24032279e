"""Light curves (``scripts/dophot.py``, ``Source.light_curve``): which sources lie on which image, and forced photometry of
every such pair in one launch.

The reference asks PostgreSQL, per subtraction, for the sources inside ``wcs.calc_footprint()`` that have no
``ForcedPhotometry`` on that image yet (``q3c_poly_query`` + an outer join), then runs ``raw_aperture_photometry`` at those
positions.  Here the footprint join is ``zm_footprint_join`` and the photometry ``zm_forced_photometry_batch_dev``
(``csrc/lightcurve.hip``), both over many images at once; the "not yet photometered" part is a set difference on the host.
DESIGN.md, "Light curves".
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import check
from .constants import APER_KEY, APERTURE_RADIUS
from .engine import get_engine

__all__ = ['footprint_join', 'forced_photometry_batch', 'pair_keys', 'drop_done', 'light_curves', 'photometry_rows',
           'write_phot_csv', 'read_phot_csv', 'PHOT_CSV_COLUMNS']

# columns and order of the table scripts/dophot.py writes (scripts/dophot.py:145-154)
PHOT_CSV_COLUMNS = ('source_id', 'image_id', 'flux', 'fluxerr', 'flags', 'ra', 'dec', 'zp', 'filtercode', 'obsjd')


def _f64(a, what, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 1 or (n is not None and a.size != n):
        raise ValueError(f'{what} must be a vector' + (f' of {n} values' if n is not None else '') + f', got shape {a.shape}')
    return a


def _wcs_array(wcss):
    structs = [_lib.wcs_struct(w) for w in wcss]
    return (_lib.zm_wcs * max(len(structs), 1))(*structs), len(structs)


def footprint_join(wcss, ra, dec, engine=None):
    """The sources inside the footprint of each image (``zm_footprint_join``).

    ``wcss``: WCS objects (or header dicts) with NAXIS set; ``ra``, ``dec``: degrees.  The footprint is the spherical
    quadrilateral through the centres of the four corner pixels (``WCS.calc_footprint``), edges great circles, boundary
    inclusive; a position that is not finite joins nothing.  Returns ``(offsets int64 [nimg + 1], src_idx int32)``: the
    sources of image ``i`` are ``src_idx[offsets[i]:offsets[i + 1]]``, ascending."""
    ra = _f64(ra, 'ra')
    dec = _f64(dec, 'dec', ra.size)
    arr, nimg = _wcs_array(wcss)
    eng = engine or get_engine()
    offsets = np.zeros(nimg + 1, np.int64)
    cap = max(ra.size, 1024)
    while True:
        src_idx = np.empty(cap, np.int32)
        n = C.c_int64(0)
        check(eng.L.zm_footprint_join(eng.ctx, nimg, arr, ra.size, ra.ctypes.data, dec.ctypes.data, cap, offsets.ctypes.data,
                                      src_idx.ctypes.data, C.byref(n)), 'zm_footprint_join')
        if n.value <= cap:
            return offsets, src_idx[:n.value].copy()
        cap = int(n.value)


def pair_keys(image, source):
    """(image index, source index) pairs packed into one int64 each: image in the upper half."""
    return (np.asarray(image, dtype=np.int64) << 32) | np.asarray(source, dtype=np.int64)


def drop_done(offsets, src_idx, done):
    """The join without the pairs of ``done``: the outer join of ``unphotometered_sources`` (``scripts/dophot.py:58-83``)
    as a set difference on packed 64-bit keys.  ``done``: a set or list of ``(image index, source index)`` pairs, or an
    array of shape [n, 2].  Order within an image is kept."""
    offsets = np.asarray(offsets, dtype=np.int64)
    src_idx = np.asarray(src_idx, dtype=np.int32)
    nimg = offsets.size - 1
    image = np.repeat(np.arange(nimg, dtype=np.int64), np.diff(offsets))
    d = np.asarray(sorted(done) if isinstance(done, (set, frozenset)) else done, dtype=np.int64).reshape(-1, 2)
    keep = ~np.isin(pair_keys(image, src_idx), pair_keys(d[:, 0], d[:, 1]))
    out = np.zeros(nimg + 1, np.int64)
    np.cumsum(np.bincount(image[keep], minlength=nimg), out=out[1:])
    return out, src_idx[keep].copy()


def _resident(im, torch, device):
    """(img, rms, mask, wcs, ny, nx) of one image as device tensors: a dict of resident tensors, or an image object."""
    from .wcs import WCS
    if isinstance(im, dict):
        img, rms, mask, w = im['img'], im.get('rms'), im.get('mask'), im['wcs']
    else:
        img, rms, mask, w = im.data, im.rms_image.data, im.mask_image.data, im.wcs

    def dev(a, dt):
        if a is None:
            return None
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a))
        return a.to(device=device, dtype=dt).contiguous()
    img, rms, mask = dev(img, torch.float32), dev(rms, torch.float32), dev(mask, torch.int32)
    if isinstance(w, dict):
        w = WCS.from_header(w)
    ny, nx = img.shape
    for p, what in ((rms, 'rms'), (mask, 'mask')):
        if p is not None and tuple(p.shape) != (ny, nx):
            raise ValueError(f'the {what} plane is {tuple(p.shape)}, the image {(ny, nx)}')
    return img, rms, mask, w, ny, nx


def _psf_of(im):
    """The ``PSFModel`` of one image of a PSF batch: a dict's ``psf``, an image object's ``psf_model``."""
    from .psf import PSFModel
    psf = im.get('psf') if isinstance(im, dict) else getattr(im, 'psf_model', None)
    if psf is None:
        raise ValueError('forced_photometry_batch: method=\'psf\' needs a model for every image (the dict\'s `psf`, '
                         'the image\'s `psf_model`)')
    if not isinstance(psf, PSFModel):
        psf = PSFModel(psf)
    return psf


def forced_photometry_batch(images, ra, dec, done=None, engine=None, radius=APERTURE_RADIUS, method='aperture',
                            fit_radius=None, fit_sky=0, bad_bits=None):
    """Forced photometry of every (image, source) pair whose source lies inside the image's footprint: one join and one
    launch for the whole batch (``zm_footprint_join_dev``, ``zm_forced_photometry_batch_dev``).

    ``images``: dicts of resident planes - ``img`` (float32), ``rms`` and ``mask`` (or None), torch tensors in HBM or
    arrays, and ``wcs`` - or image objects (``data``, ``rms_image``, ``mask_image``, ``wcs``); sizes may differ.  The
    footprint is that of the plane: NAXIS of the WCS is taken from it.  ``done``: pairs ``(image index, source index)`` to
    leave out (see ``drop_done``).  Returns a dict of arrays with one row per pair, images in order and sources ascending
    within an image: ``image``, ``source``, ``x``, ``y`` (0-based pixels), ``flux``, ``fluxerr``, ``flags``; and
    ``offsets`` (int64 [nimg + 1]).

    ``method='psf'``: a linear fit of each image's PSF model in place of the aperture sum (``zm_psf_photometry_batch_dev``;
    DESIGN.md, "PSF photometry"); any other value than 'aperture' or 'psf' raises ``ValueError``.  An image dict carries
    its model under ``psf`` (a ``PSFModel`` or its array), an image object as ``psf_model``.  ``fit_radius``: pixels;
    None takes the ``PSFFITR`` card the models carry (6 without one), and models that disagree on it are an error: say
    which radius is meant.  ``fit_sky``: fit a constant beside the flux.  ``bad_bits``: the mask bits that take a pixel out
    of a fit (default ``BAD_SUM``).  ``flags`` are then those of the fit (``psf.PSF_FLAGS``) and the table gains ``chi2``,
    ``npix``, ``cover`` and ``sky``.  ``radius`` belongs to the aperture, ``fit_radius`` / ``fit_sky`` / ``bad_bits`` to
    the fit."""
    import torch
    if method not in ('aperture', 'psf'):
        raise ValueError(f'forced_photometry_batch: method {method!r} is neither \'aperture\' nor \'psf\'')
    eng = engine or get_engine()
    device = torch.device('cuda', eng.device)
    ra = _f64(ra, 'ra')
    dec = _f64(dec, 'dec', ra.size)
    planes = [_resident(im, torch, device) for im in images]
    nimg, nsrc = len(planes), ra.size
    recs = (_lib.zm_lc_image * max(nimg, 1))()
    wcs = (_lib.zm_wcs * max(nimg, 1))()
    for k, (img, rms, mask, w, ny, nx) in enumerate(planes):
        s = _lib.wcs_struct(w)
        s.naxis[0], s.naxis[1] = nx, ny
        wcs[k] = s
        recs[k].img, recs[k].rms, recs[k].mask = img.data_ptr(), rms.data_ptr() if rms is not None else None, \
            mask.data_ptr() if mask is not None else None
        recs[k].wcs, recs[k].nx, recs[k].ny = s, nx, ny
    d_ra, d_dec = torch.from_numpy(ra).to(device), torch.from_numpy(dec).to(device)
    d_off = torch.zeros(nimg + 1, dtype=torch.int64, device=device)
    torch.cuda.synchronize(device)                      # planes and positions may come from any stream; the engine has its own
    cap = max(nsrc, 1024)
    while True:
        d_idx = torch.empty(cap, dtype=torch.int32, device=device)
        n = C.c_int64(0)
        check(eng.L.zm_footprint_join_dev(eng.ctx, nimg, wcs, nsrc, d_ra.data_ptr(), d_dec.data_ptr(), cap, d_off.data_ptr(),
                                          d_idx.data_ptr(), C.byref(n)), 'zm_footprint_join_dev')
        if n.value <= cap:
            break
        cap = int(n.value)
    eng.synchronize()
    npairs = int(n.value)
    offsets, src_idx = d_off.cpu().numpy(), d_idx[:npairs].cpu().numpy()
    if done is not None and len(done):
        offsets, src_idx = drop_done(offsets, src_idx, done)
        npairs = src_idx.size
        d_off = torch.from_numpy(offsets).to(device)
        d_idx = torch.from_numpy(src_idx).to(device) if npairs else d_idx
        torch.cuda.synchronize(device)
    if method == 'psf':
        return _psf_batch(eng, torch, device, images, planes, wcs, d_off, d_idx, offsets, src_idx, npairs, nsrc, d_ra, d_dec,
                          fit_radius, fit_sky, bad_bits)
    res = torch.empty((4, max(npairs, 1)), dtype=torch.float64, device=device)
    flg = torch.empty(max(npairs, 1), dtype=torch.int32, device=device)
    check(eng.L.zm_forced_photometry_batch_dev(eng.ctx, nimg, recs, d_off.data_ptr(), d_idx.data_ptr(), npairs, nsrc,
                                               d_ra.data_ptr(), d_dec.data_ptr(), float(radius), res[0].data_ptr(),
                                               res[1].data_ptr(), res[2].data_ptr(), res[3].data_ptr(), flg.data_ptr()),
          'zm_forced_photometry_batch_dev')
    eng.synchronize()
    r = res[:, :npairs].cpu().numpy()
    return dict(image=np.repeat(np.arange(nimg, dtype=np.int32), np.diff(offsets)), source=src_idx.astype(np.int32),
                x=r[0].copy(), y=r[1].copy(), flux=r[2].copy(), fluxerr=r[3].copy(),
                flags=flg[:npairs].cpu().numpy().copy(), offsets=offsets)


def _psf_batch(eng, torch, device, images, planes, wcs, d_off, d_idx, offsets, src_idx, npairs, nsrc, d_ra, d_dec, fit_radius,
               fit_sky, bad_bits):
    """The launch of ``forced_photometry_batch(method='psf')`` behind the join."""
    from .constants import BAD_SUM
    nimg = len(planes)
    psfs = [_psf_of(im) for im in images]
    if fit_radius is None:
        radii = sorted({p.fit_radius for p in psfs})
        if len(radii) > 1:
            raise ValueError(f'forced_photometry_batch: the models of this batch carry different PSFFITR ({radii}): pass fit_radius')
        fit_radius = radii[0] if radii else 6.0
    models = [torch.from_numpy(p.data).to(device) for p in psfs]
    recs = (_lib.zm_psf_image * max(nimg, 1))()
    for k, (img, rms, mask, w, ny, nx) in enumerate(planes):
        recs[k].img, recs[k].rms, recs[k].mask = img.data_ptr(), rms.data_ptr() if rms is not None else None, \
            mask.data_ptr() if mask is not None else None
        recs[k].wcs, recs[k].nx, recs[k].ny = wcs[k], nx, ny
        recs[k].model, recs[k].half = models[k].data_ptr(), psfs[k].half
    torch.cuda.synchronize(device)
    res = torch.empty((7, max(npairs, 1)), dtype=torch.float64, device=device)
    ints = torch.empty((2, max(npairs, 1)), dtype=torch.int32, device=device)
    check(eng.L.zm_psf_photometry_batch_dev(eng.ctx, nimg, recs, d_off.data_ptr(), d_idx.data_ptr(), npairs, nsrc,
                                            d_ra.data_ptr(), d_dec.data_ptr(), int(BAD_SUM if bad_bits is None else bad_bits),
                                            float(fit_radius), int(bool(fit_sky)), *(res[k].data_ptr() for k in range(7)),
                                            ints[0].data_ptr(), ints[1].data_ptr()), 'zm_psf_photometry_batch_dev')
    eng.synchronize()
    r = res[:, :npairs].cpu().numpy()
    i = ints[:, :npairs].cpu().numpy()
    return dict(image=np.repeat(np.arange(nimg, dtype=np.int32), np.diff(offsets)), source=src_idx.astype(np.int32),
                x=r[0].copy(), y=r[1].copy(), flux=r[2].copy(), fluxerr=r[3].copy(), flags=i[1].copy(), offsets=offsets,
                chi2=r[4].copy(), npix=i[0].copy(), cover=r[6].copy(), sky=r[5].copy())


def photometry_rows(table, headers, ra, dec, source_ids=None, image_ids=None, method='aperture'):
    """The rows ``scripts/dophot.py`` writes (``scripts/dophot.py:144-156``) from the table of
    ``forced_photometry_batch``: one dict per pair with the keys of ``PHOT_CSV_COLUMNS``.  ``headers``: the header of
    each image: ``zp = MAGZP + APCOR4``, ``obsjd`` and ``filtercode`` ('z' + the last letter of FILTER) as
    ``raw_aperture_photometry`` takes them.  ``method='psf'`` (a table of PSF fits): ``zp = MAGZP + PSFCOR``."""
    if method not in ('aperture', 'psf'):
        raise ValueError(f'photometry_rows: method {method!r} is neither \'aperture\' nor \'psf\'')
    zp = [h['MAGZP'] + h[APER_KEY if method == 'aperture' else 'PSFCOR'] for h in headers]
    jd = [h.get('OBSJD') for h in headers]
    fc = ['z' + str(h['FILTER'])[-1] if 'FILTER' in h else None for h in headers]
    rows = []
    for k in range(len(table['source'])):
        i, s = int(table['image'][k]), int(table['source'][k])
        rows.append({'source_id': s if source_ids is None else source_ids[s],
                     'image_id': i if image_ids is None else image_ids[i],
                     'flux': float(table['flux'][k]), 'fluxerr': float(table['fluxerr'][k]), 'flags': int(table['flags'][k]),
                     'ra': float(ra[s]), 'dec': float(dec[s]), 'zp': zp[i], 'filtercode': fc[i], 'obsjd': jd[i]})
    return rows


def write_phot_csv(path, rows, append=False):
    """The CSV of ``scripts/dophot.py`` (``pd.DataFrame(output).to_csv(outfile, index=False)``): a header line, then one
    line per row in the reference's column order; floats with ``repr`` (they read back to the same bits)."""
    def fmt(v):
        if v is None:
            return ''
        if isinstance(v, (float, np.floating)):
            return repr(float(v))
        return str(v)
    new = not (append and os.path.exists(path))
    with open(path, 'a' if append else 'w') as f:
        if new:
            f.write(','.join(PHOT_CSV_COLUMNS) + '\n')
        for r in rows:
            f.write(','.join(fmt(r[c]) for c in PHOT_CSV_COLUMNS) + '\n')


def read_phot_csv(path):
    """Rows of a file ``write_phot_csv`` (or the reference's driver) wrote: a list of dicts; ``flux``, ``fluxerr``, ``ra``,
    ``dec``, ``zp`` and ``obsjd`` as float, ``flags`` as int, ids and ``filtercode`` as written (an id of digits: int)."""
    rows = []
    with open(path) as f:
        cols = f.readline().strip().split(',')
        if tuple(cols) != PHOT_CSV_COLUMNS:
            raise ValueError(f'{path}: columns {cols}, expected {list(PHOT_CSV_COLUMNS)}')
        for line in f:
            line = line.rstrip('\n')
            if not line:
                continue
            v = dict(zip(cols, line.split(',')))
            for c in ('flux', 'fluxerr', 'ra', 'dec', 'zp', 'obsjd'):
                v[c] = float(v[c]) if v[c] != '' else None
            v['flags'] = int(v['flags'])
            for c in ('source_id', 'image_id'):
                if v[c].lstrip('-').isdigit():
                    v[c] = int(v[c])
            v['filtercode'] = v['filtercode'] or None
            rows.append(v)
    return rows


def light_curves(rows, sources=None):
    """Rows (dicts with the keys of ``PHOT_CSV_COLUMNS``, or ``ForcedPhotometry`` objects) grouped by source, each group
    ordered by ``obsjd``: ``{source_id: [ForcedPhotometry, ...]}``.  With ``sources`` (``Source`` objects) every point is
    also appended to its source's ``forced_photometry`` (ids that match no source are kept in the result only)."""
    from .photometry import ForcedPhotometry
    by_id = {s.id: s for s in sources} if sources is not None else {}
    out = {}
    for r in rows:
        if isinstance(r, dict):
            sid = r['source_id']
            r = ForcedPhotometry(flux=r['flux'], fluxerr=r['fluxerr'], flags=r['flags'], ra=r['ra'], dec=r['dec'], zp=r['zp'],
                                 obsjd=r['obsjd'], filtercode=r['filtercode'], image=r['image_id'],
                                 source=by_id.get(sid, sid))
        else:
            sid = getattr(r.source, 'id', r.source)
        out.setdefault(sid, []).append(r)
    for sid, pts in out.items():
        pts.sort(key=lambda p: (p.obsjd is None, p.obsjd or 0.0))
        if sid in by_id:
            by_id[sid].forced_photometry.extend(pts)
    return out
