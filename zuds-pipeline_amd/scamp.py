"""Astrometric refit (``zuds/scamp.py``): ``calibrate_astrometry`` with the reference's signature and effects, without
a SCAMP process.

The reference copies the frames' catalogs into a scratch directory, runs ``scamp -c default.scamp`` on them, strips the
photometric cards from the ``.head`` files SCAMP leaves and either copies those next to the images and their masks or
writes their cards into the files (``zuds/scamp.py:16-113``).  Here the solver is ``zm_astrom_solve``
(``csrc/astrometry.hip``; DESIGN.md, "Astrometric refit"): a vote for the gross offset between a frame's detections and
the star catalogue, then rounds of cross-identification and a clipped polynomial fit, all frames of a call in one batch
of launches.  It takes SCAMP's parameters where ``default.scamp`` sets them; it is this project's own operator, and
SCAMP's digits, its global multi-exposure solution and its search in rotation and scale are not claimed.

The star catalogue comes from a file (``ASTREF_CATALOG FILE``, ``ASTREFCAT_NAME``): the default of ``default.scamp``,
GAIA-DR2, is fetched over the network by SCAMP and cannot be had here.
"""
import ctypes as C
import warnings
from pathlib import Path

import numpy as np

from . import _lib
from . import fits as _fits
from .wcs import NPV, WCS

__all__ = ['calibrate_astrometry', 'read_astrefcat', 'write_astrefcat', 'read_head', 'write_head']

PARAM_NAMES = ('position_maxerr', 'match_resol', 'crossid_radius', 'clip_nsigma', 'degree', 'match', 'match_nmax',
               'max_rounds', 'max_clip')
ASTREF_COLUMNS = ('X_WORLD', 'Y_WORLD', 'ERRA_WORLD', 'ERRB_WORLD', 'MAG', 'OBSDATE')
NEEDED_COLUMNS = ('XWIN_IMAGE', 'YWIN_IMAGE', 'ERRAWIN_IMAGE', 'ERRBWIN_IMAGE', 'FLAGS', 'ELONGATION', 'FLUX_AUTO',
                  'FLUXERR_AUTO', 'FWHM_IMAGE')
# cards the reference strips from SCAMP's .head files (zuds/scamp.py:82-85); none of them is ever written here
STRIPPED_CARDS = ('FLXSCALE', 'MAGZEROP', 'PHOTIRMS', 'PHOTINST', 'PHOTLINK', 'COMMENT', 'HISTORY')
MATCH_NMAX_AUTO = 1024


def astrom_params(**kw):
    """``zm_astrom_params`` with the defaults of the library and ``kw`` laid over them."""
    p = _lib.zm_astrom_params()
    _lib.lib().zm_astrom_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in PARAM_NAMES:
            raise TypeError(f'astrometry: unknown parameter {k!r} (known: {", ".join(PARAM_NAMES)})')
        setattr(p, k, type(getattr(p, k))(v))
    return p


def _results(wcs_list, res, match, used, offsets):
    out_w, out_i = [], []
    for f, r in enumerate(res):
        out_w.append(WCS.from_struct(r.wcs))
        lo, hi = int(offsets[f]), int(offsets[f + 1])
        out_i.append(dict(status=_lib.ASTROM_STATUS[r.status], shift=(r.shift[0], r.shift[1]), vote_peak=int(r.vote_peak),
                          vote_runner_up=int(r.vote_runner_up), nmatch=int(r.nmatch), nused=int(r.nused),
                          rounds=int(r.rounds), rms=(r.rms[0], r.rms[1]), chi2=float(r.chi2), match=match[lo:hi],
                          used=used[lo:hi]))
    return out_w, out_i


def solve(wcs_list, detections, ref, engine=None, **params):
    """Refit the headers ``wcs_list`` (``zm_astrom_solve``).  ``detections``: per frame ``(x, y, sd, snr)`` - FITS
    1-based pixels, position sigma in pixels, rank key; ``ref``: ``(ra, dec, sig)`` of the star catalogue in degrees and
    arcsec.  Returns ``(list of WCS, list of dict)``: per frame ``status`` (``OK``, ``TOO_FEW``, ``AMBIGUOUS``,
    ``SINGULAR``, ``NOT_CONVERGED``), ``shift``, ``vote_peak``, ``vote_runner_up``, ``nmatch``, ``nused``, ``rounds``,
    ``rms``, ``chi2``, ``match`` (int32 per detection: its star or -1) and ``used`` (uint8)."""
    from .engine import get_engine
    eng = engine or get_engine()
    nf = len(wcs_list)
    if len(detections) != nf:
        raise ValueError(f'{nf} headers but {len(detections)} detection lists')
    cols = [[np.ascontiguousarray(d[k], dtype=np.float64).ravel() for d in detections] for k in range(4)]
    offsets = np.zeros(nf + 1, np.int32)
    for f in range(nf):
        if len({cols[k][f].size for k in range(4)}) != 1:
            raise ValueError(f'frame {f}: x, y, sd and snr differ in length')
        offsets[f + 1] = offsets[f] + cols[0][f].size
    x, y, sd, snr = (np.concatenate(c) if nf else np.zeros(0) for c in cols)
    ra, dec, sig = (np.ascontiguousarray(v, dtype=np.float64).ravel() for v in ref)
    if not ra.size == dec.size == sig.size:
        raise ValueError('ref: ra, dec and sig differ in length')
    w0 = (_lib.zm_wcs * max(nf, 1))(*[_lib.wcs_struct(w) for w in wcs_list])
    res = (_lib.zm_astrom_result * max(nf, 1))()
    match, used = np.full(x.size, -1, np.int32), np.zeros(x.size, np.uint8)
    p = astrom_params(**params)
    _lib.check(eng.L.zm_astrom_solve(eng.ctx, nf, w0, offsets.ctypes.data, x.ctypes.data, y.ctypes.data, sd.ctypes.data,
                                     snr.ctypes.data, ra.size, ra.ctypes.data, dec.ctypes.data, sig.ctypes.data, C.byref(p),
                                     res, match.ctypes.data, used.ctypes.data), 'zm_astrom_solve')
    return _results(wcs_list, res[:nf], match, used, offsets)


def solve_dev(wcs_list, offsets, x, y, sd, snr, ref_ra, ref_dec, ref_sig, engine=None, stream=None, **params):
    """``solve`` on float64 torch tensors that lie in HBM (``zm_astrom_solve_dev``): the rows of all frames concatenated,
    frame f owning rows ``offsets[f] .. offsets[f + 1] - 1``.  ``match`` and ``used`` of the result are device tensors
    (views per frame).  The call waits for one word per frame after the vote and after every round."""
    import torch
    from .engine import get_engine
    from .source import _dev_f64
    eng = engine or get_engine()
    nf = len(wcs_list)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    if offsets.size != nf + 1:
        raise ValueError(f'offsets must hold {nf + 1} entries')
    n, m = x.numel(), ref_ra.numel()
    _dev_f64(x, 'x'), _dev_f64(y, 'y', n), _dev_f64(sd, 'sd', n), _dev_f64(snr, 'snr', n)
    _dev_f64(ref_ra, 'ref_ra'), _dev_f64(ref_dec, 'ref_dec', m), _dev_f64(ref_sig, 'ref_sig', m)
    if nf and int(offsets[-1]) > n:
        raise ValueError(f'offsets end at {int(offsets[-1])} but there are {n} rows')
    w0 = (_lib.zm_wcs * max(nf, 1))(*[_lib.wcs_struct(w) for w in wcs_list])
    res = (_lib.zm_astrom_result * max(nf, 1))()
    p = astrom_params(**params)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(x.device):
        # (no fill kernels here: they would run on torch's stream, unordered with the context's, which initialises both)
        match = torch.empty(n, dtype=torch.int32, device=x.device)
        used = torch.empty(n, dtype=torch.uint8, device=x.device)
        _lib.check(eng.L.zm_astrom_solve_dev(eng.ctx, nf, w0, offsets.ctypes.data, x.data_ptr(), y.data_ptr(), sd.data_ptr(),
                                             snr.data_ptr(), m, ref_ra.data_ptr(), ref_dec.data_ptr(), ref_sig.data_ptr(),
                                             C.byref(p), res, match.data_ptr(), used.data_ptr()), 'zm_astrom_solve_dev')
    return _results(wcs_list, res[:nf], match, used, offsets)


# ---- source selection -------------------------------------------------------------------------------------------------
def select(cat, sn_threshold=10.0, ellipticity_max=0.5, flags_mask=0x00f0, fwhm_thresholds=(0.0, 100.0)):
    """The source selection of ``default.scamp`` on a wide catalog table (``columns='param'``): ``FLAGS & flags_mask
    == 0``, ellipticity ``1 - 1 / ELONGATION <= ellipticity_max``, ``FLUX_AUTO / FLUXERR_AUTO >= sn_threshold`` and
    ``FWHM_IMAGE`` within ``fwhm_thresholds``.  Returns a dict: ``rows`` (indices kept), ``x``, ``y`` (``XWIN_IMAGE``,
    ``YWIN_IMAGE``), ``sd`` (``sqrt((ERRAWIN_IMAGE^2 + ERRBWIN_IMAGE^2) / 2)``) and ``snr``."""
    names = cat.dtype.names or ()
    missing = [c for c in NEEDED_COLUMNS if c not in names]
    if missing:
        raise ValueError(f"the catalog lacks {', '.join(missing)}: make it with columns='param'")
    f64 = lambda k: np.asarray(cat[k], dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        snr = f64('FLUX_AUTO') / f64('FLUXERR_AUTO')
        ell = 1.0 - 1.0 / f64('ELONGATION')
        fwhm = f64('FWHM_IMAGE')
        keep = ((np.asarray(cat['FLAGS']).astype(np.int64) & int(flags_mask)) == 0) & (ell <= ellipticity_max) & \
               (snr >= sn_threshold) & (fwhm >= fwhm_thresholds[0]) & (fwhm <= fwhm_thresholds[1])
    rows = np.flatnonzero(keep)
    sd = np.sqrt((f64('ERRAWIN_IMAGE')[rows] ** 2 + f64('ERRBWIN_IMAGE')[rows] ** 2) / 2.0)
    return dict(rows=rows, x=f64('XWIN_IMAGE')[rows], y=f64('YWIN_IMAGE')[rows], sd=sd, snr=snr[rows])


# ---- the star catalogue -----------------------------------------------------------------------------------------------
def _mjd_to_year(mjd):
    return 2000.0 + (np.asarray(mjd, dtype=np.float64) - 51544.5) / 365.25


def write_astrefcat(path, ra, dec, erra=None, errb=None, mag=None, obsdate=2015.5, pmra=None, pmdec=None):
    """A star catalogue in the FITS_LDAC layout SCAMP reads with ``ASTREF_CATALOG FILE``: ``X_WORLD``, ``Y_WORLD``,
    ``ERRA_WORLD``, ``ERRB_WORLD`` (degrees), ``MAG``, ``OBSDATE`` (Julian years) and, when given, ``PMALPHA_J2000``
    (including cos dec) and ``PMDELTA_J2000`` in mas / yr."""
    ra = np.asarray(ra, dtype=np.float64).ravel()
    n = ra.size
    full = lambda v, d: np.broadcast_to(np.asarray(d if v is None else v, dtype=np.float64), (n,))
    fields = [(c, 'f8') for c in ASTREF_COLUMNS]
    if pmra is not None or pmdec is not None:
        fields += [('PMALPHA_J2000', 'f8'), ('PMDELTA_J2000', 'f8')]
    tab = np.zeros(n, dtype=fields)
    tab['X_WORLD'], tab['Y_WORLD'] = ra, full(dec, 0.0)
    tab['ERRA_WORLD'], tab['ERRB_WORLD'] = full(erra, 1e-3 / 3600.0), full(errb if errb is not None else erra, 1e-3 / 3600.0)
    tab['MAG'], tab['OBSDATE'] = full(mag, 15.0), full(obsdate, 2015.5)
    if len(fields) > len(ASTREF_COLUMNS):
        tab['PMALPHA_J2000'], tab['PMDELTA_J2000'] = full(pmra, 0.0), full(pmdec, 0.0)
    _fits.write_ldac(path, tab, {}, {})


def read_astrefcat(path, mjd=None):
    """``(ra, dec, sig)`` of a star catalogue written as ``write_astrefcat`` writes it: degrees, and
    ``sig = sqrt((ERRA_WORLD^2 + ERRB_WORLD^2) / 2)`` in arcsec.  With ``mjd`` and proper-motion columns every star is
    moved from its ``OBSDATE`` to that epoch; ``PMALPHA_J2000`` includes cos dec."""
    tab = _fits.read_ldac(str(path))[0]
    names = tab.dtype.names or ()
    missing = [c for c in ASTREF_COLUMNS if c not in names]
    if missing:
        raise ValueError(f'{path}: not an astrometric reference catalogue (no {", ".join(missing)})')
    ra, dec = np.array(tab['X_WORLD'], dtype=np.float64), np.array(tab['Y_WORLD'], dtype=np.float64)
    sig = 3600.0 * np.sqrt((np.asarray(tab['ERRA_WORLD'], np.float64) ** 2 + np.asarray(tab['ERRB_WORLD'], np.float64) ** 2) / 2.0)
    if mjd is not None and 'PMALPHA_J2000' in names and 'PMDELTA_J2000' in names:
        dt = _mjd_to_year(mjd) - np.asarray(tab['OBSDATE'], np.float64)
        mas = 1.0 / 3.6e6
        with np.errstate(divide='ignore', invalid='ignore'):
            dra = np.asarray(tab['PMALPHA_J2000'], np.float64) * mas * dt / np.cos(np.radians(dec))
        ra = np.mod(ra + np.where(np.isfinite(dra), dra, 0.0), 360.0)
        dec = dec + np.asarray(tab['PMDELTA_J2000'], np.float64) * mas * dt
    return ra, dec, sig


# ---- .head files ------------------------------------------------------------------------------------------------------
def solution_cards(wcs, rms=None):
    """[(key, value, comment)] of a solved header: what SCAMP leaves in a ``.head`` file once the reference has stripped
    its photometric cards.  ``rms``: the two residuals in arcsec; ``ASTRRMS1 / 2`` are written in degrees, as SCAMP
    writes them."""
    h = wcs.to_header()
    cards = [('EQUINOX', 2000.0, 'Mean equinox'), ('RADESYS', 'ICRS', 'Astrometric system')]
    for k in ('CTYPE1', 'CTYPE2', 'CUNIT1', 'CUNIT2', 'CRVAL1', 'CRVAL2', 'CRPIX1', 'CRPIX2', 'CD1_1', 'CD1_2', 'CD2_1', 'CD2_2'):
        cards.append((k, h[k], ''))
    cards += [(k, v, '') for k, v in h.items() if k.startswith(('PV1_', 'PV2_'))]
    if rms is not None:
        cards += [('ASTRRMS1', float(rms[0]) / 3600.0, 'Astrom. dispersion RMS along axis 1 (deg)'),
                  ('ASTRRMS2', float(rms[1]) / 3600.0, 'Astrom. dispersion RMS along axis 2 (deg)')]
    return cards


def _head_card(key, value, comment):
    """A card whose float keeps every digit (free format: the 20-column field of ``fits._card`` holds 15)."""
    if isinstance(value, float) and np.isfinite(value):
        body = f'{key:<8}= {repr(value).upper():>20}' + (f' / {comment}' if comment else '')
        return body[:80].ljust(80)
    return _fits._card(key, value, comment)


def write_head(path, wcs, rms=None):
    """A ``.head`` file: 80-column cards, one per line, ending in ``END``."""
    lines = [_head_card(k, v, c) for k, v, c in solution_cards(wcs, rms)] + ['END'.ljust(80)]
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def read_head(path, naxis=(0, 0)):
    """``(WCS, header dict, comments dict)`` of a ``.head`` file (``naxis``: a ``.head`` file carries none)."""
    header, comments = {}, {}
    with open(path) as f:
        for line in f:
            card = line.rstrip('\n')
            key = card[:8].strip()
            if key == 'END':
                break
            if not key or key in ('COMMENT', 'HISTORY') or card[8:10] != '= ':
                continue
            val, com = _fits._parse_value(card[10:])
            if val is not None:
                header[key], comments[key] = val, com
    w = WCS.from_header(header)
    w.naxis = (int(naxis[0]), int(naxis[1]))
    return w, header, comments


def fold_linear(wcs):
    """A TPV header whose polynomials are linear as the TAN header that maps every pixel to the same place:
    ``(xi, eta) = t + M CD (p - CRPIX)`` with ``M = [[PV1_1, PV1_2], [PV2_2, PV2_1]]`` and ``t = (PV1_0, PV2_0)`` is
    ``CD' (p - CRPIX')`` with ``CD' = M CD`` and ``CRPIX' = CRPIX - CD'^-1 t``."""
    keep = (0, 1, 2)
    if any(wcs.pv1[k] != 0.0 or wcs.pv2[k] != 0.0 for k in range(NPV) if k not in keep):
        raise ValueError('fold_linear: the header has terms beyond the first degree')
    M = np.array([[wcs.pv1[1], wcs.pv1[2]], [wcs.pv2[2], wcs.pv2[1]]])
    cd = M @ wcs.cd
    crpix = wcs.crpix - np.linalg.solve(cd, np.array([wcs.pv1[0], wcs.pv2[0]]))
    return WCS(crpix, wcs.crval, cd, naxis=wcs.naxis)


# ---- scamp_kws --------------------------------------------------------------------------------------------------------
# keys of default.scamp that would change the operator and are not built: accepted with these values only
_SCAMP_FIXED = {
    'SOLVE_ASTROM': ('Y',), 'SOLVE_PHOTOM': ('N',), 'MATCH_FLIPPED': ('N',), 'MOSAIC_TYPE': ('UNCHANGED',),
    'STABILITY_TYPE': ('INSTRUMENT',), 'ASTRINSTRU_KEY': ('FILTER,QRUNID',),
    'CENTROID_KEYS': ('XWIN_IMAGE,YWIN_IMAGE',), 'CENTROIDERR_KEYS': ('ERRAWIN_IMAGE,ERRBWIN_IMAGE,ERRTHETAWIN_IMAGE',),
    'DISTORT_KEYS': ('XWIN_IMAGE,YWIN_IMAGE',), 'DISTORT_GROUPS': ('1,1',), 'ASTREF_BAND': ('DEFAULT',),
    'ASTREFMAG_LIMITS': ('-99.0,99.0', '-99,99'), 'PIXSCALE_MAXERR': ('1.2',), 'POSANGLE_MAXERR': ('5.0', '5'),
    'HEADER_SUFFIX': ('.HEAD',), 'AHEADER_SUFFIX': ('.AHEAD',),
    'ASTREFCENT_KEYS': ('X_WORLD,Y_WORLD',), 'ASTREFERR_KEYS': ('ERRA_WORLD,ERRB_WORLD,ERRTHETA_WORLD',),
    'ASTREFPROP_KEYS': ('PMALPHA_J2000,PMDELTA_J2000',), 'ASTREFMAG_KEY': ('MAG',), 'ASTREFOBSDATE_KEY': ('OBSDATE',),
}
_SCAMP_IGNORED = ('REF_SERVER', 'SAVE_REFCATALOG', 'REFOUT_CATPATH', 'MERGEDOUTCAT_TYPE', 'MERGEDOUTCAT_NAME',
                  'FULLOUTCAT_TYPE', 'FULLOUTCAT_NAME', 'CHECKPLOT_DEV', 'CHECKPLOT_TYPE', 'CHECKPLOT_NAME',
                  'VERBOSE_TYPE', 'WRITE_XML', 'XML_NAME', 'NTHREADS', 'MAGZERO_OUT', 'MAGZERO_INTERR', 'MAGZERO_REFERR',
                  'PHOTINSTRU_KEY', 'MAGZERO_KEY', 'EXPOTIME_KEY', 'AIRMASS_KEY', 'EXTINCT_KEY', 'PHOTOMFLAG_KEY',
                  'PHOTFLUX_KEY', 'PHOTFLUXERR_KEY')


def _yn(v):
    return str(v).strip().upper() in ('Y', 'YES', 'TRUE', '1')


def _pair(v, what):
    tok = str(v).replace('(', '').replace(')', '').split(',') if not isinstance(v, (list, tuple, np.ndarray)) else list(v)
    if len(tok) != 2:
        raise ValueError(f'scamp_kws: {what} takes two values (got {v!r})')
    return float(tok[0]), float(tok[1])


def settings_from_kws(scamp_kws=None):
    """``scamp_kws`` (the ``-KEY value`` pass-through of ``zuds/scamp.py:65-67``) -> dict(astrefcat, params, selection,
    projection).  Keys that are built map onto the solver; a key that would change the operator and is not built raises
    ``ValueError`` unless it carries ``default.scamp``'s value (the rule of ``swarp.py`` and ``hotpants.py``);
    bookkeeping keys are ignored."""
    kws = {str(k).upper(): v for k, v in (scamp_kws or {}).items()}
    cat = str(kws.pop('ASTREF_CATALOG', 'GAIA-DR2')).strip().upper()
    name = kws.pop('ASTREFCAT_NAME', None)
    if cat != 'FILE':
        raise ValueError(f'scamp_kws: ASTREF_CATALOG {cat} is fetched over the network by SCAMP and is not available '
                         f'here: pass ASTREF_CATALOG=FILE and ASTREFCAT_NAME=<a FITS_LDAC star catalogue>')
    if not name:
        raise ValueError('scamp_kws: ASTREF_CATALOG=FILE needs ASTREFCAT_NAME=<a FITS_LDAC star catalogue>')
    params, sel, projection = {}, {}, 'SAME'
    for k, v in kws.items():
        if k == 'CROSSID_RADIUS':
            params['crossid_radius'] = float(v)
        elif k == 'POSITION_MAXERR':
            params['position_maxerr'] = 60.0 * float(v)                 # arcmin in SCAMP, arcsec in the solver
        elif k == 'MATCH':
            params['match'] = 1 if _yn(v) else 0
        elif k == 'MATCH_RESOL':
            params['match_resol'] = float(v)
        elif k == 'MATCH_NMAX':
            params['match_nmax'] = int(v) or MATCH_NMAX_AUTO            # 0 = auto
        elif k == 'DISTORT_DEGREES':
            deg = int(str(v).split(',')[0]) if len(str(v).split(',')) == 1 else None
            if deg not in (1, 2, 3):
                raise ValueError(f'scamp_kws: DISTORT_DEGREES {v}: one group of degree 1, 2 or 3')
            params['degree'] = deg
        elif k == 'PROJECTION_TYPE':
            projection = str(v).strip().upper()
            if projection not in ('SAME', 'TPV'):
                raise ValueError(f'scamp_kws: PROJECTION_TYPE {v}: SAME or TPV')
        elif k == 'SN_THRESHOLDS':
            sel['sn_threshold'] = _pair(v, 'SN_THRESHOLDS')[0]          # the second is SCAMP's high-S/N sample: not built
        elif k == 'ELLIPTICITY_MAX':
            sel['ellipticity_max'] = float(v)
        elif k == 'FLAGS_MASK':
            sel['flags_mask'] = int(v, 0) if isinstance(v, str) else int(v)
        elif k == 'FWHM_THRESHOLDS':
            sel['fwhm_thresholds'] = _pair(v, 'FWHM_THRESHOLDS')
        elif k in _SCAMP_FIXED:
            if str(v).replace(' ', '').upper() not in _SCAMP_FIXED[k]:
                raise ValueError(f'scamp_kws: -{k} {v} changes the astrometric solution and is not implemented '
                                 f'(the solver works with {" / ".join(_SCAMP_FIXED[k])})')
        elif k in _SCAMP_IGNORED:
            continue
        else:
            raise ValueError(f'scamp_kws: -{k} {v} is not implemented by the astrometric refit')
    return dict(astrefcat=str(name), params=params, selection=sel, projection=projection)


# ---- calibrate_astrometry ---------------------------------------------------------------------------------------------
def solve_images(images, scamp_kws=None, engine=None):
    """The solution of every image of ``images`` in one call: ``[(WCS, info dict)]``.  Makes a wide catalog where an
    image has none.  Changes nothing else; raises ``RuntimeError`` on a frame whose status is not ``OK``.

    The catalogue's stars are moved by their proper motions to ONE epoch per call, the median ``MJD-OBS`` of the frames
    that carry the card.  A frame without it gets the reference's warning and does not count towards the epoch; it is
    still matched against the stars at that epoch, since all frames of a call share one catalogue (only a call in
    which no frame has ``MJD-OBS`` leaves the stars unmoved)."""
    from .catalog import PipelineFITSCatalog
    st = settings_from_kws(scamp_kws)
    mjds = []
    for image in images:
        if getattr(image, 'catalog', None) is None:
            PipelineFITSCatalog.from_image(image, columns='param')
        if 'MJD-OBS' in image.header:
            mjds.append(float(image.header['MJD-OBS']))
        else:
            warnings.warn(f'Image "{image.basename}" header does not contain MJD-OBS keyword, proper motions may '
                          f'not be used in deriving astrometric solution... (the stars of a call share one epoch, the '
                          f'median MJD-OBS of the frames that carry one: this frame does not count towards it)')
    # one epoch per call: the median MJD-OBS of the frames that carry one (none at all: the stars stay where they are)
    ref = read_astrefcat(st['astrefcat'], mjd=float(np.median(mjds)) if mjds else None)
    wcs0 = [image.wcs for image in images]
    dets = []
    for image in images:
        s = select(image.catalog.data, **st['selection'])
        dets.append((s['x'], s['y'], s['sd'], s['snr']))
    solved, infos = solve(wcs0, dets, ref, engine=engine, **st['params'])
    out = []
    for image, w0, w, info in zip(images, wcs0, solved, infos):
        if info['status'] != 'OK':
            raise RuntimeError(f'astrometric refit of "{image.basename}" failed: status {info["status"]}, nmatch '
                               f'{info["nmatch"]}, vote peak {info["vote_peak"]}, runner-up {info["vote_runner_up"]}')
        if st['projection'] == 'SAME' and not w0.has_pv and st['params'].get('degree', 3) == 1:
            w = fold_linear(w)
        out.append((w, info))
    return out


def apply_solution(header, comments, wcs, rms):
    """Write the solved cards into a header dict (and its comments): every old PVi_j goes first."""
    for k in [k for k in header if str(k).startswith(('PV1_', 'PV2_'))]:
        header.pop(k)
        comments.pop(k, None)
    for k, v, c in solution_cards(wcs, rms):
        header[k] = v
        comments[k] = c


def transaction_copies(images):
    """Shallow copies of ``images`` and of their masks with header dicts of their own: what a coadd that solves its
    inputs first works on, so that the caller's objects keep their headers (``zuds/coadd.py:77-118`` copies the files
    into a scratch directory for the same reason)."""
    import copy
    out = []
    for image in images:
        new = copy.copy(image)
        objs = [new]
        if getattr(image, 'mask_image', None) is not None:
            new.mask_image = copy.copy(image.mask_image)
            objs.append(new.mask_image)
        for obj in objs:
            obj.header = dict(obj.header or {})
            obj.header_comments = dict(obj.header_comments or {})
        out.append(new)
    return out


def solve_into(images, scamp_kws=None):
    """Solve ``images`` in one call and write the solved cards into their header dicts and their masks': no file is
    touched (the `.head` files SCAMP leaves for SWarp, kept in memory)."""
    for image, (w, info) in zip(images, solve_images(images, scamp_kws)):
        for obj in (image, getattr(image, 'mask_image', None)):
            if obj is not None:
                apply_solution(obj.header, obj.header_comments, w, info['rms'])


def calibrate_astrometry(image_or_images, scamp_kws=None, inplace=False, tmpdir='/tmp'):
    """Derive the astrometric solution of the input images (``zuds/scamp.py:16-113``).

    ``scamp_kws``: SCAMP configuration keys; ``ASTREF_CATALOG='FILE'`` and ``ASTREFCAT_NAME`` are required.
    ``inplace``: write the solved cards into the headers of each image and of its mask and save both files; otherwise
    write ``<basename>.head`` beside the image and beside its mask.  ``tmpdir`` is accepted for the reference's
    signature: nothing is exchanged through files."""
    images = np.atleast_1d(image_or_images).tolist()
    solutions = solve_images(images, scamp_kws)
    for image, (w, info) in zip(images, solutions):
        for target in (image, getattr(image, 'mask_image', None)):
            if target is None:
                continue
            if inplace:
                if target.header_comments is None:
                    target.header_comments = {}
                apply_solution(target.header, target.header_comments, w, info['rms'])
                target.save()
            else:
                write_head(Path(target.local_path).parent / target.basename.replace('.fits', '.head'), w, info['rms'])
    return [info for _, info in solutions]
