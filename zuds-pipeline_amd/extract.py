"""Source extraction (``zm_extract``): object table + segmentation map of one image.

The GPU counterpart of the SExtractor run behind ``PipelineFITSCatalog.from_image`` (``zuds/catalog.py:96-130``);
the operator is stated in DESIGN.md ("Source extraction").  ``Engine.extract`` takes host arrays,
``Engine.extract_dev`` device planes (a ``DeviceSubtraction``'s resident difference, noise and mask planes); both are
attached to ``Engine`` when ``engine.py`` is imported (its last line imports this module).  Like every call on an engine,
they use the context's one stream and scratch buffers: one call at a time per engine.

Two steps of ``sextractor.conf`` are opt-in keywords of both calls: ``deblend=True | dict(nthresh=, mincont=)``
(multi-threshold deblending; the table gains PARENT_NUMBER) and ``clean=True | dict(param=)`` (the CLEAN pass on the
objects of the pass before; the table gains NMERGED).  ``Engine.clean_decide`` is CLEAN's decision alone on a table,
``Engine.clean_stats`` the per-object sums of the last ``clean=`` call.  A third, ``MASK_TYPE``, belongs to the wide
table: ``columns='param', mask='blank' | 'correct'`` runs the masked second pass (``zm_extract_measure_masked``; the table
gains ``MASK_COLUMNS`` and its FLUX_APER / FLUXERR_APER are the masked values).
"""
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import as_f32, as_i32, check, ptr, wcs_struct
from .engine import Engine

__all__ = ['CATALOG_COLUMNS', 'PARAM_COLUMNS', 'extract_params', 'measure_params', 'deblend_params', 'deblend_settings',
           'clean_params', 'clean_settings', 'mask_params', 'mask_setting', 'MASK_COLUMNS', 'TooManyDetectionsError']

# column of the catalog <- field of zm_object (include/zudsmi.h); columns that are not computed are absent
CATALOG_COLUMNS = [('NUMBER', 'number', 'i4'), ('X_IMAGE', 'x_image', 'f8'), ('Y_IMAGE', 'y_image', 'f8'),
                   ('X_WORLD', 'x_world', 'f8'), ('Y_WORLD', 'y_world', 'f8'),
                   ('XMIN_IMAGE', 'xmin', 'i4'), ('XMAX_IMAGE', 'xmax', 'i4'), ('YMIN_IMAGE', 'ymin', 'i4'),
                   ('YMAX_IMAGE', 'ymax', 'i4'), ('ISOAREA_IMAGE', 'npix', 'i4'),
                   ('A_IMAGE', 'a_image', 'f8'), ('B_IMAGE', 'b_image', 'f8'), ('THETA_IMAGE', 'theta_image', 'f8'),
                   ('ELONGATION', 'elongation', 'f8'), ('FWHM_IMAGE', 'fwhm_image', 'f8'),
                   ('FLUX_ISO', 'flux_iso', 'f8'), ('FLUX_MAX', 'flux_max', 'f8'),
                   ('FLUX_APER', 'flux_aper', 'f8'), ('FLUXERR_APER', 'fluxerr_aper', 'f8'),
                   ('FLAGS', 'flags', 'i4'), ('FLAGS_WEIGHT', 'flags_weight', 'i4'),
                   ('IMAFLAGS_ISO', 'imaflags_iso', 'i4')]
TABLE_DTYPE = np.dtype([(c, t) for c, _, t in CATALOG_COLUMNS])
MAX_OBJECTS = 1 << 16
# the wide table (columns='param'): every column of zuds/astromatic/sextractor.param, and the three columns that say how
# the Kron and windowed values were reached; column <- field of zm_object_ext
EXT_COLUMNS = [('MAG_AUTO', 'mag_auto', 'f8'), ('MAGERR_AUTO', 'magerr_auto', 'f8'),
               ('FLUX_AUTO', 'flux_auto', 'f8'), ('FLUXERR_AUTO', 'fluxerr_auto', 'f8'),
               ('XWIN_IMAGE', 'xwin_image', 'f8'), ('YWIN_IMAGE', 'ywin_image', 'f8'),
               ('XWIN_WORLD', 'xwin_world', 'f8'), ('YWIN_WORLD', 'ywin_world', 'f8'),
               ('AWIN_IMAGE', 'awin_image', 'f8'), ('BWIN_IMAGE', 'bwin_image', 'f8'),
               ('ERRAWIN_IMAGE', 'errawin_image', 'f8'), ('ERRBWIN_IMAGE', 'errbwin_image', 'f8'),
               ('ERRTHETAWIN_IMAGE', 'errthetawin_image', 'f8'),
               ('ERRA_WORLD', 'erra_world', 'f8'), ('ERRB_WORLD', 'errb_world', 'f8'),
               ('ERRTHETA_WORLD', 'errtheta_world', 'f8'),
               ('KRON_RADIUS', 'kron_radius', 'f8'), ('FLAGS_AUTO', 'flags_auto', 'i4'), ('FLAGS_WIN', 'flags_win', 'i4')]
PARAM_COLUMNS = CATALOG_COLUMNS + EXT_COLUMNS
PARAM_DTYPE = np.dtype([(c, t) for c, _, t in PARAM_COLUMNS])
COLUMN_SETS = ('isophotal', 'param')
# what a masked second pass (mask='blank' | 'correct') adds to the wide table; column <- field of zm_object_mask
MASK_COLUMNS = [('NREPL_AUTO', 'nrepl_auto', 'i4'), ('NLOST_AUTO', 'nlost_auto', 'i4'),
                ('NREPL_APER', 'nrepl_aper', 'i4'), ('NLOST_APER', 'nlost_aper', 'i4'),
                ('NREPL_WIN', 'nrepl_win', 'i4'), ('NLOST_WIN', 'nlost_win', 'i4')]
MASK_TYPES = {'blank': _lib.MASK_BLANK, 'correct': _lib.MASK_CORRECT}


class TooManyDetectionsError(Exception):
    """More objects than a caller is prepared to take (``scripts/dosub.py:121`` of the reference)."""


def extract_params(detect_thresh=1.5, detect_minarea=5, filter=True, satur_level=50000.0, aper_radius=3.0):
    """zm_extract_params with the values of sextractor.conf."""
    p = _lib.zm_extract_params()
    _lib.lib().zm_extract_params_default(C.byref(p))
    p.detect_thresh = float(detect_thresh)
    p.detect_minarea = int(detect_minarea)
    p.filter = int(bool(filter))
    p.satur_level = float(satur_level)
    p.aper_radius = float(aper_radius)
    return p


def measure_params(kron_fact=2.5, kron_min_radius=3.5, filter=True):
    """zm_measure_params with the PHOT_AUTOPARAMS of sextractor.conf; ``filter``: as the extraction that made the rows."""
    p = _lib.zm_measure_params()
    _lib.lib().zm_measure_params_default(C.byref(p))
    p.kron_fact = float(kron_fact)
    p.kron_min_radius = float(kron_min_radius)
    p.filter = int(bool(filter))
    return p


DEBLEND_DEFAULTS = dict(nthresh=32, mincont=0.005)      # DEBLEND_NTHRESH, DEBLEND_MINCONT of sextractor.conf


def deblend_settings(deblend=True):
    """``None`` (no deblending) or dict(nthresh=, mincont=) from ``deblend=False | True | dict(nthresh=, mincont=)``.
    ``nthresh`` must be a power of two in 2 .. 64 and ``mincont`` lie in [0, 1]; anything else raises ValueError."""
    if deblend is None or deblend is False:
        return None
    kw = {} if deblend is True else dict(deblend)
    unknown = set(kw) - set(DEBLEND_DEFAULTS)
    if unknown:
        raise ValueError(f'deblend: unknown keys {sorted(unknown)} (nthresh, mincont)')
    nthresh, mincont = kw.get('nthresh', DEBLEND_DEFAULTS['nthresh']), float(kw.get('mincont', DEBLEND_DEFAULTS['mincont']))
    if int(nthresh) != nthresh or not 2 <= int(nthresh) <= 64 or int(nthresh) & (int(nthresh) - 1):
        raise ValueError(f'deblend: nthresh={nthresh!r} must be a power of two in 2 .. 64')
    if not 0.0 <= mincont <= 1.0:
        raise ValueError(f'deblend: mincont={mincont!r} must lie in [0, 1]')
    return dict(nthresh=int(nthresh), mincont=mincont)


def deblend_params(deblend=True):
    """``None`` or the zm_deblend_params of ``deblend_settings(deblend)``."""
    kw = deblend_settings(deblend)
    if kw is None:
        return None
    p = _lib.zm_deblend_params()
    _lib.lib().zm_deblend_params_default(C.byref(p))
    p.nthresh, p.mincont = kw['nthresh'], kw['mincont']
    return p


CLEAN_DEFAULTS = dict(param=1.0)                        # CLEAN_PARAM of sextractor.conf


def clean_settings(clean=True):
    """``None`` (no CLEAN pass) or dict(param=) from ``clean=False | True | dict(param=)``.  ``param`` must be finite and
    lie in [0.1, 10]; anything else raises ValueError."""
    if clean is None or clean is False:
        return None
    kw = {} if clean is True else dict(clean)
    unknown = set(kw) - set(CLEAN_DEFAULTS)
    if unknown:
        raise ValueError(f'clean: unknown keys {sorted(unknown)} (param)')
    try:
        param = float(kw.get('param', CLEAN_DEFAULTS['param']))
    except (TypeError, ValueError):
        raise ValueError(f'clean: param={kw.get("param")!r} must be a number in [0.1, 10]') from None
    if not (np.isfinite(param) and 0.1 <= param <= 10.0):
        raise ValueError(f'clean: param={param!r} must be finite and lie in [0.1, 10]')
    return dict(param=param)


def clean_params(clean=True):
    """``None`` or the zm_clean_params of ``clean_settings(clean)``."""
    kw = clean_settings(clean)
    if kw is None:
        return None
    p = _lib.zm_clean_params()
    _lib.lib().zm_clean_params_default(C.byref(p))
    p.param = kw['param']
    return p


def mask_setting(mask=None):
    """``None`` (the plain second pass) or 'blank' / 'correct' from ``mask=None | 'none' | 'blank' | 'correct'`` (any
    case: MASK_TYPE of sextractor.conf is upper case); anything else raises ValueError."""
    if mask is None or mask is False:
        return None
    if isinstance(mask, str) and mask.strip().lower() == 'none':
        return None
    if not isinstance(mask, str) or mask.strip().lower() not in MASK_TYPES:
        raise ValueError(f"mask={mask!r}: None, 'blank' or 'correct'")
    return mask.strip().lower()


def mask_params(mask, aper_radius=3.0):
    """``None`` or the zm_mask_params of ``mask_setting(mask)`` with the aperture radius of the first pass."""
    kind = mask_setting(mask)
    if kind is None:
        return None
    p = _lib.zm_mask_params()
    _lib.lib().zm_mask_params_default(C.byref(p))
    p.type, p.aper_radius = MASK_TYPES[kind], float(aper_radius)
    return p


def extract_options(columns='isophotal', deblend=False, clean=False, mask=None):
    """The one place the options of an extraction are validated: (columns, ``deblend_settings(deblend)``,
    ``clean_settings(clean)``, ``mask_setting(mask)``).  ``columns`` must be one of ``COLUMN_SETS`` and a mask needs the wide
    table; anything else raises ValueError."""
    if columns not in COLUMN_SETS:
        raise ValueError(f'columns={columns!r}: one of {COLUMN_SETS}')
    kind = mask_setting(mask)
    if kind is not None and columns != 'param':
        raise ValueError(f"mask={mask!r} needs columns='param': masking belongs to the second pass")
    return columns, deblend_settings(deblend), clean_settings(clean), kind


def with_columns(tab, columns):
    """``tab`` with more columns behind its own: ``columns`` is a list of (name, type, values); values beyond the table's
    length are left out."""
    out = np.zeros(len(tab), dtype=np.dtype(tab.dtype.descr + [(name, t) for name, t, _ in columns]))
    for c in tab.dtype.names:
        out[c] = tab[c]
    for name, _, values in columns:
        out[name] = values[:len(tab)]
    return out.view(np.recarray)


def with_column(tab, name, values):
    """``tab`` with one more int32 column."""
    return with_columns(tab, [(name, 'i4', values)])


def with_parent(tab, parent):
    """``tab`` with a PARENT_NUMBER column (int32: the first-pass NUMBER of the object a row was part of)."""
    return with_column(tab, 'PARENT_NUMBER', parent)


def _split_params(columns, params, mask=None):
    """(extraction keywords, zm_measure_params or None, zm_mask_params or None) of a call's ``columns``, keyword
    arguments and ``mask``."""
    columns, _, _, kind = extract_options(columns, mask=mask)
    params = dict(params)
    if columns != 'param':
        return params, None, None
    mp = measure_params(params.pop('kron_fact', 2.5), params.pop('kron_min_radius', 3.5), params.get('filter', True))
    return params, mp, mask_params(kind, params.get('aper_radius', 3.0))


def ext_to_table(rows, ext, n):
    """The wide table (``PARAM_COLUMNS``) from the first n rows of a zm_object array and of its zm_object_ext array."""
    raw = np.frombuffer(rows, dtype=np.dtype(_lib.zm_object), count=n) if n else np.zeros(0, np.dtype(_lib.zm_object))
    rext = np.frombuffer(ext, dtype=np.dtype(_lib.zm_object_ext), count=n) if n else np.zeros(0, np.dtype(_lib.zm_object_ext))
    tab = np.zeros(n, dtype=PARAM_DTYPE)
    for col, field, _ in CATALOG_COLUMNS:
        tab[col] = raw[field]
    for col, field, _ in EXT_COLUMNS:
        tab[col] = rext[field]
    return tab.view(np.recarray), rext.copy().view(np.recarray)


def masked_table(rows, ext, msk, n):
    """The wide table of a masked second pass from the first n rows of a zm_object array, its zm_object_ext array and its
    zm_object_mask array: FLUX_APER / FLUXERR_APER are the masked values, FLAGS gains bit 1 where ``crowded`` is set, and
    ``MASK_COLUMNS`` are added.  Returns (table, ext rows, mask rows)."""
    wide, rext = ext_to_table(rows, ext, n)
    rmsk = np.frombuffer(msk, dtype=np.dtype(_lib.zm_object_mask), count=n) if n else np.zeros(0, np.dtype(_lib.zm_object_mask))
    tab = with_columns(wide, [(col, t, rmsk[field]) for col, field, t in MASK_COLUMNS])
    tab['FLUX_APER'], tab['FLUXERR_APER'] = rmsk['flux_aper'], rmsk['fluxerr_aper']
    tab['FLAGS'] |= (rmsk['crowded'] != 0).astype(np.int32)
    return tab, rext, rmsk.copy().view(np.recarray)


def _measure(self, dev, img, sigma, bad, segm, nx, ny, wcs, mp, n, mk=None):
    """The second pass on the rows the extraction of this thread has just written: (wide table, zm_object_ext rows,
    zm_object_mask rows or None).  ``dev``: device planes; ``mk``: the zm_mask_params of a masked pass."""
    rows = self.__dict__['_extract_rows'][threading.get_ident()]
    ext = (_lib.zm_object_ext * max(n, 1))()
    w = wcs_struct(wcs) if wcs is not None else None
    what = 'zm_extract_measure' + ('_masked' if mk is not None else '') + ('_dev' if dev else '')
    args = (self._ctx, img, sigma, bad, segm, nx, ny, C.byref(w) if w is not None else None, C.byref(mp), int(n),
            C.cast(rows, C.c_void_p), C.cast(ext, C.c_void_p))
    if mk is None:
        check(getattr(self.L, what)(*args), what)
        return ext_to_table(rows, ext, n) + (None,)
    msk = (_lib.zm_object_mask * max(n, 1))()
    check(getattr(self.L, what)(*args, C.byref(mk), C.cast(msk, C.c_void_p)), what)
    return masked_table(rows, ext, msk, n)


def rows_to_table(rows, n):
    """numpy record array with the catalog's column names from the first n rows of a zm_object array."""
    raw = np.frombuffer(rows, dtype=np.dtype(_lib.zm_object), count=n) if n else np.zeros(0, np.dtype(_lib.zm_object))
    tab = np.zeros(n, dtype=TABLE_DTYPE)
    for col, field, _ in CATALOG_COLUMNS:
        tab[col] = raw[field]
    return tab.view(np.recarray)


# (clean set, deblend set) -> the entry point of the first pass; the device-plane forms end in _dev
ENTRY_POINTS = {(False, False): 'zm_extract', (False, True): 'zm_extract_deblend',
                (True, False): 'zm_extract_clean', (True, True): 'zm_extract_clean'}


def _call(self, dev, img, sigma, bad, flag, nx, ny, wcs, params, max_objects, segm, filtered, deblend=None, clean=None):
    """The first pass: (table, number found, status word).  ``deblend`` / ``clean``: zm_deblend_params / zm_clean_params
    or None; the deblending form takes two more arguments and gives one more column (PARENT_NUMBER), the CLEAN form takes
    both parameter blocks and gives NMERGED always, PARENT_NUMBER only with deblending."""
    # the row array is kept between calls (12 MB at the default capacity: allocating and clearing it takes longer than
    # the extraction of a frame), one per calling thread: threads that share an engine do not share rows
    nrows = max(int(max_objects), 1)
    cache = self.__dict__.setdefault('_extract_rows', {})
    rows = cache.get(threading.get_ident())
    if rows is None or len(rows) < nrows:
        rows = cache[threading.get_ident()] = (_lib.zm_object * nrows)()
    nw, nf, st = C.c_int(), C.c_int(), C.c_int()
    w = wcs_struct(wcs) if wcs is not None else None
    what = ENTRY_POINTS[clean is not None, deblend is not None] + ('_dev' if dev else '')
    more, carried = [], []
    if deblend is not None or clean is not None:
        parent = np.zeros(nrows, np.int32)
        more = [C.byref(deblend) if deblend is not None else None, ptr(parent)]
        if deblend is not None:
            carried.append(('PARENT_NUMBER', 'i4', parent))
    if clean is not None:
        nmerged = np.zeros(nrows, np.int32)
        more = [more[0], C.byref(clean), more[1], ptr(nmerged)]
        carried.append(('NMERGED', 'i4', nmerged))
    check(getattr(self.L, what)(self._ctx, img, sigma, bad, flag, nx, ny, C.byref(w) if w is not None else None,
                                C.byref(params), int(max_objects), C.cast(rows, C.c_void_p), segm, filtered, C.byref(nw),
                                C.byref(nf), C.byref(st), *more), what)
    tab = rows_to_table(rows, nw.value)
    return (with_columns(tab, carried) if carried else tab), nf.value, st.value


def _passes(self, dev, options, img, sigma, bad, flag, nx, ny, wcs, max_objects, segm, filtered):
    """What ``Engine.extract`` (``dev`` False: host arrays as pointers) and ``Engine.extract_dev`` (device addresses) share:
    the first pass, the second pass where ``columns='param'`` asked for one, and the columns of the first pass that the
    wide table carries on.  ``options``: what ``_options`` returned.  Returns a dict with the keys of ``full=True`` but
    the planes."""
    p, mp, mk, db, cl = options
    tab, nfound, status = _call(self, dev, img, sigma, bad, flag, nx, ny, wcs, p, max_objects, segm, filtered, db, cl)
    out = dict(nfound=nfound, status=status)
    if mp is not None:
        first = tab
        tab, out['ext'], maskrows = _measure(self, dev, img, sigma, bad, segm, nx, ny, wcs, mp, len(tab), mk)
        if mk is not None:
            out['maskrows'] = maskrows
        carried = [(c, 'i4', first[c]) for c in ('PARENT_NUMBER', 'NMERGED') if c in first.dtype.names]
        if carried:
            tab = with_columns(tab, carried)
    out['table'] = tab
    return out


def _options(columns, deblend, clean, mask, params):
    """(zm_extract_params, zm_measure_params or None, zm_mask_params or None, zm_deblend_params or None, zm_clean_params or
    None) of a call's keywords."""
    params, mp, mk = _split_params(columns, params, mask)
    db, cl = deblend_params(deblend), clean_params(clean)
    return extract_params(**params), mp, mk, db, cl


def _engine_extract(self, img, sigma, bad=None, flag=None, wcs=None, max_objects=MAX_OBJECTS, full=False,
                    columns='isophotal', deblend=False, clean=False, mask=None, **params):
    """Object table (numpy record array, columns ``CATALOG_COLUMNS``) and segmentation map (int32, 0 = sky) of ``img``
    (background already subtracted) with per-pixel noise ``sigma``, bad-pixel map ``bad`` and flag plane ``flag``.

    ``params``: detect_thresh, detect_minarea, filter, satur_level, aper_radius.  More than ``max_objects`` objects:
    the table holds the first ones in NUMBER order, the map all of them.  ``full=True`` returns a dict with the
    filtered plane, the number found and the status word as well.

    ``columns='param'``: the wide table (``PARAM_COLUMNS``: every column of sextractor.param) from a second pass,
    ``zm_extract_measure``; ``params`` may then carry kron_fact and kron_min_radius (PHOT_AUTOPARAMS), and ``full=True``
    adds ``ext``, the rows of that pass with every intermediate value.

    ``deblend=True`` or ``dict(nthresh=, mincont=)``: multi-threshold deblending (``zm_extract_deblend``; DESIGN.md,
    "Deblending").  Objects are numbered after the split, sub-objects of a split parent carry FLAGS bit 2, and the table
    gains the column PARENT_NUMBER.  Where nothing splits, table and map are those of the default call.

    ``clean=True`` or ``dict(param=)``: the CLEAN pass (``zm_extract_clean``; DESIGN.md, "CLEAN") on the objects of the
    pass before, deblended or not: an object whose neighbour's wing explains it is folded into that neighbour, the merged
    objects are renumbered and measured on the union of their pixels, and the table gains the column NMERGED (objects
    from before CLEAN in the row; 1 = untouched).  Where nothing is absorbed, table and map are those of the same call
    without ``clean``.

    ``mask='blank'`` or ``'correct'`` (needs ``columns='param'``): MASK_TYPE of sextractor.conf for the second pass
    (``zm_extract_measure_masked``; DESIGN.md, "MASK_TYPE").  The Kron, windowed and aperture sums leave out the pixels of
    other objects and the object's own bad pixels, or under ``'correct'`` take their mirror about the centre instead.
    FLUX_APER / FLUXERR_APER are then the masked values, FLAGS gains bit 1 where a tenth of a footprint was replaced or
    lost, the table gains ``MASK_COLUMNS``, and ``full=True`` adds ``maskrows`` (the zm_object_mask rows).  The map
    is the final one, after ``deblend`` and ``clean``."""
    options = _options(columns, deblend, clean, mask, params)
    img, sigma, flag = as_f32(img), as_f32(sigma), as_i32(flag)
    ny, nx = img.shape
    if sigma.shape != img.shape:
        raise ValueError(f'sigma has shape {sigma.shape}, expected {img.shape}')
    if bad is not None:
        bad = np.ascontiguousarray(np.asarray(bad) != 0).view(np.uint8)
    for a, nm in ((bad, 'bad'), (flag, 'flag')):
        if a is not None and a.shape != img.shape:
            raise ValueError(f'{nm} has shape {a.shape}, expected {img.shape}')
    segm = np.empty((ny, nx), np.int32)
    filt = np.empty((ny, nx), np.float32) if full else None
    out = _passes(self, False, options, ptr(img), ptr(sigma), ptr(bad), ptr(flag), nx, ny, wcs, max_objects, ptr(segm),
                  ptr(filt))
    if full:
        return dict(table=out.pop('table'), segm=segm, filtered=filt, **out)
    return out['table'], segm


def _engine_extract_dev(self, img, sigma, bad, flag, nx, ny, wcs=None, max_objects=MAX_OBJECTS, segm=None,
                        columns='isophotal', deblend=False, clean=False, mask=None, **params):
    """The same on device planes (addresses: float32 img, sigma; uint8 bad or None; int32 flag or None; ``segm``: an
    int32 device plane that takes the segmentation map, or None).  Returns (table, number found).
    ``columns='param'`` needs the segmentation map for its second pass: without ``segm`` a plane is allocated for the
    call.  ``deblend``, ``clean``, ``mask``: as for ``Engine.extract``."""
    options = _options(columns, deblend, clean, mask, params)
    own = None
    if options[1] is not None and not segm:
        from . import hipmem
        own = hipmem.DeviceBuffer(int(nx) * int(ny) * 4)         # (freed when this call returns)
        segm = own.ptr
    out = _passes(self, True, options, int(img), int(sigma), int(bad) if bad else None, int(flag) if flag else None,
                  int(nx), int(ny), wcs, max_objects, int(segm) if segm else None, None)
    return out['table'], out['nfound']


def _engine_clean_stats(self):
    """(F, T, m) of every object from before CLEAN of this engine's last ``clean=`` call (``zm_extract_clean_stats``):
    float64 sum of the filtered values, float32 threshold at the peak pixel, float32 DETECT_MINAREA-th largest excess over
    the local threshold."""
    n = C.c_int()
    check(self.L.zm_extract_clean_stats(self._ctx, 0, None, None, None, C.byref(n)), 'zm_extract_clean_stats')
    F, T, m = np.zeros(n.value, np.float64), np.zeros(n.value, np.float32), np.zeros(n.value, np.float32)
    if n.value:
        check(self.L.zm_extract_clean_stats(self._ctx, n.value, ptr(F), ptr(T), ptr(m), C.byref(n)), 'zm_extract_clean_stats')
    return F, T, m


def _engine_clean_decide(self, rows, fdflux, dthresh, mthresh, minarea=5, clean=True):
    """(into, root) of ``zm_clean_decide``: the CLEAN decision alone on a table.  ``rows``: a numpy array of dtype
    ``np.dtype(_lib.zm_object)`` (number = index + 1); the NUMBER of the absorber of every object (0: none) and the NUMBER at
    the end of its chain."""
    rows = np.ascontiguousarray(rows, np.dtype(_lib.zm_object))
    n = len(rows)
    F, T, m = (np.ascontiguousarray(a, dt) for a, dt in ((fdflux, np.float64), (dthresh, np.float32), (mthresh, np.float32)))
    if not len(F) == len(T) == len(m) == n:
        raise ValueError('clean_decide: rows, fdflux, dthresh and mthresh differ in length')
    cl = clean_params(clean)
    if cl is None:
        raise ValueError('clean_decide: clean must be True or dict(param=)')
    into, root = np.zeros(n, np.int32), np.zeros(n, np.int32)
    check(self.L.zm_clean_decide(self._ctx, n, ptr(rows), ptr(F), ptr(T), ptr(m), int(minarea), C.byref(cl), ptr(into),
                                 ptr(root)), 'zm_clean_decide')
    return into, root


Engine.extract = _engine_extract
Engine.clean_stats = _engine_clean_stats
Engine.clean_decide = _engine_clean_decide
Engine.extract_dev = _engine_extract_dev
