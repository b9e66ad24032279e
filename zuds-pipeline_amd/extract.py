"""Source extraction (``zm_extract``): object table + segmentation map of one image.

The GPU counterpart of the SExtractor run behind ``PipelineFITSCatalog.from_image`` (``zuds/catalog.py:96-130``);
the operator is stated in DESIGN.md ("Source extraction").  ``Engine.extract`` takes host arrays,
``Engine.extract_dev`` device planes (a ``DeviceSubtraction``'s resident difference, noise and mask planes); both are
attached to ``Engine`` when ``engine.py`` is imported (its last line imports this module).  Like every call on an engine,
they use the context's one stream and scratch buffers: one call at a time per engine.
"""
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import as_f32, as_i32, check, ptr, wcs_struct
from .engine import Engine

__all__ = ['CATALOG_COLUMNS', 'extract_params', 'TooManyDetectionsError']

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


def rows_to_table(rows, n):
    """numpy record array with the catalog's column names from the first n rows of a zm_object array."""
    raw = np.frombuffer(rows, dtype=np.dtype(_lib.zm_object), count=n) if n else np.zeros(0, np.dtype(_lib.zm_object))
    tab = np.zeros(n, dtype=TABLE_DTYPE)
    for col, field, _ in CATALOG_COLUMNS:
        tab[col] = raw[field]
    return tab.view(np.recarray)


def _call(self, fn, what, img, sigma, bad, flag, nx, ny, wcs, params, max_objects, segm, filtered):
    # the row array is kept between calls (12 MB at the default capacity: allocating and clearing it takes longer than
    # the extraction of a frame), one per calling thread: threads that share an engine do not share rows
    nrows = max(int(max_objects), 1)
    cache = self.__dict__.setdefault('_extract_rows', {})
    rows = cache.get(threading.get_ident())
    if rows is None or len(rows) < nrows:
        rows = cache[threading.get_ident()] = (_lib.zm_object * nrows)()
    nw, nf, st = C.c_int(), C.c_int(), C.c_int()
    w = wcs_struct(wcs) if wcs is not None else None
    check(fn(self._ctx, img, sigma, bad, flag, nx, ny, C.byref(w) if w is not None else None, C.byref(params),
             int(max_objects), C.cast(rows, C.c_void_p), segm, filtered, C.byref(nw), C.byref(nf), C.byref(st)), what)
    return rows_to_table(rows, nw.value), nf.value, st.value


def _engine_extract(self, img, sigma, bad=None, flag=None, wcs=None, max_objects=MAX_OBJECTS, full=False, **params):
    """Object table (numpy record array, columns ``CATALOG_COLUMNS``) and segmentation map (int32, 0 = sky) of ``img``
    (background already subtracted) with per-pixel noise ``sigma``, bad-pixel map ``bad`` and flag plane ``flag``.

    ``params``: detect_thresh, detect_minarea, filter, satur_level, aper_radius.  More than ``max_objects`` objects:
    the table holds the first ones in NUMBER order, the map all of them.  ``full=True`` returns a dict with the
    filtered plane, the number found and the status word as well."""
    img, sigma, flag = as_f32(img), as_f32(sigma), as_i32(flag)
    ny, nx = img.shape
    if sigma.shape != img.shape:
        raise ValueError(f'sigma has shape {sigma.shape}, expected {img.shape}')
    if bad is not None:
        bad = np.ascontiguousarray(np.asarray(bad) != 0).view(np.uint8)
    for a, nm in ((bad, 'bad'), (flag, 'flag')):
        if a is not None and a.shape != img.shape:
            raise ValueError(f'{nm} has shape {a.shape}, expected {img.shape}')
    p = extract_params(**params)
    segm = np.empty((ny, nx), np.int32)
    filt = np.empty((ny, nx), np.float32) if full else None
    tab, nfound, status = _call(self, self.L.zm_extract, 'zm_extract', ptr(img), ptr(sigma), ptr(bad), ptr(flag), nx, ny,
                                wcs, p, max_objects, ptr(segm), ptr(filt))
    if full:
        return dict(table=tab, segm=segm, filtered=filt, nfound=nfound, status=status)
    return tab, segm


def _engine_extract_dev(self, img, sigma, bad, flag, nx, ny, wcs=None, max_objects=MAX_OBJECTS, segm=None, **params):
    """The same on device planes (addresses: float32 img, sigma; uint8 bad or None; int32 flag or None; ``segm``: an
    int32 device plane that takes the segmentation map, or None).  Returns (table, number found)."""
    p = extract_params(**params)
    tab, nfound, _ = _call(self, self.L.zm_extract_dev, 'zm_extract_dev', int(img), int(sigma), int(bad) if bad else None,
                           int(flag) if flag else None, int(nx), int(ny), wcs, p, max_objects,
                           int(segm) if segm else None, None)
    return tab, nfound


Engine.extract = _engine_extract
Engine.extract_dev = _engine_extract_dev
