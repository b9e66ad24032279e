"""Catalogue cross-matches of an alert (``zuds/crossmatch.py``), batched, against local tables that stay in HBM.

The reference runs five cone searches per detection through remote services: the three nearest PS1 and LegacySurvey DR8
rows within 30 arcsec, and every ZTF alert, milliquas and TNS row within 1.5 arcsec.  Here a table is an
``ExternalCatalog`` - columns in host memory, positions in a ``SkyIndex`` that is built once and stays on the device
(``csrc/skyindex.hip``) - and ``xmatch`` takes all positions of a batch at once: one ``knn`` launch per k-nearest table,
one ``within`` per name table.  No network, no database.  DESIGN.md, "Alert packets".

Two places where the reference's code contradicts its own documentation are decided here:

* ``ps1()`` sorts the distances but takes ids and magnitudes from the unsorted list (``matches[ii]``,
  ``crossmatch.py:156-182``).  Here every field of slot i comes from the i-th nearest row.
* ``legacysurvey()`` orders by ``rank desc limit 3``: the three FARTHEST.  Here it is the three nearest, ascending, as the
  schema's field documentation says.
"""
import ctypes as C

import numpy as np

from ._lib import check
from .engine import get_engine

__all__ = ['SkyIndex', 'ExternalCatalog', 'abmag', 'ps1', 'legacysurvey', 'ztfalerts', 'milliquas', 'tns', 'xmatch',
           'KNN_RADIUS_ARCSEC', 'NAME_RADIUS_ARCSEC', 'KNN_K', 'CATALOG_COLUMNS', 'NAME_FIELDS']

KNN_RADIUS_ARCSEC = 30.0              # ps1, legacysurvey: the nearest three within (crossmatch.py:114)
NAME_RADIUS_ARCSEC = 1.5              # ztfalerts, milliquas, tns: every row within (crossmatch.py:265)
KNN_K = 3
KMAX = 8

# payload columns of every table (beside ra and dec)
LS_COLUMNS = ('OBJID', 'TYPE', 'EBV', 'FLUX_G', 'FLUX_R', 'FLUX_Z', 'FLUX_W1', 'FLUX_W2', 'FLUX_W3', 'FLUX_W4',
              'GAIA_PHOT_G_MEAN_MAG', 'PARALLAX', 'z_phot_mean', 'z_phot_median', 'z_phot_std', 'z_phot_l68', 'z_phot_u68',
              'z_phot_l95', 'z_phot_u95', 'z_spec')
CATALOG_COLUMNS = {
    'ps1': ('objid', 'gMeanPSFMag', 'rMeanPSFMag', 'iMeanPSFMag', 'zMeanPSFMag', 'ps_score'),
    'legacysurvey': LS_COLUMNS,
    'ztfalerts': ('objectId',),
    'milliquas': ('Name',),
    'tns': ('name',),
}
# candidate field of each name table, and the column it joins
NAME_FIELDS = {'ztfalerts': ('ztfname', 'objectId'), 'milliquas': ('mqid', 'Name'), 'tns': ('tnsid', 'name')}


def _f64(a, what, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 1 or (n is not None and a.size != n):
        raise ValueError(f'{what} must be a vector' + (f' of {n} values' if n is not None else '') + f', got shape {a.shape}')
    return a


def _dev_f64(t, what, n=None):
    import torch
    if t.dtype != torch.float64 or t.dim() != 1 or not t.is_contiguous() or not t.is_cuda or (n is not None and t.numel() != n):
        raise ValueError(f'{what} must be a contiguous float64 device vector' + (f' of {n} values' if n is not None else ''))
    return t


class SkyIndex(object):
    """A catalogue's positions, indexed once for cone searches of at most ``max_radius_arcsec`` and resident on the
    device until ``close()`` (``zm_skyindex_create``).  ``ra``, ``dec``: degrees, arrays or float64 device tensors; a row
    that is not finite is matched by nothing."""

    def __init__(self, ra, dec, max_radius_arcsec, engine=None):
        self.engine = engine or get_engine()
        self.max_radius_arcsec = float(max_radius_arcsec)
        self._h = C.c_void_p()
        L, ctx = self.engine.L, self.engine.ctx
        if hasattr(ra, 'data_ptr'):
            _dev_f64(ra, 'ra'), _dev_f64(dec, 'dec', ra.numel())
            self.m = int(ra.numel())
            check(L.zm_skyindex_create_dev(ctx, self.m, ra.data_ptr(), dec.data_ptr(), self.max_radius_arcsec, C.byref(self._h)),
                  'zm_skyindex_create_dev')
        else:
            ra = _f64(ra, 'ra')
            dec = _f64(dec, 'dec', ra.size)
            self.m = int(ra.size)
            check(L.zm_skyindex_create(ctx, self.m, ra.ctypes.data, dec.ctypes.data, self.max_radius_arcsec, C.byref(self._h)),
                  'zm_skyindex_create')

    def _handle(self):
        if not self._h:
            raise ValueError('the index is closed')
        return self._h

    def close(self):
        if getattr(self, '_h', None):
            self.engine.L.zm_skyindex_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def stats(self):
        """``rows`` indexed (the finite ones), ``cells`` in use, ``capacity`` of the cell table and the longest probe
        ``probe_max`` of one insertion (``zm_skyindex_stats``)."""
        out = (C.c_int64 * 4)()
        check(self.engine.L.zm_skyindex_stats(self._handle(), out), 'zm_skyindex_stats')
        return dict(rows=int(out[0]), cells=int(out[1]), capacity=int(out[2]), probe_max=int(out[3]))

    def knn(self, ra, dec, radius_arcsec, k):
        """The ``k`` (1 .. 8) nearest rows within ``radius_arcsec`` (inclusive) of every position: ``(idx int32 [n, k],
        sep float64 [n, k], count int32 [n])``.  A row of ``idx`` ascends by (separation, catalogue row); slots that are
        not filled hold ``-1`` / ``NaN``; ``count`` is the number of rows within the radius and may exceed ``k``."""
        ra = _f64(ra, 'ra')
        dec = _f64(dec, 'dec', ra.size)
        k = int(k)
        n, kk = ra.size, max(1, min(k, KMAX))
        idx = np.full((n, kk), -1, np.int32)
        sep = np.full((n, kk), np.nan, np.float64)
        count = np.zeros(n, np.int32)
        check(self.engine.L.zm_cone_knn(self.engine.ctx, self._handle(), n, ra.ctypes.data, dec.ctypes.data, float(radius_arcsec), k,
                                        idx.ctypes.data, sep.ctypes.data, count.ctypes.data), 'zm_cone_knn')
        return idx, sep, count

    def knn_dev(self, ra, dec, radius_arcsec, k, stream=None):
        """``knn`` on float64 torch tensors in HBM (``zm_cone_knn_dev``): enqueued on the engine's stream (``stream``: the
        torch stream it is bound to), nothing waited for.  Returns device tensors."""
        import torch
        n, k = ra.numel(), int(k)
        _dev_f64(ra, 'ra'), _dev_f64(dec, 'dec', n)
        kk = max(1, min(k, KMAX))
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(ra.device):
            idx = torch.empty((n, kk), dtype=torch.int32, device=ra.device)
            sep = torch.empty((n, kk), dtype=torch.float64, device=ra.device)
            count = torch.empty(n, dtype=torch.int32, device=ra.device)
            check(self.engine.L.zm_cone_knn_dev(self.engine.ctx, self._handle(), n, ra.data_ptr(), dec.data_ptr(),
                                                float(radius_arcsec), k, idx.data_ptr(), sep.data_ptr(), count.data_ptr()),
                  'zm_cone_knn_dev')
        return idx, sep, count

    def within(self, ra, dec, radius_arcsec):
        """Every row within ``radius_arcsec`` (inclusive) of every position: ``(offsets int64 [n + 1], cat_idx int32)``;
        the rows of position ``i`` are ``cat_idx[offsets[i]:offsets[i + 1]]``, ascending.  Called again once, with room
        for all, when the first list was too short."""
        ra = _f64(ra, 'ra')
        dec = _f64(dec, 'dec', ra.size)
        offsets = np.zeros(ra.size + 1, np.int64)
        cap = max(ra.size, 1024)
        while True:
            cat_idx = np.empty(cap, np.int32)
            n = C.c_int64(0)
            check(self.engine.L.zm_cone_within(self.engine.ctx, self._handle(), ra.size, ra.ctypes.data, dec.ctypes.data,
                                               float(radius_arcsec), cap, offsets.ctypes.data, cat_idx.ctypes.data, C.byref(n)),
                  'zm_cone_within')
            if n.value <= cap:
                return offsets, cat_idx[:n.value].copy()
            cap = int(n.value)

    def within_dev(self, ra, dec, radius_arcsec, capacity=None, stream=None):
        """``within`` on float64 torch tensors in HBM (``zm_cone_within_dev``).  Returns device tensors ``(offsets,
        cat_idx)`` and the number of pairs; ``cat_idx`` has ``max(capacity, pairs)`` entries of which the first ``pairs``
        are meaningful (a second call is made when ``capacity`` was too small).  The call waits for the pair count."""
        import torch
        n = ra.numel()
        _dev_f64(ra, 'ra'), _dev_f64(dec, 'dec', n)
        cap = int(capacity) if capacity is not None else max(n, 1024)
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(ra.device):
            offsets = torch.empty(n + 1, dtype=torch.int64, device=ra.device)
            while True:
                cat_idx = torch.empty(max(cap, 1), dtype=torch.int32, device=ra.device)
                np_ = C.c_int64(0)
                check(self.engine.L.zm_cone_within_dev(self.engine.ctx, self._handle(), n, ra.data_ptr(), dec.data_ptr(),
                                                       float(radius_arcsec), cap, offsets.data_ptr(), cat_idx.data_ptr(),
                                                       C.byref(np_)), 'zm_cone_within_dev')
                if np_.value <= cap:
                    return offsets, cat_idx, int(np_.value)
                cap = int(np_.value)


class ExternalCatalog(object):
    """A local copy of one of the tables the reference queries remotely: ``name`` (a key of ``CATALOG_COLUMNS``),
    ``table`` (a mapping of equally long columns: ``ra``, ``dec`` and the payload columns of that table) and the
    ``SkyIndex`` of its positions, built for queries of at most ``max_radius_arcsec``."""

    def __init__(self, name, table, max_radius_arcsec=None, engine=None):
        if name not in CATALOG_COLUMNS:
            raise ValueError(f'unknown catalogue {name!r}: one of {sorted(CATALOG_COLUMNS)}')
        self.name = name
        self.table = {k: np.asarray(table[k]) for k in (table.files if hasattr(table, 'files') else table.keys())}
        missing = [c for c in ('ra', 'dec') + tuple(CATALOG_COLUMNS[name]) if c not in self.table]
        if missing:
            raise ValueError(f'catalogue {name!r}: columns {missing} are missing')
        n = self.table['ra'].shape[0]
        for k, v in self.table.items():
            if v.ndim != 1 or v.shape[0] != n:
                raise ValueError(f'catalogue {name!r}: column {k!r} has shape {v.shape}, ra has {n} rows')
        if max_radius_arcsec is None:
            max_radius_arcsec = NAME_RADIUS_ARCSEC if name in NAME_FIELDS else KNN_RADIUS_ARCSEC
        self.index = SkyIndex(self.table['ra'], self.table['dec'], max_radius_arcsec, engine=engine)

    def __len__(self):
        return int(self.table['ra'].shape[0])

    def close(self):
        self.index.close()

    @classmethod
    def from_npz(cls, path, name=None, max_radius_arcsec=None, engine=None):
        """The table of ``path`` (``NAME.npz``: one array per column, strings as fixed-width unicode; read with
        ``allow_pickle=False``).  ``name`` defaults to the file's base name."""
        import os
        name = name or os.path.splitext(os.path.basename(str(path)))[0]
        with np.load(path, allow_pickle=False) as z:
            return cls(name, {k: z[k] for k in z.files}, max_radius_arcsec, engine=engine)


def abmag(flux):
    """Flux in nanomaggies -> AB magnitude; 0 where the flux is <= 0 (``crossmatch.py:45-50``).  Scalars or arrays."""
    f = np.asarray(flux, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        out = np.where(f > 0, -2.5 * np.log10(np.where(f > 0, f, 1.0)) + 22.5, 0.0)
    return float(out) if out.ndim == 0 else out


def _value(v):
    """A table entry as a plain Python value (what the reference's JSON and SQL rows hold)."""
    v = v.item() if hasattr(v, 'item') else v
    return v.decode() if isinstance(v, bytes) else v


def _knn_of(cat, ra, dec, idx, sep, count, k=KNN_K, radius=KNN_RADIUS_ARCSEC):
    if idx is None:
        idx, sep, count = cat.index.knn(ra, dec, radius, k)
    return np.asarray(idx), np.asarray(sep), np.asarray(count)


def ps1(cat, ra, dec, idx=None, sep=None, count=None):
    """One dict per position with ``objectidps``, ``sgscore``, ``distpsnr``, ``psgmag``, ``psrmag``, ``psimag`` and
    ``pszmag`` 1 .. 3 of the three nearest ``ps1`` rows within 30 arcsec: slot i is the i-th nearest row in every field.
    A slot without a match is absent.  ``idx``, ``sep``, ``count``: the result of ``cat.index.knn`` when the caller has
    it already."""
    idx, sep, count = _knn_of(cat, ra, dec, idx, sep, count)
    t = cat.table
    out = []
    for rows, seps in zip(idx.tolist(), sep.tolist()):
        d = {}
        for ii, (j, s) in enumerate(zip(rows[:KNN_K], seps[:KNN_K])):
            if j < 0:
                break
            n = ii + 1
            d['objectidps%d' % n] = _value(t['objid'][j])
            d['sgscore%d' % n] = float(t['ps_score'][j])
            d['distpsnr%d' % n] = float(s)
            d['psgmag%d' % n] = _value(t['gMeanPSFMag'][j])
            d['psrmag%d' % n] = _value(t['rMeanPSFMag'][j])
            d['psimag%d' % n] = _value(t['iMeanPSFMag'][j])
            d['pszmag%d' % n] = _value(t['zMeanPSFMag'][j])
        out.append(d)
    return out


_LS_MAGS = (('lsg', 'FLUX_G'), ('lsr', 'FLUX_R'), ('lsz', 'FLUX_Z'), ('lsw1_', 'FLUX_W1'), ('lsw2_', 'FLUX_W2'),
            ('lsw3_', 'FLUX_W3'), ('lsw4_', 'FLUX_W4'))
_LS_PLAIN = (('lsgaiag', 'GAIA_PHOT_G_MEAN_MAG'), ('lsgaiap', 'PARALLAX'), ('lszphotmean', 'z_phot_mean'),
             ('lszphotmed', 'z_phot_median'), ('lszphotstd', 'z_phot_std'), ('lszphotl68', 'z_phot_l68'),
             ('lszphotu68', 'z_phot_u68'), ('lszphotl95', 'z_phot_l95'), ('lszphotu95', 'z_phot_u95'), ('lszspec', 'z_spec'))


def legacysurvey(cat, ra, dec, idx=None, sep=None, count=None):
    """One dict per position with the ``ls*`` fields 1 .. 3 of the three NEAREST ``legacysurvey`` rows within 30 arcsec,
    ascending (``crossmatch.py:218-240``; fluxes through ``abmag``).  A slot without a match is absent."""
    idx, sep, count = _knn_of(cat, ra, dec, idx, sep, count)
    t = cat.table
    out = []
    for rows, seps in zip(idx.tolist(), sep.tolist()):
        d = {}
        for ii, (j, s) in enumerate(zip(rows[:KNN_K], seps[:KNN_K])):
            if j < 0:
                break
            n = ii + 1
            d['lsdistnr%d' % n] = float(s)
            d['lsobjectid%d' % n] = _value(t['OBJID'][j])
            d['lstype%d' % n] = str(_value(t['TYPE'][j]))
            d['lsebv%d' % n] = _value(t['EBV'][j])
            for key, col in _LS_MAGS:
                d['%s%d' % (key, n)] = abmag(_value(t[col][j]))
            for key, col in _LS_PLAIN:
                d['%s%d' % (key, n)] = _value(t[col][j])
        out.append(d)
    return out


def _names(cat, column, ra, dec, offsets, cat_idx):
    if offsets is None:
        offsets, cat_idx = cat.index.within(ra, dec, NAME_RADIUS_ARCSEC)
    col = cat.table[column]
    offsets = np.asarray(offsets).tolist()
    return [np.unique(np.asarray(col[np.asarray(cat_idx[a:b], dtype=np.int64)], dtype=str)) for a, b in zip(offsets[:-1], offsets[1:])]


def ztfalerts(cat, ra, dec, offsets=None, cat_idx=None):
    """Per position the ``objectId`` of every ``ztfalerts`` row within 1.5 arcsec: unique and sorted (``np.unique``)."""
    return _names(cat, 'objectId', ra, dec, offsets, cat_idx)


def milliquas(cat, ra, dec, offsets=None, cat_idx=None):
    """Per position the ``Name`` of every ``milliquas`` row within 1.5 arcsec: unique and sorted."""
    return _names(cat, 'Name', ra, dec, offsets, cat_idx)


def tns(cat, ra, dec, offsets=None, cat_idx=None):
    """Per position the ``name`` of every ``tns`` row within 1.5 arcsec: unique and sorted."""
    return _names(cat, 'name', ra, dec, offsets, cat_idx)


def xmatch(ra, dec, catalogs=None):
    """The catalogue fields of the ``candidate`` record for every position (``crossmatch.py:386-412``): one dict each.

    ``catalogs``: ``ExternalCatalog`` objects (a list, or a dict by name).  One ``knn`` launch per k-nearest table (``ps1``,
    ``legacysurvey``) and one ``within`` per name table (``ztfalerts``, ``milliquas``, ``tns``) serve the whole batch.  A table
    that is not supplied contributes no keys, except that the three name fields are then ``''``."""
    ra = _f64(np.atleast_1d(ra), 'ra')
    dec = _f64(np.atleast_1d(dec), 'dec', ra.size)
    if catalogs is None:
        catalogs = {}
    if not isinstance(catalogs, dict):
        catalogs = {c.name: c for c in catalogs}
    unknown = sorted(set(catalogs) - set(CATALOG_COLUMNS))
    if unknown:
        raise ValueError(f'unknown catalogues {unknown}: known are {sorted(CATALOG_COLUMNS)}')
    out = [dict() for _ in range(ra.size)]
    for name, fn in (('ps1', ps1), ('legacysurvey', legacysurvey)):
        if name in catalogs:
            for d, more in zip(out, fn(catalogs[name], ra, dec)):
                d.update(more)
    for name, fn in (('ztfalerts', ztfalerts), ('milliquas', milliquas), ('tns', tns)):
        field = NAME_FIELDS[name][0]
        joined = [','.join(v) for v in fn(catalogs[name], ra, dec)] if name in catalogs else [''] * ra.size
        for d, v in zip(out, joined):
            d[field] = v
    return out
