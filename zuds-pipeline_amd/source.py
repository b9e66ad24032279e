"""Source association (``nersc/makesources.py:263-456``): a night's detections into sources, on the GPU.

The reference joins new detections to known sources with q3c at 2 arcsec, links the rest with ``search_around_sky`` at
2 arcsec, clusters that graph with ``DBSCAN(eps=2, min_samples=2, metric='precomputed')``, gives every cluster the
position of its best-S/N detection and the sum of its real / bogus scores, and vetoes sources within 1.5 arcsec of a
star (``makesources.py:150-155``).  Here the two geometric steps are ``zm_crossmatch`` and ``zm_associate``
(``csrc/associate.hip``: unit vectors binned into a hash table of cubic cells, label propagation in separate launches);
the bookkeeping around them is plain Python on plain objects.  DESIGN.md, "Source association".
"""
import ctypes as C

import numpy as np

from ._lib import check
from .constants import ASSOC_RADIUS_ARCSEC, ASSOC_RB_MIN, MJD_TO_JD, STAR_VETO_ARCSEC
from .detections import Detection
from .engine import get_engine

__all__ = ['crossmatch', 'cluster', 'crossmatch_dev', 'cluster_dev', 'assoc_stats', 'Source', 'associate',
           'detections_from_cat', 'write_source_tables', 'read_sources_table']


def _f64(a, what, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 1 or (n is not None and a.size != n):
        raise ValueError(f'{what} must be a vector' + (f' of {n} values' if n is not None else '') + f', got shape {a.shape}')
    return a


def crossmatch(ra, dec, cat_ra, cat_dec, radius_arcsec, engine=None):
    """For each position the nearest catalogue position within ``radius_arcsec`` (inclusive; ties: the lowest catalogue
    index).  Degrees in; returns ``(idx int32 [n], sep float64 [n])`` with ``-1`` / ``NaN`` where nothing lies in range
    or the position is not finite (``zm_crossmatch``)."""
    ra = _f64(ra, 'ra')
    dec = _f64(dec, 'dec', ra.size)
    cra = _f64(cat_ra, 'cat_ra')
    cdec = _f64(cat_dec, 'cat_dec', cra.size)
    eng = engine or get_engine()
    idx = np.full(ra.size, -1, np.int32)
    sep = np.full(ra.size, np.nan, np.float64)
    check(eng.L.zm_crossmatch(eng.ctx, ra.size, ra.ctypes.data, dec.ctypes.data, cra.size, cra.ctypes.data, cdec.ctypes.data,
                              float(radius_arcsec), idx.ctypes.data, sep.ctypes.data), 'zm_crossmatch')
    return idx, sep


def cluster(ra, dec, snr, rb=None, radius_arcsec=ASSOC_RADIUS_ARCSEC, engine=None):
    """Connected components of "within ``radius_arcsec`` of each other", labelled as
    ``DBSCAN(eps=radius, min_samples=2, metric='precomputed')`` labels them (``zm_associate``).  Returns a dict:

    * ``label`` int32 [n]: ``-1`` for a row without a neighbour (or with an ``ra``, ``dec`` or ``snr`` that is not
      finite), else its source; sources are numbered by the rank of their smallest row;
    * ``nsrc``; ``offsets`` int32 [nsrc + 1] and ``members`` int32: CSR of the rows of every source, ascending;
    * ``best`` int32 [nsrc]: the row of greatest ``snr`` (ties: the lowest row, pandas ``idxmax``);
    * ``count`` int32 [nsrc]; ``sumrb`` float64 [nsrc]: the sum of ``rb`` in member order (zeros without ``rb``)."""
    ra = _f64(ra, 'ra')
    n = ra.size
    dec, snr = _f64(dec, 'dec', n), _f64(snr, 'snr', n)
    rb = None if rb is None else _f64(rb, 'rb', n)
    eng = engine or get_engine()
    label = np.full(n, -1, np.int32)
    nsrc = C.c_int32(0)
    offsets = np.zeros(n + 1, np.int32)
    members, best, count = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    sumrb = np.zeros(n, np.float64)
    check(eng.L.zm_associate(eng.ctx, n, ra.ctypes.data, dec.ctypes.data, snr.ctypes.data,
                             rb.ctypes.data if rb is not None else None, float(radius_arcsec), label.ctypes.data,
                             C.byref(nsrc), offsets.ctypes.data, members.ctypes.data, best.ctypes.data, count.ctypes.data,
                             sumrb.ctypes.data), 'zm_associate')
    ns = int(nsrc.value)
    offsets = offsets[:ns + 1].copy()
    return dict(label=label, nsrc=ns, offsets=offsets, members=members[:int(offsets[ns])].copy(), best=best[:ns].copy(),
                count=count[:ns].copy(), sumrb=sumrb[:ns].copy())


def _dev_f64(t, what, n=None):
    import torch
    if t.dtype != torch.float64 or t.dim() != 1 or not t.is_contiguous() or not t.is_cuda or (n is not None and t.numel() != n):
        raise ValueError(f'{what} must be a contiguous float64 device vector' + (f' of {n} values' if n is not None else ''))
    return t


def crossmatch_dev(ra, dec, cat_ra, cat_dec, radius_arcsec, engine=None, stream=None):
    """``crossmatch`` on float64 torch tensors that lie in HBM (``zm_crossmatch_dev``): enqueued on the engine's stream
    (``stream``: the torch stream it is bound to), nothing waited for.  Returns device tensors ``(idx, sep)``."""
    import torch
    eng = engine or get_engine()
    n, m = ra.numel(), cat_ra.numel()
    _dev_f64(ra, 'ra'), _dev_f64(dec, 'dec', n), _dev_f64(cat_ra, 'cat_ra'), _dev_f64(cat_dec, 'cat_dec', m)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(ra.device):
        idx = torch.empty(n, dtype=torch.int32, device=ra.device)
        sep = torch.empty(n, dtype=torch.float64, device=ra.device)
        check(eng.L.zm_crossmatch_dev(eng.ctx, n, ra.data_ptr(), dec.data_ptr(), m, cat_ra.data_ptr(), cat_dec.data_ptr(),
                                      float(radius_arcsec), idx.data_ptr(), sep.data_ptr()), 'zm_crossmatch_dev')
    return idx, sep


def cluster_dev(ra, dec, snr, rb=None, radius_arcsec=ASSOC_RADIUS_ARCSEC, engine=None, stream=None):
    """``cluster`` on float64 torch tensors that lie in HBM (``zm_associate_dev``).  Returns a dict of device tensors
    with room for n entries each (``offsets``: n + 1) and ``nsrc`` as a device tensor of one int32: entries past
    ``nsrc`` of the per-source arrays are not meaningful (``offsets[nsrc:]`` all hold the number of clustered rows).
    The call waits for the verdict of each propagation round; the compaction behind them is enqueued only."""
    import torch
    eng = engine or get_engine()
    n = ra.numel()
    _dev_f64(ra, 'ra'), _dev_f64(dec, 'dec', n), _dev_f64(snr, 'snr', n)
    if rb is not None:
        _dev_f64(rb, 'rb', n)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(ra.device):
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=ra.device)
        out = dict(label=i32(n), nsrc=i32(1), offsets=i32(n + 1), members=i32(n), best=i32(n), count=i32(n),
                   sumrb=torch.empty(n, dtype=torch.float64, device=ra.device))
        check(eng.L.zm_associate_dev(eng.ctx, n, ra.data_ptr(), dec.data_ptr(), snr.data_ptr(),
                                     rb.data_ptr() if rb is not None else None, float(radius_arcsec), out['label'].data_ptr(),
                                     out['nsrc'].data_ptr(), out['offsets'].data_ptr(), out['members'].data_ptr(),
                                     out['best'].data_ptr(), out['count'].data_ptr(), out['sumrb'].data_ptr()),
              'zm_associate_dev')
    return out


def assoc_stats(engine=None):
    """What the last ``cluster`` / ``crossmatch`` call on the engine did: propagation ``rounds``, ``capacity`` of the cell
    table, ``probes`` summed over every insertion and the longest probe ``probe_max`` (``zm_assoc_stats``)."""
    eng = engine or get_engine()
    out = (C.c_int64 * 4)()
    check(eng.L.zm_assoc_stats(eng.ctx, out), 'zm_assoc_stats')
    return dict(rounds=int(out[0]), capacity=int(out[1]), probes=int(out[2]), probe_max=int(out[3]))


class Source(object):
    """One source: the attributes of the reference's ``Source`` that association sets (``makesources.py:374-379``,
    ``:125-127``, ``:150-155``)."""

    def __init__(self, id=None, ra=None, dec=None, detections=None, score=0.0, altdata=None, best_detection=None):
        self.id, self.ra, self.dec = id, ra, dec
        self.detections = list(detections) if detections is not None else []
        self.score, self.altdata, self.best_detection = score, altdata, best_detection
        self.forced_photometry = []

    @property
    def rejected(self):
        return bool(self.altdata) and 'rejected' in self.altdata

    @property
    def light_curve(self):
        """The table of ``zuds/source.py:84-112`` from ``forced_photometry`` (a ``PhotTable``; a source without
        photometry: every column present, length 0).  ``id`` is the point's own id, or its position in the list."""
        from .photometry import PhotTable
        pts = self.forced_photometry
        f = lambda name: np.array([getattr(p, name) for p in pts], dtype=np.float64)
        t = PhotTable()
        t['mjd'] = f('obsjd') - MJD_TO_JD
        t['filter'] = np.array(['ztf' + p.filtercode[-1] for p in pts], dtype=object)
        t['zp'] = f('zp')
        t['zpsys'] = np.array(['ab'] * len(pts), dtype=object)
        t['flux'] = f('flux')
        t['fluxerr'] = f('fluxerr')
        t['flags'] = np.array([p.flags for p in pts], dtype=np.int64)
        with np.errstate(invalid='ignore', divide='ignore'):
            t['lim_mag'] = -2.5 * np.log10(5 * t['fluxerr']) + t['zp']
        t['id'] = np.array([k if getattr(p, 'id', None) is None else p.id for k, p in enumerate(pts)], dtype=object)
        return t

    def images(self, images, engine=None):
        """The ``images`` (objects with a ``wcs``) whose footprint holds this source: the ``q3c_poly_query`` of
        ``zuds/source.py:60-71`` as ``footprint_join``; the radial pre-filter of the reference is the join's own cap."""
        from .lightcurve import footprint_join
        images = list(images)
        if not images:
            return []
        offsets, _ = footprint_join([im.wcs for im in images], [self.ra], [self.dec], engine=engine)
        return [im for im, n in zip(images, np.diff(offsets).tolist()) if n]

    def unphotometered_images(self, images=(), engine=None):
        """Of ``images``, those that hold this source and on which it has no ``ForcedPhotometry`` yet
        (``zuds/source.py:114-134``)."""
        have = {id(p.image) for p in self.forced_photometry}
        return [im for im in self.images(images, engine=engine) if id(im) not in have]

    def force_photometry(self, images=(), assume_background_subtracted=True, method='aperture'):
        """Photometry of this source on every image of ``images`` that holds it and has none yet
        (``zuds/source.py:136-153``); the points are returned, not recorded.  ``method='psf'``: fits of each image's
        ``psf_model`` (``CalibratedImage.force_photometry``)."""
        out = []
        for im in self.unphotometered_images(images):
            kw = {} if method == 'aperture' else {'method': method}
            out.extend(im.force_photometry(self, assume_background_subtracted=assume_background_subtracted, use_cutout=True, **kw))
        return out

    def __repr__(self):
        return f'<Source {self.id} ra={self.ra:.6f} dec={self.dec:.6f} ndet={len(self.detections)} score={self.score:.3f}>'


def detections_from_cat(table, image=None):
    """``Detection`` objects of the ``GOODCUT == 1`` rows of a filtered catalog table (``out['cat']`` of a
    ``SubtractionJob(detect=True)``, or ``PipelineFITSCatalog.data``; a table without the column: every row).  Each keeps
    its row number as ``row``; an ``rb`` of -99 (no model scored the row) becomes ``None``."""
    names = table.dtype.names
    keep = np.flatnonzero(table['GOODCUT'] == 1) if 'GOODCUT' in names else np.arange(len(table))
    cols = [np.asarray(table[c], dtype=np.float64)[keep].tolist() for c in ('X_WORLD', 'Y_WORLD', 'FLUX_APER', 'FLUXERR_APER')]
    rbs = np.asarray(table['rb'], dtype=np.float64)[keep].tolist() if 'rb' in names else [None] * keep.size
    rbs = [None if v == -99.0 else v for v in rbs]       # -99: the filter ran without a model (filterobjects.py:204)
    out = []
    for row, ra, dec, flux, fluxerr, rb in zip(keep.tolist(), *cols, rbs):
        d = Detection(ra=ra, dec=dec, image=image, flux=flux, fluxerr=fluxerr)
        d.rb, d.row, d.goodcut = rb, row, True if 'GOODCUT' in names else None
        out.append(d)
    return out


def _snr(d):
    try:
        v = float(d.flux) / float(d.fluxerr)
    except (TypeError, ZeroDivisionError):
        return np.nan
    return v


def _best(dets):
    """The detection of greatest finite S/N, the first of equals (the rank() = 1 row of ``makesources.py:293-301``)."""
    best, bs = None, -np.inf
    for d in dets:
        s = _snr(d)
        if np.isfinite(s) and s > bs:
            best, bs = d, s
    return best


def _default_name(k):
    return f'src{k:07d}'


def associate(detections, sources=None, stars=None, rb_min=ASSOC_RB_MIN, name=None, engine=None):
    """The reference's ``associate()`` on plain objects.

    ``detections``: ``Detection`` objects, or catalog tables (``out['cat']`` of the pool; a list may mix both) whose
    ``GOODCUT == 1`` rows become ``Detection`` objects with ``image`` = the table's position in the list.  A detection
    whose ``source`` is already set is left alone.  ``sources``: known ``Source`` objects.  ``stars``: ``(ra, dec)``
    arrays of a star catalogue, degrees.  In the reference's order:

    1. a detection within ``ASSOC_RADIUS_ARCSEC`` of a known source joins the nearest one, and every known source that
       has detections moves to the position of its best-S/N detection;
    2. the remaining detections with ``rb > rb_min`` (all of them when no detection carries an ``rb``) are clustered;
    3. each cluster becomes a ``Source`` named ``name(k)`` (k counts on from ``len(sources)``; default: a zero-padded
       counter) at the position of its best detection, with ``score`` = the sum of ``rb`` and ``detection.source`` set;
    4. a new source less than ``STAR_VETO_ARCSEC`` from a star gets ``score = -1`` and ``altdata = {'rejected': ...}``.

    Returns the known sources followed by the new ones."""
    dets = []
    if isinstance(detections, np.ndarray):
        detections = [detections]
    for k, item in enumerate(detections):
        if isinstance(item, np.ndarray):
            dets += detections_from_cat(item, image=k)
        else:
            dets.append(item)
    for d in dets:
        if not hasattr(d, 'source'):
            d.source = None
    sources = list(sources) if sources is not None else []
    name = name or _default_name
    free = [d for d in dets if d.source is None]
    ra = np.array([d.ra for d in free], dtype=np.float64)
    dec = np.array([d.dec for d in free], dtype=np.float64)

    # 1. known sources (makesources.py:269-301)
    if sources and free:
        idx, _ = crossmatch(ra, dec, [s.ra for s in sources], [s.dec for s in sources], ASSOC_RADIUS_ARCSEC, engine=engine)
        for d, j in zip(free, idx.tolist()):
            if j >= 0:
                d.source = sources[j]
                sources[j].detections.append(d)
    for s in sources:
        b = _best(s.detections)
        if b is not None:
            s.ra, s.dec, s.best_detection = b.ra, b.dec, b

    # 2. the rest, gated on the real / bogus score (makesources.py:304-340)
    has_rb = any(getattr(d, 'rb', None) is not None for d in dets)
    rest = [k for k, d in enumerate(free) if d.source is None and
            (not has_rb or (d.rb is not None and d.rb > rb_min))]
    new = []
    if rest:
        sub = [free[k] for k in rest]
        snr = np.array([_snr(d) for d in sub], dtype=np.float64)
        rb = np.array([d.rb for d in sub], dtype=np.float64) if has_rb else None
        cl = cluster(ra[rest], dec[rest], snr, rb, ASSOC_RADIUS_ARCSEC, engine=engine)
        # 3. one Source per cluster (makesources.py:369-429)
        for s in range(cl['nsrc']):
            members = [sub[j] for j in cl['members'][cl['offsets'][s]:cl['offsets'][s + 1]].tolist()]
            b = sub[int(cl['best'][s])]
            src = Source(id=name(len(sources) + s), ra=b.ra, dec=b.dec, detections=members, score=float(cl['sumrb'][s]),
                         best_detection=b)
            for d in members:
                d.source = src
            new.append(src)

    # 4. the star veto (makesources.py:150-155: sep < 1.5, strictly)
    if new and stars is not None:
        sra, sdec = stars
        if len(sra):
            idx, sep = crossmatch([s.ra for s in new], [s.dec for s in new], sra, sdec, STAR_VETO_ARCSEC, engine=engine)
            for s, j, d in zip(new, idx.tolist(), sep.tolist()):
                if j >= 0 and d < STAR_VETO_ARCSEC:
                    s.score = -1.0
                    s.altdata = {'rejected': f'matched to star {j} at {d:.3f} arcsec'}
    return sources + new


def _image_name(d):
    im = getattr(d, 'image', None)
    if im is None:
        return '-'
    im = getattr(im, 'basename', im)
    return str(im).replace(' ', '_')


def write_source_tables(sources, detections, sources_path, detsource_path):
    """The two tables of ``scripts/makesources.py`` and ``donightly.py --associate``:

    * ``sources_path``: ``id ra dec ndet score best_image rejected`` per source (``rejected``: 0 / 1, the star veto);
    * ``detsource_path``: ``image row ra dec source`` per detection (``-``: no source), in the order given."""
    with open(sources_path, 'w') as f:
        f.write('# id ra dec ndet score best_image rejected\n')
        for s in sources:
            best = _image_name(s.best_detection) if s.best_detection is not None else '-'
            f.write('%s %.8f %.8f %d %.6f %s %d\n' % (s.id, s.ra, s.dec, len(s.detections), s.score, best, int(s.rejected)))
    with open(detsource_path, 'w') as f:
        f.write('# image row ra dec source\n')
        for d in detections:
            src = getattr(d, 'source', None)
            f.write('%s %d %.8f %.8f %s\n' % (_image_name(d), getattr(d, 'row', -1), d.ra, d.dec, src.id if src is not None else '-'))


def read_sources_table(path):
    """Known sources from a table ``write_source_tables`` wrote (``makesources.py --sources``): id, position and score;
    their earlier detections are not kept in the table, so a source moves only when a new detection joins it."""
    out = []
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t or t[0].startswith('#'):
                continue
            s = Source(id=t[0], ra=float(t[1]), dec=float(t[2]), score=float(t[4]) if len(t) > 4 else 0.0)
            if len(t) > 6 and t[6] == '1':
                s.altdata = {'rejected': 'rejected in ' + str(path)}
            out.append(s)
    return out
