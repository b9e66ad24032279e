"""Alert packets (``zuds/alert.py``: ``Alert.from_detection``, driven by ``scripts/makealert.py``), on plain objects.

An alert is the ``candidate`` record of ``alert_schemas/*/candidate.avsc`` - the catalogue cross-matches of
``crossmatch.xmatch``, the image and shape fields of the detection, the date range of the reference image, the detection
history of the source - plus the source's light curve up to the detection's date and three cutouts.  The reference takes the
cross-matches from remote services and the history from its database; here the cross-matches are cone searches on the
device against local tables (``crossmatch.py``, ``csrc/skyindex.hip``) and the history is read off ``source.detections``.
Packets are dicts; Avro encoding and Kafka are not part of this package.  DESIGN.md, "Alert packets".
"""
import json
import numbers
import os
from copy import deepcopy

import numpy as np

from .constants import MJD_TO_JD
from .crossmatch import ExternalCatalog, xmatch

__all__ = ['Alert', 'make_alerts', 'validate', 'alert_fields', 'HeaderImage', 'thumbnails_of_blocks', 'SCHEMA_VERSION',
           'PUBLISHER']

SCHEMA_VERSION = '0.4'
PUBLISHER = 'ZUDS/NERSC'
MJDCUT_PAD = 0.5 / 3600. / 24.        # half a second (alert.py:179-181)
FIELDS_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'alert_fields.json')


def _is_single(image):
    """``alert.py:94-96``: a detection on a ``SingleEpochSubtraction`` makes a ``single`` alert; so does one whose image
    has no ``target_image.input_images`` to take a stack's dates from."""
    from .subtraction import SingleEpochSubtraction
    if isinstance(image, SingleEpochSubtraction):
        return True
    return not getattr(getattr(image, 'target_image', None), 'input_images', None)


def _single_mjd(image):
    """The date of a single-epoch subtraction: its science image's (``ScienceImage.obsjd - MJD_TO_JD``)."""
    target = getattr(image, 'target_image', None)
    return target.mjd if getattr(target, 'mjd', None) is not None else image.mjd


def _history(detection, mymjd):
    """``alert.py:188-250``: dates of the source's single-epoch detections before ``mymjd``, ascending, and one
    (first, last) date per distinct science coadd with a detection of the source whose first date lies before ``mymjd``,
    ordered by last date."""
    singles, coadds = [], {}
    for d in detection.source.detections:
        image = getattr(d, 'image', None)
        if image is None or isinstance(image, (str, int)):
            continue                                      # (a detection that names its image only: no dates to take)
        if _is_single(image):
            singles.append(_single_mjd(image))
        else:
            coadd = image.target_image
            dates = [i.mjd for i in coadd.input_images]
            coadds[id(coadd)] = (min(dates), max(dates))
    singledates = sorted(m for m in singles if m < mymjd)
    multidates = sorted((p for p in coadds.values() if p[0] < mymjd), key=lambda p: p[1])
    return singledates, multidates


def _light_curve_records(lc, mjdcut):
    """``lc[lc['mjd'] <= mjdcut]`` as a list of records (``to_pandas().to_dict(orient='records')``), plain values."""
    keep = np.flatnonzero(np.asarray(lc['mjd'], dtype=np.float64) <= mjdcut)
    cols = list(lc.keys())
    out = []
    for k in keep.tolist():
        rec = {}
        for c in cols:
            v = lc[c][k]
            rec[c] = v.item() if hasattr(v, 'item') else v
        out.append(rec)
    return out


class Alert(object):
    """One alert (``zuds/alert.py:17-57``, as a plain object): ``alert`` (the packet without its cutouts),
    ``cutoutscience`` / ``cutouttemplate`` / ``cutoutdifference`` (``Thumbnail`` objects), ``detection``, ``sent``."""

    def __init__(self, alert=None, cutoutscience=None, cutouttemplate=None, cutoutdifference=None, detection=None, sent=False):
        self.alert = alert
        self.cutoutscience, self.cutouttemplate, self.cutoutdifference = cutoutscience, cutouttemplate, cutoutdifference
        self.detection, self.sent = detection, sent

    def to_dict(self):
        """``alert.py:52-57``: the packet with the bytes of its three cutouts (``None`` for a cutout that was never made,
        which ``validate`` reports)."""
        base = deepcopy(self.alert)
        for key, stamp in (('cutoutScience', self.cutoutscience), ('cutoutTemplate', self.cutouttemplate),
                           ('cutoutDifference', self.cutoutdifference)):
            base[key] = stamp.bytes if stamp is not None else None
        return base

    def to_json(self):
        """One line of JSON: ``to_dict()`` with the cutouts as base64 text and numpy scalars as plain numbers."""
        import base64

        def plain(v):
            if isinstance(v, (bytes, bytearray)):
                return base64.b64encode(bytes(v)).decode('ascii')
            if hasattr(v, 'item'):
                return v.item()
            raise TypeError(f'{type(v).__name__} is not JSON serializable')
        return json.dumps(self.to_dict(), default=plain)

    @property
    def kind(self):
        return self.alert['candidate']['alert_type']

    @classmethod
    def from_detection(cls, detection, catalogs=None, candidate=None):
        """``alert.py:60-293`` in its order.  ``catalogs``: the ``ExternalCatalog`` objects ``xmatch`` searches;
        ``candidate``: the cross-match fields of this detection when the caller has them already (``make_alerts``)."""
        obj = cls()
        source = getattr(detection, 'source', None)
        if source is None:
            raise ValueError('Cannot issue an alert for a detection that is '
                             f'not associated with a source ({getattr(detection, "id", None)})')
        alert = dict()
        alert['objectId'] = source.id
        alert['candid'] = detection.id
        alert['schemavsn'] = SCHEMA_VERSION
        alert['publisher'] = PUBLISHER

        if candidate is None:
            candidate = xmatch([detection.ra], [detection.dec], catalogs)[0]
        candidate = dict(candidate)
        alert['candidate'] = candidate

        image = detection.image
        single = _is_single(image)
        alert_type = 'single' if single else 'stack'
        candidate['alert_type'] = alert_type

        candidate['fid'] = image.fid
        candidate['pid'] = image.id
        header = image.target_image.header if single else image.target_image.input_images[0].header
        candidate['programpi'] = header['PROGRMPI']
        candidate['programid'] = header['PROGRMID']
        candidate['pdiffimfilename'] = image.basename
        candidate['candid'] = detection.id
        candidate['isdiffpos'] = 't'
        candidate['field'] = image.field
        candidate['ra'] = detection.ra
        candidate['dec'] = detection.dec
        candidate['rcid'] = (image.ccdid - 1) * 4 + (image.qid - 1)

        candidate['aimage'] = detection.a_image
        candidate['bimage'] = detection.b_image
        candidate['elong'] = detection.elongation
        candidate['fwhm'] = detection.fwhm_image
        candidate['aimagerat'] = detection.a_image / detection.fwhm_image
        candidate['bimagerat'] = detection.b_image / detection.fwhm_image
        candidate['xpos'] = detection.x_image
        candidate['ypos'] = detection.y_image

        candidate['snr'] = detection.snr
        candidate['drb'] = detection.rb
        candidate['drbversion'] = detection.rb_version

        # the reference image: first and last date and number of the frames it was made of (dates as the reference
        # hands them on: obsjd - MJD_TO_JD)
        refdates = [i.mjd for i in image.reference_image.input_images]
        refmin, refmax, refcount = (min(refdates), max(refdates), len(refdates)) if refdates else (None, None, 0)

        if single:
            candidate['jd'] = image.mjd + MJD_TO_JD
            candidate['nid'] = image.target_image.nid
            candidate['diffmaglim'] = image.target_image.maglimit
            candidate['exptime'] = image.target_image.exptime
            mjdcut = image.mjd
            mymjd = image.mjd
        else:
            stackimgs = sorted(image.target_image.input_images, key=lambda i: i.mjd)
            candidate['jdstartstack'] = stackimgs[0].mjd + MJD_TO_JD
            candidate['jdendstack'] = stackimgs[-1].mjd + MJD_TO_JD
            candidate['jdmed'] = float(np.median([i.mjd + MJD_TO_JD for i in stackimgs]))
            candidate['nframesstack'] = len(stackimgs)
            candidate['exptime'] = float(np.sum([i.exptime for i in stackimgs]))
            mjdcut = stackimgs[-1].mjd
            mymjd = getattr(image.target_image, 'max_mjd', None)
            if mymjd is None:
                mymjd = stackimgs[-1].mjd
        mjdcut = mjdcut + MJDCUT_PAD

        singledates, multidates = _history(detection, mymjd)
        candidate['ndethist_single'] = len(singledates)
        candidate['ndethist_stack'] = len(multidates)
        candidate['jdstarthist_single'] = singledates[0] + MJD_TO_JD if singledates else None
        candidate['jdendhist_single'] = singledates[-1] + MJD_TO_JD if singledates else None
        candidate['jdstarthist_stack'] = multidates[0][0] + MJD_TO_JD if multidates else None
        candidate['jdendhist_stack'] = multidates[-1][1] + MJD_TO_JD if multidates else None

        lc = source.light_curve
        if callable(lc):
            lc = lc()
        if len(lc) == 0:
            raise RuntimeError('Cannot issue an alert for an object with no '
                               'light curve, please rerun forced photometry '
                               'to update the light curve of this object:'
                               f'"{source.id}".')
        alert['light_curve'] = _light_curve_records(lc, mjdcut)

        candidate['jdstartref'] = refmin
        candidate['jdendref'] = refmax
        candidate['nframesref'] = refcount

        for stamp in getattr(detection, 'thumbnails', None) or ():
            if stamp.type == 'ref':
                obj.cutouttemplate = stamp
            elif stamp.type == 'new':
                obj.cutoutscience = stamp
            elif stamp.type == 'sub':
                obj.cutoutdifference = stamp

        obj.alert = alert
        obj.detection = detection
        return obj


# ---- what a driver without a database has of an image: its header -----------------------------------------------------
class HeaderImage(object):
    """An image known by its header: the attributes an alert reads, under the reference's names (``id``, ``basename``,
    ``fid``, ``field``, ``ccdid``, ``qid``, ``mjd``, ``nid``, ``maglimit``, ``exptime``, ``header``), and the links
    ``target_image``, ``reference_image`` and ``input_images``."""
    _KEYS = (('field', ('FIELD', 'FIELDID')), ('ccdid', ('CCDID',)), ('qid', ('QID',)), ('fid', ('FID', 'FILTERID')),
             ('nid', ('NID', 'NIGHTID')), ('maglimit', ('MAGLIM', 'MAGLIMIT')), ('exptime', ('EXPTIME', 'EXPOSURE')))

    def __init__(self, header, basename=None, id=None, target_image=None, reference_image=None, input_images=None):
        self.header, self.basename, self.id = header, basename, id
        self.target_image, self.reference_image = target_image, reference_image
        self.input_images = list(input_images) if input_images is not None else []
        for attr, keys in self._KEYS:
            setattr(self, attr, next((header[k] for k in keys if k in header), None))

    @property
    def mjd(self):
        from .utils import get_time
        return get_time(self, 'mjd')


def thumbnails_of_blocks(blocks, x0, y0, nx_trim, ny_trim, detection=None):
    """The three ``Thumbnail`` objects of one row of a stamps file (``scripts/dosub.py``: ``blocks`` [3, S, S] in the order
    sub, new, ref, zero outside the grid; ``x0``, ``y0`` the stamp's origin on the grid, ``nx_trim``, ``ny_trim`` its size
    trimmed to the grid): ``bytes`` is the gzipped FITS of the trimmed stamp (``mtime=0``: equal stamps, equal bytes)."""
    import gzip
    from . import fits as _fits
    from .thumbnails import Thumbnail
    ox, oy = max(int(x0), 0) - int(x0), max(int(y0), 0) - int(y0)
    out = []
    for block, typ in zip(blocks, ('sub', 'new', 'ref')):
        data = np.ascontiguousarray(block[oy:oy + int(ny_trim), ox:ox + int(nx_trim)])
        out.append(Thumbnail(detection=detection, type=typ, bytes=gzip.compress(_fits.to_bytes(data, {}), compresslevel=9, mtime=0)))
    return out


# ---- validation against the field lists of the reference's schemas ---------------------------------------------------
_FIELDS = {}


def alert_fields(path=None):
    """``{schema_single, schema_stack} -> {alert, candidate, light_curve} -> [{name, type, nullable}]``: the field lists of
    the reference's schemas (``tests/golden/alert_fields.json``, or ``path``)."""
    path = path or FIELDS_PATH
    if path not in _FIELDS:
        with open(path) as f:
            _FIELDS[path] = json.load(f)
    return _FIELDS[path]


def _compatible(v, t):
    if t in ('int', 'long'):
        return isinstance(v, (numbers.Integral, np.integer)) and not isinstance(v, (bool, np.bool_))
    if t in ('float', 'double'):
        return isinstance(v, (numbers.Real, np.floating, np.integer)) and not isinstance(v, (bool, np.bool_))
    if t == 'string':
        return isinstance(v, str)
    if t == 'bytes':
        return isinstance(v, (bytes, bytearray, str))     # (a str: the JSON form of a packet carries its cutouts as base64)
    if t == 'boolean':
        return isinstance(v, (bool, np.bool_))
    if t == 'record':
        return isinstance(v, dict)
    if t == 'array':
        return isinstance(v, (list, tuple))
    return False


def _check_record(rec, fields, where, problems):
    known = {f['name']: f for f in fields}
    for name in rec:
        if name not in known:
            problems.append(f'{where}: unknown key {name!r}')
    for f in fields:
        name = f['name']
        if name not in rec:
            if not f['nullable']:
                problems.append(f'{where}: required field {name!r} is missing')
            continue
        v = rec[name]
        if v is None:
            if not f['nullable']:
                problems.append(f'{where}: field {name!r} is null and may not be')
            continue
        if not _compatible(v, f['type']):
            problems.append(f'{where}: field {name!r} holds {type(v).__name__}, the schema says {f["type"]}')


def validate(alert_dict, kind, fields=None):
    """Problems of a packet (``Alert.to_dict()``) of ``kind`` 'single' or 'stack' against the reference's field lists: a
    field that is not nullable must be present and not ``None``, a value must fit its field's type, no key may be unknown -
    in the packet, its ``candidate`` and every record of its ``light_curve``.  Returns a list of strings, empty when the
    packet is valid.  (Types are checked for compatibility, not width: a Python float fits ``float`` and ``double``.)"""
    if kind not in ('single', 'stack'):
        raise ValueError(f"kind must be 'single' or 'stack', got {kind!r}")
    schema = (alert_fields(fields) if fields is None or isinstance(fields, str) else fields)['schema_' + kind]
    problems = []
    _check_record(alert_dict, schema['alert'], 'alert', problems)
    cand = alert_dict.get('candidate')
    if isinstance(cand, dict):
        _check_record(cand, schema['candidate'], 'candidate', problems)
    lc = alert_dict.get('light_curve')
    if isinstance(lc, (list, tuple)):
        for k, rec in enumerate(lc):
            if isinstance(rec, dict):
                _check_record(rec, schema['light_curve'], f'light_curve[{k}]', problems)
            else:
                problems.append(f'light_curve[{k}]: not a record')
    return problems


def _as_catalogs(catalogs, engine):
    """``{name: ExternalCatalog}`` and the ones made here (from plain tables), to be closed by the caller."""
    if catalogs is None:
        return {}, []
    items = catalogs.items() if isinstance(catalogs, dict) else [(c.name, c) for c in catalogs]
    out, made = {}, []
    for name, c in items:
        if not isinstance(c, ExternalCatalog):
            c = ExternalCatalog(name, c, engine=engine)
            made.append(c)
        out[name] = c
    return out, made


def make_alerts(detections, catalogs=None, engine=None, strict=False):
    """One ``Alert`` per detection: ONE ``xmatch`` call for all of them (a launch per catalogue), then the host assembly
    of ``Alert.from_detection`` per detection.  ``catalogs``: ``ExternalCatalog`` objects (a list, or a dict by name; a
    plain table in the dict is indexed on ``engine`` for the call).  ``strict``: every packet is checked with ``validate``
    and a ``ValueError`` lists what is missing or wrong."""
    detections = list(detections)
    for d in detections:
        if getattr(d, 'source', None) is None:
            raise ValueError('Cannot issue an alert for a detection that is '
                             f'not associated with a source ({getattr(d, "id", None)})')
    cats, made = _as_catalogs(catalogs, engine)
    try:
        cands = xmatch([d.ra for d in detections], [d.dec for d in detections], cats) if detections else []
    finally:
        for c in made:
            c.close()
    alerts = [Alert.from_detection(d, candidate=c) for d, c in zip(detections, cands)]
    if strict:
        problems = []
        for a in alerts:
            problems += [f'{a.alert["candid"]}: {p}' for p in validate(a.to_dict(), a.kind)]
        if problems:
            raise ValueError(f'{len(problems)} problem(s) in {len(alerts)} alert(s): ' + '; '.join(problems))
    return alerts
