"""Detection thumbnails (``zuds/thumbnails.py``) and the real / bogus triplets (``zuds/filterobjects.py:36-54``).

The reference cuts three 63 x 63 stamps per detection - difference, new and reference image, all on the reference
image's grid - after two whole-frame SWarp runs (``scripts/dosub.py:133-150``: ``sub.aligned_to(ref)``,
``sci.aligned_to(ref)``) and keeps at most 50 x 63 x 63 pixels of each.  Here the stamps of a subtraction come from one
engine call (``zm_stamps`` / ``zm_stamps_dev``, csrc/stamps.hip) that resamples only the output tiles the stamps touch;
every pixel is the pixel the whole-frame alignment would have produced, bit for bit ("Detection thumbnails").

Two forms of one stamp: the engine writes the full ``size x size`` block with 0 outside the grid - ``Cutout2D(mode=
'partial', fill_value=0)``, what ``make_triplet_for_braai`` wants; ``make_stamp`` / ``Thumbnail`` use ``Cutout2D``'s
default ``mode='trim'``, the slice of that block that lies on the grid.  astropy is not a dependency: the origin rule
of ``astropy.nddata.utils.overlap_slices`` (first pixel = ceil(position - size / 2)) is restated, not pinned.
"""
import ctypes as C
import gzip

import numpy as np

from . import _lib
from . import fits as _fits
from ._lib import RESAMPLE, check, wcs_struct
from .constants import CUTOUT_SIZE
from .engine import Engine, _enum, get_engine
from .wcs import WCS

__all__ = ['make_stamp', 'Thumbnail', 'Cutout', 'stamp_origin', 'make_triplet_for_braai', 'triplets']

STAMP_TYPES = ('sub', 'new', 'ref')          # per detection, the order of scripts/dosub.py:144-150


def stamp_origin(wgrid, ra, dec, size=CUTOUT_SIZE):
    """(x0, y0, status) of the stamps centred on (ra, dec): ``zm_stamp_origin``, float64 on the host.  status != 0:
    the position is not finite (1) or the stamp does not overlap the grid at all (2)."""
    g = wcs_struct(wgrid)
    ra = np.ascontiguousarray(np.atleast_1d(ra), dtype=np.float64)
    dec = np.ascontiguousarray(np.atleast_1d(dec), dtype=np.float64)
    if ra.shape != dec.shape:
        raise ValueError('ra and dec must have the same shape')
    n = ra.size
    x0, y0, st = (np.zeros(n, np.int32) for _ in range(3))
    check(_lib.lib().zm_stamp_origin(C.byref(g), n, ra.ctypes.data, dec.ctypes.data, int(size), x0.ctypes.data,
                                     y0.ctypes.data, st.ctypes.data), 'zm_stamp_origin')
    return x0, y0, st


def _checked_origin(wgrid, ra, dec, size):
    x0, y0, st = stamp_origin(wgrid, ra, dec, size)
    if st.any():
        k = int(np.flatnonzero(st)[0])
        why = 'is not finite' if st[k] == _lib.STAMP_NOT_FINITE else 'does not overlap the grid'
        raise ValueError(f'stamp {k} at (ra, dec) = ({np.atleast_1d(ra)[k]}, {np.atleast_1d(dec)[k]}) {why} '
                         f'({int((st != 0).sum())} of {st.size} stamps)')
    return x0, y0


def trim_slices(x0, y0, size, nx, ny):
    """Slices of the ``size x size`` block that lie on an nx x ny grid, and the origin of the trimmed stamp."""
    xa, xb, ya, yb = max(x0, 0), min(x0 + size, nx), max(y0, 0), min(y0 + size, ny)
    return (slice(ya - y0, yb - y0), slice(xa - x0, xb - x0)), (xa, ya)


def _is_device(a):
    return not isinstance(a, np.ndarray) and hasattr(a, 'data_ptr')


def _engine_stamps(self, planes, wgrid, ra, dec, size=CUTOUT_SIZE, kernel='LANCZOS3', stream=None, device_out=False):
    """Stamps of ``planes`` around (ra, dec) on the grid ``wgrid``: (blocks[n, P, S, S] float32, norms[n, P] float64,
    x0, y0).  ``planes``: dicts ``{img, wcs, fscale (1.0), on_grid (False)}``; ``img`` float32 [ny, nx] of ``wcs``, all
    numpy arrays (``zm_stamps``: copied in) or all torch tensors on this engine's GPU (``zm_stamps_dev``: read where they
    lie; only blocks and norms cross PCIe).  A plane with ``on_grid`` is gathered, every other one resampled - only the
    tiles the stamps touch.  ``stream``: the torch stream this engine is bound to, when the planes are produced there.
    ``device_out`` (device planes only): blocks and norms are returned as the device tensors the kernels wrote, enqueued
    on the stream and not waited for - for work that reads them there (``realbogus.RBModel.score_dev``).
    A position that is not finite or whose stamp misses the grid raises ``ValueError``."""
    size = int(size)
    if not 1 <= size <= _lib.STAMP_MAX:
        raise ValueError(f'size must be 1 .. {_lib.STAMP_MAX} (got {size})')
    kern = _enum(RESAMPLE, kernel, 'RESAMPLING_TYPE')
    g = wcs_struct(wgrid)
    x0, y0 = _checked_origin(g, ra, dec, size)
    n, P = x0.size, len(planes)
    if P < 1:
        raise ValueError('stamps needs at least one plane')
    dev = [_is_device(p['img']) for p in planes]
    if any(dev) and not all(dev):
        raise ValueError('planes must be all numpy arrays or all device tensors')
    arr = (_lib.zm_stamp_plane * P)()
    keep = []
    for i, p in enumerate(planes):
        s = wcs_struct(p['wcs'])
        img = p['img']
        if dev[0]:
            import torch
            if img.dtype != torch.float32 or not img.is_contiguous():
                raise ValueError(f'plane {i}: device planes must be contiguous float32 tensors')
            arr[i].img = img.data_ptr()
        else:
            img = np.ascontiguousarray(img, dtype=np.float32)
            arr[i].img = img.ctypes.data
        if tuple(img.shape) != (s.naxis[1], s.naxis[0]):
            raise ValueError(f'plane {i}: WCS NAXIS {tuple(s.naxis)} does not match data shape {tuple(img.shape)}')
        keep.append(img)
        arr[i].wcs = s
        arr[i].fscale = float(p.get('fscale', 1.0))
        arr[i].on_grid = int(bool(p.get('on_grid', False)))
    if device_out and not dev[0]:
        raise ValueError('device_out needs device planes')
    if not dev[0]:
        blocks = np.zeros((n, P, size, size), np.float32)
        norms = np.zeros((n, P), np.float64)
        check(self.L.zm_stamps(self._ctx, P, arr, C.byref(g), kern, n, x0.ctypes.data, y0.ctypes.data, size,
                               blocks.ctypes.data, norms.ctypes.data), 'zm_stamps')
        return blocks, norms, x0, y0
    import torch
    device = keep[0].device
    if stream is None:
        torch.cuda.current_stream(device).synchronize()      # the planes are final and the outputs' memory is at rest
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(device):
        d_blocks = torch.empty((n, P, size, size), dtype=torch.float32, device=device)
        d_norms = torch.empty((n, P), dtype=torch.float64, device=device)
        check(self.L.zm_stamps_dev(self._ctx, P, arr, C.byref(g), kern, n, x0.ctypes.data, y0.ctypes.data, size,
                                   d_blocks.data_ptr(), d_norms.data_ptr()), 'zm_stamps_dev')
        if device_out:
            return d_blocks, d_norms, x0, y0
        self.synchronize()
        return d_blocks.cpu().numpy(), d_norms.cpu().numpy(), x0, y0


Engine.stamps = _engine_stamps


class Cutout(object):
    """What ``make_stamp`` returns (the attributes of astropy's ``Cutout2D`` this path reads): ``data`` (trimmed to the
    grid), ``wcs`` (the grid's WCS with CRPIX shifted by the trimmed origin), ``origin`` = (x, y) of ``data[0, 0]`` on
    the grid, ``block_origin`` = (x0, y0) of the untrimmed block."""

    def __init__(self, data, wcs, origin, block_origin, size):
        self.data, self.wcs, self.origin, self.block_origin, self.size = data, wcs, origin, block_origin, size
        self.shape = data.shape


def shifted_wcs(wcs, origin, shape):
    """``wcs`` for an array whose pixel [0, 0] is pixel ``origin`` = (x, y) of the grid (``Cutout2D.wcs``)."""
    w = wcs if isinstance(wcs, WCS) else WCS.from_header(wcs)
    return WCS((w.crpix[0] - origin[0], w.crpix[1] - origin[1]), w.crval, w.cd, w.pv1 if w.has_pv else None,
               w.pv2 if w.has_pv else None, (shape[1], shape[0]))


def _cutout_of_block(block, wcs, x0, y0, size, nx, ny):
    sl, origin = trim_slices(int(x0), int(y0), size, nx, ny)
    data = np.ascontiguousarray(block[sl])
    return Cutout(data, shifted_wcs(wcs, origin, data.shape), origin, (int(x0), int(y0)), size)


def _host_block(data, x0, y0, size):
    ny, nx = data.shape
    block = np.zeros((size, size), data.dtype)
    sl, (xa, ya) = trim_slices(x0, y0, size, nx, ny)
    h, w = sl[0].stop - sl[0].start, sl[1].stop - sl[1].start
    block[sl] = data[ya:ya + h, xa:xa + w]
    return block


def make_stamp(name, ra, dec, vmin, vmax, data, wcs, save=True, size=CUTOUT_SIZE):
    """``zuds/thumbnails.py:133-146``: the cutout of ``data`` (on the grid ``wcs``) around (ra, dec), ``Cutout2D``'s
    default ``mode='trim'``.  A plain slice: no resampling, values untouched.  ``save=True`` writes a JPEG with
    matplotlib in the reference; matplotlib is not a dependency here."""
    if save:
        raise NotImplementedError('make_stamp(save=True) writes an image file with matplotlib, which this package does '
                                  'not depend on; call it with save=False and render cutout.data yourself')
    data = np.asarray(data)
    if data.ndim != 2:
        raise ValueError('make_stamp needs a 2-D array')
    w = wcs if isinstance(wcs, WCS) else WCS.from_header(wcs)
    ny, nx = data.shape
    grid = WCS(w.crpix, w.crval, w.cd, w.pv1 if w.has_pv else None, w.pv2 if w.has_pv else None, (nx, ny))
    x0, y0 = _checked_origin(grid, [ra], [dec], int(size))
    return _cutout_of_block(_host_block(data, int(x0[0]), int(y0[0]), int(size)), grid, x0[0], y0[0], int(size), nx, ny)


def _link_image(image):
    from .image import CalibratableImageBase
    from .subtraction import Subtraction
    if isinstance(image, (Subtraction, CalibratableImageBase)):
        return image
    return getattr(image, 'parent_image', None) or image


def _type_of(linkimage):
    from .coadd import ReferenceImage
    from .subtraction import Subtraction
    if isinstance(linkimage, Subtraction):
        return 'sub'
    if isinstance(linkimage, ReferenceImage):
        return 'ref'
    return 'new'


def stamp_bytes(cutout):
    """gzip of the FITS file of a cutout with its WCS cards (``zuds/thumbnails.py:84-91``); ``mtime=0``: equal stamps
    are equal bytes."""
    raw = _fits.to_bytes(np.ascontiguousarray(cutout.data), cutout.wcs.to_header())
    return gzip.compress(raw, compresslevel=9, mtime=0)


class Thumbnail(object):
    """One stamp of one detection (``zuds/thumbnails.py:22-130``, as a plain object): ``type`` 'sub' / 'new' / 'ref',
    ``bytes`` (gzipped FITS of the trimmed stamp), ``image`` (the image the stamp is linked to), ``detection``."""

    def __init__(self, image=None, detection=None, type=None, bytes=None):
        self.image, self.detection, self.type, self.bytes = image, detection, type, bytes
        self.source = None
        self.file_uri = self.public_url = self.origin = None
        self.x0 = self.y0 = self.shape = None

    @classmethod
    def _of_cutout(cls, detection, linkimage, cutout, type=None):
        stamp = cls(image=linkimage, detection=detection, type=type or _type_of(linkimage), bytes=stamp_bytes(cutout))
        stamp.x0, stamp.y0 = cutout.block_origin
        stamp.shape = cutout.shape
        return stamp

    @classmethod
    def from_detection(cls, detection, image):
        """``zuds/thumbnails.py:54-94``: the stamp of ``image`` (already on the grid it is to be cut on) around the
        detection."""
        cutout = make_stamp(None, detection.ra, detection.dec, None, None, image.data, image.wcs, save=False,
                            size=CUTOUT_SIZE)
        return cls._of_cutout(detection, _link_image(image), cutout)

    @classmethod
    def from_detections(cls, detections, sub, size=CUTOUT_SIZE):
        """All stamps of a subtraction in ONE engine call, in the reference's order (per detection: sub, new, ref;
        ``scripts/dosub.py:133-150``).  A ``SingleEpochSubtraction``: difference and new image are resampled onto the
        grid of ``sub.reference_image`` (what ``aligned_to`` would give, only under the stamps), the reference is
        gathered; a ``MultiEpochSubtraction``: each image is gathered on its own grid."""
        detections = list(detections)
        out = []
        for blocks, _, x0, y0, images, grids in _subtraction_blocks(detections, sub, size):
            per = []
            for k, det in enumerate(detections):
                row = []
                for p, (typ, img) in enumerate(images):
                    nx, ny = grids[p].naxis
                    cut = _cutout_of_block(blocks[k, p], grids[p], x0[k], y0[k], int(size), nx, ny)
                    row.append(cls._of_cutout(det, img, cut, typ))
                per.append(row)
            out.append((images, per))
        # back into the reference's order whatever the grouping was
        stamps = []
        for k in range(len(detections)):
            row = {}
            for images, per in out:
                for s in per[k]:
                    row[s.type] = s
            stamps += [row[t] for t in STAMP_TYPES]
        return stamps

    def persist(self):
        raise NotImplementedError('persisting a thumbnail as a JPEG (zuds/thumbnails.py:96-119) is not part of this package')

    @property
    def array(self):
        """``zuds/thumbnails.py:121-130``: the pixel values of ``bytes``, flipped upside down."""
        if self.bytes is None:
            raise ValueError('Cannot coerce array from empty bytes attribute')
        data, _, _ = _fits.from_bytes(gzip.decompress(self.bytes))
        return np.flipud(data)

    @property
    def header(self):
        return _fits.from_bytes(gzip.decompress(self.bytes))[1]


def _plane_of(img, on_grid, grid):
    w = img.wcs
    fs = 1.0
    if not on_grid:
        # what run_align hands to the resampler (swarp.py: prepare_swarp_align / run_align)
        fs = get_engine().flux_scale(w, grid, float((img.header or {}).get('FLXSCALE', 1.0)))
    return dict(wcs=w, fscale=fs, on_grid=on_grid)


def _subtraction_blocks(detections, sub, size, device_out=False):
    """The engine calls behind ``Thumbnail.from_detections`` / ``triplets``: a list of (blocks, norms, x0, y0, [(type,
    image)], [grid per plane]) - one entry when all planes end on one grid.  ``device_out``: on the device route blocks and
    norms stay in HBM (torch tensors on the I/O stream, not waited for); the host route returns arrays either way."""
    from . import objdev
    from .subtraction import SingleEpochSubtraction
    ref, sci = sub.reference_image, sub.target_image
    if ref is None or sci is None:
        raise ValueError('the subtraction needs its reference_image and target_image')
    ra = np.array([d.ra for d in detections], np.float64)
    dec = np.array([d.dec for d in detections], np.float64)
    images = [('sub', sub), ('new', sci), ('ref', ref)]
    if isinstance(sub, SingleEpochSubtraction):
        grid = WCS.from_header(ref.astropy_header)
        groups = [(grid, [(t, im, False) for t, im in images[:2]] + [('ref', ref, True)])]
    else:
        groups = []
        for t, im in images:                  # one call per distinct grid (usually one)
            g = WCS.from_header(im.astropy_header)
            for gg, members in groups:
                if bytes(wcs_struct(gg)) == bytes(wcs_struct(g)):
                    members.append((t, im, True))
                    break
            else:
                groups.append((g, [(t, im, True)]))
    eng = get_engine()
    out = []
    for grid, members in groups:
        planes = [_plane_of(im, on, grid) for _, im, on in members]
        if objdev.enabled():
            # the device route: planes that are resident (or whose raw FITS blocks decode on the device) stay in HBM
            oio = objdev.get_io()
            tensors = oio.planes([(im, 'f32') for _, im, _ in members])
            eng.set_stream(oio.stream.cuda_stream)
            for p, t in zip(planes, tensors):
                p['img'] = t.contiguous()
            blocks, norms, x0, y0 = eng.stamps(planes, grid, ra, dec, size, stream=oio.stream, device_out=device_out)
        else:
            for p, (_, im, _) in zip(planes, members):
                p['img'] = np.ascontiguousarray(im.data, dtype=np.float32)
            blocks, norms, x0, y0 = eng.stamps(planes, grid, ra, dec, size)
        out.append((blocks, norms, x0, y0, [(t, im) for t, im, _ in members], [grid] * len(members)))
    return out


def make_triplet_for_braai(ra, dec, new_aligned, ref_aligned, sub_aligned, old_norm=False):
    """``zuds/filterobjects.py:36-54`` for images that are on one grid already: (63, 63, 3), channels new, ref, sub,
    each the zero-filled stamp (``Cutout2D(mode='partial', fill_value=0)``) divided by its L2 norm.  ``old_norm`` is
    the TensorFlow normalisation of the early models: not available here."""
    if old_norm:
        raise NotImplementedError('old_norm=True normalises with tensorflow.keras.utils.normalize, which this package '
                                  'does not depend on')
    triplet = np.zeros((CUTOUT_SIZE, CUTOUT_SIZE, 3))
    for i, img in enumerate([new_aligned, ref_aligned, sub_aligned]):
        data = np.asarray(img.data)
        ny, nx = data.shape
        w = img.wcs
        grid = WCS(w.crpix, w.crval, w.cd, w.pv1 if w.has_pv else None, w.pv2 if w.has_pv else None, (nx, ny))
        x0, y0 = _checked_origin(grid, [ra], [dec], CUTOUT_SIZE)
        block = _host_block(data, int(x0[0]), int(y0[0]), CUTOUT_SIZE).astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            triplet[:, :, i] = block / np.linalg.norm(block)
    return triplet


def triplets(detections, sub, size=CUTOUT_SIZE):
    """The triplets of all detections of a subtraction through the engine call of ``Thumbnail.from_detections``:
    [n, size, size, 3] float64, channels new, ref, sub (``make_triplet_for_braai``'s order), each divided by the norm
    the engine returns - the input of ``realbogus.RBModel.score_triplets`` (the filter itself scores the blocks where
    they lie: ``filter_sexcat(cat, rb_model=...)``)."""
    detections = list(detections)
    out = np.zeros((len(detections), int(size), int(size), 3))
    chan = {'new': 0, 'ref': 1, 'sub': 2}
    for blocks, norms, _, _, images, _ in _subtraction_blocks(detections, sub, size):
        for p, (typ, _) in enumerate(images):
            with np.errstate(divide='ignore', invalid='ignore'):
                out[:, :, :, chan[typ]] = blocks[:, p].astype(np.float64) / norms[:, p][:, None, None]
    return out
