"""The reference's candidate filter.

``filter_sexcat`` (``zuds/filterobjects.py:57-195``) mixes cuts on catalog columns with
three tests that need only pixels; those three are computed on the GPU for any list of
positions (``X_IMAGE``, ``Y_IMAGE``: 1-based, as SExtractor reports them) by ``pixel_cuts``:

* ``BPMCUT``  exact-overlap aperture sum (r = 6 px) of the boolean bad-pixel map; must be 0;
* ``RMSCUT``  aperture sum of the rms map / (pi 6^2); must not exceed 1.1 x the median rms of
  the good pixels;
* negative-pixel cut: a pixel of the 11 x 11 cutout below -5 sigma with a 3 x 3 neighbour above
  +5 sigma, sigma = 1.48 x MAD of the image about its median (``filterobjects.py:155-162``).

``filter_sexcat(cat)`` is the whole filter on a ``PipelineFITSCatalog``: the column cuts in the reference's order,
then the pixel cuts.  Without a model the braai CNN score is not computed: ``rb`` is -99 for every row, as the
reference leaves it for rows that never reach the network.  ``filter_sexcat(cat, rb_model=m)`` (``realbogus.load_model``)
scores the rows that survive the pixel cuts (``csrc/braai.hip``) and drops those with ``rb < RB_CUT[image.fid]``
(``zuds/filterobjects.py:196-240``).
"""
import ctypes as C

import numpy as np

from ._lib import check, ptr
from .constants import BAD_SUM, RB_CUT
from .engine import get_engine

__all__ = ['pixel_cuts', 'pixel_cuts_dev', 'column_cuts', 'filter_table', 'filter_sexcat', 'CUTSIZE', 'good_before_ml',
           'rb_cut_for']

CUTSIZE = 11          # pixels, zuds/filterobjects.py:12
CUT_RADIUS = 6.0      # zuds/filterobjects.py:102-104


def pixel_cuts(data, rms, bpm, x_image, y_image, engine=None):
    """dict(BPMCUT, RMSCUT, MEDCUT, NEGPIX, GOODCUT) for candidates at (x_image, y_image).

    ``GOODCUT`` holds 1 where all three pixel cuts pass (the catalog-column cuts of the
    reference are the caller's)."""
    eng = engine or get_engine()
    data = np.ascontiguousarray(data, dtype=np.float32)
    rms = np.ascontiguousarray(rms, dtype=np.float32)
    bpm = np.ascontiguousarray(bpm).astype(bool)
    x = np.ascontiguousarray(x_image, dtype=np.float64)
    y = np.ascontiguousarray(y_image, dtype=np.float64)
    n = x.size
    area = np.pi * CUT_RADIUS ** 2
    # photutils takes 0-based positions; the reference passes X_IMAGE / Y_IMAGE unchanged
    # (filterobjects.py:83-104), i.e. apertures sit one pixel high and right of the source.
    rmsbig, _, _ = eng.aperture_photometry(rms, x, y, radius=CUT_RADIUS)
    bpmbig, _, _ = eng.aperture_photometry(bpm.astype(np.float32), x, y, radius=CUT_RADIUS)
    med, _ = eng.median_mad(rms, bpm.astype(np.int32))
    medcut = 1.1 * med
    immed, immad = eng.median_mad(data)
    imsig = 1.48 * (immad / 1.4826)
    neg = np.zeros(n, np.int32)
    if n:
        ny, nx = data.shape
        check(eng.L.zm_negpix_test(eng.ctx, ptr(data), nx, ny, n, ptr(x), ptr(y), float(immed),
                                   float(imsig), ptr(neg)), 'zm_negpix_test')
    rmscut = rmsbig / area
    good = (bpmbig <= 0) & (rmscut <= medcut) & (neg == 0)
    return dict(BPMCUT=bpmbig, RMSCUT=rmscut, MEDCUT=medcut, NEGPIX=neg, GOODCUT=good.astype(np.uint8))


def pixel_cuts_dev(engine, img, rms, mask, x_image, y_image, bad_bits=BAD_SUM):
    """``pixel_cuts`` on planes that are already in HBM (``zm_candidate_cuts_dev``): ``img`` / ``rms`` float32 and
    ``mask`` int32 torch tensors on the engine's GPU; a pixel is bad where ``mask & bad_bits``.  The frame statistics
    are taken on the device and read there by the cuts; only the positions and the per-candidate results cross PCIe.  Enqueued on the stream the engine is bound to and
    waited for.  Same dict as ``pixel_cuts``; without candidates the kernel is not launched and ``MEDCUT`` comes from the
    select alone (``zm_median_mad_dev`` on the same planes: the same number)."""
    import torch
    for name, t, dt in (('img', img, torch.float32), ('rms', rms, torch.float32), ('mask', mask, torch.int32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != engine.device:
            raise ValueError(f'{name}: must be a tensor on the engine\'s GPU (cuda:{engine.device})')
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f'{name}: device planes must be contiguous {dt} tensors')
    if tuple(rms.shape) != tuple(img.shape) or tuple(mask.shape) != tuple(img.shape) or img.dim() != 2:
        raise ValueError('img, rms and mask must be planes of one shape')
    ny, nx = (int(v) for v in img.shape)
    x = np.ascontiguousarray(np.atleast_1d(x_image), dtype=np.float64)
    y = np.ascontiguousarray(np.atleast_1d(y_image), dtype=np.float64)
    if x.shape != y.shape:
        raise ValueError('x_image and y_image must have the same shape')
    n = x.size
    bpmcut, rmscut, neg = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
    stats = np.full(3, np.nan)
    if n == 0:
        # (zm_candidate_cuts_dev returns at once: the median of the good pixels' rms on its own)
        good_mask = mask & int(bad_bits)
        torch.cuda.current_stream(img.device).synchronize()
        med, mad = C.c_double(), C.c_double()
        check(engine.L.zm_median_mad_dev(engine.ctx, rms.data_ptr(), good_mask.data_ptr(), nx * ny, C.byref(med),
                                         C.byref(mad)), 'zm_median_mad_dev')
        stats[0] = 1.1 * med.value
    else:
        check(engine.L.zm_candidate_cuts_dev(engine.ctx, img.data_ptr(), rms.data_ptr(), mask.data_ptr(), int(bad_bits),
                                             nx, ny, n, ptr(x), ptr(y), ptr(bpmcut), ptr(rmscut), ptr(neg), ptr(stats)),
              'zm_candidate_cuts_dev')
    medcut = float(stats[0])
    good = (bpmcut <= 0) & (rmscut <= medcut) & (neg == 0)
    return dict(BPMCUT=bpmcut, RMSCUT=rmscut, MEDCUT=medcut, NEGPIX=neg, GOODCUT=good.astype(np.uint8))


def column_cuts(table, see, bpmcut, rmscut, medcut):
    """GOODCUT (uint8) after the reference's catalog-column cuts, in its order (``zuds/filterobjects.py:125-148``),
    and the number of candidates left after each of them."""
    good = np.ones(len(table), dtype=np.uint8)
    left = []
    with np.errstate(divide='ignore', invalid='ignore'):
        for name, fails in (('external flag', (table['IMAFLAGS_ISO'] & BAD_SUM) > 0),
                            ('internal flag', table['FLAGS'] > 2),
                            ('elipticity', table['A_IMAGE'] / table['B_IMAGE'] > 2.0),
                            ('fwhm', table['FWHM_IMAGE'] / see > 2.0),
                            ('sharp', table['FWHM_IMAGE'] < 0.8 * see),
                            ('bpm', np.asarray(bpmcut) > 0),
                            ('rms', np.asarray(rmscut) > medcut),
                            ('s/n > 5', table['FLUX_APER'] / table['FLUXERR_APER'] < 5)):
            good[np.where(fails)] = 0
            left.append((name, int(good.sum())))
    return good, left


def _append_columns(table, **cols):
    out = np.zeros(len(table), dtype=table.dtype.descr + [(k, np.asarray(v).dtype.str) for k, v in cols.items()])
    for n in table.dtype.names:
        out[n] = table[n]
    for k, v in cols.items():
        out[k] = v
    return out.view(np.recarray)


def rb_cut_for(fid=None, rb_cut=None):
    """The real / bogus threshold: ``rb_cut`` when given, else ``RB_CUT[fid]`` (``zuds/constants.py:18-21``).  Neither:
    ``ValueError`` - the cut differs between filters and is not guessed."""
    if rb_cut is not None:
        return float(rb_cut)
    try:
        return float(RB_CUT[int(fid)])
    except (TypeError, ValueError, KeyError):
        raise ValueError(f'no real / bogus cut: filter id {fid!r} is not one of {sorted(RB_CUT)} and no rb_cut is given')


def filter_sexcat(cat, engine=None, quiet=False, rb_model=None, rb_cut=None):
    """Filter the catalog of a subtraction (``zuds/filterobjects.py:57-246``): adds ``GOODCUT``, ``BPMCUT``,
    ``RMSCUT`` and ``rb`` columns and saves the catalog.  A catalog that already has a ``GOODCUT`` column is returned as
    it is.  ``rb_model`` (``realbogus.RBModel``): the rows that survive the pixel cuts get their triplets
    (``thumbnails._subtraction_blocks``: on the device route the blocks stay in HBM) and their score, and are cut at
    ``rb_cut`` or ``RB_CUT[image.fid]``; without it ``rb`` is -99 (the CNN step is skipped)."""
    say = (lambda *a, **k: None) if quiet else print
    if 'GOODCUT' in cat.data.dtype.names:
        return cat
    image = cat.image
    rms = image.rms_image.data
    bpm = image.mask_image.boolean.data
    table = cat.data
    say('Total number of candidates: ', len(table))
    if 'SEEING' not in image.header:
        from .seeing import estimate_seeing
        estimate_seeing(image)
    see = image.header['SEEING']
    pix = pixel_cuts(image.data, rms, bpm, table['X_IMAGE'], table['Y_IMAGE'], engine=engine)
    if rb_model is None:
        cat.data = filter_table(table, see, pix, say=say)
    else:
        cut = rb_cut_for(getattr(image, 'fid', None), rb_cut)
        rows = table[good_before_ml(table, see, pix) > 0]
        rb = _score_rows(rows, image, rb_model, engine)
        cat.data = filter_table(table, see, pix, say=say, rb=rb, rb_cut=cut)
        cat.rb_version = rb_model.name
    cat.save()
    return cat


def _score_rows(rows, sub, rb_model, engine=None):
    """rb of the catalog rows ``rows`` of the subtraction ``sub``: their stamps (sub, new, ref on the reference's grid,
    one engine call per grid) scored by ``rb_model``."""
    from . import thumbnails

    class _At(object):
        def __init__(self, ra, dec):
            self.ra, self.dec = ra, dec
    if len(rows) == 0:
        return np.zeros(0)
    dets = [_At(float(r['X_WORLD']), float(r['Y_WORLD'])) for r in rows]
    eng = engine or get_engine()
    per = {}
    for blocks, norms, _, _, images, _ in thumbnails._subtraction_blocks(dets, sub, rb_model.in_size, device_out=True):
        for p, (typ, _) in enumerate(images):
            per[typ] = (blocks[:, p], norms[:, p])
    order = thumbnails.STAMP_TYPES
    if isinstance(per[order[0]][0], np.ndarray):
        blocks = np.stack([per[t][0] for t in order], axis=1)
        norms = np.stack([per[t][1] for t in order], axis=1)
        return rb_model.score_blocks(blocks, norms, order=order, engine=eng).astype(np.float64)
    import torch
    from . import objdev
    eng = get_engine()                                    # the engine _subtraction_blocks bound to the I/O stream
    stream = objdev.get_io().stream
    with torch.cuda.stream(stream):
        blocks = torch.stack([per[t][0] for t in order], dim=1).contiguous()
        norms = torch.stack([per[t][1] for t in order], dim=1).contiguous()
        rb = rb_model.score_dev(blocks, norms, order=order, engine=eng, stream=stream)
        out = rb.cpu()
    stream.synchronize()
    return out.numpy().astype(np.float64)


def good_before_ml(table, see, pix):
    """``GOODCUT`` behind the column cuts and the negpix cut: the rows the reference hands to the network."""
    good, _ = column_cuts(table, see, pix['BPMCUT'], pix['RMSCUT'], pix['MEDCUT'])
    good[pix['NEGPIX'] != 0] = 0
    return good


def filter_table(table, see, pix, say=None, rb=None, rb_cut=None):
    """The filter itself, for any route that has the pixel cuts ``pix`` (``pixel_cuts`` / ``pixel_cuts_dev``) of the
    rows of ``table``: the column cuts in the reference's order, then the negpix cut; returns the table with the
    ``GOODCUT``, ``BPMCUT``, ``RMSCUT`` and ``rb`` columns appended.  ``say``: where the reference's count lines
    go (``filter_sexcat`` prints them).  ``rb``: the scores of the rows that still have ``GOODCUT > 0`` behind the negpix
    cut (``good_before_ml``), in table order - those rows get them, every other row keeps -99 - and ``GOODCUT`` is
    cleared where ``rb < rb_cut`` (``zuds/filterobjects.py:233-236``; NaN < cut is false: a row whose stamp has a zero
    norm keeps its ``GOODCUT``, as in the reference).  Without ``rb``: -99 everywhere, no ML cut."""
    say = say or (lambda *a, **k: None)
    good, left = column_cuts(table, see, pix['BPMCUT'], pix['RMSCUT'], pix['MEDCUT'])
    for name, n in left:
        say(f'Number of candidates after {name} cut: ', n)
    good[pix['NEGPIX'] != 0] = 0
    say('Number of candidates after negpix cut: ', int(good.sum()))
    rbcol = np.full(len(table), -99.0)
    if rb is not None:
        if rb_cut is None:
            raise ValueError('filter_table: rb needs rb_cut')
        rb = np.asarray(rb, dtype=np.float64).ravel()
        alive = np.flatnonzero(good > 0)
        if rb.size != alive.size:
            raise ValueError(f'filter_table: {alive.size} rows reach the network, {rb.size} scores given')
        rbcol[alive] = rb
        with np.errstate(invalid='ignore'):
            good[alive[rb < float(rb_cut)]] = 0
        say('Number of candidates after ML cut: ', int(good.sum()))
    return _append_columns(table, GOODCUT=good, BPMCUT=pix['BPMCUT'], RMSCUT=pix['RMSCUT'], rb=rbcol)
