"""Thumbnails of a subtraction through the object API (zuds-pipeline_amd/thumbnails.py) on the synthetic epoch of
test_catalog_gpu.py: ``Thumbnail.from_detections`` against the slow route written out here - ``sub.aligned_to(ref)`` /
``sci.aligned_to(ref)`` whole, a numpy crop by the origin rule, the same writer -, the device and the host route, the
triplets, and ``scripts/dosub.py --detect --stamps``."""
import gzip
import importlib
import os

import numpy as np
import pytest

from test_catalog_gpu import _scene, load_script, scene  # noqa: F401  (the fixture and the drivers' job files)
from util import pkg, synth

pytestmark = pytest.mark.gpu


class Det(object):
    def __init__(self, ra, dec):
        self.ra, self.dec = float(ra), float(dec)


def origin_restated(w, ra, dec, S):
    x, y = w.all_world2pix(ra, dec, 0)
    return np.ceil(x - S / 2.0).astype(int), np.ceil(y - S / 2.0).astype(int)


def crop_trim(data, x0, y0, S):
    ny, nx = data.shape
    xa, xb, ya, yb = max(x0, 0), min(x0 + S, nx), max(y0, 0), min(y0 + S, ny)
    return data[ya:yb, xa:xb], (xa, ya)


def crop_partial(data, x0, y0, S):
    out = np.zeros((S, S), data.dtype)
    t, (xa, ya) = crop_trim(data, x0, y0, S)
    out[ya - y0:ya - y0 + t.shape[0], xa - x0:xa - x0 + t.shape[1]] = t
    return out


def slow_bytes(z, data, w, x0, y0, S=63):
    """The stamp file of the reference's route: trimmed crop + the grid's WCS cards with CRPIX moved to the crop."""
    t, (xa, ya) = crop_trim(data, x0, y0, S)
    cards = w.to_header()
    cards['CRPIX1'] = float(w.crpix[0]) - xa
    cards['CRPIX2'] = float(w.crpix[1]) - ya
    return gzip.compress(z.fits.to_bytes(np.ascontiguousarray(t), cards), compresslevel=9, mtime=0)


def detections_of(scene):
    """The injected transients (where the catalog finds its detections) plus positions whose stamps hang over each edge
    and corner of the reference grid."""
    z, ref, f3 = scene['z'], scene['ref'], scene['frames'][3]
    ra, dec = f3['wcs'].all_pix2world(scene['ix'], scene['iy'], 0)
    dets = [Det(a, b) for a, b in zip(ra, dec)]
    nx, ny = ref.wcs.naxis
    for x, y in [(3.2, ny / 2.0), (nx - 2.5, ny / 3.0), (nx / 2.0, 1.0), (nx / 3.0, ny - 1.7), (0.0, 0.0), (nx - 1.0, ny - 1.0),
                 (-20.0, 40.0), (100.0, ny + 25.0)]:
        a, b = ref.wcs.all_pix2world([x], [y], 0)
        dets.append(Det(a[0], b[0]))
    return dets


@pytest.fixture(scope='module')
def slow(scene):
    """The whole-frame alignments of the reference's route (scripts/dosub.py:133-142)."""
    sub, ref, sci = scene['sub'], scene['ref'], scene['ims'][3]
    assert sub.reference_image is ref and sub.target_image is sci
    return dict(sub=sub.aligned_to(ref), new=sci.aligned_to(ref), ref=ref)


def test_stamps_of_a_single_epoch_subtraction_equal_the_slow_route(scene, slow, engine, monkeypatch):
    z, sub, ref = scene['z'], scene['sub'], scene['ref']
    dets = detections_of(scene)
    monkeypatch.delenv('ZM_OBJECT_API', raising=False)
    stamps = z.Thumbnail.from_detections(dets, sub)
    assert len(stamps) == 3 * len(dets)
    w = ref.wcs
    x0, y0 = origin_restated(w, [d.ra for d in dets], [d.dec for d in dets], 63)
    trimmed = 0
    for k, d in enumerate(dets):
        for p, typ in enumerate(('sub', 'new', 'ref')):
            t = stamps[3 * k + p]
            assert t.type == typ and t.detection is d
            assert t.image is {'sub': sub, 'new': sub.target_image, 'ref': ref}[typ]
            want = slow_bytes(z, slow[typ].data, w, int(x0[k]), int(y0[k]))
            assert t.bytes == want, (k, typ)
            # and the reference's own loop (zuds/thumbnails.py:54-94) over the aligned images gives those bytes too
            assert z.Thumbnail.from_detection(d, slow[typ]).bytes == want
            assert z.Thumbnail.from_detection(d, slow[typ]).type == typ
            trimmed += t.array.shape != (63, 63)
    assert trimmed >= 3 * 8                                   # the edge positions give smaller stamps
    # the host route: the same bytes
    monkeypatch.setenv('ZM_OBJECT_API', 'host')
    host = z.Thumbnail.from_detections(dets, sub)
    assert [t.bytes for t in host] == [t.bytes for t in stamps]
    assert [t.type for t in host] == [t.type for t in stamps]


def test_device_subtraction_stamps_equal_the_object_route(scene, slow, engine):
    """DeviceSubtraction.stamps on its resident difference image: the blocks of the slow route, zero padded."""
    import torch
    z, sub, ref, sci, f = scene['z'], scene['sub'], scene['ref'], scene['ims'][3], scene['frames'][3]
    dmod = importlib.import_module('zuds-pipeline_amd.device')
    ds = dmod.DeviceSubtraction(sci.wcs, ref.wcs, device=0, engine=engine)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to('cuda:0')
    args = (t(f['img'], np.float32), t(sci.rms_image.data, np.float32), t(f['mask'], np.int32),
            t(sci.weight_image.data, np.float32), t(ref.data, np.float32),
            t(ref.rms_image.data, np.float32), t(ref.mask_image.data, np.int32))
    torch.cuda.synchronize()
    ds.run(*args, seeing=2.0, nreg_side=1, hotpants_kws={'ko': 0, 'bgo': 0},
           ref_flxscale=float(ref.header.get('FLXSCALE', 1.0)), wait=False)
    dets = detections_of(scene)
    ra, dec = [d.ra for d in dets], [d.dec for d in dets]
    blocks, norms, x0, y0 = ds.stamps(ra, dec, args[0], args[4], sci_flxscale=float(sci.header.get('FLXSCALE', 1.0)))
    ds.stream.synchronize()
    engine.set_stream(0)
    rx, ry = origin_restated(ref.wcs, ra, dec, 63)
    assert np.array_equal(x0, rx) and np.array_equal(y0, ry)
    for k in range(len(dets)):
        for p, typ in enumerate(('sub', 'new', 'ref')):
            want = crop_partial(np.asarray(slow[typ].data, np.float32), int(x0[k]), int(y0[k]), 63)
            assert np.array_equal(blocks[k, p].view(np.uint32), want.view(np.uint32)), (k, typ)
    with pytest.raises(ValueError):
        ds.stamps([np.nan], [0.0], args[0], args[4])


def test_multi_epoch_subtraction_is_gathered_only(scene, engine, monkeypatch):
    z, ref = scene['z'], scene['ref']
    rng = np.random.default_rng(3)
    shape = ref.data.shape

    def image(cls, name, data):
        im = cls()
        im.basename = name
        im.header, im.header_comments, im.data = dict(ref.header), {}, data
        return im
    d_sub = rng.normal(0, 5, shape).astype(np.float32)
    d_new = rng.normal(150, 5, shape).astype(np.float32)
    d_sub[40, 50] = np.nan
    msub = image(z.MultiEpochSubtraction, 'sub.multi.fits', d_sub)
    msub.target_image = image(z.ScienceCoadd, 'multi.coadd.fits', d_new)
    msub.reference_image = ref
    a, b = ref.wcs.all_pix2world([52.0, 3.0, 200.7], [41.0, 300.2, 100.1], 0)
    dets = [Det(x, y) for x, y in zip(a, b)]
    seen = []
    real = z.Engine.stamps

    def spy(self, planes, *args, **kw):
        seen.append([bool(p.get('on_grid')) for p in planes])
        return real(self, planes, *args, **kw)
    monkeypatch.setattr(z.Engine, 'stamps', spy)
    for route in ('device', 'host'):
        monkeypatch.setenv('ZM_OBJECT_API', route)
        stamps = z.Thumbnail.from_detections(dets, msub)
        x0, y0 = origin_restated(ref.wcs, a, b, 63)
        for k in range(3):
            for p, (typ, data) in enumerate((('sub', d_sub), ('new', d_new), ('ref', ref.data))):
                t = stamps[3 * k + p]
                assert t.type == typ and t.bytes == slow_bytes(z, np.asarray(data, np.float32), ref.wcs, int(x0[k]), int(y0[k]))
        assert np.isnan(stamps[0].array).any()                 # a gathered NaN stays a NaN
    assert seen and all(all(flags) for flags in seen)          # nothing was resampled


def test_triplets(scene, slow, engine):
    z, sub, ref = scene['z'], scene['sub'], scene['ref']
    dets = detections_of(scene)
    t = z.triplets(dets, sub)
    assert t.shape == (len(dets), 63, 63, 3)
    x0, y0 = origin_restated(ref.wcs, [d.ra for d in dets], [d.dec for d in dets], 63)
    worst = bound = 0.0
    for k in range(len(dets)):
        for c, typ in enumerate(('new', 'ref', 'sub')):          # make_triplet_for_braai's channel order
            block = crop_partial(np.asarray(slow[typ].data, np.float32), int(x0[k]), int(y0[k]), 63).astype(np.float64)
            sq = (block ** 2).ravel()
            fwd, rev = np.sqrt(sq.sum()), np.sqrt(sq[::-1].sum())
            if fwd == 0.0:            # a stamp over ground the frame does not cover: 0 / 0, as the reference's division gives
                assert np.isnan(t[k, :, :, c]).all()
                continue
            # the engine's norm is within the order bound of numpy's (tests/test_stamps_gpu.py); dividing by it and
            # rounding each quotient to float64 adds one spacing (2^-53 relative) per element, and numpy's own norm of
            # the 3969 quotients at most 3969 spacings of its result
            tol = 10.0 * abs(fwd - rev) / fwd + 3970 * 2.0 ** -53
            worst, bound = max(worst, abs(np.linalg.norm(t[k, :, :, c]) - 1.0)), max(bound, tol)
            assert abs(np.linalg.norm(t[k, :, :, c]) - 1.0) <= tol
            np.testing.assert_allclose(t[k, :, :, c], block / np.linalg.norm(block), rtol=tol, atol=0)
            assert np.array_equal(t[k, :, :, c] == 0, block == 0)
    print(f'triplets: largest | norm - 1 | {worst:.3g} (largest bound {bound:.3g})')
    k = len(dets) - 8                                          # (3.2, ny / 2): the stamp hangs over the left edge
    assert x0[k] < 0 and np.all(t[k, :, :-x0[k], :] == 0) and np.any(t[k, :, -x0[k]:, :] != 0)
    # the function for images already on one grid gives the same channels
    one = z.make_triplet_for_braai(dets[0].ra, dets[0].dec, slow['new'], slow['ref'], slow['sub'])
    np.testing.assert_allclose(one, t[0], rtol=bound, atol=0)
    assert worst > 0.0 or bound > 0.0


def test_dosub_stamps_writes_the_stamps_file(tmp_path, engine, monkeypatch, capsys):
    z, s = pkg(), synth()
    d = str(tmp_path)
    refims, _ = _scene(z, s, d, 640, 600, 3, 4300, '201912', fwhm=2.0)
    refname = os.path.join(d, 'ref.000651_c03_q1_zg.fits')
    z.ReferenceImage.from_images(refims, refname, sci_swarp_kws={'COMBINE_TYPE': 'WEIGHTED'})
    _, spaths = _scene(z, s, d, 640, 600, 3, 4400, '202003', fwhm=2.6)
    script = load_script('dosub')
    monkeypatch.setattr(script, 'MAX_DETS', 10 ** 6)
    subnames = [z.sub_name(p, refname) for p in spaths]
    stem = [os.path.basename(n)[:-5] for n in subnames]

    def run(k, flags):
        jobs = os.path.join(d, f'images{k}.txt')
        with open(jobs, 'w') as f:
            f.write(spaths[k] + '\n')
        before = set(os.listdir(d))
        assert script.main([jobs, refname] + flags) == 0
        out = capsys.readouterr().out
        assert 'Traceback' not in out, out
        return {n.replace(stem[k], 'S') for n in set(os.listdir(d)) - before if n.startswith(stem[k])}, out
    plain, out = run(0, ['--detect'])
    assert 'stamp: ' not in out and not any('stamps' in n for n in plain)
    new, out = run(1, ['--detect', '--stamps'])
    assert 'stamp: ' in out and new == plain | {'S.stamps.fits'}, (new, plain)
    cat = z.PipelineFITSCatalog.from_file(subnames[1].replace('.fits', '.cat'))
    good = cat.data[cat.data['GOODCUT'] == 1]
    blocks, hdr, tab, _ = z.fits.read_image_table(subnames[1].replace('.fits', '.stamps.fits'))
    assert len(good) > 0 and blocks.shape == (len(good), 3, 63, 63) and blocks.dtype == np.float32
    assert len(tab) == len(good) and hdr['NDET'] == len(good) and hdr['STAMPSZ'] == 63
    assert np.array_equal(tab['ra'], good['X_WORLD']) and np.array_equal(tab['dec'], good['Y_WORLD'])
    ref = z.ReferenceImage.from_file(refname, load_others=False)
    x0, y0 = origin_restated(ref.wcs, tab['ra'], tab['dec'], 63)
    assert np.array_equal(tab['x0'], x0) and np.array_equal(tab['y0'], y0)
    for k in range(len(tab)):
        assert np.array_equal(blocks[k, 2], crop_partial(np.asarray(ref.data, np.float32), int(x0[k]), int(y0[k]), 63))
        t, _ = crop_trim(ref.data, int(x0[k]), int(y0[k]), 63)
        assert (tab['ny_trim'][k], tab['nx_trim'][k]) == t.shape
    assert np.isfinite(blocks).all() and np.any(blocks[:, 0] != 0) and np.any(blocks[:, 1] != 0)
    # --stamps without --detect is refused; the function returns the thumbnails as third item
    assert script.main([os.path.join(d, 'images1.txt'), refname, '--stamps']) == 2
    sub, dets, thumbs = script.do_one(spaths[2], z.ScienceImage, z.SingleEpochSubtraction, refname, tmpdir=d, detect=True,
                                      stamps=True)
    assert len(thumbs) == 3 * len(dets) > 0 and [t.type for t in thumbs[:3]] == ['sub', 'new', 'ref']
    assert all(isinstance(t, z.Thumbnail) for t in thumbs)
