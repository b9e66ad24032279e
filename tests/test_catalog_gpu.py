"""Subtraction -> PipelineFITSCatalog.from_image -> Detection.from_catalog on BASELINE config 0 (the set-up of
test_object_api_gpu.py: 4 frames 512 x 512, shared TAN WCS) with point sources injected into the science frame, against the numpy restatement
(tests/extract_ref.py) plus the same cuts on the same difference, noise and mask planes; scripts/dosub.py --detect."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

import extract_ref as xr
from util import pkg, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_frame(z, d, name, f):
    """sci / mask / weight FITS the way IPAC products sit on disk (as test_object_api_gpu.py writes them)."""
    path = os.path.join(d, name)
    z.fits.write(path, f['img'], f['header'])
    z.fits.write(path.replace('sciimg', 'mskimg'), f['mask'].astype(np.int16), f['header'])
    z.fits.write(path.replace('.fits', '.weight.fits'), f['wgt'], f['header'])
    im = z.ScienceImage.from_file(path)
    im.mask_image = z.MaskImage.from_file(path.replace('sciimg', 'mskimg'))
    return im


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _scene(z, s, d, nx, ny, n, seed, prefix, fwhm=2.2):
    """n dithered frames of one star field as IPAC-style files (sciimg + mskimg): the fixture of test_scripts_gpu.py"""
    base = s.ztf_wcs(nx, ny, tpv=True)
    rng = np.random.default_rng(seed)
    nst = int(nx * ny / 2500)
    xs, ys = rng.uniform(-20, nx + 20, nst), rng.uniform(-20, ny + 20, nst)
    fl = np.exp(rng.uniform(np.log(3e3), np.log(8e4), nst))
    ra, dec = base.all_pix2world(xs, ys, 0)
    ims, paths = [], []
    for i in range(n):
        w = s.ztf_wcs(nx, ny, dx=rng.uniform(-5, 5), dy=rng.uniform(-5, 5), rot_deg=rng.uniform(-0.05, 0.05))
        f = s.make_frame(nx, ny, seed + 1 + i, w, star_sky=(ra, dec, fl), fwhm=fwhm, sky=150.0 + 7 * i,
                         noise=4.0, bad_block=(60 + 37 * i, 90 + 23 * i, 4))
        hdr = f['header']
        hdr['OBSJD'] = 2458000.5 + hdr['OBSMJD'] - 58000.0 + i
        path = os.path.join(d, f'ztf_{prefix}{i:02d}_000651_zg_c03_o_q1_sciimg.fits')
        z.fits.write(path, f['img'], hdr)
        z.fits.write(path.replace('sciimg', 'mskimg'), f['mask'].astype(np.int16), hdr)
        im = z.ScienceImage.from_file(path)
        im.mask_image = z.MaskImage.from_file(path.replace('sciimg', 'mskimg'))
        ims.append(im)
        paths.append(path)
    return ims, paths


INJECT_SEED = 20240611
NINJECT = 30


def choose_injections(rng, n, nx, ny, avoid_xy, bad, border=30, apart=15.0):
    """n positions at least ``apart`` px from each other, from every position of ``avoid_xy``, from every bad pixel, and
    ``border`` px from the frame edge (rejection sampling with the given generator)."""
    by, bx = np.nonzero(bad)
    px, py = list(avoid_xy[0]), list(avoid_xy[1])
    out = []
    while len(out) < n:
        x, y = rng.uniform(border, nx - border), rng.uniform(border, ny - border)
        if len(px) and np.hypot(np.array(px) - x, np.array(py) - y).min() < apart:
            continue
        if len(bx) and np.hypot(bx - x, by - y).min() < apart:
            continue
        out.append((x, y))
        px.append(x)
        py.append(y)
    return np.array(out).T


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    z, s = pkg(), synth()
    d = str(tmp_path_factory.mktemp('detect'))
    base = s.tan_wcs(512, 512)
    rng = np.random.default_rng(1234)
    xs, ys = rng.uniform(10, 500, 40), rng.uniform(10, 500, 40)
    fl = np.exp(rng.uniform(np.log(1e3), np.log(1e5), 40))
    ra, dec = base.all_pix2world(xs, ys, 0)
    frames = []
    for i, (dx, dy) in enumerate([(0, 0), (3.3, -2.2), (-1.6, 4.1), (2.4, 1.3)]):
        w = s.tan_wcs(512, 512, dx=dx, dy=dy)
        f = s.make_frame(512, 512, 1234 + i, w, star_sky=(ra, dec, fl), fwhm=2.0,
                         bad_block=(50 + 60 * i, 80 + 40 * i, 5))
        f['header']['SEEING'] = 2.0
        frames.append(f)
    # transients: point sources of the frame's PSF added to the science frame itself (seed INJECT_SEED), bright (an
    # aperture S / N of 70 .. 180 against the frame's noise of 5 per pixel), 15 px or more from each other, from the
    # reference stars, from bad pixels, 30 px from the border
    f3 = frames[3]
    sx, sy = f3['wcs'].all_world2pix(ra, dec, 0)
    irng = np.random.default_rng(INJECT_SEED)
    ix, iy = choose_injections(irng, NINJECT, 512, 512, (sx, sy), f3['mask'] != 0)
    iflux = irng.uniform(2000.0, 5000.0, NINJECT)
    img = f3['img'].astype(np.float64)
    s.add_stars(img, ix, iy, iflux, 2.0)
    f3['img'] = img.astype(np.float32)
    ims = [write_frame(z, d, f'ztf_2020053{i}_000651_zg_c03_o_q1_sciimg.fits', f) for i, f in enumerate(frames)]
    ref = z.ReferenceImage.from_images(ims[:3], os.path.join(d, 'ref.000651_c03_q1_zg.fits'))
    sub = z.SingleEpochSubtraction.from_images(ims[3], ref, nreg_side=1, hotpants_kws={'ko': 0, 'bgo': 0})
    return dict(z=z, d=d, frames=frames, ims=ims, ref=ref, sub=sub, ix=ix, iy=iy)


def restated_detections(z, engine, sub):
    """The restatement's table on the planes the catalog route uses, kill_flagged, then filter_sexcat's cuts restated
    here in numpy (the three pixel cuts through ``pixel_cuts``, which has its own oracle test)."""
    weight = sub.weight_image.data
    _, _, plane, _ = engine.background(sub.data, weight, mesh=z.BKG_BOX_SIZE, filtersize=3, want=('sub',))
    rms, mask = sub.rms_image.data, sub.mask_image.data
    ref = xr.extract(plane, rms, bad=weight == 0, flag=mask, satur_level=float(sub.header.get('SATURATE', 50000.0)),
                     wcs=sub.wcs)
    tab = ref['table']
    tab = tab[((tab['IMAFLAGS_ISO'] & z.BAD_SUM) == 0) & (tab['FLAGS_WEIGHT'] == 0)]
    see = sub.header['SEEING']
    pix = z.pixel_cuts(sub.data, rms, sub.mask_image.boolean.data, tab['X_IMAGE'], tab['Y_IMAGE'], engine=engine)
    with np.errstate(divide='ignore', invalid='ignore'):
        good = ~((tab['IMAFLAGS_ISO'] & z.BAD_SUM) > 0) & ~(tab['FLAGS'] > 2) & ~(tab['A_IMAGE'] / tab['B_IMAGE'] > 2.0) \
            & ~(tab['FWHM_IMAGE'] / see > 2.0) & ~(tab['FWHM_IMAGE'] < 0.8 * see) & ~(pix['BPMCUT'] > 0) \
            & ~(pix['RMSCUT'] > pix['MEDCUT']) & ~(tab['FLUX_APER'] / tab['FLUXERR_APER'] < 5) & (pix['NEGPIX'] == 0)
    return ref, tab, good


def recovered(x, y, ix, iy):
    """every injection has a detection within 1 px (x, y: 1-based catalog positions)"""
    d = np.hypot(np.asarray(x)[:, None] - 1.0 - ix[None, :], np.asarray(y)[:, None] - 1.0 - iy[None, :])
    return d.min(axis=0) < 1.0 if len(x) else np.zeros(len(ix), bool)


def test_detections_equal_the_restatement_with_the_same_cuts(scene, engine):
    z, sub, ix, iy = scene['z'], scene['sub'], scene['ix'], scene['iy']
    ref, tab, good = restated_detections(z, engine, sub)
    # the input first: the restatement alone recovers every injected source after all cuts
    rec = recovered(tab['X_IMAGE'][good], tab['Y_IMAGE'][good], ix, iy)
    assert rec.all(), (np.flatnonzero(~rec), ix[~rec], iy[~rec])
    # then the GPU route
    cat = z.PipelineFITSCatalog.from_image(sub)
    assert cat.basename == sub.basename.replace('.fits', '.cat') and cat.image is sub and sub.catalog is cat
    assert os.path.exists(os.path.join(scene['d'], cat.basename))
    assert list(cat.data['NUMBER']) == list(tab['NUMBER'])              # the same rows survive kill_flagged
    dets = z.Detection.from_catalog(cat, filter=True)
    assert [d.goodcut for d in dets] == [True] * len(dets) and all(d.rb == -99.0 for d in dets)
    got_numbers = list(cat.data['NUMBER'][cat.data['GOODCUT'] == 1])
    assert got_numbers == list(tab['NUMBER'][good])
    assert len(dets) == int(good.sum())
    want = tab[good]
    for d, r in zip(dets, want):
        assert abs(d.x_image - r['X_IMAGE']) < 1e-9 and abs(d.y_image - r['Y_IMAGE']) < 1e-9
        assert d.flags == r['FLAGS'] and d.imaflags_iso == r['IMAFLAGS_ISO'] and d.image is sub
        assert abs(d.ra - r['X_WORLD']) < 1e-11 and abs(d.dec - r['Y_WORLD']) < 1e-11
    assert recovered([d.x_image for d in dets], [d.y_image for d in dets], ix, iy).all()
    # the filtered catalog on disk reloads to the same table, columns of the filter included
    again = z.PipelineFITSCatalog.from_file(cat.local_path)
    assert again.data.dtype.names == cat.data.dtype.names
    for n in ('GOODCUT', 'BPMCUT', 'RMSCUT', 'rb'):
        assert n in again.data.dtype.names
    for n in cat.data.dtype.names:
        assert np.array_equal(again.data[n], cat.data[n], equal_nan=True), n
    assert again.table_header['ZMDEBLND'] is False and again.table_header['ZMCLEAN'] is False
    # a filtered catalog is not filtered twice
    assert z.filter_sexcat(cat) is cat


def test_segm_check_image_equals_the_map(scene, engine):
    z, sub = scene['z'], scene['sub']
    ref, _, _ = restated_detections(z, engine, sub)
    sub._call_source_extractor(checkimage_type=['segm'])
    assert sub._segmimg.basename == sub.basename.replace('.fits', '.segm.fits')
    assert np.array_equal(sub._segmimg.data, ref['segm'])
    assert os.path.exists(os.path.join(scene['d'], sub._segmimg.basename))


def test_default_calls_do_no_extraction(scene, engine, monkeypatch):
    z, sub = scene['z'], scene['sub']
    sx = importlib.import_module('zuds-pipeline_amd.sextractor')

    def boom(*a, **k):
        raise AssertionError('a default call must not run the extractor')
    monkeypatch.setattr(z.Engine, 'extract', boom)
    out = sx.run_sextractor(sub, checkimage_type=['rms', 'bkg'])
    assert out[0] is None and [o.basename.split('.')[-2] for o in out[1:]] == ['rms', 'bkg']
    assert sx.run_sextractor(sub)[0] is None
    with pytest.raises(ValueError):
        sx.run_sextractor(sub, catalog=True, sextractor_kws={'DEBLEND_NTHRESH': 32})


def test_device_plane_route_gives_the_host_route_table(scene, engine):
    """DeviceSubtraction.extract on its resident planes against Engine.extract on the same planes from the host."""
    import torch
    z, sub, ref, sci, f = scene['z'], scene['sub'], scene['ref'], scene['ims'][3], scene['frames'][3]
    dmod = importlib.import_module('zuds-pipeline_amd.device')
    ds = dmod.DeviceSubtraction(sci.wcs, ref.wcs, device=0, engine=engine)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to('cuda:0')
    args = (t(f['img'], np.float32), t(sci.rms_image.data, np.float32), t(f['mask'], np.int32),
            t(sci.weight_image.data, np.float32), t(ref.data, np.float32),
            t(ref.rms_image.data, np.float32), t(ref.mask_image.data, np.int32))
    torch.cuda.synchronize()
    diff, noise, submask = ds.run(*args, seeing=2.0, nreg_side=1, hotpants_kws={'ko': 0, 'bgo': 0},
                                  ref_flxscale=float(ref.header.get('FLXSCALE', 1.0)))
    tab, nfound, segm = ds.extract()
    ds.stream.synchronize()
    engine.set_stream(0)
    assert np.array_equal(diff.cpu().numpy(), sub.data)                  # the planes the host route sees
    mask = sub.mask_image.data
    htab, hsegm = engine.extract(sub.data, sub.rms_image.data, bad=(mask & z.BAD_SUM) != 0, flag=mask, wcs=sci.wcs)
    assert nfound == len(htab) > NINJECT // 2
    assert tab.tobytes() == htab.tobytes()
    assert np.array_equal(segm.cpu().numpy(), hsegm)


def test_dosub_detect_writes_the_catalog(tmp_path, engine, monkeypatch, capsys):
    """scripts/dosub.py: without the switch the files of today; ``--detect`` through the command line's own argument
    handling; the driver's guard against too many detections."""
    z, s = pkg(), synth()
    d = str(tmp_path)
    refims, _ = _scene(z, s, d, 640, 600, 3, 4300, '201912', fwhm=2.0)
    refname = os.path.join(d, 'ref.000651_c03_q1_zg.fits')
    z.ReferenceImage.from_images(refims, refname, sci_swarp_kws={'COMBINE_TYPE': 'WEIGHTED'})
    _, spaths = _scene(z, s, d, 640, 600, 3, 4400, '202003', fwhm=2.6)
    script = load_script('dosub')
    subnames = [z.sub_name(p, refname) for p in spaths]
    stem = [os.path.basename(n)[:-5] for n in subnames]

    def listing(k, names):
        return {n.replace(stem[k], 'S') for n in names if n.startswith(stem[k])}
    before = set(os.listdir(d))
    sub = script.do_one(spaths[0], z.ScienceImage, z.SingleEpochSubtraction, refname, tmpdir=d)
    plain = listing(0, set(os.listdir(d)) - before)
    assert sub.local_path == subnames[0]
    assert plain >= {'S.fits', 'S.rms.fits', 'S.mask.fits'} and not any(n.endswith('.cat') for n in plain)
    # this scene subtracts stars of FWHM 2.6 from a FWHM 2.0 reference without injected transients: what passes the cuts
    # are star residuals, more than the driver's guard (MAX_DETS = 50, the reference's value) lets through
    assert script.MAX_DETS == 50
    monkeypatch.setattr(script, 'MAX_DETS', 10 ** 6)
    jobs = os.path.join(d, 'images.txt')
    with open(jobs, 'w') as f:
        f.write(spaths[1] + '\n')
    before = set(os.listdir(d))
    assert script.main([jobs, '--detect', refname]) == 0                  # the switch may stand anywhere
    out = capsys.readouterr().out
    assert 'cat: ' in out and 'det: ' in out and 'Traceback' not in out
    new = listing(1, set(os.listdir(d)) - before)
    # the files a plain run writes, the catalog, and the weight map the extractor asked the subtraction for (saved next
    # to it like every derived map): nothing else
    assert new - plain <= {'S.cat', 'S.weight.fits'} and 'S.cat' in new and plain <= new, (new, plain)
    cat = z.PipelineFITSCatalog.from_file(subnames[1].replace('.fits', '.cat'))
    ngood = int((cat.data['GOODCUT'] == 1).sum())
    assert 'GOODCUT' in cat.data.dtype.names and ngood > 0
    # the function itself returns the detections as well
    sub2, dets = script.do_one(spaths[2], z.ScienceImage, z.SingleEpochSubtraction, refname, tmpdir=d, detect=True)
    cat2 = z.PipelineFITSCatalog.from_file(subnames[2].replace('.fits', '.cat'))
    assert len(dets) == int((cat2.data['GOODCUT'] == 1).sum()) > 0
    assert all(isinstance(x, z.Detection) for x in dets)
    # and the guard raises
    monkeypatch.setattr(script, 'MAX_DETS', len(dets) - 1)
    os.remove(subnames[2])
    with pytest.raises(z.TooManyDetectionsError):
        script.do_one(spaths[2], z.ScienceImage, z.SingleEpochSubtraction, refname, tmpdir=d, detect=True)
