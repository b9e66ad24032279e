"""Detections in the nightly pool: ``DeviceSubtraction.candidates`` against its pieces composed by hand, and
``SubtractionJob(detect=True, stamps=True)`` in every lane form of ``SubtractionPool``."""
import importlib

import numpy as np
import pytest

import cuts_ref as cref
from util import pkg, synth

pytestmark = pytest.mark.gpu

NTRANS = 6


def choose_injections(rng, n, nx, ny, avoid_xy, clean, border=40, apart=15.0):
    """n positions at least ``apart`` px from each other and from every position of ``avoid_xy``, ``border`` px from the
    frame edge, on pixels where ``clean`` holds (rejection sampling with the given generator)."""
    px, py = list(avoid_xy[0]), list(avoid_xy[1])
    out = []
    for _ in range(100000):
        if len(out) == n:
            break
        x, y = rng.uniform(border, nx - border), rng.uniform(border, ny - border)
        if not clean[int(round(y)), int(round(x))]:
            continue
        if np.hypot(np.array(px) - x, np.array(py) - y).min() < apart:
            continue
        out.append((x, y))
        px.append(x)
        py.append(y)
    assert len(out) == n, 'the scene has no room for its transients'
    return np.array(out).T


def clean_ground(z, res, half=13):
    """Where a transient can pass the reference's filter at all, from the products of the same job WITHOUT transients:
    pixels whose (2 half + 1)^2 neighbourhood (the r = 6 aperture, one pixel off centre, with margin) holds no BAD_SUM
    pixel of the subtraction mask - the frames' own bad pixels, and the margins the subtraction masks around stars
    above its upper data limit (bit 17): a detection there is dropped by the kill_flagged rule or fails BPMCUT - and no
    noise above 1.05 x the median noise of the good pixels (RMSCUT, an aperture mean, is held to 1.1 x that median)."""
    import torch
    bad = (res['mask'] & z.BAD_SUM) != 0
    noise = res['noise']
    med = noise[~bad].median()
    dirty = (bad | (noise > 1.05 * med)).to(torch.float32)[None, None]
    dirty = torch.nn.functional.max_pool2d(dirty, 2 * half + 1, stride=1, padding=half)[0, 0]
    return (dirty == 0).cpu().numpy()


_SCENES = {}


def scene(torch, z, s, njob, nx=640, ny=600, seed=4100):
    """Frames as tests/test_nightly_gpu.py makes them, each science frame with NTRANS point sources the reference does not
    have.  The transients are planted where the job's own products, made once without them, are clean (clean_ground),
    15 px or more from each other and from the reference's stars, 40 px from the border (tests/test_catalog_gpu.py plants
    its injections by the same rules, from the input masks; here the subtraction's own mask is asked)."""
    if njob in _SCENES:
        return _SCENES[njob]
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    base = s.ztf_wcs(nx, ny, tpv=True)
    rng = np.random.default_rng(seed)
    nst = int(nx * ny / 2500)
    xs, ys = rng.uniform(-10, nx + 10, nst), rng.uniform(-10, ny + 10, nst)
    fl = np.exp(rng.uniform(np.log(3e3), np.log(8e4), nst))
    ra, dec = base.all_pix2world(xs, ys, 0)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to('cuda:0')
    rf = s.make_frame(nx, ny, seed, base, star_sky=(ra, dec, fl), fwhm=2.0, noise=1.0, nbad=20)
    ref = dict(img=dev(rf['img'], np.float32), rms=dev(np.full((ny, nx), 1.0), np.float32),
               mask=dev(rf['mask'], np.int32), wcs=base, flxscale=1.0)
    radec = base.all_pix2world(rng.uniform(20, nx - 20, 40), rng.uniform(20, ny - 20, 40), 0)
    frames, scis = [], []
    for i in range(njob):
        w = s.ztf_wcs(nx, ny, dx=rng.uniform(-6, 6), dy=rng.uniform(-6, 6), rot_deg=rng.uniform(-0.05, 0.05))
        f = s.make_frame(nx, ny, seed + 1 + i, w, star_sky=(ra, dec, fl), fwhm=2.4, sky=180.0 + 10 * i, nbad=30)
        frames.append(f)
        scis.append(dict(img=dev(f['img'], np.float32), rms=dev(np.full((ny, nx), 5.0), np.float32),
                         mask=dev(f['mask'], np.int32), wgt=dev(f['wgt'], np.float32), wcs=w, seeing=2.4))
    pool = nm.SubtractionPool(1)
    scout = pool.map([nm.SubtractionJob(sci, ref, nreg_side=2, hotpants_kws={'ko': 1, 'bgo': 0}, tag=i)
                      for i, sci in enumerate(scis)])
    pool.close()
    planted = []
    for f, sci, res in zip(frames, scis, scout):
        assert 'error' not in res
        sx, sy = sci['wcs'].all_world2pix(ra, dec, 0)
        tx, ty = choose_injections(rng, NTRANS, nx, ny, (sx, sy), clean_ground(z, res))
        img = f['img'].astype(np.float64)
        s.add_stars(img, tx, ty, rng.uniform(2000.0, 5000.0, NTRANS), 2.4)
        sci['img'] = dev(img, np.float32)
        planted.append((tx, ty))
    _SCENES[njob] = (scis, ref, radec, planted)
    return _SCENES[njob]


def make_jobs(torch, z, s, njob, **jobkw):
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    scis, ref, radec, planted = scene(torch, z, s, njob)
    jobs = [nm.SubtractionJob(sci, ref, radec=radec, nreg_side=2, hotpants_kws={'ko': 1, 'bgo': 0}, tag=i, **jobkw)
            for i, sci in enumerate(scis)]
    return jobs, planted


def same_table(a, b, exact=True):
    assert a.dtype.names == b.dtype.names and len(a) == len(b)
    for name in a.dtype.names:
        if not exact and name in ('BPMCUT', 'RMSCUT'):
            scale = cref.AREA if name == 'RMSCUT' else 1.0
            np.testing.assert_allclose(a[name] * scale, b[name] * scale, rtol=cref.PIN_RTOL, atol=cref.PIN_ATOL)
        else:
            assert np.array_equal(a[name], b[name], equal_nan=True), name


def test_candidates_equal_the_pieces_composed_by_hand(engine):
    import torch
    z, s = pkg(), synth()
    devmod = importlib.import_module('zuds-pipeline_amd.device')
    fo = importlib.import_module('zuds-pipeline_amd.filterobjects')
    (job,), _ = make_jobs(torch, z, s, 1)
    sci, ref = job.sci, job.ref
    ch = devmod.DeviceSubtraction(sci['wcs'], ref['wcs'], engine=engine)
    ch.run(sci['img'], sci['rms'], sci['mask'], sci['wgt'], ref['img'], ref['rms'], ref['mask'], seeing=2.4,
           nreg_side=2, hotpants_kws={'ko': 1, 'bgo': 0})
    tab, nfound = ch.candidates(2.4)
    # by hand, on clones of the resident planes taken to the host
    ch.stream.synchronize()
    diff, noise, sub = (t.clone().cpu().numpy() for t in (ch.diff, ch.noise, ch.submask))
    raw, nraw, _ = ch.extract()
    assert nraw == nfound
    raw = raw[((raw['IMAFLAGS_ISO'] & z.BAD_SUM) == 0) & (raw['FLAGS_WEIGHT'] == 0)]
    pix = z.pixel_cuts(diff, noise, (sub & z.BAD_SUM) != 0, raw['X_IMAGE'], raw['Y_IMAGE'], engine=engine)
    want = fo.filter_table(raw, 2.4, pix)
    same_table(tab, want, exact=False)
    assert len(tab) > NTRANS and (tab['rb'] == -99).all()
    assert 0 < int(tab['GOODCUT'].sum()) < len(tab)


def results_equal(torch, a, b, products=True):
    assert a['tag'] == b['tag']
    same_table(a['cat'], b['cat'])
    assert a.get('too_many') == b.get('too_many')
    assert ('stamps' in a) == ('stamps' in b)
    if 'stamps' in a:
        for k in ('blocks', 'norms', 'x0', 'y0', 'ra', 'dec'):
            assert np.array_equal(a['stamps'][k], b['stamps'][k], equal_nan=True), k
    if products:
        for k in ('diff', 'noise', 'mask'):
            assert torch.equal(a[k], b[k]), k
        for k in ('flux', 'fluxerr', 'flags'):
            assert np.array_equal(a['phot'][k], b['phot'][k], equal_nan=True), k


def test_pool_detections_do_not_depend_on_the_lane_form_and_change_no_product(engine):
    import torch
    z, s = pkg(), synth()
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    jobs, planted = make_jobs(torch, z, s, 5, detect=True, stamps=True)
    plain, _ = make_jobs(torch, z, s, 5)
    one = nm.SubtractionPool(1)
    a = one.map(jobs)
    p = one.map(plain)
    one.close()
    three = nm.SubtractionPool(3, batch=1)
    assert three.batch == 0 and three.njobs == 3
    b = three.map(jobs)
    three.close()
    lanes = nm.SubtractionPool(2, batch=4)
    assert lanes.batch == 4
    c = lanes.map(jobs)
    pc = lanes.map(plain)
    lanes.close()
    for ra_, rb_, rc_, rp_, rpc_, (tx, ty) in zip(a, b, c, p, pc, planted):
        assert 'error' not in ra_ and 'detect_error' not in ra_ and 'stamps_error' not in ra_
        results_equal(torch, ra_, rb_)
        results_equal(torch, ra_, rc_)
        # with and without detect: the same products, bit for bit, and nothing new in the result
        for r0 in (rp_, rpc_):
            assert 'cat' not in r0 and 'stamps' not in r0 and r0['info'] == ra_['info']
            for k in ('diff', 'noise', 'mask'):
                assert torch.equal(ra_[k], r0[k]), k
            for k in ('flux', 'fluxerr', 'flags'):
                assert np.array_equal(ra_['phot'][k], r0['phot'][k], equal_nan=True), k
        # the planted transients are found, and pass the filter
        cat = ra_['cat']
        good = cat[cat['GOODCUT'] == 1]
        for x, y in zip(tx, ty):
            da = np.hypot(cat['X_IMAGE'] - 1 - x, cat['Y_IMAGE'] - 1 - y)
            row = cat[int(np.argmin(da))]
            print(f'job {ra_["tag"]}: transient at ({x:.1f}, {y:.1f}): nearest row {da.min():.2f} px away, '
                  + ', '.join(f'{n}={row[n]}' for n in ('FLAGS', 'IMAFLAGS_ISO', 'A_IMAGE', 'B_IMAGE', 'FWHM_IMAGE',
                                                        'FLUX_APER', 'FLUXERR_APER', 'BPMCUT', 'RMSCUT', 'GOODCUT')))
        for x, y in zip(tx, ty):
            d = np.hypot(good['X_IMAGE'] - 1 - x, good['Y_IMAGE'] - 1 - y)
            assert d.size and d.min() < 1.0, (x, y)
        st = ra_['stamps']
        assert st['blocks'].shape == (len(good), 3, 63, 63) and st['norms'].shape == (len(good), 3)
        assert np.array_equal(st['ra'], good['X_WORLD']) and np.array_equal(st['dec'], good['Y_WORLD'])
        assert len(good) <= 50 and not ra_.get('too_many')


def test_a_job_over_max_detections_keeps_its_products_and_gets_no_stamps(engine):
    import torch
    z, s = pkg(), synth()
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    jobs, _ = make_jobs(torch, z, s, 2, detect=True, stamps=True, max_detections=NTRANS - 1)
    jobs[1].max_detections = 50
    for pool in (nm.SubtractionPool(1), nm.SubtractionPool(1, batch=2)):
        r = pool.map(jobs)
        pool.close()
        assert r[0].get('too_many') is True and 'stamps' not in r[0]
        assert int((r[0]['cat']['GOODCUT'] == 1).sum()) > NTRANS - 1
        assert r[0]['info']['status'] == 0 and r[0]['diff'].shape == (600, 640) and 'flux' in r[0]['phot']
        assert 'stamps' in r[1] and not r[1].get('too_many')
    with pytest.raises(ValueError):
        nm.SubtractionJob(jobs[0].sci, jobs[0].ref, stamps=True)


def test_a_frame_without_a_valid_pixel_fails_its_job_with_detect_as_without(engine):
    """The subtraction's own refusal ('every pixel is masked', tests/test_device_chain_gpu.py) is not the detection
    step's to swallow: with ``detect`` the job comes back as ``{'tag', 'error'}`` without products, in both lane forms,
    exactly as without it; its neighbour in the same map is untouched."""
    import torch
    z, s = pkg(), synth()
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    scis, ref, radec, _ = scene(torch, z, s, 2)
    dead = dict(scis[0], mask=torch.full_like(scis[0]['mask'], 256))
    outs = {}
    for kw in (dict(), dict(detect=True, stamps=True)):
        jobs = [nm.SubtractionJob(sci, ref, radec=radec, nreg_side=2, hotpants_kws={'ko': 1, 'bgo': 0}, tag=i, **kw)
                for i, sci in enumerate((dead, scis[1]))]
        for form, pool in (('worker', nm.SubtractionPool(1)), ('lane', nm.SubtractionPool(1, batch=2))):
            r = pool.map(jobs)
            pool.close()
            assert set(r[0]) == {'tag', 'error'} and 'every pixel is masked' in r[0]['error'], (form, kw, r[0].keys())
            assert 'error' not in r[1] and r[1]['info']['status'] == 0 and ('cat' in r[1]) == bool(kw)
            outs[form, bool(kw)] = r[1]
    for form in ('worker', 'lane'):
        for k in ('diff', 'noise', 'mask'):
            assert torch.equal(outs[form, True][k], outs['worker', False][k]), (form, k)


def test_candidates_without_a_single_object(engine):
    """A threshold nothing reaches: the table keeps its columns, the cuts launch nothing."""
    import torch
    z, s = pkg(), synth()
    devmod = importlib.import_module('zuds-pipeline_amd.device')
    scis, ref, _, _ = scene(torch, z, s, 2)
    sci = scis[1]
    ch = devmod.DeviceSubtraction(sci['wcs'], ref['wcs'], engine=engine)
    ch.run(sci['img'], sci['rms'], sci['mask'], sci['wgt'], ref['img'], ref['rms'], ref['mask'], seeing=2.4,
           nreg_side=2, hotpants_kws={'ko': 1, 'bgo': 0})
    tab, nfound = ch.candidates(2.4, detect_thresh=1e6)
    assert nfound == 0 and len(tab) == 0
    for n in ('X_IMAGE', 'GOODCUT', 'BPMCUT', 'RMSCUT', 'rb'):
        assert n in tab.dtype.names
    full, _ = ch.candidates(2.4)
    assert tab.dtype == full.dtype and len(full) > 0
