"""``csrc/psf.hip`` and ``psf.py`` on the GPU against the float64 restatement (tests/psf_ref.py) on the scenes of
tests/psf_scenes.py, whose conditions tests/test_psf_ref.py asserts on the restatement alone: under them the pixels of
every fit and the support of every model are well defined, and npix, n_used, flags and NaN patterns are compared exactly.
The floats hold within the tolerances of psf_ref.py (set by tests/measure_psf_tolerance.py from the restatement alone);
every test prints the largest difference it saw.  Host and ``_dev`` entry points run on the same scenes."""
import contextlib
import functools

import numpy as np
import pytest

import lightcurve_ref as lr
import psf_ref as pr
import psf_scenes as ps
from util import pkg

pytestmark = pytest.mark.gpu


def psf():
    return pkg().psf


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


@contextlib.contextmanager
def on_a_stream(engine):
    """The engine bound to a torch stream that is current, as the ``_dev`` forms ask of their caller."""
    import torch
    stream = torch.cuda.Stream('cuda:0')
    engine.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            yield stream
        stream.synchronize()
    finally:
        engine.set_stream(0)


def close(got, ref, tol, what):
    """NaN pattern exact, finite entries within ``tol`` (a scalar or an array); prints the largest difference."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, 'NaN pattern', int(np.isnan(got).sum()), int(np.isnan(ref).sum()))
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (what, 'finite pattern')
    d = np.abs(got - ref)[fin]
    t = np.broadcast_to(tol, ref.shape)[fin]
    worst = float(np.max(d / t)) if d.size else 0.0
    print(f'{what}: {d.size} values, largest difference {d.max() if d.size else 0.0:.3e}, {worst:.3e} of its tolerance')
    assert worst <= 1.0, what
    return float(d.max()) if d.size else 0.0


def run_build(engine, g, n, device, want_cutouts=True, **kw):
    p = psf()
    kw = dict(dict(half=g.half, mask=g.mask, bad_bits=ps.BAD_BITS, engine=engine, want_cutouts=want_cutouts), **kw)
    if not device:
        return p.psf_build(g.img, g.x[:n], g.y[:n], g.sky[:n], g.norm[:n], **kw)
    mask = kw.pop('mask')
    with on_a_stream(engine):
        out = p.psf_build_dev(dev(g.img), dev(g.x[:n]), dev(g.y[:n]), dev(g.sky[:n]), dev(g.norm[:n]), mask=dev(mask), **kw)
    return tuple(v.cpu().numpy() for v in out)


# ---- cutouts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('half', [1, 12, 15])
def test_cutout_edges(engine, half, device):
    """dx of exactly 0, exactly 0.5 and one ulp below 1; a footprint that leaves the frame by one tap on one side; a bad
    pixel under exactly one tap; a NaN pixel; dx == 0 beside a bad column its delta does not touch; norm and sky that are
    not finite or not positive; positions that are not finite."""
    g = ps.cutout_edges(half)
    ref = pr.cutouts(g.img, g.x, g.y, g.sky, g.norm, half, mask=g.mask, bad_bits=ps.BAD_BITS)
    _, _, cut = run_build(engine, g, len(g.x), device, norm_radius=10.0, min_stars_pixel=1)
    close(cut, ref, pr.MODEL_TOL, f'cutouts half {half}')
    nn = dict(zip(g.names, np.isnan(cut).reshape(len(g.names), -1).sum(1)))
    w = 2 * half + 1
    assert nn['dx-zero'] == nn['dx-zero-beside-bad-column'] == nn['generic'] == 0 and nn['norm-zero'] == nn['x-nan'] == w * w
    assert nn['off-frame-one-tap-left'] == w and nn['bad-under-one-tap'] == min(6, w)


@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65])
def test_star_counts_and_the_model(engine, n, device):
    """nstar = 0 writes nothing; otherwise cutouts, model and n_used against the restatement (an outlier pixel in one
    star's cutout is clipped)."""
    g = ps.cutout_many()
    kw = dict(norm_radius=3.0, clip_sigma=3.0, clip_iter=5, min_stars_pixel=3)
    model, n_used, cut = run_build(engine, g, n, device, **kw)
    if n == 0:
        assert np.isnan(model).all() and not n_used.any() and cut.shape == (0, 7, 7)       # as they were handed in
        return
    rm, rn, rc = pr.build_model(g.img, g.x[:n], g.y[:n], g.sky[:n], g.norm[:n], half=g.half, mask=g.mask, bad_bits=ps.BAD_BITS,
                                **kw)
    close(cut, rc, pr.MODEL_TOL, f'{n} stars: cutouts')
    assert np.array_equal(n_used, rn), (n_used, rn)
    close(model, rm, pr.MODEL_TOL, f'{n} stars: model')
    if n >= 3:
        assert abs(model.sum() - 1.0) < 1e-14 and model[0, 0] == 0.0 and n_used.max() <= n
    else:
        assert np.isnan(model).all()                    # below MIN_STARS_PIXEL everywhere: no positive sum


@pytest.mark.parametrize('floor', [3, 4])
def test_min_stars_pixel_at_its_boundary(engine, floor):
    """An entry that is NaN for every star is 0 with n_used 0; entries with 2 and 3 stars left against a floor of 3, 4."""
    g = ps.model_floor()
    kw = dict(norm_radius=3.5, clip_sigma=3.0, clip_iter=0, min_stars_pixel=floor)
    model, n_used = run_build(engine, g, 5, False, want_cutouts=False, **kw)
    rm, rn, _ = pr.build_model(g.img, g.x, g.y, g.sky, g.norm, half=4, mask=g.mask, bad_bits=ps.BAD_BITS, **kw)
    assert np.array_equal(n_used, rn) and np.array_equal(model == 0.0, rm == 0.0)
    close(model, rm, pr.MODEL_TOL, f'floor {floor}: model')
    assert n_used[5, 6] == 0 and model[5, 6] == 0.0 and n_used[3, 5] == 2 and model[3, 5] == 0.0
    assert n_used[6, 3] == 3 and (model[6, 3] != 0.0) == (floor == 3)


def test_too_many_stars_and_bad_arguments_set_the_last_error(engine):
    z = pkg()
    L = engine.L
    n = z._lib.CLIPMED_NMAX + 1
    img = np.zeros((16, 16), np.float32)
    v = np.full(n, 8.0)
    with pytest.raises(z.ZMError, match='clipped median holds at most'):
        psf().psf_build(img, v, v, v, v, half=2, engine=engine)
    with pytest.raises(z.ZMError, match='half 16 outside'):
        psf().psf_build(img, v[:3], v[:3], v[:3], v[:3], half=16, engine=engine)
    model = ps.model_gaussian(8)
    with pytest.raises(z.ZMError, match='needs a model of half width'):
        psf().psf_photometry((img, None, None), [8.0], [8.0], model, fit_radius=4.6, engine=engine)
    assert L.zm_psf_photometry(engine.ctx, None, None, None, 0, 4, 4, 1, None, None, None, 3, 1.0, 0, None, None, None, None,
                               None, None, None) != 0
    assert b'zm_psf_photometry' in L.zm_last_error()
    assert L.zm_psf_photometry_batch_dev(engine.ctx, -1, None, None, None, 0, 0, None, None, 0, 6.0, 0, None, None, None, None,
                                         None, None, None, None, None) != 0
    assert b'zm_psf_photometry_batch_dev' in L.zm_last_error()


# ---- fits ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_ref(case, half=12):
    R, fit_sky, with_rms, with_mask = case
    s = ps.fit_main(half)
    return s, pr.fit(s.img, s.x, s.y, s.model, R, fit_sky, rms=s.rms if with_rms else None, mask=s.mask if with_mask else None,
                     bad_bits=ps.BAD_BITS)


def run_fit(engine, s, n, case, device):
    R, fit_sky, with_rms, with_mask = case
    rms, mask = s.rms if with_rms else None, s.mask if with_mask else None
    p = psf()
    if not device:
        return p.psf_photometry((s.img, rms, mask), s.x[:n], s.y[:n], s.model, fit_radius=R, fit_sky=fit_sky,
                                bad_bits=ps.BAD_BITS, engine=engine)
    with on_a_stream(engine):
        out = p.psf_photometry_dev(dev(s.img), dev(s.x[:n]), dev(s.y[:n]), dev(s.model), fit_radius=R, fit_sky=fit_sky,
                                   rms=dev(rms), mask=dev(mask), bad_bits=ps.BAD_BITS, engine=engine)
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare_fit(got, ref, n, what):
    sl = slice(0, n)
    assert np.array_equal(got['npix'], ref['npix'][sl]), (what, got['npix'], ref['npix'][sl])
    assert np.array_equal(got['flags'], ref['flags'][sl]), (what, got['flags'], ref['flags'][sl])
    seen = {}
    seen['flux'] = close(got['flux'], ref['flux'][sl], pr.FLUX_ATOL + pr.FLUX_RTOL * np.abs(ref['flux'][sl]), f'{what} flux')
    seen['sky'] = close(got['sky'], ref['sky'][sl], pr.FLUX_ATOL + pr.FLUX_RTOL * np.abs(ref['sky'][sl]), f'{what} sky')
    seen['err'] = close(got['fluxerr'], ref['err'][sl], pr.ERR_RTOL * np.abs(ref['err'][sl]), f'{what} err')
    seen['cover'] = close(got['cover'], ref['cover'][sl], pr.ERR_RTOL * np.abs(ref['cover'][sl]), f'{what} cover')
    seen['chi2'] = close(got['chi2'], ref['chi2'][sl], pr.CHI2_RTOL * ref['chi2_scale'][sl], f'{what} chi2')
    return seen


@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('case', ps.FIT_CASES, ids=lambda c: f'R{c[0]:g}-sky{c[1]}-rms{int(c[2])}-mask{int(c[3])}')
def test_fit_scene(engine, case, device):
    """fx = -0.5, 0 and just under +0.5; the corner, half outside, fully outside (SINGULAR); one masked pixel, every pixel
    masked, all but one masked (SINGULAR with a sky term); rms with a 0, a NaN and an inf; a NaN pixel; positions that are
    not finite; rms NULL and mask NULL; R = 1, 6 and h - 3.5; 65 positions."""
    s, ref = fit_ref(case)
    got = run_fit(engine, s, len(s.x), case, device)
    compare_fit(got, ref, len(s.x), f'fit {case}')
    again = run_fit(engine, s, len(s.x), case, device)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)          # the same bits on every run


@pytest.mark.parametrize('n', [0, 1])
def test_fit_counts_and_the_largest_box(engine, n):
    s, ref = fit_ref(ps.FIT_CASES[1])
    for device in (False, True):
        got = run_fit(engine, s, n, ps.FIT_CASES[1], device)
        assert all(v.shape == (n,) for v in got.values())
        if n:
            compare_fit(got, ref, n, f'{n} position')
    if n:                                                # half 15, R = 11.5: the largest box a fit walks (27 x 27)
        case = (11.5, 1, True, True)
        s15, r15 = fit_ref(case, 15)
        compare_fit(run_fit(engine, s15, len(s15.x), case, False), r15, len(s15.x), 'R 11.5, half 15')


# ---- batch --------------------------------------------------------------------------------------------------------------
def test_batch_of_three_images(engine):
    """96 x 80 with all planes and half 12, 130 x 70 without rms and half 10, 71 x 37 without a mask and half 15; sources on
    both sides of each footprint.  Bit for bit zm_psf_photometry_dev at the batch's own positions, positions within
    POS_TOL_PX of the oracle, fits within tolerance of the restatement; the default table is the bytes it was."""
    z = pkg()
    ws, ows, planes, ra, dec = lr.batch_scene()
    halves = (12, 10, 15)
    models = [ps.model_gaussian(h, norm_radius=min(10.0, h)) for h in halves]
    images = [dict(img=p[0], rms=p[1], mask=p[2], wcs=w, psf=m) for w, p, m in zip(ws, planes, models)]
    for fit_sky in (0, 1):
        t = psf().psf_photometry_batch(images, ra, dec, engine=engine, fit_radius=6.0, fit_sky=fit_sky, bad_bits=ps.BAD_BITS)
        off, idx = lr.membership(ows, ra, dec)
        assert np.array_equal(t['offsets'], off) and np.array_equal(t['source'], idx) and (np.diff(off) > 10).all()
        pos = lr.photometry(ows, planes, ra, dec, off, idx)
        dx, dy = np.abs(t['x'] - pos['x']).max(), np.abs(t['y'] - pos['y']).max()
        print(f'batch sky {fit_sky}: {idx.size} pairs, worst |x - oracle| {dx:.3e}, |y - oracle| {dy:.3e} px (bound {lr.POS_TOL_PX:.3e})')
        assert dx <= lr.POS_TOL_PX and dy <= lr.POS_TOL_PX
        for k, (img, rms, mask) in enumerate(planes):
            a, b = int(off[k]), int(off[k + 1])
            with on_a_stream(engine):
                one = psf().psf_photometry_dev(dev(img), dev(t['x'][a:b]), dev(t['y'][a:b]), dev(models[k]), fit_radius=6.0,
                                               fit_sky=fit_sky, rms=dev(rms), mask=dev(mask), bad_bits=ps.BAD_BITS, engine=engine)
            for key in ('flux', 'fluxerr', 'chi2', 'sky', 'cover', 'npix', 'flags'):
                assert one[key].cpu().numpy().tobytes() == t[key][a:b].tobytes(), (k, key)
            ref = pr.fit(img, t['x'][a:b], t['y'][a:b], models[k], 6.0, fit_sky, rms=rms, mask=mask, bad_bits=ps.BAD_BITS)
            assert ref['margin'].min() >= ps.MARGIN
            compare_fit({key: t[key][a:b] for key in ('flux', 'fluxerr', 'chi2', 'sky', 'cover', 'npix', 'flags')}, ref, b - a,
                        f'batch sky {fit_sky} image {k}')
        again = psf().psf_photometry_batch(images, ra, dec, engine=engine, fit_radius=6.0, fit_sky=fit_sky, bad_bits=ps.BAD_BITS)
        assert all(np.asarray(t[k]).tobytes() == np.asarray(again[k]).tobytes() for k in t)
    # done pairs are left out, and an image without a model is refused
    some = [(0, int(idx[0])), (2, int(idx[off[2]]))]
    less = psf().psf_photometry_batch(images, ra, dec, done=some, engine=engine, fit_radius=6.0)
    assert less['source'].size == idx.size - 2
    with pytest.raises(ValueError, match='needs a model'):
        z.lightcurve.forced_photometry_batch([dict(img=planes[0][0], wcs=ws[0])], ra, dec, engine=engine, method='psf')
    for bad in ('PSF', 'optimal', None):
        with pytest.raises(ValueError, match='neither'):
            z.lightcurve.forced_photometry_batch(images, ra, dec, engine=engine, method=bad)
    # models that carry different PSFFITR: the radius has to be said; said, or carried alike, it is the one used
    carded = [dict(im, psf=psf().PSFModel(m, cards={'PSFFITR': r})) for im, m, r in zip(images, models, (6.0, 6.0, 5.0))]
    with pytest.raises(ValueError, match='different PSFFITR'):
        psf().psf_photometry_batch(carded, ra, dec, engine=engine)
    t6 = psf().psf_photometry_batch(carded, ra, dec, engine=engine, fit_radius=6.0, bad_bits=ps.BAD_BITS)
    assert t6['flux'].tobytes() == psf().psf_photometry_batch(images, ra, dec, engine=engine, fit_radius=6.0,
                                                              bad_bits=ps.BAD_BITS)['flux'].tobytes()
    alike = [dict(im, psf=psf().PSFModel(m, cards={'PSFFITR': 5.0})) for im, m in zip(images, models)]
    t5 = psf().psf_photometry_batch(alike, ra, dec, engine=engine, bad_bits=ps.BAD_BITS)
    assert t5['npix'].max() < t6['npix'].max()
    # the aperture table with default arguments: the same bytes as the per-image aperture kernel, as before
    lc = z.lightcurve
    plain = [dict(img=p[0], rms=p[1], mask=p[2], wcs=w) for w, p in zip(ws, planes)]
    t0 = lc.forced_photometry_batch(plain, ra, dec, engine=engine)
    t1 = lc.forced_photometry_batch(images, ra, dec, engine=engine, method='aperture')
    assert sorted(t0) == sorted(t1) == ['flags', 'flux', 'fluxerr', 'image', 'offsets', 'source', 'x', 'y']
    assert all(np.asarray(t0[k]).tobytes() == np.asarray(t1[k]).tobytes() for k in t0)
    import torch
    for k, (img, rms, mask) in enumerate(planes):
        a, b = int(off[k]), int(off[k + 1])
        f, e = torch.empty(b - a, dtype=torch.float64, device='cuda'), torch.empty(b - a, dtype=torch.float64, device='cuda')
        fl = torch.empty(b - a, dtype=torch.int32, device='cuda')
        d = [dev(v) for v in (img, rms, mask, t0['x'][a:b], t0['y'][a:b])]
        torch.cuda.synchronize()
        z._lib.check(engine.L.zm_aperture_photometry_dev(engine.ctx, d[0].data_ptr(), d[1].data_ptr() if d[1] is not None else None,
                                                         d[2].data_ptr() if d[2] is not None else None, img.shape[1], img.shape[0],
                                                         b - a, d[3].data_ptr(), d[4].data_ptr(), lr.RADIUS, f.data_ptr(),
                                                         e.data_ptr(), fl.data_ptr()))
        engine.synchronize()
        assert f.cpu().numpy().tobytes() == t0['flux'][a:b].tobytes() and fl.cpu().numpy().tobytes() == t0['flags'][a:b].tobytes()


# ---- the operator ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def night():
    """A 256^2 TPV frame: 60 catalogue stars of FWHM 2.4 px on a sky of 200 with noise 5, 40 planted faint sources."""
    z = pkg()
    nt = ps.night_planes()
    w = z.synth.ztf_wcs(256, 256, tpv=True)
    ra, dec = w.all_pix2world(nt['x'], nt['y'], 0)
    return dict(nt, wcs=w, stars=(ra, dec, 25.0 - 2.5 * np.log10(nt['flux'])))


@pytest.mark.parametrize('fit_sky', [0, 1])
def test_build_psf_cards_against_the_restatement(engine, fit_sky):
    """``build_psf_planes`` with a catalogue: the stars come from photcal's route (pinned by tests/test_photcal_gpu.py); from
    their positions, sky and norm on, the model, the stars' own fits, the used stars and the cards are restated."""
    nt = night()
    res = psf().build_psf_planes(nt['img'], wcs=nt['wcs'], mask=nt['mask'], rms=nt['rms'], stars=nt['stars'], engine=engine,
                                 bad_bits=ps.BAD_BITS, fit_sky=fit_sky)
    model, cards = res['psf'], res['psf'].cards
    assert len(res['x']) >= 40 and model.half == 12
    ref = pr.cards(nt['img'], res['x'], res['y'], res['sky'], res['norm'], fit_sky, rms=nt['rms'], mask=nt['mask'],
                   bad_bits=ps.BAD_BITS)
    assert np.array_equal(model.n_used, ref['n_used'])
    close(model.data, ref['model'], pr.MODEL_TOL, 'night: model')
    assert np.array_equal(ref['used'], res['used'])
    nu = ref['PSFNSTAR']
    want = {'PSFCOR': ref['PSFCOR'], 'PSFCORUN': ref['PSFCORUN']}
    for k, v in want.items():
        print(f'night sky {fit_sky}: {k} {cards[k]:.6f}, restated {v:.6f}, difference {abs(cards[k] - v):.3e} (CARD_TOL {pr.CARD_TOL:.3e})')
        assert abs(cards[k] - v) <= pr.CARD_TOL, k
    assert cards['PSFNSTAR'] == nu and cards['PSFHALF'] == 12 and cards['PSFFITR'] == 6.0 and cards['ZMPSF'] is True
    assert abs(cards['PSFCOR']) < 0.05 and 2.2 < cards['PSFFWHM'] < 2.7
    # the planted faint sources: PSF fluxes at the true positions, corrected by PSFCOR, scatter about the planted flux
    fx, fy = nt['faint']
    got = psf().psf_photometry((nt['img'], nt['rms'], nt['mask']), fx, fy, model, fit_sky=1, bad_bits=ps.BAD_BITS, engine=engine)
    ref = pr.fit(nt['img'], fx, fy, model.data, 6.0, 1, rms=nt['rms'], mask=nt['mask'], bad_bits=ps.BAD_BITS)
    compare_fit(got, ref, 40, 'night: faint sources')
    pull = (got['flux'] * 10 ** (-0.4 * cards['PSFCOR']) - 800.0) / got['fluxerr']
    print(f'night: faint sources, median pull {np.median(pull):.2f}, 1.4826 MAD {1.4826 * np.median(np.abs(pull - np.median(pull))):.2f}')
    assert abs(np.median(pull)) < 1.0


def test_too_few_stars_is_an_error(engine):
    nt = night()
    with pytest.raises(RuntimeError, match='MIN_STARS'):
        psf().build_psf_planes(nt['img'], wcs=nt['wcs'], mask=nt['mask'], rms=nt['rms'], stars=nt['stars'], engine=engine,
                               bad_bits=ps.BAD_BITS, min_stars=500)
