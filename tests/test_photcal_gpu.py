"""``csrc/photcal.hip`` and ``photcal.py`` on the GPU against the float64 restatement (tests/photcal_ref.py) on the scenes
of tests/photcal_scenes.py, whose conditions tests/test_photcal_ref.py asserts on the restatement alone: under them the
set of used pixels and the set of used stars are well defined, and both are compared exactly.  Host and ``_dev`` entry
points run on the same scenes."""
import contextlib
import functools
import importlib
import os

import numpy as np
import pytest

import photcal_ref as pr
import photcal_scenes as ps
from util import pkg

pytestmark = pytest.mark.gpu


def photcal():
    return importlib.import_module('zuds-pipeline_amd.photcal')


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


@functools.lru_cache(maxsize=None)
def growth_ref(name):
    g = ps.growth_many() if name == 'many' else ps.GROWTH[name]()
    return g, pr.growth(g.img, g.x, g.y, g.radii, rms=g.rms, mask=g.mask, bad_bits=ps.BAD_BITS, saturate=g.saturate,
                        r_in=g.annulus[0], r_out=g.annulus[1], kappa=3.0, maxiter=5, nsky_min=g.nsky_min)


def run_growth(engine, g, n, device):
    p = photcal()
    kw = dict(saturate=g.saturate, annulus=g.annulus, bad_bits=ps.BAD_BITS, kappa=3.0, maxiter=5, nsky_min=g.nsky_min,
              engine=engine)
    if not device:
        return p.growth_curves(g.img, g.x[:n], g.y[:n], g.radii, rms=g.rms, mask=g.mask, **kw)
    with on_a_stream(engine):
        out = p.growth_curves_dev(dev(g.img), dev(g.x[:n]), dev(g.y[:n]), g.radii, rms=dev(g.rms), mask=dev(g.mask), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare_growth(got, ref, n, what):
    sl = slice(0, n)
    assert np.array_equal(got['nsky'], ref['nsky'][sl]), what
    assert np.array_equal(got['flags'], ref['flags'][sl]), (what, got['flags'], ref['flags'][sl])
    for k in ('sky', 'sky_sigma'):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k][sl])), (what, k)
        np.testing.assert_allclose(got[k], ref[k][sl], rtol=1e-12, atol=0, err_msg=f'{what} {k}')
    ftol, etol = pr.growth_tolerances(ref)
    for k, tol in (('flux', ftol), ('err', etol)):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k][sl])), (what, k, got[k], ref[k][sl])
        fin = np.isfinite(ref[k][sl])
        d = np.abs(got[k] - ref[k][sl])[fin]
        worst = float(np.max(d / tol[sl][fin])) if d.size else 0.0
        print(f'{what} {k}: {d.size} values, worst difference {d.max() if d.size else 0.0:.3e}, {worst:.3e} of its tolerance')
        assert worst <= 1.0, (what, k)


@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('name', list(ps.GROWTH))
def test_growth_scenes(engine, name, device):
    g, ref = growth_ref(name)
    assert len(g.radii) == {'main': 7, 'sky': 1, 'rout20': 8}[name]
    compare_growth(run_growth(engine, g, g.x.size, device), ref, g.x.size, f'{name} {"dev" if device else "host"}')


@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('n', ps.COUNTS)
def test_growth_star_counts(engine, n, device):
    g, ref = growth_ref('many')
    compare_growth(run_growth(engine, g, n, device), ref, n, f'{n} stars')


def test_growth_with_no_star_writes_nothing_and_bad_arguments_are_refused(engine):
    z, p = pkg(), photcal()
    g = ps.growth_main()
    out = p.growth_curves(g.img, [], [], g.radii, engine=engine)
    assert out['flux'].shape == (0, 7) and out['flags'].size == 0
    # nstar == 0 returns before anything is read or written: null outputs do no harm
    L = engine.L
    r = np.array([1.0, 2.0])
    img = np.ascontiguousarray(g.img)
    one = np.zeros(4)
    i1 = np.zeros(2, np.int32)
    args = lambda nstar, naper, radii, r_out: (engine.ctx, img.ctypes.data, None, None, 0, 0.0, ps.NX, ps.NY, nstar,
                                              one.ctypes.data, one.ctypes.data, naper, radii.ctypes.data, 12.0, r_out, 3.0, 5,
                                              50, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                                              i1.ctypes.data, i1.ctypes.data)
    assert L.zm_growth(*args(0, 2, r, 18.0)) == 0 and not one.any() and not i1.any()
    with pytest.raises(z.ZMError, match='r_out 20.5 beyond the largest supported annulus radius'):
        p.growth_curves(g.img, [40.0], [40.0], g.radii, annulus=(12.0, 20.5), engine=engine)
    with pytest.raises(z.ZMError, match='the radii must ascend'):
        p.growth_curves(g.img, [40.0], [40.0], (3.0, 2.0), engine=engine)
    with pytest.raises(ValueError, match='1 to 8 radii'):
        p.growth_curves(g.img, [40.0], [40.0], np.arange(1.0, 10.0), engine=engine)
    assert L.zm_growth(*args(1, 9, np.arange(1.0, 10.0), 18.0)) != 0 and b'naper 9 outside 1 .. 8' in L.zm_last_error()


# ---------------------------------------------------------------------------------------------------- clipped median
@functools.lru_cache(maxsize=None)
def clipmed_ref(n, maxiter):
    a = ps.clipmed_columns(n)
    return a, pr.clipped_median(a[:, :7], 3.0, maxiter)[0]


def compare_clipmed(got, want, what):
    assert np.array_equal(got[:, 2:], want[:, 2:]), (what, got[:, 2:], want[:, 2:])          # n_used, n_valid: exact
    assert np.array_equal(np.isnan(got[:, :2]), np.isnan(want[:, :2])), what
    fin = np.isfinite(want[:, 0])
    assert np.array_equal(got[fin, 0], want[fin, 0]), (what, got[:, 0], want[:, 0])            # the median: bit-equal
    np.testing.assert_allclose(got[fin, 1], want[fin, 1], rtol=1e-12, atol=0, err_msg=what)


@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('n', ps.CM_ROWS)
def test_clipped_median_rows(engine, n, device):
    p = photcal()
    for maxiter in (5, 0):
        a, want = clipmed_ref(n, maxiter)
        if device:
            with on_a_stream(engine):
                got = p.clipped_median_dev(dev(a)[:, :7], 3.0, maxiter, engine=engine).cpu().numpy()
        else:
            got = p.clipped_median(a[:, :7], 3.0, maxiter, engine=engine)
        compare_clipmed(got, want, f'n {n} maxiter {maxiter}')
        # one column (1-D input, stride 1 on the host; a view with stride 9 on the device)
        if device:
            with on_a_stream(engine):
                one = p.clipped_median_dev(dev(a)[:, 2:3], 3.0, maxiter, engine=engine).cpu().numpy()
        else:
            one = p.clipped_median(a[:, 2], 3.0, maxiter, engine=engine)[None, :]
        compare_clipmed(one, want[2:3], f'n {n} maxiter {maxiter} one column')


def test_clipped_median_refuses_more_rows_than_lds_holds(engine):
    z, p = pkg(), photcal()
    with pytest.raises(z.ZMError, match='16385 rows, a launch holds at most 16384'):
        p.clipped_median(np.zeros(16385), engine=engine)
    with on_a_stream(engine):
        with pytest.raises(z.ZMError, match='16385 rows'):
            p.clipped_median_dev(dev(np.zeros((16385, 1))), engine=engine)


# ------------------------------------------------------------------------------------------------ limiting magnitude
@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('name', ps.MAGLIM)
def test_limiting_magnitude(engine, name, device):
    p = photcal()
    m = ps.maglim(name)
    med, nused, npts, sig, bound = pr.maglim_sigma(m.rms, m.mask, ps.BAD_BITS, m.radius, m.step)
    if device:
        with on_a_stream(engine):
            got = p.limiting_magnitude((dev(m.rms), dev(m.mask)), 26.0, radius=m.radius, step=m.step, engine=engine)
    else:
        got = p.limiting_magnitude((m.rms, m.mask), 26.0, radius=m.radius, step=m.step, engine=engine)
    print(f'{name}: {nused} of {npts} lattice points used, median sigma_ap {med!r}, got {got["sigma_ap"]!r}')
    assert (got['nused'], got['npoints'], got['step']) == (nused, npts, m.step)
    assert npts > 1
    if name.endswith('none'):
        assert nused == 0 and np.isnan(got['sigma_ap']) and np.isnan(got['maglim'])
        return
    assert 0 < nused and (name.endswith('flat') or nused < npts)
    tol = max(pr.FLUX_ATOL + pr.FLUX_RTOL * med, float(np.nanmax(bound)))
    assert abs(got['sigma_ap'] - med) <= tol
    if name.endswith('flat'):
        assert abs(med - 2.5 * np.sqrt(np.pi * 9.0)) <= 1e-9
    assert abs(got['maglim'] - (26.0 - 2.5 * np.log10(5.0 * med))) <= pr.CARD_TOL


def test_limiting_magnitude_doubles_the_step_of_a_lattice_that_is_too_fine(engine):
    p = photcal()
    rms = np.full((300, 300), 1.5, np.float32)
    got = p.limiting_magnitude((rms, None), 25.0, step=1, engine=engine)
    # 293 x 293 centres at step 1 are more than 16384; 146 x 146 at step 2 too; 73 x 73 at step 4 are not
    assert got['step'] == 4 and got['npoints'] == 73 * 73 == got['nused']
    assert abs(got['sigma_ap'] - 1.5 * np.sqrt(np.pi * 9.0)) <= 1e-9
    z = pkg()
    import torch
    out = torch.empty(3, dtype=torch.float64, device='cuda:0')
    d = dev(rms)
    torch.cuda.synchronize()
    assert engine.L.zm_maglim_dev(engine.ctx, d.data_ptr(), None, 0, 300, 300, 3.0, 1, out.data_ptr()) != 0
    assert b'take a coarser step' in engine.L.zm_last_error()


# --------------------------------------------------------------------------------------------------------- end to end
def make_e2e(d):
    """The three dithered frames of tests/measure_photcal_tolerance.py as files, and the star catalogue."""
    import measure_photcal_tolerance as mt
    z = pkg()
    scamp = importlib.import_module('zuds-pipeline_amd.scamp')
    paths = []
    for i in range(3):
        f = mt.e2e_frame(i)
        path = os.path.join(d, f'ztf_202002{i:02d}_000651_zg_c03_o_q1_sciimg.fits')
        z.fits.write(path, f['img'], f['header'])
        z.fits.write(path.replace('sciimg', 'mskimg'), f['mask'].astype(np.int16), f['header'])
        paths.append(path)
    cat = os.path.join(d, 'stars.cat')
    ra, dec, mag = mt.e2e_catalogue()
    scamp.write_astrefcat(cat, ra, dec, mag=mag)
    return paths, cat


def load(paths):
    z = pkg()
    ims = []
    for p in paths:
        im = z.ScienceImage.from_file(p)
        im.mask_image = z.MaskImage.from_file(p.replace('sciimg', 'mskimg'))
        ims.append(im)
    return ims


def digest(paths):
    import hashlib
    return [hashlib.sha256(open(p, 'rb').read()).hexdigest() for p in paths]


def reference_of(engine, image, stars=True):
    """The restatement on the planes of an image object; the centroids are taken on the background-subtracted plane the
    package makes (``zm_background``, pinned to the oracle by tests/test_background_gpu.py)."""
    import measure_photcal_tolerance as mt
    data = np.ascontiguousarray(image.data, dtype=np.float32)
    mask = np.ascontiguousarray(image.mask_image.data).astype(np.int32)
    rms = np.ascontiguousarray(image.rms_image.data, dtype=np.float32)
    wgt = np.where((mask & ps.BAD_BITS) != 0, 0.0, 1.0).astype(np.float32)
    sub = engine.background(data, wgt, want=('sub',))[2]
    sat = image.header.get('SATURATE')
    return mt.reference_on_planes(data, mask, rms, image.wcs, float(sat) if sat else None, sub=sub, stars=stars)


def check_conditions(ref):
    sn = ref['sn'][np.isfinite(ref['sn'])]
    assert np.min(np.abs(sn / 50.0 - 1.0)) >= 0.01
    sh = ref['shift_all'][np.isfinite(ref['shift_all'])]
    assert np.min(np.abs(sh / 2.0 - 1.0)) >= 0.01
    for st in ref['apcor_stats'] + [ref['zp_stats']] + [s for s in ref['growth']['sky_stats'] if s is not None]:
        assert st['margin'] >= 1e-6


@pytest.mark.parametrize('route', ['device', 'host'])
def test_coadd_with_calibrate_photometry(tmp_path, engine, monkeypatch, route):
    monkeypatch.setenv('ZM_OBJECT_API', route)
    z, p = pkg(), photcal()
    d = str(tmp_path)
    paths, cat = make_e2e(d)
    out = os.path.join(d, 'stack.coadd.fits')
    coadd = z.ScienceCoadd.from_images(load(paths), out, calibrate_photometry=True, photcal_kws={'PHOTREF_NAME': cat},
                                       tmpdir=d)
    info = coadd.photcal_info
    ref = reference_of(engine, coadd)
    check_conditions(ref)
    # the same stars
    assert np.array_equal(info['index'], ref['index'])
    assert np.array_equal(info['index'][info['used']], ref['index'][ref['used']])
    assert int(info['used'].sum()) >= 20
    # every card, in the object and in the file
    hdr = z.fits.read(out)[1]
    got = {k: v for k, v, _ in info['cards']}
    assert set(got) == set(ref['cards']) and hdr['ZMPHOTCA'] is True and 'MAGLIM' in got and 'MAGZP' in got
    worst = 0.0
    for k, want in ref['cards'].items():
        assert k in coadd.header and k in hdr and coadd.header_comments[k], k
        if k in ('NMATCHES', 'ZMPHOTCA'):
            assert got[k] == want and hdr[k] == want, k
            continue
        worst = max(worst, abs(got[k] - want))
        assert abs(got[k] - want) <= pr.CARD_TOL, (k, got[k], want)
        assert abs(hdr[k] - want) <= pr.CARD_TOL + 1e-9 * abs(want), k           # (the file keeps 15 digits of a float)
    print(f'{route}: {int(info["used"].sum())} stars used of {info["used"].size}; MAGZP {got["MAGZP"]:.5f} +- '
          f'{got["MAGZPUNC"]:.5f} (the coadd is scaled to 25), APCOR4 {got["APCOR4"]:.5f}, MAGLIM {got["MAGLIM"]:.3f}; '
          f'largest card difference from the restatement {worst:.3e} mag (tolerance {pr.CARD_TOL:.3e})')
    assert abs(got['MAGZP'] - 25.0) < 0.01
    # forced photometry and magnitudes on the calibrated coadd
    import measure_photcal_tolerance as mt
    ra, dec, mag = mt.e2e_catalogue()
    k = info['index'][info['used']][:5]

    class Src:
        def __init__(self, ra, dec):
            self.ra, self.dec = ra, dec
    pts = z.CalibratedImage.force_photometry(coadd, [Src(a, b) for a, b in zip(ra[k], dec[k])])
    mags = np.array([pt.mag for pt in pts])
    print(f'{route}: forced magnitudes {np.round(mags, 3).tolist()} for catalogue {np.round(mag[k], 3).tolist()}')
    assert np.all(np.abs(mags - mag[k]) < 0.05)
    tab = z.aperture_photometry(coadd, ra[k], dec[k], apply_calibration=True)
    assert np.allclose(tab['mag'], mags, rtol=0, atol=1e-12)


def test_own_stars_give_apcor_and_leave_magzp_alone(tmp_path, engine):
    """``stars=None``: the image's own stars; MAGZP is not written, MAGLIM comes from the header's zero point.  The
    restatement takes the peaks from the package's star finder (pinned by tests/test_seeing_gpu.py)."""
    import measure_photcal_tolerance as mt
    z, p = pkg(), photcal()
    f = mt.e2e_frame(1)
    got = p.measure_planes(f['img'], mask=f['mask'], rms=f['rms'], saturate=f['saturate'], magzp=f['zp'], engine=engine)
    cards = {k: v for k, v, _ in got['cards']}
    assert 'MAGZP' not in cards and 'NMATCHES' not in cards and cards['ZMPHOTCA'] is True and 'MAGLIM' in cards
    wgt = np.where((f['mask'] & ps.BAD_BITS) != 0, 0.0, 1.0).astype(np.float32)
    sub = engine.background(f['img'], wgt, want=('sub',))[2]
    ref = pr.measure(f['img'], sub, got['peaks'], mt.oracle_centroid, rms=f['rms'], mask=f['mask'], bad_bits=ps.BAD_BITS,
                     saturate=f['saturate'], magzp=f['zp'])
    assert np.array_equal(got['used'], ref['used']) and got['used'].sum() >= 20
    assert set(cards) == set(ref['cards'])
    for k, want in ref['cards'].items():
        assert abs(cards[k] - want) <= pr.CARD_TOL, (k, cards[k], want)
    with pytest.raises(RuntimeError, match='Unable to calibrate the photometry'):
        p.measure_planes(f['img'], mask=f['mask'], rms=f['rms'], saturate=f['saturate'], engine=engine, min_stars=500)


def test_defaults_change_no_product_and_calibrate_photometry_keeps_the_callers_objects(tmp_path, engine, monkeypatch):
    monkeypatch.setenv('ZM_OBJECT_API', 'host')
    z, p = pkg(), photcal()
    d = str(tmp_path)
    paths, cat = make_e2e(d)
    names = lambda stem: [os.path.join(d, stem + s) for s in ('.fits', '.weight.fits', '.mask.fits')]
    a = z.ScienceCoadd.from_images(load(paths), names('a.coadd')[0], tmpdir=d)
    b = z.ScienceCoadd.from_images(load(paths), names('b.coadd')[0], tmpdir=d, calibrate_photometry=False, photcal_kws=None)
    assert digest(names('a.coadd')) == digest(names('b.coadd'))
    assert 'ZMPHOTCA' not in a.header and 'APCOR4' not in a.header
    # transaction copies unless inplace: the caller's object and file stay as they are
    before, header = digest(names('a.coadd')), dict(a.header)
    res = p.calibrate_photometry(a, photcal_kws={'PHOTREF_NAME': cat})[0]
    assert a.header == header and digest(names('a.coadd')) == before
    assert res['image'] is not a and res['image'].header['ZMPHOTCA'] is True and 'MAGZP' in res['image'].header
    # write_maglim: from the header's zero point; without one the card is skipped with a warning
    with pytest.warns(UserWarning, match='has no MAGZP / APCOR4 card'):
        assert p.write_maglim(a) is None
    assert 'MAGLIM' not in a.header
    p.calibrate_photometry(a, photcal_kws={'PHOTREF_NAME': cat}, inplace=True)
    saved = z.fits.read(names('a.coadd')[0])[1]
    assert saved['ZMPHOTCA'] is True and abs(saved['MAGZP'] - res['image'].header['MAGZP']) < 1e-9
    del a.header['MAGLIM']
    ml = p.write_maglim(a)
    assert abs(ml['maglim'] - saved['MAGLIM']) <= pr.CARD_TOL + 1e-9 and 'MAGLIM' in z.fits.read(names('a.coadd')[0])[1]
    with pytest.raises(ValueError, match='is not a key'):
        z.ScienceCoadd.from_images(load(paths), names('c.coadd')[0], tmpdir=d, calibrate_photometry=True,
                                   photcal_kws={'SEEING': 2})


def test_device_subtraction_maglim_reads_the_resident_planes(engine):
    """``DeviceSubtraction.maglim``: the noise plane and the mask of the chain, as they lie in HBM."""
    z = pkg()
    synth = importlib.import_module('zuds-pipeline_amd.synth')
    m = ps.maglim('large-graded')
    ny, nx = m.rms.shape
    w = synth.tan_wcs(nx, ny)
    import torch
    device = importlib.import_module('zuds-pipeline_amd.device')
    ds = device.DeviceSubtraction(w, w, engine=engine)
    try:
        rms, mask = dev(m.rms), dev(m.mask)
        torch.cuda.synchronize()
        with torch.cuda.stream(ds.stream):
            ds.noise.copy_(rms)
            ds.submask.copy_(mask)
        got = ds.maglim(26.2, step=m.step)
    finally:
        engine.set_stream(0)
    med, nused, npts, _, bound = pr.maglim_sigma(m.rms, m.mask, ps.BAD_BITS, 3.0, m.step)
    assert (got['nused'], got['npoints']) == (nused, npts)
    assert abs(got['sigma_ap'] - med) <= max(pr.FLUX_ATOL + pr.FLUX_RTOL * med, float(np.nanmax(bound)))
    assert abs(got['maglim'] - (26.2 - 2.5 * np.log10(5.0 * med))) <= pr.CARD_TOL


def test_subtraction_of_the_calibrated_coadd_carries_maglim(tmp_path, engine):
    """The chain the cards exist for: a calibrated science coadd, a reference, their subtraction with ``--maglim``
    semantics (``write_maglim``: the subtraction's own rms plane, the ``MAGZP`` / ``APCOR4`` it copied), and the limit an
    alert reads from the header (``HeaderImage.maglimit``, which ``make_alerts`` puts into ``diffmaglim``)."""
    z, p = pkg(), photcal()
    alert = importlib.import_module('zuds-pipeline_amd.alert')
    d = str(tmp_path)
    paths, cat = make_e2e(d)
    kws = {'PHOTREF_NAME': cat}
    sci = z.ScienceCoadd.from_images(load(paths), os.path.join(d, 'stack.coadd.fits'), calibrate_photometry=True,
                                     photcal_kws=kws, tmpdir=d)
    ref = z.ReferenceImage.from_images(load(paths[:2]), os.path.join(d, 'ref.000651_c03_q1_zg.fits'), tmpdir=d)
    sub = z.SingleEpochSubtraction.from_images(sci, ref, nreg_side=1, hotpants_kws={'ko': 0, 'bgo': 0}, tmpdir=d)
    # (copied through the file on the device route: a card keeps 15 digits)
    assert abs(sub.header['MAGZP'] - sci.header['MAGZP']) < 1e-12 and abs(sub.header['APCOR4'] - sci.header['APCOR4']) < 1e-12
    # (a subtraction inherits its science image's header, MAGLIM included: write_maglim replaces it with its own)
    ml = p.write_maglim(sub)
    assert ml['maglim'] != sci.header['MAGLIM']
    saved = z.fits.read(sub.local_path)[1]
    assert np.isfinite(ml['maglim']) and sub.header['MAGLIM'] == ml['maglim'] and abs(saved['MAGLIM'] - ml['maglim']) < 1e-9
    # the restatement on the subtraction's planes
    rms = np.ascontiguousarray(sub.rms_image.data, dtype=np.float32)
    mask = np.ascontiguousarray(sub.mask_image.data).astype(np.int32)
    med, nused, npts, _, bound = pr.maglim_sigma(rms, mask, ps.BAD_BITS, 3.0, 32)
    assert (ml['nused'], ml['npoints']) == (nused, npts) and nused > 0
    want = sub.header['MAGZP'] + sub.header['APCOR4'] - 2.5 * np.log10(5.0 * med)
    assert abs(ml['maglim'] - want) <= pr.CARD_TOL
    print(f'MAGLIM of the subtraction {ml["maglim"]:.3f} ({nused} of {npts} apertures), of the science coadd '
          f'{sci.header["MAGLIM"]:.3f}')
    # make_alerts on a detection of this subtraction, its images known by their headers as scripts/makealert.py knows
    # them: diffmaglim is target_image.maglimit, the measured card
    import alert_scenes as sc
    frames = [alert.HeaderImage(z.fits.read(q)[1], basename=os.path.basename(q)) for q in paths[:2]]
    reference = alert.HeaderImage({}, basename='reference', input_images=frames)
    cards = dict(saved, PROGRMPI='Kulkarni', PROGRMID=2)      # (the survey's programme cards: synthetic frames have none)
    science = alert.HeaderImage(cards, basename=sub.basename)
    image = alert.HeaderImage(cards, basename=sub.basename, id=1, target_image=science, reference_image=reference)
    assert science.maglimit == saved['MAGLIM']
    import measure_photcal_tolerance as mt
    ra, dec, _ = mt.e2e_catalogue()
    src = z.Source(id='ZUDS20cal', ra=float(ra[0]), dec=float(dec[0]))
    sc.photometry(z, src, [57999.0, 58000.5, 58001.0, 58002.5])
    det = sc.detection(z, image, src, id=4242, ra=float(ra[0]), dec=float(dec[0]))
    packet, = z.make_alerts([det], engine=engine)
    lim = packet.alert['candidate']['diffmaglim']
    assert np.isfinite(lim) and lim == saved['MAGLIM'] and abs(lim - ml['maglim']) < 1e-9
