"""The float64 restatement of the fake-source injection (tests/inject_ref.py) held to known answers, the conditions of the
scenes (tests/inject_scenes.py), the tolerance constants held to tests/measure_inject_tolerance.py, ``zm_inject_layers``
(host only) against the O(n^2) definition, and the CPU side of fakes.py: the draw, the efficiency curve, the settings, the
CSV file, the job's argument errors and the scripts' switches.  No GPU."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import inject_ref as ir
import inject_scenes as isc
import measure_inject_tolerance as mt
from util import pkg, synth


def fakes():
    return pkg().fakes


# ---- the restatement and its scenes ---------------------------------------------------------------------------------------
def test_the_restatement_on_known_answers():
    model = isc.model_dyadic()
    img = np.zeros((20, 24), np.float32)
    r = ir.inject(img, [10.0], [8.0], [16.0], model)
    want = np.zeros((20, 24), np.float32)
    want[7:10, 9:12] = 16.0 * model
    assert np.array_equal(r['img'], want) and r['out_sum'][0] == 16.0 and r['flags'][0] == 0
    assert int(r['nwrites'].sum()) == 9 and not np.shares_memory(r['img'], img) and not img.any()
    # half a pixel off: the profile keeps its sum to rounding, spreads over the taps, and has negative lobes
    r = ir.inject(img, [10.5], [8.0], [16.0], model)
    assert abs(r['out_sum'][0] - 16.0) < 1e-13 and (r['img'] < 0).any() and int(r['nwrites'].sum()) == 3 * 8
    # the rms rule, by hand
    rms = np.full((20, 24), 3.0, np.float32)
    r = ir.inject(img, [10.0], [8.0], [16.0], model, rms=rms, gain=2.0)
    assert r['rms'][8, 10] == np.float32(math.sqrt(9.0 + 4.0 / 2.0)) and r['rms'][0, 0] == 3.0
    assert np.array_equal(ir.inject(img, [10.0], [8.0], [-16.0], model, rms=rms, gain=2.0)['rms'], rms)
    # flags
    r = ir.inject(img, [0.0, -5.0, np.nan, 3.0], [0.0, 8.0, 1.0, 3.0], [1.0, 1.0, 1.0, np.inf], model)
    assert list(r['flags']) == [ir.CLIPPED, ir.CLIPPED | ir.OUTSIDE, ir.BADPOS, ir.BADPOS]
    assert r['out_sum'][1] == 0 and np.isnan(r['out_sum'][2]) and np.isnan(r['out_sum'][3])


def test_the_pixel_rule():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    mid = 0.5 * (float(one) + float(up))
    ok, near = ir.pixel_rule([one, up, up, up, one], [1.0 + 1e-12, mid - 1e-13, mid - 1e-9, mid + 1e-13, mid + 1e-13], 1e-12)
    assert list(ok) == [True, True, False, True, True] and list(near) == [False, True, False, False, True]
    ok, _ = ir.pixel_rule(np.array([np.nan, np.inf, -np.inf, np.inf], np.float32), [np.nan, np.inf, np.inf, 1.0], 1.0)
    assert list(ok) == [True, True, False, False]


def test_scene_conditions():
    """No pixel of a tolerance scene is written twice; the planted special values lie where the scenes say; every flag
    and special case the GPU test names is present; the two precisions agree on every float32 pixel."""
    seen = 0
    for sc in isc.tolerance_scenes():
        assert sc.img.shape[0] <= 80 and sc.img.shape[1] <= 96
        r = mt.run(sc, ir.F64)
        assert int(r['nwrites'].max()) == 1 and int(r['rms_nwrites'].max()) == 1, sc.name
        for (yy, xx) in sc.unwritten:
            assert r['nwrites'][yy, xx] == 0 and ir.same_bits(r['img'][yy, xx], sc.img[yy, xx]), (sc.name, yy, xx)
        for (yy, xx) in sc.written:
            assert r['nwrites'][yy, xx] == 1, (sc.name, yy, xx)
        assert mt.measure_scene(sc)['disagree'] == 0, sc.name
        seen |= int(np.bitwise_or.reduce(r['flags']))
        fl = dict(zip(sc.names, r['flags']))
        if sc.name.startswith('interior'):
            assert fl['phase-zero'] == 0 and fl['negative'] == ir.BAD and fl['fx-minus-half'] == 0
            fx, fy = sc.x - np.floor(sc.x + 0.5), sc.y - np.floor(sc.y + 0.5)
            assert fx[0] == 0 and fy[0] == 0 and fx[1] == -0.5 and fy[2] == -0.5 and fx[3] == 0.25 and fy[3] == 0
            assert 0 < 0.5 - fx[2] < 1e-13
            # the rms specials keep their bytes, the pixels around them move
            assert ir.same_bits(r['rms'], sc.rms).sum() < sc.rms.size and int(r['rms_nwrites'].sum()) > 0
            for (yy, xx) in ((19, 57), (19, 56), (20, 57), (18, 56)):
                assert r['nwrites'][yy, xx] == 1 and r['rms_nwrites'][yy, xx] == 0
        if sc.name.startswith('edges'):
            assert fl['over-specials'] == ir.BAD | ir.NONFINITE and fl['flux-zero'] == ir.BAD
            assert fl['left'] == fl['top'] == fl['corner-high'] == ir.CLIPPED
            assert fl['inside-by-one'] == ir.CLIPPED and r['out_sum'][sc.names.index('inside-by-one')] == 0
            assert fl['outside-by-one'] == fl['outside-left'] == fl['huge'] == ir.CLIPPED | ir.OUTSIDE
            assert fl['x-nan'] == fl['y-inf'] == fl['flux-nan'] == fl['flux-inf'] == ir.BADPOS
            assert np.signbit(sc.img[40, 49]) and sc.img[40, 49] == 0
    assert seen == ir.CLIPPED | ir.OUTSIDE | ir.BAD | ir.NONFINITE | ir.BADPOS


def test_exact_scenes_are_exact_and_the_order_matters_where_planted():
    for sc in isc.exact_scenes():
        a, b = mt.run(sc, ir.F64), mt.run(sc, np.longdouble)
        assert ir.same_bits(a['img'], b['img']).all() and np.array_equal(a['out_sum'], b['out_sum'].astype(np.float64)), sc.name
    for order, want in isc.CHAIN_LAYERS.items():
        sc = isc.chain(order)
        assert tuple(ir.layers(sc.x, sc.y, sc.half)[0]) == want
        # every sum exact: the order cannot matter
        assert np.array_equal(mt.run(sc, ir.F64)['img'], mt.run(isc.chain('abc'), ir.F64)['img'])
    assert int(mt.run(isc.chain('abc'), ir.F64)['nwrites'].max()) == 2
    assert int(mt.run(isc.same_position(), ir.F64)['nwrites'].max()) == 3
    ab, ba = mt.run(isc.order_matters(False), ir.F64)['img'], mt.run(isc.order_matters(True), ir.F64)['img']
    assert ab[15, 25] == np.float32(1.0 + 2.0 ** -23) and ba[15, 25] == np.float32(1.0 + 2.0 ** -22)
    assert int((~ir.same_bits(ab, ba)).sum()) == 1


def test_the_tolerances_are_what_the_measurement_gives():
    seen, disagree = mt.measure()
    for name, key in mt.CONSTANTS:
        print(f'{name}: measured {seen[key]:.3e}, recorded {ir.MEASURED[key]:.3e}, constant 2^{int(math.log2(getattr(ir, name)))}')
        assert getattr(ir, name) == mt.pow2_up(seen[key]), name
        assert abs(seen[key] - ir.MEASURED[key]) <= 1e-3 * ir.MEASURED[key], name
    assert not any(disagree.values()), disagree


# ---- zm_inject_layers -----------------------------------------------------------------------------------------------------
def test_layers_against_the_definition():
    f = fakes()
    rng = np.random.default_rng(5)
    for half in (1, 12):
        x, y = rng.uniform(-20, 276, 2000), rng.uniform(-20, 276, 2000)
        x[::97], y[::131] = np.nan, np.inf
        x[5], y[6] = 1.0e300, -1.0e300
        got, nl = f.inject_layers(x, y, half)
        want, wl = ir.layers(x, y, half)
        assert np.array_equal(got, want) and nl == wl and nl > (3 if half == 12 else 1), (half, nl, wl)
    for order, want in isc.CHAIN_LAYERS.items():
        sc = isc.chain(order)
        got, nl = f.inject_layers(sc.x, sc.y, sc.half)
        assert tuple(got) == want and nl == max(want), order
    # boxes exactly 2 (half + 3) apart share a pixel, one further they do not
    assert tuple(f.inject_layers([10.0, 18.0, 27.0], [5.0, 5.0, 5.0], 1)[0]) == (1, 2, 1)
    assert tuple(f.inject_layers([10.4, 18.6], [5.0, 5.0], 1)[0]) == (1, 1)          # ix 10 and 19
    got, nl = f.inject_layers(np.full(50, 7.25), np.full(50, 9.5), 3)
    assert list(got) == list(range(1, 51)) and nl == 50
    got, nl = f.inject_layers([], [], 5)
    assert got.size == 0 and nl == 0
    got, nl = f.inject_layers([3.0], [4.0], 5)
    assert list(got) == [1] and nl == 1
    got, nl = f.inject_layers([np.nan, 3.0], [4.0, np.inf], 5)
    assert list(got) == [0, 0] and nl == 0
    L = pkg()._lib.lib()
    nl = C.c_int(-1)
    assert L.zm_inject_layers(1, None, None, 5, None, C.byref(nl)) != 0 and b'zm_inject_layers' in L.zm_last_error()
    with pytest.raises(pkg().ZMError, match='zm_inject_layers'):
        f.inject_layers([1.0], [1.0], 16)


# ---- the draw -------------------------------------------------------------------------------------------------------------
def test_draw_fakes():
    f, s = fakes(), synth()
    w = s.tan_wcs(300, 260)
    st = f.fake_settings(dict(N=20, MAG_MIN=18.0, MAG_MAX=21.0, SEED=7))
    assert st['min_sep'] == 31.0 and st['border'] == 15.0 and st['match_radius'] == 2.0 and st['gain'] == 0.0
    a, b = f.draw_fakes((260, 300), w, 27.5, st), f.draw_fakes((260, 300), w, 27.5, st)
    assert a.dtype == f.FAKE_DTYPE and a.tobytes() == b.tobytes() and len(a) == 20 and list(a['id']) == list(range(20))
    assert a.tobytes() != f.draw_fakes((260, 300), w, 27.5, dict(st, seed=8)).tobytes()
    assert (a['mag'] >= 18.0).all() and (a['mag'] < 21.0).all()
    assert np.array_equal(a['flux'], 10.0 ** (-0.4 * (a['mag'] - 27.5)))
    assert (a['x'] >= 15).all() and (a['x'] <= 299 - 15).all() and (a['y'] >= 15).all() and (a['y'] <= 259 - 15).all()
    d = np.hypot(a['x'][:, None] - a['x'][None, :], a['y'][:, None] - a['y'][None, :]) + 1e9 * np.eye(20)
    assert d.min() >= 31.0
    box = np.maximum(np.abs(a['x'][:, None] - a['x'][None, :]), np.abs(a['y'][:, None] - a['y'][None, :])) + 1e9 * np.eye(20)
    assert box.min() >= 31.0                                                          # apart along x or along y
    assert f.inject_layers(a['x'], a['y'], 12)[1] == 1                                # the default MIN_SEP: one layer
    ra, dec = w.all_pix2world(a['x'], a['y'], 0)
    assert np.array_equal(a['ra'], ra) and np.array_equal(a['dec'], dec)
    # avoid_xy and clean
    ax, ay = np.array([150.0, 60.0, np.nan]), np.array([130.0, 200.0, 5.0])
    clean = np.zeros((260, 300), bool)
    clean[:, 100:] = True
    c = f.draw_fakes((260, 300), w, 27.5, dict(st, n=8), avoid_xy=(ax, ay), clean=clean)
    assert (np.hypot(c['x'][:, None] - ax[None, :2], c['y'][:, None] - ay[None, :2]) >= 31.0).all()
    assert (np.floor(c['x'] + 0.5) >= 100).all()
    # no room: too many for the frame, a frame smaller than its border, nowhere clean
    with pytest.raises(RuntimeError, match='no room'):
        f.draw_fakes((260, 300), w, 27.5, dict(st, n=200))
    with pytest.raises(RuntimeError, match='no room'):
        f.draw_fakes((30, 30), None, 27.5, dict(st, n=1))
    with pytest.raises(RuntimeError, match='no room'):
        f.draw_fakes((260, 300), w, 27.5, dict(st, n=1), clean=np.zeros((260, 300), bool))
    assert len(f.draw_fakes((260, 300), None, 27.5, dict(st, n=0))) == 0
    assert np.isnan(f.draw_fakes((260, 300), None, 27.5, dict(st, n=2))['ra']).all()


def test_fake_settings():
    f, p = fakes(), pkg().psf
    with pytest.raises(ValueError, match='FWHM'):
        f.fake_settings({'FWHM': 3, 'MAG_MIN': 1, 'MAG_MAX': 2})
    with pytest.raises(ValueError, match='unknown setting'):
        f.fake_settings(mag_min=1, mag_max=2, sigma=1)
    with pytest.raises(ValueError, match='MAGLIM'):
        f.fake_settings()
    with pytest.raises(ValueError):
        f.fake_settings(mag_min=3, mag_max=2)
    with pytest.raises(ValueError):
        f.fake_settings(mag_min=1, mag_max=2, match_radius=0)
    st = f.fake_settings(header={'MAGLIM': 20.5, 'GAIN': 6.2})
    assert (st['n'], st['mag_min'], st['mag_max'], st['seed'], st['gain']) == (200, 18.0, 21.5, 0, 6.2)
    model = p.PSFModel(np.full((11, 11), 1.0 / 121), cards={'PSFFITR': 1.5})
    st = f.fake_settings({'-N': '7', 'MAG_MAX': 19}, header={'MAGLIM': 20.5}, psf=model, seed=3)
    assert (st['n'], st['mag_max'], st['seed'], st['min_sep'], st['border'], st['core_radius']) == (7, 19.0, 3, 17.0, 8.0, 1.5)


# ---- the efficiency curve ---------------------------------------------------------------------------------------------------
def _table(mag, rec, flags=None):
    t = np.zeros(len(mag), [('mag', np.float64), ('recovered', np.bool_), ('inj_flags', np.int32)])
    t['mag'], t['recovered'] = mag, rec
    if flags is not None:
        t['inj_flags'] = flags
    return t


def test_efficiency():
    f = fakes()
    # bins 18 .. 22 of one mag: 4 / 4, 3 / 4, 1 / 4, 0 / 4
    mag = np.repeat([18.5, 19.5, 20.5, 21.5], 4) + np.tile([-0.3, -0.1, 0.1, 0.3], 4)
    rec = np.array([1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0], bool)
    e = f.efficiency(_table(mag, rec), step=1.0)
    assert list(e['edges']) == [18.0, 19.0, 20.0, 21.0, 22.0] and list(e['n']) == [4] * 4 and list(e['nrec']) == [4, 3, 1, 0]
    assert list(e['eff']) == [1.0, 0.75, 0.25, 0.0] and e['nused'] == 16 and e['nskipped'] == 0
    # Wilson at z = 1, n = 4: (p + 1/8 -+ sqrt(p (1 - p) / 4 + 1/64)) / (1 + 1/4)
    for k, p in enumerate([1.0, 0.75, 0.25, 0.0]):
        hw = math.sqrt(p * (1 - p) / 4 + 1 / 64) / 1.25
        assert abs(e['lo'][k] - ((p + 0.125) / 1.25 - hw)) < 1e-15 and abs(e['hi'][k] - ((p + 0.125) / 1.25 + hw)) < 1e-15
    assert abs(e['lo'][3]) < 1e-15 and abs(e['hi'][3] - 0.2) < 1e-15 and abs(e['lo'][0] - 0.8) < 1e-15 and abs(e['hi'][0] - 1) < 1e-15
    # 0.75 at 19.5 -> 0.25 at 20.5: 0.5 half way; 1.0 at 18.5 -> 0.75 at 19.5: 0.8 at 18.5 + 0.8
    assert abs(e['m50'] - 20.0) < 1e-12 and abs(e['m80'] - 19.3) < 1e-12
    # explicit edges with an empty bin in the middle of the fall: the crossing is between the bins that have fakes
    e = f.efficiency(_table([18.5, 18.6, 21.5, 21.6], [1, 1, 0, 0]), edges=[18, 19, 20, 21, 22])
    assert list(e['n']) == [2, 0, 0, 2] and np.isnan(e['eff'][1]) and np.isnan(e['lo'][2]) and np.isnan(e['hi'][1])
    assert abs(e['m50'] - 20.0) < 1e-12 and abs(e['m80'] - (18.5 + 0.2 * 3)) < 1e-12
    # no crossing: everything found, nothing found, a rise
    assert np.isnan(f.efficiency(_table(mag, np.ones(16, bool)), step=1.0)['m50'])
    assert np.isnan(f.efficiency(_table(mag, np.zeros(16, bool)), step=1.0)['m50'])
    assert np.isnan(f.efficiency(_table(mag, rec[::-1]), step=1.0)['m50'])
    # the first crossing counts: 1, 0, 1, 0
    e = f.efficiency(_table([18.5, 19.5, 20.5, 21.5], [1, 0, 1, 0]), step=1.0)
    assert abs(e['m50'] - 19.0) < 1e-12
    # fakes that never reached the frame are left out and counted
    fl = np.zeros(16, np.int32)
    fl[0], fl[5], fl[9] = 3, 16, 1
    e = f.efficiency(_table(mag, rec, fl), step=1.0)
    assert e['nskipped'] == 2 and e['nused'] == 14 and list(e['n']) == [3, 3, 4, 4] and list(e['nrec']) == [3, 2, 1, 0]
    e = f.efficiency(_table([], []))
    assert e['nused'] == 0 and np.isnan(e['m50']) and np.isnan(e['eff']).all()
    with pytest.raises(ValueError):
        f.efficiency(_table(mag, rec), edges=[20, 19])


def test_csv_round_trip(tmp_path):
    f, s = fakes(), synth()
    st = f.fake_settings(dict(N=12, MAG_MIN=18.0, MAG_MAX=21.0))
    t = f.draw_fakes((200, 200), s.tan_wcs(200, 200), 27.123456789, st)
    rng = np.random.default_rng(1)
    full = f._append_columns(t, [('flux_in', np.float64, t['flux'] * (1 - 1e-9)), ('inj_flags', np.int32, rng.integers(0, 32, 12)),
                                 ('detected', np.bool_, rng.uniform(size=12) < 0.7), ('recovered', np.bool_, rng.uniform(size=12) < 0.5),
                                 ('det_number', np.int32, rng.integers(-1, 99, 12)), ('sep_px', np.float64, rng.uniform(0, 2, 12)),
                                 ('flux_aper', np.float64, rng.normal(size=12)), ('fluxerr_aper', np.float64, rng.uniform(size=12))])
    full['sep_px'][3] = full['flux_aper'][3] = np.nan
    for tab in (t, full):
        path = f.write_fakes_csv(tmp_path / 'x.fakes.csv', tab)
        back = f.read_fakes_csv(path)
        assert back.dtype == tab.dtype and back.tobytes() == tab.tobytes()
    assert open(path).readline().strip().split(',')[:3] == ['id', 'x', 'y']


# ---- the pool's job and the scripts, as far as no GPU is needed ---------------------------------------------------------------
def test_job_argument_errors():
    nightly = importlib.import_module('zuds-pipeline_amd.nightly')
    p = pkg().psf
    model = p.PSFModel(np.full((25, 25), 1.0 / 625))
    good = dict(psf=model, zp=27.0, MAG_MIN=18, MAG_MAX=21)
    with pytest.raises(ValueError, match='fakes needs detect'):
        nightly.SubtractionJob({}, {}, fakes=good)
    with pytest.raises(ValueError, match='PSFModel'):
        nightly.SubtractionJob({}, {}, detect=True, fakes=dict(zp=27.0, MAG_MIN=18, MAG_MAX=21))
    with pytest.raises(ValueError, match='PSFModel'):
        nightly.SubtractionJob({}, {}, detect=True, fakes=dict(good, psf=model.data))
    with pytest.raises(ValueError, match='zp'):
        nightly.SubtractionJob({}, {}, detect=True, fakes=dict(psf=model, MAG_MIN=18, MAG_MAX=21))
    with pytest.raises(ValueError, match='zp'):
        nightly.SubtractionJob({}, {}, detect=True, fakes=dict(good, zp=float('nan')))
    with pytest.raises(ValueError, match='FWHM'):
        nightly.SubtractionJob({}, {}, detect=True, fakes=dict(good, FWHM=2))
    with pytest.raises(ValueError, match='MAGLIM'):
        nightly.SubtractionJob({}, {}, detect=True, fakes=dict(psf=model, zp=27.0))
    job = nightly.SubtractionJob({'header': {'MAGLIM': 20.0, 'GAIN': 2.0}}, {}, detect=True, fakes=dict(psf=model, zp=27.0, N=9))
    assert job.fake_settings['n'] == 9 and job.fake_settings['mag_max'] == 21.0 and job.fake_settings['gain'] == 2.0
    assert job.fakes['zp'] == 27.0 and job.fakes['psf'] is model
    assert nightly.SubtractionJob({}, {}, detect=True).fakes is None


def test_scripts_refuse_fakes_without_detect_or_a_model(capsys, tmp_path):
    from test_catalog_gpu import load_script
    for name in ('dosub', 'donightly'):
        script = load_script(name)
        assert script.main(['images.txt', 'ref.fits', '--fakes']) == 2
        assert '--fakes needs --detect' in capsys.readouterr().err
        assert script.main(['images.txt', 'ref.fits', '--psf', '--fakes', '50']) == 2
        assert '--fakes needs --detect' in capsys.readouterr().err
        assert script.main(['images.txt', 'ref.fits', '--detect', '--fake-seed', '3']) == 2
        assert '--fake-seed needs --fakes' in capsys.readouterr().err
        assert script.main(['images.txt', 'ref.fits', '--detect', '--fake-mags', '18,21']) == 2
        assert '--fake-mags needs --fakes' in capsys.readouterr().err
        assert script.main(['images.txt', 'ref.fits', '--detect', '--psf', '--fakes', '--fake-mags', '21']) == 2
        assert '--fake-mags' in capsys.readouterr().err
        assert script.main(['images.txt', 'ref.fits', '--detect', '--psf', '--fakes', '-5']) == 2
        assert '--fakes' in capsys.readouterr().err
        # no --psf and no <sci>.psf.fits beside the frame
        lst = tmp_path / f'{name}.txt'
        lst.write_text(str(tmp_path / 'sci_a.fits') + '\n')
        assert script.main([str(lst), 'ref.fits', '--detect', '--fakes']) == 2
        assert '--fakes needs a PSF model' in capsys.readouterr().err
