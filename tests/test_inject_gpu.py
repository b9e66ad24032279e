"""``csrc/inject.hip`` and ``fakes.py`` on the GPU against the float64 restatement (tests/inject_ref.py) on the scenes of
tests/inject_scenes.py, whose conditions tests/test_inject_ref.py asserts on the restatement alone.  Flags are compared
exactly, ``out_sum`` within ``SUM_RTOL``, written pixels by the pixel rule of inject_ref.py (at most ``MAX_NEAR`` pixels of
a scene may need its second clause; every test prints how many did), every pixel that is not written as ``uint32``.  The
exact scenes are compared bit for bit.  Host and ``_dev`` entry points run on the same scenes.  Then the recovery pass and
the pool on one science frame of tests/test_pool_detect_gpu.py."""
import importlib

import numpy as np
import pytest

import inject_ref as ir
import inject_scenes as isc
from psf_scenes import BAD_BITS, model_gaussian
from test_psf_gpu import dev, on_a_stream
from util import pkg, synth

pytestmark = pytest.mark.gpu


def fakes():
    return pkg().fakes


def run(engine, sc, device, sel=None, gain=None, with_rms=True, img=None):
    """(img, rms, out_sum, flags) of the scene's fakes (``sel``: a subset or an order of them) through the host or the
    ``_dev`` form."""
    f = fakes()
    sel = np.arange(sc.x.size) if sel is None else np.asarray(sel, dtype=np.int64)
    gain = sc.gain if gain is None else gain
    x, y, flux = sc.x[sel], sc.y[sel], sc.flux[sel]
    img = sc.img if img is None else img
    if not device:
        r = f.inject((img, sc.rms if with_rms else None, sc.mask), (x, y, flux), sc.model, gain=gain,
                     core_radius=sc.core_radius, bad_bits=BAD_BITS, engine=engine)
        return r['img'], r['rms'], r['flux_in'], r['inj_flags']
    with on_a_stream(engine):
        dimg, drms = dev(img), dev(sc.rms) if with_rms else None
        s, fl = f.inject_dev(dimg, x, y, flux, dev(sc.model), rms=drms, mask=dev(sc.mask), gain=gain,
                             core_radius=sc.core_radius, bad_bits=BAD_BITS, engine=engine)
    return dimg.cpu().numpy(), None if drms is None else drms.cpu().numpy(), s.cpu().numpy(), fl.cpu().numpy()


def reference(sc, sel=None, gain=None, with_rms=True):
    sel = np.arange(sc.x.size) if sel is None else np.asarray(sel, dtype=np.int64)
    return ir.inject(sc.img, sc.x[sel], sc.y[sel], sc.flux[sel], sc.model, rms=sc.rms if with_rms else None, mask=sc.mask,
                     bad_bits=BAD_BITS, gain=sc.gain if gain is None else gain, core_radius=sc.core_radius)


def hold(sc, got, ref, what):
    """The comparison of one call on a tolerance scene (no pixel written twice)."""
    img, rms, out_sum, flags = got
    assert np.array_equal(flags, ref['flags']), (what, list(zip(flags, ref['flags'])))
    assert np.array_equal(np.isnan(out_sum), np.isnan(ref['out_sum'])), what
    fin = np.isfinite(ref['out_sum'])
    d = np.abs(out_sum - ref['out_sum'])[fin]
    worst = float(np.max(d / np.maximum(np.abs(ref['out_sum'][fin]), 1e-300))) if d.size else 0.0
    w = ref['nwrites'] > 0
    assert ir.same_bits(img, sc.img)[~w].all(), (what, 'a pixel no fake writes changed')
    with np.errstate(invalid='ignore', over='ignore'):
        want = ref['base'].astype(np.float64) + ref['v']
        slack = ir.INJ_TOL * (np.abs(ref['base'].astype(np.float64)) + np.abs(ref['v']))
    ok, near = ir.pixel_rule(img[w], want[w], slack[w])
    nnear = int(near.sum())
    nrms = 0
    if rms is not None:
        rw = ref['rms_nwrites'] > 0
        assert ir.same_bits(rms, sc.rms)[~rw].all(), (what, 'an rms pixel the rule does not write changed')
        rok, rnear = ir.pixel_rule(rms[rw], ref['rms_want'][rw], ir.RMS_TOL * ref['rms_want'][rw])
        assert rok.all(), (what, 'rms', int((~rok).sum()))
        nrms = int(rw.sum())
        nnear += int(rnear.sum())
    print(f'{what}: {int(w.sum())} image and {nrms} rms pixels written, {nnear} needed the second clause of the pixel rule; '
          f'out_sum off by {worst:.3e} relative ({worst / ir.SUM_RTOL:.3e} of its tolerance)')
    assert ok.all(), (what, int((~ok).sum()))
    assert (out_sum[fin][ref['out_sum'][fin] == 0] == 0).all() and worst <= ir.SUM_RTOL, what
    assert nnear <= ir.MAX_NEAR, what


# ---- phases, edges, special values ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('half', [1, 12, 15])
def test_phases_and_specials(engine, half, device):
    """fx, fy of exactly 0, exactly -0.5 and one ulp below 0.5; a negative flux; a bad pixel just inside and just outside
    the core radius; a NaN with a payload and a -0.0 in the box where the profile is 0 (bytes kept); rms entries that are
    0, negative, NaN and inf under a footprint (bytes kept, the pixels around them written)."""
    sc = isc.interior(half)
    hold(sc, run(engine, sc, device), reference(sc), f'{sc.name} {"dev" if device else "host"}')


@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('half', [1, 12, 15])
def test_edges_and_positions(engine, half, device):
    """Boxes cut at each edge and at two corners, a box that touches the frame with a column of zeros, boxes wholly outside
    (by one pixel, far, at 1e300), x, y and flux that are not finite, a flux of 0, and NaN, inf and -0.0 under a footprint."""
    sc = isc.edges(half)
    got = run(engine, sc, device)
    hold(sc, got, reference(sc), f'{sc.name} {"dev" if device else "host"}')
    k = sc.names.index('over-specials')
    assert np.isnan(got[0][40, 48]) and np.isposinf(got[0][41, 48]) and got[0][40, 49] != 0 and got[3][k] & ir.NONFINITE


@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65])
def test_counts(engine, n, device):
    sc = isc.counts()
    sel = np.arange(n)
    got = run(engine, sc, device, sel=sel)
    assert got[2].shape == (n,) and got[3].shape == (n,)
    hold(sc, got, reference(sc, sel=sel), f'counts n = {n} {"dev" if device else "host"}')
    if n == 0:
        assert ir.same_bits(got[0], sc.img).all() and ir.same_bits(got[1], sc.rms).all()


# ---- the rms plane ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
def test_rms_is_left_alone_without_a_gain_or_a_plane(engine, device):
    sc = isc.interior(12)
    ref = reference(sc)
    assert int(ref['rms_nwrites'].sum()) > 100 and (ref['v'][ref['nwrites'] > 0] < 0).any()      # the rule has work, and v < 0 occurs
    img0, rms0, sum0, fl0 = run(engine, sc, device, gain=0.0)
    assert ir.same_bits(rms0, sc.rms).all()
    img1, rms1, sum1, fl1 = run(engine, sc, device, with_rms=False)
    assert rms1 is None
    img2, rms2, _, _ = run(engine, sc, device)
    assert not ir.same_bits(rms2, sc.rms).all()
    # the image does not depend on what happens to the rms plane
    for a in (img0, img1):
        assert ir.same_bits(a, img2).all()
    assert np.array_equal(sum0, sum1) and np.array_equal(fl0, fl1)
    # v > 0 decides: of the fake of negative flux only the pixels under the negative lobes of its profile move
    neg = ref['rms_nwrites'][57 - 15:57 + 16, 57 - 15:57 + 16]
    assert sc.flux[3] < 0 and int(neg.sum()) > 0 and int(neg.sum()) < int(ref['nwrites'][57 - 15:57 + 16, 57 - 15:57 + 16].sum()) / 2


# ---- overlaps, exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
def test_overlaps_are_added_in_index_order(engine, device):
    """The a - b - c chain in four index orders, two fakes on one position, and the scene whose result depends on the order
    by a planted tie: bit for bit what adding the fakes one at a time gives."""
    for sc in isc.exact_scenes():
        ref = reference(sc)
        img, rms, out_sum, flags = run(engine, sc, device)
        assert ir.same_bits(img, ref['img']).all(), sc.name
        assert np.array_equal(out_sum, ref['out_sum']) and np.array_equal(flags, ref['flags']), sc.name
        assert ir.same_bits(rms, sc.rms).all()
    ab = run(engine, isc.order_matters(False), device)[0]
    ba = run(engine, isc.order_matters(True), device)[0]
    assert ab[15, 25] == np.float32(1.0 + 2.0 ** -23) and ba[15, 25] == np.float32(1.0 + 2.0 ** -22)


# ---- reproducibility ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('device', [False, True], ids=['host', 'dev'])
def test_same_bytes_on_every_run_and_in_every_order_of_disjoint_fakes(engine, device):
    sc = isc.counts()
    a = run(engine, sc, device)
    b = run(engine, sc, device)
    for u, v in zip(a[:2], b[:2]):
        assert ir.same_bits(u, v).all()
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    perm = np.random.default_rng(3).permutation(sc.x.size)
    c = run(engine, sc, device, sel=perm)
    for u, v in zip(a[:2], c[:2]):
        assert ir.same_bits(u, v).all()
    assert np.array_equal(a[2][perm], c[2]) and np.array_equal(a[3][perm], c[3])
    # and a many-layer call: the 65 fakes on nine positions
    pos = np.arange(65) % 9
    x, y = sc.x[pos], sc.y[pos]
    assert fakes().inject_layers(x, y, sc.half)[1] == 8
    f = fakes()
    outs = [f.inject((sc.img, sc.rms, sc.mask), (x, y, sc.flux), sc.model, gain=sc.gain, core_radius=2.0, bad_bits=BAD_BITS,
                     engine=engine) for _ in range(2)]
    want = ir.inject(sc.img, x, y, sc.flux, sc.model, rms=sc.rms, mask=sc.mask, bad_bits=BAD_BITS, gain=sc.gain, core_radius=2.0)
    assert ir.same_bits(outs[0]['img'], outs[1]['img']).all() and ir.same_bits(outs[0]['rms'], outs[1]['rms']).all()
    assert np.array_equal(outs[0]['inj_flags'], want['flags'])
    # eight additions deep, the float32 value each starts from is the kernel's own: the planes equal the restatement's except
    # where an addition came within INJ_TOL of a tie, which the cap of the pixel rule allows for
    off = int((~ir.same_bits(outs[0]['img'], want['img'])).sum()) + int((~ir.same_bits(outs[0]['rms'], want['rms'])).sum())
    print(f'eight layers: {off} pixel(s) differ from the restatement')
    assert off <= ir.MAX_NEAR


def test_arguments(engine):
    z, f = pkg(), fakes()
    L = engine.L
    img = np.zeros((16, 16), np.float32)
    one = np.array([8.0])
    m = isc.model_dyadic()
    fl = np.zeros(1, np.int32)
    args = lambda **kw: [engine.ctx, kw.get('img', img.ctypes.data), None, None, 0, 16, 16, kw.get('n', 1), one.ctypes.data, one.ctypes.data,
                         kw.get('flux', one.ctypes.data), m.ctypes.data, kw.get('half', 1), kw.get('gain', 0.0), kw.get('core', 2.0), None,
                         kw.get('flags', fl.ctypes.data)]
    for fn, name in ((L.zm_inject, b'zm_inject'), (L.zm_inject_dev, b'zm_inject_dev')):
        for kw in (dict(half=0), dict(half=16), dict(gain=-1.0), dict(gain=float('nan')), dict(core=-0.5), dict(core=float('inf')),
                   dict(img=None), dict(flux=None), dict(flags=None)):
            assert fn(*args(**kw)) != 0 and name in L.zm_last_error(), (name, kw)
        assert fn(*args(n=0, flux=None, flags=None)) == 0                      # n == 0 returns at once
    assert L.zm_inject(*args()) == 0 and img[8, 8] == 2.0 and fl[0] == 0
    with pytest.raises(ValueError):
        f.inject(np.zeros((4, 4, 4), np.float32), (one, one, one), m, engine=engine)
    with pytest.raises(z.ZMError, match='zm_inject'):
        f.inject(img, (one, one, one), np.zeros((33, 33)), engine=engine)
    src = np.zeros((16, 16), np.float32)
    out = f.inject(src, (one, one, one), m, engine=engine)
    assert not src.any() and out['img'][8, 8] == 2.0 and out['rms'] is None and out['flux_in'][0] == 8.0


# ---- round trip through the PSF fit -----------------------------------------------------------------------------------------------
def test_round_trip_through_the_psf_fit(engine):
    """Fakes injected into a plane of zeros and fitted with the same model (unit weights, no sky term, R = 6) come back to
    2^-23: each pixel is rounded to float32 once (2^-24 relative), with a factor 2 over it."""
    z = pkg()
    model = model_gaussian(12)
    rng = np.random.default_rng(8)
    gx, gy = np.meshgrid(20.0 + 32.0 * np.arange(4), 20.0 + 32.0 * np.arange(3))
    x = gx.ravel() + np.array([0.0, -0.5, 0.25, 0.5 - 2.0 ** -40] + list(rng.uniform(-0.5, 0.5, 8)))
    y = gy.ravel() + np.array([0.0, 0.3, -0.5, 0.1] + list(rng.uniform(-0.5, 0.5, 8)))
    flux = np.full(12, 1.0e3)
    with on_a_stream(engine):
        img = dev(np.zeros((104, 136), np.float32))
        s, fl = fakes().inject_dev(img, x, y, flux, dev(model), engine=engine)
        fit = z.psf.psf_photometry_dev(img, dev(x), dev(y), dev(model), fit_radius=6.0, fit_sky=0, engine=engine)
    got = fit['flux'].cpu().numpy()
    assert (fl.cpu().numpy() == 0).all() and (fit['flags'].cpu().numpy() == 0).all()
    worst = float(np.max(np.abs(got / flux - 1.0)))
    print(f'round trip: largest |flux_fit / flux - 1| = {worst:.3e} ({worst / 2.0 ** -23:.3f} of 2^-23); '
          f'deposited / flux - 1 up to {float(np.max(np.abs(s.cpu().numpy() / flux - 1.0))):.3e}')
    assert worst <= 2.0 ** -23


# ---- recovery through the subtraction ---------------------------------------------------------------------------------------------
_REC = {}


def recovery_scene(engine):
    """One science frame of tests/test_pool_detect_gpu.py, its products without fakes, and 30 positions on its clean ground
    away from the stars and the planted transients."""
    if _REC:
        return _REC
    import torch
    import test_pool_detect_gpu as tp
    z, s = pkg(), synth()
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    scis, ref, radec, planted = tp.scene(torch, z, s, 1)
    sci = scis[0]
    kw = dict(nreg_side=2, hotpants_kws={'ko': 1, 'bgo': 0})
    pool = nm.SubtractionPool(1)
    plain = pool.map([nm.SubtractionJob(sci, ref, radec=radec, tag=0, detect=True, **kw)])[0]
    pool.close()
    assert 'error' not in plain and plain['cat'] is not None
    f = fakes()
    model = z.psf.PSFModel(model_gaussian(12, fwhm=2.4), cards={'PSFFITR': 6.0})
    # the stars, as tp.scene draws them (its generator's first draws), the planted transients and what the run without
    # fakes detected; 15 px from all of them and from each other, 40 px from the border: the rules tp.scene plants by
    rng = np.random.default_rng(4100)
    nst = int(640 * 600 / 2500)
    xs, ys = rng.uniform(-10, 650, nst), rng.uniform(-10, 610, nst)
    sra, sdec = s.ztf_wcs(640, 600, tpv=True).all_pix2world(xs, ys, 0)
    sx, sy = sci['wcs'].all_world2pix(sra, sdec, 0)
    cat = plain['cat']
    avoid = (np.concatenate([sx, cat['X_IMAGE'] - 1.0, planted[0][0]]), np.concatenate([sy, cat['Y_IMAGE'] - 1.0, planted[0][1]]))
    st = f.fake_settings(dict(N=30, MAG_MIN=20.0, MAG_MAX=20.0, SEED=11, MIN_SEP=15.0, BORDER=40.0), psf=model)
    zp = 20.0 + 2.5 * np.log10(3000.0)                     # mag 20 is a flux of 3000
    table = f.draw_fakes((600, 640), sci['wcs'], zp, st, avoid_xy=avoid, clean=tp.clean_ground(z, plain))
    np.testing.assert_allclose(table['flux'], 3000.0, rtol=1e-12)
    _REC.update(sci=sci, ref=ref, radec=radec, kw=kw, plain=plain, model=model, st=st, zp=zp, table=table)
    return _REC


def recover(engine, R, table):
    devmod = importlib.import_module('zuds-pipeline_amd.device')
    sci, ref = R['sci'], R['ref']
    ch = devmod.DeviceSubtraction(sci['wcs'], ref['wcs'], engine=engine)
    try:
        return fakes().recover_dev(ch, sci['img'], sci['rms'], sci['mask'], sci['wgt'], ref['img'], ref['rms'], ref['mask'], 2.4,
                                   table, R['model'], run_kws=dict(R['kw'], ref_flxscale=1.0), candidate_kws=dict(wcs=sci['wcs']),
                                   match_radius=R['st']['match_radius'])
    finally:
        engine.set_stream(0)


def test_recovery_of_bright_fakes_and_of_fakes_of_no_flux(engine):
    import torch
    import test_pool_detect_gpu as tp
    R = recovery_scene(engine)
    table, plain, radius = R['table'], R['plain'], R['st']['match_radius']
    # the scene's condition: the run without fakes has no GOODCUT row within MATCH_RADIUS of a drawn position
    good = plain['cat'][plain['cat']['GOODCUT'] == 1]
    d = np.hypot(good['X_IMAGE'][None, :] - 1.0 - table['x'][:, None], good['Y_IMAGE'][None, :] - 1.0 - table['y'][:, None])
    assert d.size == 0 or d.min() > radius
    before = [R['sci'][k].clone() for k in ('img', 'rms')]
    got, cat, nfound = recover(engine, R, table)
    torch.cuda.synchronize()
    for k, b in zip(('img', 'rms'), before):
        assert torch.equal(R['sci'][k].view(torch.int32), b.view(torch.int32)), k
    print(f'30 fakes of flux 3000: {int(got["detected"].sum())} detected, {int(got["recovered"].sum())} recovered, largest '
          f'separation {np.nanmax(got["sep_px"]):.3f} px, flux_aper / flux {np.nanmin(got["flux_aper"] / 3000):.3f} .. '
          f'{np.nanmax(got["flux_aper"] / 3000):.3f}; {len(cat)} rows against {len(plain["cat"])} without fakes')
    assert got['recovered'].all() and got['detected'].all() and (got['sep_px'] < radius).all()
    assert (got['inj_flags'] == 0).all() and (got['det_number'] > 0).all()
    np.testing.assert_allclose(got['flux_in'], 3000.0, rtol=1e-6)
    e = fakes().efficiency(got)
    assert e['nused'] == 30 and e['nskipped'] == 0 and int(e['nrec'].sum()) == 30 and np.isnan(e['m50'])
    # fakes of no flux: nothing is written, the table is the one of the run without fakes, none is recovered
    zero = table.copy()
    zero['flux'] = 0.0
    got0, cat0, nfound0 = recover(engine, R, zero)
    tp.same_table(cat0, plain['cat'])
    assert cat0.tobytes() == plain['cat'].tobytes() and nfound0 == plain['nfound']
    assert not got0['recovered'].any() and (got0['flux_in'] == 0).all() and (got0['inj_flags'] == 0).all()


def test_pool_job_with_fakes_changes_nothing_else(engine):
    import torch
    import test_pool_detect_gpu as tp
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    R = recovery_scene(engine)
    sci, ref, plain = R['sci'], R['ref'], R['plain']
    spec = dict(psf=R['model'], zp=R['zp'], N=30, MAG_MIN=20.0, MAG_MAX=20.0, SEED=11, MIN_SEP=15.0, BORDER=40.0)
    job = nm.SubtractionJob(sci, ref, radec=R['radec'], tag=0, detect=True, fakes=spec, **R['kw'])
    pool = nm.SubtractionPool(1)
    out = pool.map([job])[0]
    again = pool.map([nm.SubtractionJob(sci, ref, radec=R['radec'], tag=0, detect=True, **R['kw'])])[0]
    pool.close()
    assert 'error' not in out and set(out) - set(plain) == {'fakes', 'efficiency'}
    for other in (plain, again):                       # (again: the worker's chain held a fake run in between)
        tp.results_equal(torch, out, other)
        assert out['info'] == other['info'] and out['nfound'] == other['nfound']
    t, e = out['fakes'], out['efficiency']
    assert len(t) == 30 and e['nused'] == 30 and {'flux_in', 'inj_flags', 'recovered', 'sep_px'} <= set(t.dtype.names)
    print(f'pool job: {int(t["recovered"].sum())} of 30 fakes of flux 3000 recovered (they avoid only what the job detected)')
    lanes = nm.SubtractionPool(1, batch=2)
    try:
        with pytest.raises(ValueError, match='fakes'):
            lanes.map([job])
    finally:
        lanes.close()


def test_a_fake_pass_that_fails_costs_the_job_nothing(engine):
    """No room for the fakes: the job keeps every product of the real run and says why it has no efficiency."""
    import torch
    import test_pool_detect_gpu as tp
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    R = recovery_scene(engine)
    spec = dict(psf=R['model'], zp=R['zp'], N=500, MAG_MIN=20.0, MAG_MAX=20.0)       # (at 31 px apart at most 19 x 17 fit)
    pool = nm.SubtractionPool(1)
    out = pool.map([nm.SubtractionJob(R['sci'], R['ref'], radec=R['radec'], tag=0, detect=True, fakes=spec, **R['kw'])])[0]
    pool.close()
    assert 'error' not in out and out['fakes'] is None and out['efficiency'] is None and 'no room' in out['fakes_error']
    tp.results_equal(torch, out, R['plain'])
    assert out['info'] == R['plain']['info']


def test_with_a_real_bogus_model_the_stamps_show_the_fakes(engine, monkeypatch):
    """The network scores triplets of THIS run: the 'new' cutout of a recovered fake holds the fake, in ``recover_dev`` even
    when the caller names the frame without the fakes as ``sci``, and in the pool's job.  (A VGG6 with Glorot weights scores
    every row 0.5; the cut is far below.)"""
    import torch
    import braai_ref as br
    z = pkg()
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    devmod = importlib.import_module('zuds-pipeline_amd.device')
    rbmod = importlib.import_module('zuds-pipeline_amd.realbogus')
    R = recovery_scene(engine)
    sci, ref, table = R['sci'], R['ref'], R['table']
    size, nch, spec = br.vgg6_spec()
    model = rbmod.RBModel(open(br.VGG6_JSON).read(), br.glorot_weights(size, nch, spec, 5), name='glorot')
    calls = []
    real = devmod.DeviceSubtraction.stamps

    def spy(self, ra, dec, sci_, ref_, **kw):
        out = real(self, ra, dec, sci_, ref_, **kw)
        calls.append(dict(ra=np.array(ra), dec=np.array(dec), sci=sci_, new=out[0][:, 1]))
        return out
    monkeypatch.setattr(devmod.DeviceSubtraction, 'stamps', spy)
    peak = 0.25 * 3000.0 * float(R['model'].data.max())           # a quarter of the least a fake's brightest pixel can hold ...
    assert peak > 10 * 5.0                                         # ... is far above the frame's noise of 5

    def shows_the_fakes(call, got):
        assert call['sci'] is not sci['img']
        added = (call['sci'] - sci['img']).cpu().numpy()
        iy, ix = np.floor(table['y'] + 0.5).astype(int), np.floor(table['x'] + 0.5).astype(int)
        assert (added[iy, ix] > peak).all()
        new = call['new'].cpu().numpy() if hasattr(call['new'], 'cpu') else np.asarray(call['new'])
        assert got['recovered'].all()                            # as without a model: every score is far above the cut
        for f in got:
            d = np.hypot((call['ra'] - f['ra']) * np.cos(np.deg2rad(f['dec'])), call['dec'] - f['dec']) * 3600.0
            k = int(np.argmin(d))
            assert d[k] < 2.5, (f['id'], d[k])                    # (MATCH_RADIUS of 2 px at about 1 arcsec per px)
            c = size // 2
            assert new[k, c - 3:c + 4, c - 3:c + 4].max() - np.median(new[k]) > peak, f['id']

    ch = devmod.DeviceSubtraction(sci['wcs'], ref['wcs'], engine=engine)
    try:
        got, cat, _ = fakes().recover_dev(ch, sci['img'], sci['rms'], sci['mask'], sci['wgt'], ref['img'], ref['rms'], ref['mask'],
                                          2.4, table, R['model'], run_kws=dict(R['kw'], ref_flxscale=1.0),
                                          candidate_kws=dict(wcs=sci['wcs'], rb_model=model, rb_cut=0.01, sci=sci['img'],
                                                             ref=ref['img']))
    finally:
        engine.set_stream(0)
    assert len(calls) == 1 and (cat['rb'][cat['GOODCUT'] == 1] > 0.01).all()
    shows_the_fakes(calls[0], got)
    # the pool's job: the real run's stamps come from the caller's frame, the fake run's from the frame with the fakes
    del calls[:]
    spec = dict(psf=R['model'], zp=R['zp'], N=30, MAG_MIN=20.0, MAG_MAX=20.0, SEED=11, MIN_SEP=15.0, BORDER=40.0)
    pool = nm.SubtractionPool(1)
    out = pool.map([nm.SubtractionJob(sci, ref, radec=R['radec'], tag=0, detect=True, rb_model=model, rb_cut=0.01, fakes=spec,
                                      **R['kw'])])[0]
    pool.close()
    assert 'error' not in out and 'fakes_error' not in out and len(calls) == 2 and calls[0]['sci'] is sci['img']
    added = (calls[1]['sci'] - sci['img']).cpu().numpy()
    t = out['fakes']
    assert calls[1]['sci'] is not sci['img']
    assert (added[np.floor(t['y'] + 0.5).astype(int), np.floor(t['x'] + 0.5).astype(int)] > peak).all()
