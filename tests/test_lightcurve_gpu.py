"""The footprint join and the batched forced photometry (csrc/lightcurve.hip) on an MI355X, against the restatement of
tests/lightcurve_ref.py.

Membership is compared exactly, every pair: every scene keeps its sources 1e-3 arcsec clear of every edge
(``lr.assert_clear``; float64 rounding is some 1e-10 arcsec).  Sums: ``flux``, ``fluxerr`` and ``flags`` equal
``zm_aperture_photometry_dev`` at the batch's own ``x``, ``y`` bit for bit, and lie within the bounds of
tests/aperture_ref.py (``sums_bounds``: ``generic_limit`` / ``tangent_limit`` per pixel fraction plus the roundings of the
sum) of the independent aperture reference there; no row is left out unless its restated sum is not finite, which on
these scenes happens only where a test plants a NaN pixel.

Positions: ``x``, ``y`` against ``oracle/wcs.py`` within ``lr.POS_TOL_PX`` = 2^-31 = 4.66e-10 px.  Where it comes from:
tests/measure_lightcurve_tolerance.py measures, on exactly the joined pairs of these scenes, the host's ``zm_wcs_sky2pix``
and the float64 oracle against a 50-digit evaluation: 9.877e-11 px at worst (the frame across RA 0; 2.2e-11 .. 3.7e-11
elsewhere); 4 x that = 3.95e-10, rounded up to a power of two.  (tests/test_abi.py grants the host's round trip 1e-7 px.)
"""
import ctypes as C

import numpy as np
import pytest

import aperture_ref as ar
import lightcurve_ref as lr
from util import pkg, to_oracle_wcs

pytestmark = pytest.mark.gpu


def lc():
    return pkg().lightcurve


def as_images(ws, planes):
    return [dict(img=p[0], rms=p[1], mask=p[2], wcs=w) for w, p in zip(ws, planes)]


def held_to_reference(table, ows, planes, ra, dec, what, may_be_nan=False):
    """Every row of a batch table against the restatement: membership exact, positions within POS_TOL_PX of the oracle,
    flags exact, flux and variance within aperture_ref's bounds at the batch's own positions."""
    off, idx = lr.membership(ows, ra, dec)
    assert np.array_equal(table['offsets'], off) and np.array_equal(table['source'], idx), what
    assert np.array_equal(table['image'], np.repeat(np.arange(len(ows)), np.diff(off))), what
    pos = lr.photometry(ows, planes, ra, dec, off, idx)
    dx, dy = np.abs(table['x'] - pos['x']), np.abs(table['y'] - pos['y'])
    ref = lr.photometry(ows, planes, ra, dec, off, idx, xy=(table['x'], table['y']))
    bf, bv = ar.sums_bounds(ref['terms'])
    fin, efin = np.isfinite(ref['flux']), np.isfinite(ref['fluxerr'])
    df = np.abs(table['flux'] - ref['flux'])[fin]
    dv = np.abs(table['fluxerr'] ** 2 - ref['fluxerr'] ** 2)[efin]
    print(f'\n{what}: {idx.size} pairs; worst |x - oracle| {dx.max(initial=0):.3e}, |y - oracle| {dy.max(initial=0):.3e} px '
          f'(bound {lr.POS_TOL_PX:.3e}); worst flux - ref {df.max(initial=0):.3e} (ratio to its bound '
          f'{np.max(df / np.maximum(bf[fin], 1e-300), initial=0):.3f}), worst var - ref {dv.max(initial=0):.3e} (ratio '
          f'{np.max(dv / np.maximum(bv[efin], 1e-300), initial=0):.3f}); {int((~fin).sum())} rows with a restated sum that is not finite')
    assert (dx <= lr.POS_TOL_PX).all() and (dy <= lr.POS_TOL_PX).all(), what
    assert np.array_equal(table['flags'], ref['flags']), what
    assert np.array_equal(np.isfinite(table['flux']), fin) and np.array_equal(np.isfinite(table['fluxerr']), efin), what
    assert may_be_nan or (fin.all() and efin.all()), what
    assert (df <= bf[fin]).all() and (dv <= bv[efin]).all(), what
    return off, idx, ref


def per_image_kernel(engine, planes, table):
    """``zm_aperture_photometry_dev`` per image at the table's own positions: (flux, err, flags) per pair."""
    import torch
    n = table['source'].size
    flux, err, flags = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
    off = table['offsets']
    for k, (img, rms, mask) in enumerate(planes):
        a, b = int(off[k]), int(off[k + 1])
        if a == b:
            continue
        ny, nx = img.shape
        d = [None if p is None else torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in (img, rms, mask)]
        x, y = (torch.from_numpy(np.ascontiguousarray(table[c][a:b])).cuda() for c in ('x', 'y'))
        f, e = torch.empty(b - a, dtype=torch.float64, device='cuda'), torch.empty(b - a, dtype=torch.float64, device='cuda')
        fl = torch.empty(b - a, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        pkg()._lib.check(engine.L.zm_aperture_photometry_dev(
            engine.ctx, d[0].data_ptr(), d[1].data_ptr() if d[1] is not None else None,
            d[2].data_ptr() if d[2] is not None else None, nx, ny, b - a, x.data_ptr(), y.data_ptr(), lr.RADIUS, f.data_ptr(),
            e.data_ptr(), fl.data_ptr()), 'zm_aperture_photometry_dev')
        engine.synchronize()
        flux[a:b], err[a:b], flags[a:b] = f.cpu().numpy(), e.cpu().numpy(), fl.cpu().numpy()
    return flux, err, flags


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ('offsets', 'image', 'source', 'x', 'y', 'flux',
                                                                                   'fluxerr', 'flags'))


def test_counts_of_zero_one_and_two(engine):
    w, ow, ra, dec, _ = lr.frame_scene('tpv')
    inside, outside = ow.pix2sky(np.array([40.0]), np.array([30.0])), ow.pix2sky(np.array([140.0]), np.array([30.0]))
    ra2, dec2 = np.array([outside[0][0], inside[0][0]]), np.array([outside[1][0], inside[1][0]])
    far = lr.frame_wcs('negdet')
    far = type(far)(far.crpix, (200.0, -40.0), far.cd, None, None, far.naxis)
    e0 = np.zeros(0)
    for wcss, a, d, want_off, want_idx in (([], e0, e0, [0], []), ([], ra2, dec2, [0], []), ([w], e0, e0, [0, 0], []),
                                           ([w], ra2[1:], dec2[1:], [0, 1], [0]), ([w], ra2[:1], dec2[:1], [0, 0], []),
                                           ([w], ra2, dec2, [0, 1], [1]), ([w, w], ra2, dec2, [0, 1, 2], [1, 1]),
                                           ([far, w], ra2, dec2, [0, 0, 1], [1]), ([w, far], ra2, dec2, [0, 1, 1], [1])):
        off, idx = lc().footprint_join(wcss, a, d, engine=engine)
        assert off.dtype == np.int64 and idx.dtype == np.int32
        assert off.tolist() == want_off and idx.tolist() == want_idx, (len(wcss), a.size)
        r_off, r_idx = lr.membership([to_oracle_wcs(v) for v in wcss], a, d)
        assert r_off.tolist() == want_off and r_idx.tolist() == want_idx
    planes = lr.make_planes(96, 80, 3)
    for imgs, a, d, n in (([], ra2, dec2, 0), (as_images([w], [planes]), e0, e0, 0), (as_images([w], [planes]), ra2, dec2, 1),
                          (as_images([w, w], [planes, planes]), ra2, dec2, 2)):
        t = lc().forced_photometry_batch(imgs, a, d, engine=engine)
        assert t['source'].size == n == t['flux'].size == t['x'].size and t['offsets'].size == len(imgs) + 1
    assert abs(t['x'][0] - 39.0) < 1e-6 and abs(t['y'][0] - 29.0) < 1e-6 and t['flux'][0] == t['flux'][1]


@pytest.mark.parametrize('name', lr.FRAMES)
def test_frames_membership_positions_and_sums(engine, name):
    """Sources 1.5 px inside and outside along each edge and beside each corner, 0.25 px inside (clipped boxes), and
    random ones: both signs of det(CD), a rotation, TPV, RA 0 inside the frame, a pole inside the frame."""
    w, ow, ra, dec, known = lr.frame_scene(name)
    lr.assert_clear([ow], ra, dec)
    off, idx = lc().footprint_join([w], ra, dec, engine=engine)
    assert np.array_equal(idx, np.flatnonzero(known)) and off.tolist() == [0, idx.size]
    assert (np.diff(idx) > 0).all()
    planes = lr.make_planes(*ow.naxis, seed=31)
    t = lc().forced_photometry_batch(as_images([w], [planes]), ra, dec, engine=engine)
    _, _, ref = held_to_reference(t, [ow], [planes], ra, dec, name)
    assert (ref['terms'][4] < 49).sum() >= 12 and (ref['terms'][4] == 49).any()          # clipped boxes and whole ones
    f, e, fl = per_image_kernel(engine, [planes], t)
    assert f.tobytes() == t['flux'].tobytes() and e.tobytes() == t['fluxerr'].tobytes() and fl.tobytes() == t['flags'].tobytes()


@pytest.mark.parametrize('n', [63, 64, 65, 300])
def test_wave_boundaries_of_the_compaction(engine, n):
    w, ow, ra, dec = lr.count_scene(n)
    lr.assert_clear([ow], ra, dec)
    off, idx = lc().footprint_join([w], ra, dec, engine=engine)
    r_off, r_idx = lr.membership([ow], ra, dec)
    assert off.tolist() == [0, n] == r_off.tolist()
    assert (np.diff(idx) > 0).all() and np.array_equal(idx, r_idx)
    planes = lr.make_planes(96, 80, seed=n)
    t = lc().forced_photometry_batch(as_images([w], [planes]), ra, dec, engine=engine)
    held_to_reference(t, [ow], [planes], ra, dec, f'{n} inside')


@pytest.mark.parametrize('copies, nsrc', [(1, 30000), (52, 110000)])
def test_the_scan_across_its_blocks_and_a_capacity_that_has_to_grow(engine, copies, nsrc):
    """3 and 156 images against 3e4 and 1.1e5 sources: 1 416 and 268 320 wave counts - more than one block of the scan
    (1024 each) and, at 156 images, more than the 256 block totals one pass of its top level takes, with more pairs than
    the first capacity the Python layer tries.  The join alone, exact against the restatement."""
    ws, ows, planes, _, _ = lr.batch_scene()
    rng = np.random.default_rng(nsrc)
    ra, dec = ows[0].pix2sky(rng.uniform(-40.0, 136.0, nsrc), rng.uniform(-30.0, 110.0, nsrc))
    clear = (lr.edge_distance_arcsec(ows, ra, dec) >= lr.EDGE_BAND_ARCSEC).all(axis=0)      # the condition on a scene, enforced
    ra, dec = ra[clear], dec[clear]
    assert nsrc - 40 < ra.size
    r_off, r_idx = lr.membership(ows, ra, dec)
    lists = [r_idx[r_off[k]:r_off[k + 1]] for k in range(3)] * copies
    want_off = np.concatenate([[0], np.cumsum([v.size for v in lists])])
    nwave = 4 * ((ra.size + 255) // 256)
    assert 3 * copies * nwave > (1024 if copies == 1 else 1024 * 256) and (copies == 1 or want_off[-1] > max(ra.size, 1024))
    off, idx = lc().footprint_join(ws * copies, ra, dec, engine=engine)
    assert np.array_equal(off, want_off) and np.array_equal(idx, np.concatenate(lists))


def test_three_images_of_different_sizes_in_one_batch(engine):
    """96 x 80 with all planes, 130 x 70 without rms, 71 x 37 without a mask: the pointer table and the strides.  Bit for
    bit against the per-image kernel, within bounds of the independent reference, and the same bytes on a second run."""
    ws, ows, planes, ra, dec = lr.batch_scene()
    lr.assert_clear(ows, ra, dec)
    t = lc().forced_photometry_batch(as_images(ws, planes), ra, dec, engine=engine)
    off, idx, ref = held_to_reference(t, ows, planes, ra, dec, 'batch of three')
    assert (np.diff(off) > 10).all()
    for k in range(3):
        assert (np.diff(idx[off[k]:off[k + 1]]) > 0).all()
    assert not t['fluxerr'][off[1]:off[2]].any() and t['fluxerr'][:off[1]].all() and t['fluxerr'][off[2]:].all()
    assert not t['flags'][off[2]:].any() and t['flags'][:off[2]].any()
    f, e, fl = per_image_kernel(engine, planes, t)
    assert f.tobytes() == t['flux'].tobytes() and e.tobytes() == t['fluxerr'].tobytes() and fl.tobytes() == t['flags'].tobytes()
    again = lc().forced_photometry_batch(as_images(ws, planes), ra, dec, engine=engine)
    assert same_bytes(t, again)
    j1 = lc().footprint_join(ws, ra, dec, engine=engine)
    j2 = lc().footprint_join(ws, ra, dec, engine=engine)
    assert j1[0].tobytes() == j2[0].tobytes() == off.tobytes() and j1[1].tobytes() == j2[1].tobytes() == idx.tobytes()
    # the order of the images is the order of the rows
    back = lc().forced_photometry_batch(as_images(ws[::-1], planes[::-1]), ra, dec, engine=engine)
    a, b = int(back['offsets'][2]), int(back['offsets'][3])
    assert back['flux'][a:b].tobytes() == t['flux'][:off[1]].tobytes() and np.array_equal(back['source'][a:b], idx[:off[1]])


def test_done_pairs_are_left_out(engine):
    ws, ows, planes, ra, dec = lr.batch_scene()
    full = lc().forced_photometry_batch(as_images(ws, planes), ra, dec, engine=engine)
    pairs = list(zip(full['image'].tolist(), full['source'].tolist()))
    done = set(pairs[::3]) | {(0, 10 ** 6), (2, int(full['source'][0]))}
    rest = lc().forced_photometry_batch(as_images(ws, planes), ra, dec, done=done, engine=engine)
    keep = np.array([p not in done for p in pairs])
    assert keep.sum() < len(pairs) and list(zip(rest['image'].tolist(), rest['source'].tolist())) == [p for p in pairs if p not in done]
    for c in ('x', 'y', 'flux', 'fluxerr', 'flags'):
        assert rest[c].tobytes() == full[c][keep].tobytes(), c
    none = lc().forced_photometry_batch(as_images(ws, planes), ra, dec, done=set(pairs), engine=engine)
    assert none['source'].size == 0 and none['offsets'].tolist() == [0, 0, 0, 0]


def test_a_position_that_is_not_finite_joins_nothing(engine):
    w, ow, ra, dec, known = lr.frame_scene('posdet')
    inside = np.flatnonzero(known)
    ra, dec = ra.copy(), dec.copy()
    ra[inside[0]], dec[inside[1]], ra[inside[2]], dec[inside[3]] = np.nan, np.inf, -np.inf, np.nan
    off, idx = lc().footprint_join([w], ra, dec, engine=engine)
    assert np.array_equal(idx, inside[4:]) and off.tolist() == [0, inside.size - 4]
    assert np.array_equal(lr.membership([ow], ra, dec)[1], idx)


def test_a_nan_pixel_in_a_box_gives_nan_flux(engine):
    w, ow, ra, dec, known = lr.frame_scene('negdet')
    img, rms, mask = lr.make_planes(96, 80, seed=2)
    off, idx = lr.membership([ow], ra, dec)
    x, y = ow.sky2pix(ra[idx], dec[idx])
    k = int(np.argmin(np.hypot(x - 1.0 - 50.0, y - 1.0 - 40.0)))
    i, j = int(round(x[k] - 1.0)), int(round(y[k] - 1.0))
    img, rms = img.copy(), rms.copy()
    img[j + 3, i + 3] = np.nan                       # a corner of the 7 x 7 box, outside the circle: 0 * NaN = NaN
    rms[j, i] = np.inf
    t = lc().forced_photometry_batch(as_images([w], [(img, rms, mask)]), ra, dec, engine=engine)
    _, _, ref = held_to_reference(t, [ow], [(img, rms, mask)], ra, dec, 'NaN pixel', may_be_nan=True)
    assert np.isnan(t['flux'][k]) and not np.isfinite(t['fluxerr'][k])
    assert 1 <= (~np.isfinite(t['flux'])).sum() <= 4 and np.isfinite(t['flux']).sum() > 60


def test_capacity_one_short(engine):
    """The needed count comes back and nothing is written past the end (``zm_find_stars``'s contract); the offsets are
    complete either way."""
    import torch
    z = pkg()
    ws, ows, planes, ra, dec = lr.batch_scene()
    off, idx = lr.membership(ows, ra, dec)
    n = int(off[-1])
    arr = (z._lib.zm_wcs * 3)(*[z._lib.wcs_struct(w) for w in ws])
    for cap in (n - 1, 0, n):
        got_off = np.full(4, -1, np.int64)
        got = np.full(n + 8, -7, np.int32)
        cnt = C.c_int64(-1)
        z._lib.check(engine.L.zm_footprint_join(engine.ctx, 3, arr, ra.size, ra.ctypes.data, dec.ctypes.data, cap,
                                                got_off.ctypes.data, got.ctypes.data, C.byref(cnt)), 'zm_footprint_join')
        assert cnt.value == n and np.array_equal(got_off, off)
        assert np.array_equal(got[:cap], idx[:cap]) and (got[cap:] == -7).all()
    # the device form: a guard band behind the capacity stays as it was
    d_ra, d_dec = torch.from_numpy(ra).cuda(), torch.from_numpy(dec).cuda()
    d_off = torch.full((4,), -1, dtype=torch.int64, device='cuda')
    d_idx = torch.full((n + 64,), -7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    cnt = C.c_int64(-1)
    z._lib.check(engine.L.zm_footprint_join_dev(engine.ctx, 3, arr, ra.size, d_ra.data_ptr(), d_dec.data_ptr(), n - 1,
                                                d_off.data_ptr(), d_idx.data_ptr(), C.byref(cnt)), 'zm_footprint_join_dev')
    engine.synchronize()
    got = d_idx.cpu().numpy()
    assert cnt.value == n and np.array_equal(d_off.cpu().numpy(), off)
    assert np.array_equal(got[:n - 1], idx[:n - 1]) and (got[n - 1:] == -7).all()


def test_a_degenerate_footprint_is_an_error(engine):
    z = pkg()
    w = lr.frame_wcs('negdet')
    ra, dec = np.array([w.crval[0]]), np.array([w.crval[1]])
    flat = type(w)(w.crpix, w.crval, [w.cd[0, 0], 0.0, w.cd[0, 0], 0.0], None, None, w.naxis)      # singular CD
    line = type(w)(w.crpix, w.crval, w.cd, None, None, (96, 1))                                    # corners coincide in pairs
    for bad, word in ((flat, 'singular'), (line, 'degenerate')):
        with pytest.raises(z.ZMError, match=word):
            lc().footprint_join([w, bad], ra, dec, engine=engine)
    assert lc().footprint_join([w], ra, dec, engine=engine)[1].tolist() == [0]                     # the engine is fine after it


def test_object_layer_on_the_footprint(engine):
    """``Source.images`` / ``unphotometered_images`` and ``CalibratedImage.unphotometered_sources`` /
    ``force_photometry`` on objects: the footprint decides, and a point that exists is not asked for again."""
    z = pkg()
    ws, ows, planes, ra, dec = lr.batch_scene()
    off, idx = lr.membership(ows, ra, dec)
    images = []
    for k, (w, (img, rms, mask)) in enumerate(zip(ws, planes)):
        im = z.CalibratedImage()
        im.data = img
        im.header = dict(w.to_header(), NAXIS1=img.shape[1], NAXIS2=img.shape[0], MAGZP=26.0 + k, APCOR4=-0.05,
                         OBSJD=2458800.5 + k, FILTER='ZTF r')
        im.header_comments = {}
        im.basename = f'sub{k}.fits'
        rm, mk = z.FITSImage(), z.MaskImage()
        rm.data = rms if rms is not None else np.ones_like(img)
        mk.data = mask if mask is not None else np.zeros(img.shape, np.int32)
        im._rmsimg, im.mask_image = rm, mk
        images.append(im)
    sources = [z.Source(id=f's{k}', ra=float(a), dec=float(d)) for k, (a, d) in enumerate(zip(ra, dec))]
    on0 = idx[off[0]:off[1]].tolist()
    assert [s.id for s in images[0].unphotometered_sources(sources)] == [f's{k}' for k in on0]
    s = sources[int(np.intersect1d(idx[off[0]:off[1]], idx[off[1]:off[2]])[0])]
    holds = [k for k in range(3) if int(s.id[1:]) in idx[off[k]:off[k + 1]].tolist()]
    assert [im.basename for im in s.images(images)] == [f'sub{k}.fits' for k in holds] and len(holds) >= 2
    pts = s.force_photometry(images)
    assert [p.image.basename for p in pts] == [f'sub{k}.fits' for k in holds]
    t = lc().forced_photometry_batch(images, ra, dec, engine=engine)
    for p, k in zip(pts, holds):
        row = int(off[k]) + idx[off[k]:off[k + 1]].tolist().index(int(s.id[1:]))
        assert abs(p.flux - t['flux'][row]) <= 1e-9 * max(1.0, abs(p.flux))      # host sky2pix against the device's
        assert p.flags == t['flags'][row] and p.zp == 26.0 + k - 0.05 and p.obsjd == 2458800.5 + k and p.filtercode == 'zr'
        assert p.source is s and p.ra == s.ra
    s.forced_photometry.extend(pts[:1])
    images[holds[0]].forced_photometry.extend(pts[:1])
    assert [im.basename for im in s.unphotometered_images(images)] == [f'sub{k}.fits' for k in holds[1:]]
    assert s not in images[holds[0]].unphotometered_sources(sources) and s in images[holds[1]].unphotometered_sources(sources)
    assert len(s.light_curve) == 1 and s.light_curve['filter'].tolist() == ['ztfr']
