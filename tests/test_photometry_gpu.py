"""Forced aperture photometry against the oracle."""
import math
import os

import numpy as np
import pytest

from oracle import photometry as ophot
from util import pkg, synth

pytestmark = pytest.mark.gpu


def test_matches_oracle_including_edges(engine):
    rng = np.random.default_rng(1)
    ny, nx = 120, 150
    img = rng.normal(5, 2, (ny, nx)).astype(np.float32)
    rms = rng.uniform(1, 3, (ny, nx)).astype(np.float32)
    mask = (rng.uniform(size=(ny, nx)) < 0.02).astype(np.int32) * rng.choice([1, 256, 2048], (ny, nx))
    x = np.concatenate([rng.uniform(-5, nx + 5, 300), [0.0, nx - 1.0, 10.5, 40.0, -50.0]])
    y = np.concatenate([rng.uniform(-5, ny + 5, 300), [0.0, ny - 1.0, 20.5, 40.0, 10.0]])
    for r in (3.0, 1.2, 7.5):
        f, e, fl = engine.aperture_photometry(img, x, y, rms=rms, mask=mask, radius=r)
        rf, re, rfl = ophot.aperture_photometry(img, rms, mask, x, y, r)
        np.testing.assert_allclose(f, rf, rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(e, re, rtol=1e-10, atol=1e-9)
        assert np.array_equal(fl, rfl)            # integer work: bit exact


def test_constant_image_gives_the_circle_area(engine):
    img = np.full((64, 64), 2.0, np.float32)
    f, e, fl = engine.aperture_photometry(img, [31.3, 20.0], [30.7, 20.5], rms=np.ones_like(img))
    np.testing.assert_allclose(f, 2.0 * np.pi * 9.0, rtol=1e-12)
    np.testing.assert_allclose(e, np.sqrt(np.pi * 9.0), rtol=1e-12)
    assert not fl.any()


def test_object_api_on_a_subtraction_like_image(engine, tmp_path):
    z = pkg()
    s = synth()
    f = s.make_frame(200, 180, 5, s.ztf_wcs(200, 180), nstars=0, sky=0.0, noise=1.0, nbad=30)
    f['header'].update({'OBSJD': 2458000.5, 'FILTER': 'ZTF_g'})
    img = np.zeros((180, 200))
    s.add_stars(img, [100.3], [90.6], [5000.0], 2.0)
    p = str(tmp_path / 'sub.fits')
    z.fits.write(p, img.astype(np.float32), f['header'])
    z.fits.write(p.replace('.fits', '.rms.fits'), np.ones((180, 200), np.float32), f['header'])
    z.fits.write(p.replace('.fits', '.mask.fits'), f['mask'], f['header'])
    ra, dec = f['wcs'].all_pix2world([100.3], [90.6], 0)
    t = z.raw_aperture_photometry(p, p.replace('.fits', '.rms.fits'), p.replace('.fits', '.mask.fits'),
                                  ra, dec)
    assert set(['flux', 'fluxerr', 'flags', 'zp', 'obsjd', 'filtercode']) <= set(t.colnames)
    # a Gaussian of FWHM 2 px: 98.6 % of the flux falls within r = 3 px
    assert abs(t['flux'][0] / 5000.0 - (1 - np.exp(-0.5 * (3 / (2 / 2.3548)) ** 2))) < 2e-3
    assert abs(t['fluxerr'][0] - np.sqrt(np.pi * 9)) < 1e-6
    assert t['zp'][0] == f['header']['MAGZP'] + f['header']['APCOR4']
    assert t['filtercode'][0] == 'zg' and t['obsjd'][0] == 2458000.5
    im = z.ScienceImage.from_file(p)
    im.mask_image = z.MaskImage.from_file(p.replace('.fits', '.mask.fits'))
    t2 = z.aperture_photometry(im, ra, dec, assume_background_subtracted=True, apply_calibration=True)
    assert t2['flux'][0] == t['flux'][0] and np.isfinite(t2['mag'][0])


# ----------------------------------------------------------------------------------------------------------------
# Against tests/aperture_ref.py: a reference that shares no formula with the kernel or the oracle (its own accuracy is
# pinned to 50-digit arithmetic in tests/test_aperture_ref.py).  Limits: aperture_ref.generic_limit / tangent_limit,
# both taken from the CPU measurement of the closed form against that reference, never from the kernel's own figures.
import aperture_ref as ar        # noqa: E402

EPS = ar.EPS
IMPULSE_RADII = ar.RADII + (float(np.nextafter(7.5, 0)), 200.5 - 64 * EPS)


def impulse_offsets(r, rng):
    """Pixel - centre offsets for the impulse map: a lattice of centres across the pixel's whole neighbourhood
    (binary fractions: half-integers make an edge tangent or put a corner on the circle for the radii 0.5,
    sqrt(0.5), 3, 7.5), every ring pixel about special, hair-from-tangent and random centres, thinned to a few
    thousand with the pixels nearest to tangent kept."""
    if r <= 8:
        step = 0.0625 if r < 1 else (0.125 if r < 2 else (0.25 if r < 4 else 0.5))
        g = np.arange(-(math.ceil(r) + 1.5), math.ceil(r) + 1.5 + step / 2, step)
        lx, ly = (v.ravel() for v in np.meshgrid(g, g))
    else:                                                    # the ring only: eight directions, +-1 px in 1 / 8 steps
        g = np.arange(-1.0, 1.0 + 1e-9, 0.125)
        ang = np.arange(8) * (np.pi / 4) + 0.1
        m = [np.meshgrid(np.round(r * np.cos(a) * 8) / 8 + g, np.round(r * np.sin(a) * 8) / 8 + g) for a in ang]
        lx, ly = np.concatenate([v[0].ravel() for v in m]), np.concatenate([v[1].ravel() for v in m])
    centres = ar.SPECIAL_CENTRES + ar.TANGENT_CENTRES + [tuple(rng.uniform(-0.5, 0.5, 2)) for _ in range(6)]
    dx, dy = ar.ring_cases(r, centres, rng, nfill=40)
    if dx.size > 4000:
        e = np.abs(np.stack([dx - 0.5, dx + 0.5, dy - 0.5, dy + 0.5]))
        order = np.argsort(np.abs(r - e).min(axis=0))
        keep = np.concatenate([order[:1000], rng.choice(order[1000:], 3000, replace=False)])
        dx, dy = dx[keep], dy[keep]
    return np.concatenate([lx, dx]), np.concatenate([ly, dy])


@pytest.mark.parametrize('r', IMPULSE_RADII, ids=lambda r: f'r{r:.15g}')
def test_fraction_of_one_pixel_by_impulse(engine, r):
    """The image is 0 but for one pixel = 1, the rms plane likewise: flux[k] IS the kernel's fraction of that pixel
    for centre k, and err[k]^2 the same fraction.  Worst kernel - reference per radius: DESIGN.md, "Forced aperture
    photometry"."""
    rng = np.random.default_rng(int(r * 977))
    nx, ny, px, py = 71, 37, 33, 17
    img = np.zeros((ny, nx), np.float32)
    img[py, px] = 1.0
    dx, dy = impulse_offsets(r, rng)
    x, y = px - dx, py - dy
    f, e, fl = engine.aperture_photometry(img, x, y, rms=img, radius=r)
    edges = ar.pixel_edges(px, py, x, y)
    i0, i1, j0, j1, ok = ar.boxes(x, y, r, nx, ny)
    inbox = ok & (i0 <= px) & (px < i1) & (j0 <= py) & (py < j1)
    ref = np.where(inbox, ar.edges_fraction(*edges, r), 0.0)
    assert (ar.edges_fraction(*edges, r)[~inbox] == 0).all()       # the box rule leaves out no pixel the circle reaches
    tang = ar.edges_near_tangent(*edges, r)
    zero = ref == 0
    lim = np.where(tang & ~zero, ar.tangent_limit(r), ar.generic_limit(r))
    df, dv = np.abs(f - ref), np.abs(e * e - ref)
    gen = ~tang & ~zero
    print(f'\nimpulse r = {r!r}: {x.size} centres, {int(gen.sum())} generic, {int((tang & ~zero).sum())} near tangent, '
          f'{int(zero.sum())} where the reference is 0 ({int((f[zero] != 0).sum())} of them not 0 in the kernel, '
          f'min {f.min():.2e}); worst flux - ref: generic {df[gen].max(initial=0):.3e} = '
          f'{df[gen].max(initial=0) / (EPS * r * r):.1f} eps r^2 (limit {ar.generic_limit(r):.3e}), near tangent '
          f'{df[tang & ~zero].max(initial=0):.3e} (limit {ar.tangent_limit(r):.3e}), at 0 {df[zero].max(initial=0):.3e}; '
          f'worst err^2 - ref {dv.max():.3e}')
    assert gen.sum() > 300 and zero.sum() > 50 and ((ref == 1).sum() > 20 or r < 1)
    assert np.isfinite(f).all() and np.isfinite(e).all() and (e >= 0).all() and not fl.any()
    assert (df <= lim).all(), (x[np.argmax(df - lim)], y[np.argmax(df - lim)], df.max())
    assert (dv <= lim + 4 * EPS).all()          # sqrt and its square: two roundings of a value <= 1
    if r in (0.5, 3.0, 7.5):
        assert (tang & ~zero).sum() > 0          # exact tangency is among the lattice points


def edge_frame(nx, ny):
    """Impulses (powers of two: every product is exact) and one mask bit each at the corners and the mid-edges."""
    img = np.zeros((ny, nx), np.float32)
    mask = np.zeros((ny, nx), np.int32)
    spots = sorted({(j, i) for j in (0, ny // 2, ny - 1) for i in (0, nx // 2, nx - 1)} - ({(ny // 2, nx // 2)} if nx > 1 and ny > 1 else set()))
    for k, (j, i) in enumerate(spots):
        img[j, i] = 2.0 ** (k - 3)
        mask[j, i] = 1 << (3 * k + 1)
    return img, mask, spots


def held_to_reference(engine, img, rms, mask, x, y, r, what):
    """One launch against aperture_sums: flags exact, flux and variance within sum |img| * (fraction limit of each
    pixel's regime) + n eps sum |img * frac|; every position counts."""
    f, e, fl = engine.aperture_photometry(img, x, y, rms=rms, mask=mask, radius=r)
    rf, re, rfl, t = ar.aperture_sums(img, rms, mask, x, y, r, with_terms=True)
    bf, bv = ar.sums_bounds(t)
    fin, efin = np.isfinite(rf), np.isfinite(re)
    df, dv = np.abs(f - rf)[fin], np.abs(e * e - re * re)[efin]
    print(f'\n{what}, r = {r:g}: {len(f)} positions ({int((t[4] == 0).sum())} without a box); worst flux - ref '
          f'{df.max(initial=0):.3e} (largest bound {bf.max():.3e}, worst ratio {np.max(df / np.maximum(bf[fin], 1e-300), initial=0):.3f}); '
          f'worst var - ref {dv.max(initial=0):.3e} (worst ratio {np.max(dv / np.maximum(bv[efin], 1e-300), initial=0):.3f})')
    assert np.array_equal(fl, rfl), what
    assert np.array_equal(np.isfinite(f), fin) and np.array_equal(np.isfinite(e), efin), what
    assert (df <= bf[fin]).all() and (dv <= bv[efin]).all(), what
    empty = t[4] == 0
    assert not f[empty].any() and not e[empty].any() and not fl[empty].any(), what
    return (f, e, fl), (rf, re, rfl)


@pytest.mark.parametrize('shape', [(67, 41), (1, 41), (67, 1), (130, 3)])
def test_frame_edges_and_the_box_rule(engine, shape):
    """Apertures that slide off each corner and mid-edge, from inside to beyond r + 1 outside, in quarter-pixel steps:
    x - r + 0.5 is an integer on the way, on both sides.  Flags follow the box, not the circle, bit for bit."""
    nx, ny = shape
    img, mask, spots = edge_frame(nx, ny)
    rms = np.sqrt(img)
    for r in (0.5, 1.2, 2.5, 3.0):
        s = np.arange(-(r + 2.0), r + 2.0 + 0.125, 0.25)
        xs, ys = [], []
        for j, i in spots:
            xs += [i + s, np.full(s.size, i + 0.25), i + s]
            ys += [np.full(s.size, j - 0.25), j + s, j + s]
        x, y = np.concatenate(xs), np.concatenate(ys)
        _, (rf, re, rfl) = held_to_reference(engine, img, rms, mask, x, y, r, f'edges {nx}x{ny}')
        assert (rfl != 0).any() and (rfl == 0).any() and (rf != 0).any()
        # a flag without flux: a pixel of the box that the circle does not reach
        assert ((rfl != 0) & (rf == 0)).any() or r < 1


def test_positions_no_oracle_could_take(engine):
    """NaN, infinities, positions beyond int's range and the last ulp on either side of an empty box, between
    ordinary positions in one launch.  (The kernel clamps the box bounds as doubles before they become int.)"""
    rng = np.random.default_rng(8)
    nx, ny, r = 150, 120, 3.0
    img = rng.normal(5, 2, (ny, nx)).astype(np.float32)
    rms = rng.uniform(1, 3, (ny, nx)).astype(np.float32)
    mask = (1 << rng.integers(0, 31, (ny, nx))).astype(np.int32)          # every pixel flags: an empty box shows
    big = [np.nan, np.inf, -np.inf, 1e300, -1e300, 1e12, -1e12, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 + 1, 2.0 ** 31 - 1,
           -2.0 ** 31 + 1, -2.0 ** 31 - 1, 2.0 ** 63, -2.0 ** 63, 1.7e308, -1.7e308]
    hi, lo = nx - 1 + r + 0.5, -r - 0.5
    hiy = ny - 1 + r + 0.5
    brink = [hi, np.nextafter(hi, 0), np.nextafter(hi, 1e9), lo, np.nextafter(lo, 0), np.nextafter(lo, -1e9)]
    brinky = [hiy, np.nextafter(hiy, 0), np.nextafter(hiy, 1e9), lo, np.nextafter(lo, 0), np.nextafter(lo, -1e9)]
    ox = np.array(big + [40.0] * len(big) + big + brink + [60.5] * 6 + brink)
    oy = np.array([50.0] * len(big) + big + big[::-1] + [30.25] * 6 + brinky + brinky[::-1])
    nodd = ox.size
    gx, gy = rng.uniform(-2, nx + 2, nodd + 1), rng.uniform(-2, ny + 2, nodd + 1)
    gx[4], gy[4] = 70.3, 60.2
    gx[5], gy[5] = gx[4], gy[4]                                           # duplicates, adjacent and far apart
    gx[-1], gy[-1] = gx[0], gy[0]
    x, y = np.empty(2 * nodd + 1), np.empty(2 * nodd + 1)
    x[0::2], y[0::2], x[1::2], y[1::2] = gx, gy, ox, oy
    (f, e, fl), (rf, re, rfl) = held_to_reference(engine, img, rms, mask, x, y, r, 'odd positions')
    bad = ~(np.isfinite(x) & np.isfinite(y)) | (np.abs(x) > 1e6) | (np.abs(y) > 1e6)
    assert bad.sum() == 3 * len(big)
    assert not f[bad].any() and not e[bad].any() and not fl[bad].any()
    # the brink: one ulp inside has a box (a flag, whatever the flux), the exact value and one ulp outside have none
    k = 2 * (3 * len(big)) + 1
    assert [bool(v) for v in fl[k:k + 12:2]] == [False, True, False, False, True, False]
    # the ordinary neighbours, and the duplicates, to the bit
    g = engine.aperture_photometry(img, gx, gy, rms=rms, mask=mask, radius=r)
    for a, b in zip((f, e, fl), g):
        assert a[0::2].tobytes() == b.tobytes()
    assert (f[8], e[8], fl[8]) == (f[10], e[10], fl[10]) and (f[0], e[0], fl[0]) == (f[-1], e[-1], fl[-1])
    assert f[8] != 0


def test_optional_planes_counts_and_radius_limits(engine):
    z = pkg()
    rng = np.random.default_rng(12)
    nx, ny = 90, 70
    img = rng.normal(5, 2, (ny, nx)).astype(np.float32)
    rms = rng.uniform(1, 3, (ny, nx)).astype(np.float32)
    mask = ((rng.uniform(size=(ny, nx)) < 0.05) * (1 << rng.integers(0, 15, (ny, nx)))).astype(np.int32)
    ux, uy = rng.uniform(-4, nx + 4, 500), rng.uniform(-4, ny + 4, 500)
    (f, e, fl), _ = held_to_reference(engine, img, rms, mask, ux, uy, 3.0, 'all planes')
    # rms = None: err == 0; mask = None: flags == 0; the flux to the bit either way
    f1, e1, fl1 = engine.aperture_photometry(img, ux, uy, mask=mask)
    f2, e2, fl2 = engine.aperture_photometry(img, ux, uy, rms=rms)
    f3, e3, fl3 = engine.aperture_photometry(img, ux, uy)
    assert f1.tobytes() == f.tobytes() and f2.tobytes() == f.tobytes() and f3.tobytes() == f.tobytes()
    assert not e1.any() and not e3.any() and e2.tobytes() == e.tobytes()
    assert not fl2.any() and not fl3.any() and np.array_equal(fl1, fl) and fl.any()
    # bit 31 comes back as it went in; an int16 plane (widened by the engine: this entry point takes int32) gives
    # the flags of its sign-extended copy
    m31 = mask.copy()
    m31[::7, ::5] |= np.int32(-2 ** 31)
    g = engine.aperture_photometry(img, ux, uy, rms=rms, mask=m31)
    want = ar.aperture_sums(img, rms, m31, ux, uy, 3.0)[2]
    assert g[2].dtype == np.int32 and np.array_equal(g[2], want) and (g[2] < 0).any() and (g[2] >= 0).any()
    m16 = mask.astype(np.int16)
    m16[::9, ::4] |= np.int16(-2 ** 15)
    g16 = engine.aperture_photometry(img, ux, uy, rms=rms, mask=m16)
    g32 = engine.aperture_photometry(img, ux, uy, rms=rms, mask=m16.astype(np.int32))
    assert np.array_equal(g16[2], g32[2]) and np.array_equal(g16[2], ar.aperture_sums(img, None, m16, ux, uy, 3.0)[2])
    assert g16[0].tobytes() == f.tobytes() and (g16[2] < 0).any()
    # npos: 0, 1, the wave size and its neighbours, more than 65535 blocks
    for n in (0, 1, 63, 64, 65, 70000):
        a = engine.aperture_photometry(img, np.resize(ux, n), np.resize(uy, n), rms=rms, mask=mask)
        for got, one in zip(a, (f, e, fl)):
            assert got.shape == (n,) and got.tobytes() == np.resize(one, n).tobytes(), n
    # radii: (0, 512) open at both ends; NaN fails both comparisons
    for bad in (512.0, 0.0, -1.0, float('nan'), float('inf'), 1e300):
        with pytest.raises(z._lib.ZMError):
            engine.aperture_photometry(img, ux[:3], uy[:3], rms=rms, mask=mask, radius=bad)
    # 511.5 is accepted: an aperture that swallows the frame, one wave over all of it
    held_to_reference(engine, img, rms, mask, [40.0, 300.0], [30.0, -200.0], 511.5, 'r = 511.5')
    # ... and one wave over 3.6e5 and 1.05e6 pixels
    big = rng.normal(0, 1, (1030, 1040)).astype(np.float32)
    held_to_reference(engine, big, np.abs(big), None, [520.3, 100.0], [515.1, 900.7], 300.0, 'r = 300')
    held_to_reference(engine, big, np.abs(big), None, [519.7], [514.6], 511.5, 'r = 511.5, 1040 x 1030')
    # a circle inside one pixel
    (fs, es, _), _ = held_to_reference(engine, img, rms, mask, [20.0, 20.1, 33.19], [30.0, 29.9, 8.81], 0.3, 'r = 0.3')
    np.testing.assert_allclose(fs, np.pi * 0.09 * img[[30, 30, 9], [20, 20, 33]].astype(np.float64), rtol=1e-12)


@pytest.mark.parametrize('r', [1.2, 3.0, 7.5, 40.0])
def test_random_frames_at_depth(engine, r):
    """Noise, stars and bad-pixel masks; 2 000 positions, off-frame ones included; no position is left out."""
    rng = np.random.default_rng(21)
    nx, ny = 333, 250
    img = rng.normal(100.0, 5.0, (ny, nx))
    synth().add_stars(img, rng.uniform(0, nx, 150), rng.uniform(0, ny, 150), 10 ** rng.uniform(2.5, 5.5, 150), 2.4)
    img = img.astype(np.float32)
    rms = np.sqrt(np.maximum(img, 1.0)).astype(np.float32)
    mask = ((rng.uniform(size=(ny, nx)) < 0.01) * (1 << rng.integers(0, 31, (ny, nx)))).astype(np.int32)
    mask[100:104, 200:230] |= 1 << 20
    x = np.concatenate([rng.uniform(-r - 3, nx + r + 3, 1900), rng.integers(0, nx, 50) + 0.5, rng.integers(0, nx, 50)])
    y = np.concatenate([rng.uniform(-r - 3, ny + r + 3, 1900), rng.integers(0, ny, 50), rng.integers(0, ny, 50) + 0.5])
    (f, e, fl), (rf, re, rfl) = held_to_reference(engine, img, rms, mask, x, y, r, 'random frame')
    assert (rf == 0).sum() > 5 and (rfl != 0).sum() > 50


def test_nonfinite_pixels_under_an_aperture(engine):
    """DESIGN.md "Forced aperture photometry": the sums are products over the clipped box, so a pixel that is not
    finite makes the sum it enters non-finite wherever in the box it lies - also in a box pixel the circle does not
    reach, where the fraction is 0 (or the closed form's 1e-16) and 0 * NaN = NaN.  A NaN in one plane leaves the
    other plane's sum alone.  NaN is never turned into a number: the error of a NaN variance is NaN, not 0."""
    rng = np.random.default_rng(4)
    nx, ny, r = 64, 48, 3.0
    img = rng.normal(5, 2, (ny, nx)).astype(np.float32)
    rms = rng.uniform(1, 3, (ny, nx)).astype(np.float32)
    x, y = np.array([20.3, 40.0, 50.2]), np.array([20.6, 30.0, 10.1])
    clean = engine.aperture_photometry(img, x, y, rms=rms, radius=r)
    # position 0: NaN well inside the circle; position 1: NaN in the box's corner pixel (43, 33), outside the circle;
    # position 2 stays clean
    a = img.copy()
    a[21, 20] = np.nan
    a[33, 43] = np.nan
    assert ar.pixel_fraction(43 - 40.0, 33 - 30.0, r) == 0 and ar.boxes([40.0], [30.0], r, nx, ny)[1][0] == 44
    f, e, _ = engine.aperture_photometry(a, x, y, rms=rms, radius=r)
    assert np.isnan(f[0]) and np.isnan(f[1]) and f[2] == clean[0][2]
    assert e.tobytes() == clean[1].tobytes()
    rf, re, _ = ar.aperture_sums(a, rms, None, x, y, r)
    assert np.array_equal(np.isnan(rf), np.isnan(f)) and np.array_equal(np.isnan(re), np.isnan(e))
    # one pixel outside the box: nothing
    b = img.copy()
    b[34, 43] = b[33, 44] = b[26, 40] = np.nan
    f, e, _ = engine.aperture_photometry(b, x, y, rms=rms, radius=r)
    assert f.tobytes() == clean[0].tobytes()
    # NaN (and inf) in the rms plane only
    s = rms.copy()
    s[21, 20] = np.nan
    s[33, 43] = np.inf
    f, e, _ = engine.aperture_photometry(img, x, y, rms=s, radius=r)
    assert f.tobytes() == clean[0].tobytes()
    assert np.isnan(e[0]) and not np.isfinite(e[1]) and e[2] == clean[1][2]
    re = ar.aperture_sums(img, s, None, x, y, r)[1]
    assert np.isnan(re[0]) and np.isnan(re[1])
    # infinities in the image: not finite, whatever their sign and fraction
    c = img.copy()
    c[21, 20], c[20, 21], c[33, 43] = np.inf, -np.inf, np.inf
    f, e, _ = engine.aperture_photometry(c, x, y, rms=rms, radius=r)
    assert not np.isfinite(f[0]) and not np.isfinite(f[1]) and f[2] == clean[0][2]
    # the oracle follows the same rule
    of, oe, _ = ophot.aperture_photometry(a, s, None, x, y, r)
    assert np.isnan(of[0]) and np.isnan(of[1]) and np.isnan(oe[0]) and not np.isfinite(oe[1]) and np.isfinite(of[2])
