"""The numpy restatement of the source extractor (tests/extract_ref.py) against things that are not ours (CPU)."""
import numpy as np
import pytest
from scipy import ndimage

import extract_ref as xr
from util import synth


def same_partition(a, b):
    """Two label images name the same components (up to renumbering); a: -1 = background, b: 0 = background."""
    if not np.array_equal(a >= 0, b > 0):
        return False
    m = a >= 0
    pairs = np.unique(np.stack([a[m], b[m]]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


@pytest.mark.parametrize('density', [0.02, 0.2, 0.4, 0.5, 0.6, 0.9])
@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (64, 96), (129, 257)])
def test_labels_equal_scipy_up_to_renumbering(density, shape):
    rng = np.random.default_rng(int(density * 100) + shape[0])
    fg = rng.uniform(size=shape) < density
    lab = xr.label8(fg)
    ref, n = ndimage.label(fg, structure=np.ones((3, 3)))
    assert same_partition(lab, ref)
    # the identity of a component is its smallest linear index
    flat = lab.ravel()
    for r in np.unique(flat[flat >= 0]):
        assert np.flatnonzero(flat == r)[0] == r


def test_diagonal_only_contacts_are_connected():
    fg = np.zeros((6, 6), bool)
    fg[0, 0] = fg[1, 1] = fg[2, 2] = fg[3, 1] = True        # touches by corners only
    fg[5, 5] = True
    lab = xr.label8(fg)
    assert len(np.unique(lab[lab >= 0])) == 2
    ref4, n4 = ndimage.label(fg)                            # 4-connectivity would see five
    assert n4 == 5
    anti = np.zeros((4, 4), bool)
    anti[0, 3] = anti[1, 2] = anti[2, 1] = anti[3, 0] = True
    assert len(np.unique(xr.label8(anti)[anti])) == 1


def gaussian(nx, ny, xc, yc, s, amp):
    y, x = np.mgrid[:ny, :nx]
    return (amp * np.exp(-0.5 * ((x - xc) ** 2 + (y - yc) ** 2) / s ** 2)).astype(np.float32)


@pytest.mark.parametrize('centre', [(40.0, 37.0), (40.5, 37.5), (40.3, 36.8)])
def test_noise_free_gaussian_star(centre):
    """A Gaussian of sigma s sampled at pixel centres, filtered by default.conv, cut at t = 1.5.  Every bound below is
    computed from the star's own samples outside the isophote (its tail), not chosen:

    * Over the whole plane the filtered samples F have first moment = the centre and variance s^2 + 1 / 2 per axis (a
      sampled Gaussian of this width has the continuous moments to exp(-2 pi^2 s^2) ~ 1e-41; a convolution adds the
      kernel's variance, 1 / 2, exactly).  F is made here by scipy in float64, not by the restatement.
    * The object is M = {F > t}.  Its sums are the whole-plane sums minus the tail's, so
      |barycentre - centre| <= sum_tail F |p - c| / sum_M F,
      (V - sum_tail F dx^2 / S) - shift^2 <= x2 <= V S / sum_M F   with V = s^2 + 1 / 2, S = sum_all F,
      |xy| <= sum_tail F |dx dy| / sum_M F + shift^2;  A^2 + B^2 = x2 + y2 and A^2 - B^2 <= |x2 - y2| + 2 |xy|.
    * FLUX_ISO = 2 pi s^2 amp - sum_tail img, to the float32 rounding of the samples (2^-23 relative).
    * FWHM_IMAGE: the level is half the sampled peak, so FWHM = 2 sqrt(n / pi) with n the lattice points inside the
      half-maximum contour of radius rho; n lies between pi (rho - 1 / sqrt2)^2 and pi (rho + 1 / sqrt2)^2 (every unit
      square that meets the circle is within half a diagonal of it), so |FWHM - 2 rho| <= sqrt2.  rho comes from the
      Gaussian of variance s^2 + 1 / 2 through the sampled peak; that the filtered profile is that Gaussian is the one
      approximation here (its relative error at half maximum is of the order 1 / (8 s^4) ~ 0.5 %, far inside sqrt2).
    The moments themselves are pinned to rounding against np.cov / eigvalsh on the member pixels."""
    xc, yc = centre
    s, amp, nx, ny = 2.2, 4000.0, 81, 75
    img = gaussian(nx, ny, xc, yc, s, amp)
    sigma = np.full((ny, nx), 1.0, np.float32)
    res = xr.extract(img, sigma)
    tab = res['table']
    assert len(tab) == 1
    r = tab[0]
    F = ndimage.convolve(img.astype(np.float64), np.array(xr.KERNEL, np.float64) / 16.0, mode='constant')
    assert np.abs(F - res['filtered']).max() <= 2.0 ** -22 * F.max()          # the float32 filter against float64
    M = F > 1.5
    assert np.array_equal(M, res['segm'] == 1)
    yy, xx = np.mgrid[:ny, :nx]
    dx, dy = xx - xc, yy - yc
    S, SM, tail = F.sum(), F[M].sum(), ~M
    V = s * s + 0.5
    # the premise, checked; what is left is the float32 rounding of the samples (2^-24 each), carried into the bounds
    Vx, Vy = (F * dx * dx).sum() / S, (F * dy * dy).sum() / S
    off = np.hypot((F * dx).sum(), (F * dy).sum()) / S
    assert abs(Vx - V) < 2.0 ** -23 * dx.max() ** 2 and abs(Vy - V) < 2.0 ** -23 * dy.max() ** 2 and off < 2.0 ** -23 * dx.max()
    shift = (F[tail] * np.hypot(dx, dy)[tail]).sum() / SM + off * S / SM
    assert np.hypot(r['X_IMAGE'] - (xc + 1), r['Y_IMAGE'] - (yc + 1)) <= shift + 1e-12
    lo = [W - (F[tail] * d[tail] ** 2).sum() / S - shift ** 2 for W, d in ((Vx, dx), (Vy, dy))]
    hi = max(Vx, Vy) * S / SM
    xybound = ((F[tail] * np.abs(dx * dy)[tail]).sum() + abs((F * dx * dy).sum())) / SM + shift ** 2
    a2, b2 = r['A_IMAGE'] ** 2, r['B_IMAGE'] ** 2
    assert lo[0] + lo[1] - 1e-12 <= a2 + b2 <= 2 * hi + 1e-12
    assert a2 - b2 <= max(hi - lo[0], hi - lo[1]) + 2 * xybound + 1e-12        # round: THETA carries no information
    # moments of the member pixels, computed here without the restatement's code path
    mm = res['segm'] == 1
    my_, mx_ = np.nonzero(mm)
    v = res['filtered'][mm].astype(np.float64)
    cx, cy = (v * mx_).sum() / v.sum(), (v * my_).sum() / v.sum()
    cov = np.cov(np.stack([mx_ - cx, my_ - cy]), aweights=v, bias=True)
    np.testing.assert_allclose([b2, a2], np.sort(np.linalg.eigvalsh(cov)), rtol=1e-10)
    total = 2 * np.pi * s * s * amp
    want = total - img[tail].astype(np.float64).sum()
    assert abs(r['FLUX_ISO'] - want) <= 2.0 ** -23 * total
    rho = np.sqrt(2 * V * np.log(2 * (amp * s * s / V) / F.max()))
    assert abs(r['FWHM_IMAGE'] - 2 * rho) <= np.sqrt(2.0)
    assert r['FLAGS'] == 0 and r['FLAGS_WEIGHT'] == 0 and r['IMAFLAGS_ISO'] == 0


@pytest.mark.parametrize('angle', [0.0, 30.0, 75.0, 120.0])
def test_moments_do_not_depend_on_the_position_angle(angle):
    """An elliptical Gaussian (axes 3.0 and 1.6 px) turned by ``angle``: A, B stay, THETA follows the angle."""
    nx = ny = 101
    y, x = np.mgrid[:ny, :nx] - 50.0
    t = np.deg2rad(angle)
    u, w = x * np.cos(t) + y * np.sin(t), -x * np.sin(t) + y * np.cos(t)
    img = (5000.0 * np.exp(-0.5 * (u * u / 9.0 + w * w / 2.56))).astype(np.float32)
    r = xr.extract(img, np.ones_like(img))['table']
    assert len(r) == 1
    # filter adds 1/2 to both variances; truncation at 1.5 / ~4000 takes off a few 1e-3
    assert abs(r['A_IMAGE'][0] ** 2 - 9.5) < 0.1 and abs(r['B_IMAGE'][0] ** 2 - 3.06) < 0.05
    d = (r['THETA_IMAGE'][0] - angle + 90.0) % 180.0 - 90.0
    assert abs(d) < 0.2


def test_one_pixel_wide_line_gets_the_twelfth():
    img = np.zeros((9, 30), np.float32)
    img[4, 5:25] = 100.0
    r = xr.extract(img, np.ones_like(img), use_filter=False)['table']
    assert len(r) == 1 and r['ISOAREA_IMAGE'][0] == 20
    # y2 = 0 exactly -> x2 y2 - xy^2 < 0.00694 -> both moments get 1 / 12: B^2 = 1 / 12, A^2 = (20^2 - 1) / 12 + 1 / 12
    np.testing.assert_allclose(r['B_IMAGE'][0] ** 2, 1.0 / 12.0, rtol=1e-12)
    np.testing.assert_allclose(r['A_IMAGE'][0] ** 2, 400.0 / 12.0, rtol=1e-12)
    # a fat source does not
    img[3:6, 5:25] = 100.0
    r = xr.extract(img, np.ones_like(img), use_filter=False)['table']
    np.testing.assert_allclose(r['B_IMAGE'][0] ** 2, 8.0 / 12.0, rtol=1e-12)


def star_field(nx=400, ny=360, seed=77, nstars=40, noise=3.0, fwhm=2.4):
    rng = np.random.default_rng(seed)
    img = rng.normal(0.0, noise, (ny, nx))
    x, y = rng.uniform(10, nx - 10, nstars), rng.uniform(10, ny - 10, nstars)
    flux = 10 ** rng.uniform(np.log10(300.0), np.log10(3e4), nstars)
    synth().add_stars(img, x, y, flux, fwhm)
    return img.astype(np.float32), np.full((ny, nx), noise, np.float32), x, y, flux


def test_star_field_is_recovered_without_noise_objects():
    img, sigma, x, y, flux = star_field()
    tab = xr.extract(img, sigma)['table']
    d = np.hypot(tab['X_IMAGE'][:, None] - 1 - x[None, :], tab['Y_IMAGE'][:, None] - 1 - y[None, :])
    assert (d.min(axis=1) < 2.0).all()                       # every object sits on a star: no noise-only object
    found = (d.min(axis=0) < 1.5).sum()
    assert found >= 39                                       # one close pair merges: there is no deblending
    assert (np.diff(tab['NUMBER']) == 1).all() and tab['NUMBER'][0] == 1


def test_bad_pixels_flags_and_saturation():
    img, sigma, x, y, flux = star_field(seed=5)
    bad = np.zeros(img.shape, np.uint8)
    flag = np.zeros(img.shape, np.int32)
    k = int(np.argmax(flux))
    xi, yi = int(round(x[k])), int(round(y[k]))
    img[yi, xi] = 60000.0
    flag[yi, xi + 1] = 2
    k2 = int(np.argsort(flux)[-2])
    bad[int(round(y[k2])) + 2, int(round(x[k2]))] = 1
    img[10, 10] = np.nan
    sigma[20, 20] = 0.0
    res = xr.extract(img, sigma, bad, flag)
    assert res['bad'][10, 10] and res['bad'][20, 20] and not res['fg'][res['bad']].any()
    tab = res['table']
    i = np.argmin(np.hypot(tab['X_IMAGE'] - 1 - x[k], tab['Y_IMAGE'] - 1 - y[k]))
    assert tab['FLAGS'][i] & 4 and tab['IMAFLAGS_ISO'][i] == 2
    j = np.argmin(np.hypot(tab['X_IMAGE'] - 1 - x[k2], tab['Y_IMAGE'] - 1 - y[k2]))
    assert tab['FLAGS_WEIGHT'][j] == 1 and tab['FLAGS'][j] & 16
    clean = (tab['FLAGS'] == 0) & (tab['FLAGS_WEIGHT'] == 0)
    assert clean.sum() >= len(tab) - 6


def test_reversed_summation_moves_only_the_last_bits():
    img, sigma, *_ = star_field(seed=9)
    a = xr.extract(img, sigma)['table']
    b = xr.extract(img, sigma, reverse=True)['table']
    for c in xr.INT_COLUMNS:
        assert np.array_equal(a[c], b[c])
    bounds = xr.order_bounds(a, b)
    for c in ('X_IMAGE', 'Y_IMAGE', 'FLUX_ISO', 'A_IMAGE', 'B_IMAGE'):
        assert bounds[c] < 1e-9 * max(1.0, np.abs(a[c]).max())
