"""tests/measure_ref.py (the numpy restatement of the extractor's second pass) against things that are not it.

Analytic cases.  The restatement sums pixel-centre samples with hard (Kron) or exactly overlapped (window) edges; the
closed forms are integrals.  The tolerance is that pixel-sampling error and is measured here, not picked: every case
is evaluated a second time on a grid 9 x finer (the same scene, every length times 9, values over 81), and the case may
differ from its closed form by 2 x |coarse - fine|, plus 256 spacings of the value for the rounding of sums of a few
thousand float64 terms (the Gaussians' own sampling error is far below one spacing, so for them that term is what is
left).  The measured figures are printed.
"""
import numpy as np
import pytest

import extract_ref as xr
import measure_ref as mr

F = 9


def gaussian(nx, ny, xc, yc, s1, s2=None, theta=0.0, total=1.0):
    s2 = s1 if s2 is None else s2
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    c, s = np.cos(theta), np.sin(theta)
    u, v = (xx - xc) * c + (yy - yc) * s, -(xx - xc) * s + (yy - yc) * c
    return total * np.exp(-0.5 * (u * u / s1 ** 2 + v * v / s2 ** 2)) / (2.0 * np.pi * s1 * s2)


def fine(x):
    """A 0-based pixel coordinate on the grid F x finer."""
    return F * (x + 0.5) - 0.5


def coarse(xf):
    return (xf + 0.5) / F - 0.5


def both(nx, ny, xc, yc, s1, s2=None, theta=0.0):
    """The scene on the frame and on the F x finer frame (total 1 on both)."""
    return (gaussian(nx, ny, xc, yc, s1, s2, theta),
            gaussian(F * nx, F * ny, fine(xc), fine(yc), F * s1, None if s2 is None else F * s2, theta))


def planes(img):
    return img, np.ones_like(img), np.zeros(img.shape, bool)


def tol(a, b, value):
    return 2.0 * abs(a - b) + 256.0 * np.spacing(abs(value))


def row(xc, yc, x2, y2, xy=0.0, fwhm=0.0):
    a, b, th = mr.ellipse(x2, y2, xy, thin=False)
    return dict(xc=xc, yc=yc, x2=x2, y2=y2, xy=xy, fwhm=fwhm, a=a, b=b, theta=th)


def test_gaussian_takes_the_minimum_radius_and_its_flux_inside_it():
    s = 2.0
    c, f = both(64, 64, 31.3, 32.6, s)
    k1 = mr.kron(*planes(c), row(31.3, 32.6, s * s, s * s))
    k2 = mr.kron(*planes(f), row(fine(31.3), fine(32.6), (F * s) ** 2, (F * s) ** 2))
    # r1, in units of the ellipse (= sigma): int r^2 e^(-r^2/2) / int r e^(-r^2/2) over 0 .. 6
    from math import erf, exp, pi, sqrt
    r1 = (sqrt(pi / 2) * erf(6 / sqrt(2)) - 6 * exp(-18.0)) / (1 - exp(-18.0))
    assert abs(r1 - sqrt(pi / 2)) < 1e-6
    print(f'r1 {k1["r1"]:.9f} fine {k2["r1"]:.9f} closed {r1:.9f}; flux {k1["flux_auto"]:.9f} fine {k2["flux_auto"]:.9f}')
    assert abs(k1['r1'] - r1) <= tol(k1['r1'], k2['r1'], r1)
    assert k1['kron_radius'] == 3.5 and k1['flags_auto'] == 0
    want = 1.0 - exp(-3.5 ** 2 / 2)
    assert abs(k1['flux_auto'] - want) <= tol(k1['flux_auto'], k2['flux_auto'], want)
    assert k1['mag_auto'] == -2.5 * np.log10(k1['flux_auto'])
    assert k1['npix_auto'] > 140 and k1['nskip_auto'] == 0
    assert k1['fluxerr_auto'] == np.sqrt(k1['npix_auto'])                     # sigma = 1 everywhere


def test_exponential_profile_gets_a_radius_above_the_floor():
    yy, xx = np.mgrid[0:96, 0:96].astype(np.float64)
    img = (20.0 * np.exp(-np.hypot(xx - 47.4, yy - 48.2) / 3.0)).astype(np.float32)
    sigma = np.ones_like(img)
    base = xr.extract(img, sigma)
    base.update(img=img, sigma=sigma)
    rows = mr.measure(base)
    assert len(rows) == 1
    r = rows[0]
    print(f'exponential: r1 {r["r1"]:.4f}, KRON_RADIUS {r["kron_radius"]:.4f}')
    assert r['kron_radius'] == 2.5 * r['r1'] > 3.5 and r['flags_auto'] == 0
    # and a Gaussian through the same steps stays at the floor
    g = (2000.0 * gaussian(96, 96, 47.4, 48.2, 2.0)).astype(np.float32)
    base = xr.extract(g, sigma)
    base.update(img=g, sigma=sigma)
    assert mr.measure(base)[0]['kron_radius'] == 3.5


@pytest.mark.parametrize('off', [(0.0, 0.0), (0.5, 0.5), (0.25, -0.4), (-0.13, 0.37), (0.49, 0.01), (-0.33, -0.21)])
def test_window_finds_the_centre_of_a_gaussian(off):
    s = 1.7
    xc, yc = 32.0 + off[0], 31.0 + off[1]
    c, f = both(64, 64, xc, yc, s)
    # started 0.3 px away, as an isophotal barycentre may be
    w1 = mr.window(*planes(c), row(xc + 0.21, yc - 0.22, s * s, s * s, fwhm=2.35482 * s))
    w2 = mr.window(*planes(f), row(fine(xc + 0.21), fine(yc - 0.22), (F * s) ** 2, (F * s) ** 2, fwhm=2.35482 * F * s))
    assert w1['flags_win'] == 0 and 1 <= w1['niter_win'] < 16
    for key, true in (('xwin_image', xc + 1.0), ('ywin_image', yc + 1.0)):
        a, b = w1[key], coarse(w2[key] - 1.0) + 1.0
        # the iteration stops when its step is below 1e-4 px: what is left is the last step times rho / (1 - rho)
        left = w1['steps'][-1] * w1['rho'] / (1.0 - w1['rho'])
        print(f'{key} {off}: off by {a - true:.3g}, coarse - fine {a - b:.3g}, left by the stop {left:.3g}')
        assert abs(a - true) <= tol(a, b, true) + left


def test_window_returns_sigma_when_the_source_has_the_windows_width():
    s = 2.0
    c, f = both(64, 64, 30.7, 33.2, s)
    w1 = mr.window(*planes(c), row(30.7, 33.2, s * s, s * s, fwhm=2.35482 * s))
    w2 = mr.window(*planes(f), row(fine(30.7), fine(33.2), (F * s) ** 2, (F * s) ** 2, fwhm=2.35482 * F * s))
    # source times window is a Gaussian of variance sigma^2 / 2 cut at 4 sigma: u = 16 in
    # <x^2> = (sigma^2 / 2) (1 - (1 + u) e^-u) / (1 - e^-u); the factor 2 of the operator undoes the halving
    u = 16.0
    want = s * np.sqrt((1.0 - (1.0 + u) * np.exp(-u)) / (1.0 - np.exp(-u)))
    assert abs(want - s) < 2e-6 * s
    for key in ('awin_image', 'bwin_image'):
        a, b = w1[key], w2[key] / F
        print(f'{key}: {a!r}, fine {b!r}, closed form {want!r}')
        assert abs(a - want) <= tol(a, b, want)
    assert abs(w1['sigma_win'] - s) < 1e-15


def test_window_returns_the_angle_of_a_rotated_ellipse():
    s1, s2, th = 3.0, 1.5, np.radians(33.0)
    c, f = both(80, 80, 40.2, 39.6, s1, s2, th)
    cov = lambda a, b: (a * a * np.cos(th) ** 2 + b * b * np.sin(th) ** 2, a * a * np.sin(th) ** 2 + b * b * np.cos(th) ** 2,
                        (a * a - b * b) * np.sin(th) * np.cos(th))              # noqa: E731
    x2, y2, xy = cov(s1, s2)
    fw = 2.35482 * 2.0
    w1 = mr.window(*planes(c), row(40.2, 39.6, x2, y2, xy, fwhm=fw))
    x2f, y2f, xyf = cov(F * s1, F * s2)
    w2 = mr.window(*planes(f), row(fine(40.2), fine(39.6), x2f, y2f, xyf, fwhm=F * fw))
    a, b = w1['thetawin_image'], w2['thetawin_image']
    print(f'THETAWIN {a!r}, fine {b!r}, true 33; A / B {w1["awin_image"] / w1["bwin_image"]:.4f}')
    # a circular window keeps the principal axes of the source
    assert abs(a - 33.0) <= tol(a, b, 33.0)
    assert w1['awin_image'] > 1.2 * w1['bwin_image']
    k = mr.kron(*planes(c), row(40.2, 39.6, x2, y2, xy))
    assert k['kron_radius'] == 3.5 and abs(k['flux_auto'] - (1 - np.exp(-3.5 ** 2 / 2))) < 2e-3


def test_skipped_pixels_fallback_and_flags():
    img, sigma, bad = planes(gaussian(48, 40, 20.0, 18.0, 2.0))
    o = row(20.0, 18.0, 4.0, 4.0, fwhm=4.7)
    full = mr.kron(img, sigma, bad, o)
    bad = bad.copy()
    bad[18, 20:24] = True
    k = mr.kron(img, sigma, bad, o)
    assert k['nskip_auto'] == 4 and k['npix_auto'] == full['npix_auto'] - 4 and k['flags_auto'] == 0
    assert k['flux_auto'] == pytest.approx(full['flux_auto'] - img[18, 20:24].sum(), rel=1e-12)
    bad[10:18, :] = True
    assert mr.kron(img, sigma, bad, o)['flags_auto'] & 1
    assert mr.kron(img, sigma, planes(img)[2], row(2.0, 18.0, 4.0, 4.0))['flags_auto'] & 2          # leaves the frame
    neg = mr.kron(-img, sigma, planes(img)[2], o)
    assert neg['flags_auto'] == 4 and neg['kron_radius'] == 3.5 and neg['mag_auto'] == 99.0 and neg['magerr_auto'] == 99.0
    w = mr.window(-img, sigma, planes(img)[2], dict(o, errx2=1.0, erry2=2.0, errxy=0.5))
    assert w['flags_win'] == 1 and w['niter_win'] == 1
    assert (w['xwin_image'], w['ywin_image'], w['awin_image'], w['bwin_image'], w['thetawin_image']) == \
        (21.0, 19.0, o['a'], o['b'], o['theta'])
    assert (w['errx2win'], w['erry2win'], w['errxywin']) == (1.0, 2.0, 0.5)
