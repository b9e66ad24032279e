"""Small scenes for the PSF photometry (tests/test_psf_ref.py asserts their conditions on the restatement alone,
tests/test_psf_gpu.py runs the kernels on them, tests/measure_psf_tolerance.py sets the tolerances on them).  numpy only;
every scene is built once and shared.  Frames are 64^2 to 128^2."""
import functools
from typing import NamedTuple

import numpy as np

BAD_BITS = 198589                # BAD_SUM of the package
BIT8 = 1 << 8                    # one of the bad bits
BIT1 = 1 << 1                    # not a bad bit
FWHM = 2.4
K_FWHM = 2.3548200450309493
MARGIN = 1e-9                    # how far every pixel centre stays from every circle (asserted in tests/test_psf_ref.py)


def gaussians(img, items, fwhm=FWHM):
    s = fwhm / K_FWHM
    jj, ii = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    for x, y, f in items:
        if np.isfinite(x) and np.isfinite(y):
            img += f / (2 * np.pi * s * s) * np.exp(-0.5 * ((ii - x) ** 2 + (jj - y) ** 2) / (s * s))
    return img


def model_gaussian(half, fwhm=FWHM, norm_radius=10.0):
    """A unit-sum sampled Gaussian on the model grid, 0 beyond ``norm_radius``: an input for the fit scenes."""
    s = fwhm / K_FWHM
    jj, ii = np.mgrid[-half:half + 1, -half:half + 1]
    m = np.exp(-0.5 * (ii * ii + jj * jj) / (s * s))
    m[ii * ii + jj * jj > norm_radius * norm_radius] = 0.0
    return m / m.sum()


class Stars(NamedTuple):
    img: np.ndarray
    mask: np.ndarray
    x: np.ndarray
    y: np.ndarray
    sky: np.ndarray
    norm: np.ndarray
    half: int
    names: tuple


@functools.lru_cache(maxsize=None)
def cutout_edges(half):
    """One star per case on a 128^2 frame, 40 px apart so that no planted pixel reaches a neighbour's footprint."""
    n = 128
    rng = np.random.default_rng(100 + half)
    jj, ii = np.mgrid[0:n, 0:n]
    img = 150.0 + 0.05 * ii - 0.03 * jj + rng.normal(0.0, 4.0, (n, n))
    mask = np.zeros((n, n), np.int32)
    stars = [('dx-zero', 24.0, 24.37), ('dx-half', 64.5, 24.61), ('dx-ulp-below-one', np.nextafter(105.0, 0.0), 24.13),
             ('off-frame-one-tap-left', half + 1 + 0.3, 64.42),         # floor(x) - half - 2 = -1
             ('bad-under-one-tap', 64.37, 64.21), ('nan-pixel', 104.6, 64.8),
             ('dx-zero-beside-bad-column', 24.0, 104.45), ('generic', 64.71, 104.29), ('dy-zero', 104.33, 104.0),
             ('norm-nan', 64.71, 104.29), ('norm-inf', 64.71, 104.29), ('norm-zero', 64.71, 104.29),
             ('norm-negative', 64.71, 104.29), ('sky-nan', 64.71, 104.29), ('x-nan', np.nan, 104.29), ('y-inf', 64.71, np.inf)]
    gaussians(img, [(x, y, 3.0e4) for _, x, y in stars[:9]])
    mask[64 - 1, 64 + half + 3] |= BIT8              # the last tap of column i = +half of 'bad-under-one-tap'
    mask[30, 64] |= BIT1                             # not a bad bit, inside 'dx-half': changes nothing
    img[60, 100] = np.nan                            # inside 'nan-pixel'
    mask[104 - half - 3:104 + half + 4, 24 + half + 1] |= BIT8     # the column a six-wide footprint of 'dx-zero-beside' would touch
    x = np.array([s[1] for s in stars])
    y = np.array([s[2] for s in stars])
    sky = np.full(x.size, 150.0) + 0.05 * np.nan_to_num(x, nan=0.0, posinf=0.0) - 0.03 * np.nan_to_num(y, nan=0.0, posinf=0.0)
    norm = np.full(x.size, 3.0e4)
    names = tuple(s[0] for s in stars)
    norm[names.index('norm-nan')] = np.nan
    norm[names.index('norm-inf')] = np.inf
    norm[names.index('norm-zero')] = 0.0
    norm[names.index('norm-negative')] = -5.0
    sky[names.index('sky-nan')] = np.nan
    return Stars(img.astype(np.float32), mask, x, y, sky, norm, half, names)


@functools.lru_cache(maxsize=None)
def cutout_many():
    """65 stars (for nstar = 0, 1, 63, 64, 65) on a 128^2 frame, half 3: the model test too (a clipped median over many
    stars, an outlier star among them)."""
    n, half = 128, 3
    rng = np.random.default_rng(7)
    img = 20.0 + rng.normal(0.0, 1.0, (n, n))
    x = rng.uniform(10.0, n - 11.0, 65)
    y = rng.uniform(10.0, n - 11.0, 65)
    f = rng.uniform(2.0e4, 6.0e4, 65)
    gaussians(img, zip(x, y, f))
    img[int(y[5]) + 1, int(x[5])] += 2.0e4           # an outlier in one star's cutout: clipped
    mask = np.zeros((n, n), np.int32)
    return Stars(img.astype(np.float32), mask, x, y, np.full(65, 20.0), f, half, tuple(f's{k}' for k in range(65)))


@functools.lru_cache(maxsize=None)
def model_floor():
    """Five stars, half 4, norm radius 3.5: one entry is NaN for every star (a planted bad pixel at the same offset from
    each), one for all but two, one for all but three: MIN_STARS_PIXEL = 3 at its boundary."""
    n, half = 96, 4
    rng = np.random.default_rng(9)
    img = rng.normal(0.0, 1.0, (n, n))
    x = np.array([20.0, 50.0, 80.0, 30.0, 65.0])     # dx = dy = 0: the footprint of an entry is one pixel
    y = np.array([20.0, 22.0, 24.0, 60.0, 62.0])
    gaussians(img, [(a, b, 4.0e4) for a, b in zip(x, y)])
    mask = np.zeros((n, n), np.int32)
    for k in range(5):
        mask[int(y[k]) + 1, int(x[k]) + 2] |= BIT8           # offset (2, 1): every star
        if k >= 2:
            mask[int(y[k]) - 1, int(x[k]) + 1] |= BIT8       # offset (1, -1): two stars left
        if k >= 3:
            mask[int(y[k]) + 2, int(x[k]) - 1] |= BIT8       # offset (-1, 2): three stars left
    return Stars(img.astype(np.float32), mask, x, y, np.zeros(5), np.full(5, 4.0e4), half, tuple('abcde'))


@functools.lru_cache(maxsize=None)
def night_planes():
    """The frame of the end-to-end test: 256^2, 60 stars of FWHM 2.4 px on a jittered 8 x 8 grid over a sky of 200 with
    noise 5, and 40 planted faint sources of flux 800.  dict(img, rms, mask, x, y, flux, faint)."""
    n = 256
    rng = np.random.default_rng(77)
    gx, gy = np.meshgrid(np.linspace(24.0, n - 25.0, 8), np.linspace(24.0, n - 25.0, 8))
    keep = rng.permutation(64)[:60]
    sx = gx.ravel()[keep] + rng.uniform(-3.0, 3.0, 60)
    sy = gy.ravel()[keep] + rng.uniform(-3.0, 3.0, 60)
    flux = rng.uniform(3.0e4, 1.5e5, 60)
    img = 200.0 + rng.normal(0.0, 5.0, (n, n))
    gaussians(img, zip(sx, sy, flux), fwhm=2.4)
    fx, fy = rng.uniform(12.0, n - 13.0, 40), rng.uniform(12.0, n - 13.0, 40)
    gaussians(img, zip(fx, fy, np.full(40, 800.0)), fwhm=2.4)
    return dict(img=img.astype(np.float32), rms=np.full((n, n), 5.0, np.float32), mask=np.zeros((n, n), np.int32), x=sx, y=sy,
                flux=flux, faint=(fx, fy))


class Fits(NamedTuple):
    img: np.ndarray
    rms: np.ndarray
    mask: np.ndarray
    x: np.ndarray
    y: np.ndarray
    model: np.ndarray
    names: tuple


@functools.lru_cache(maxsize=None)
def fit_main(half=12):
    """96^2, noise 4 on a sky of 20, sources of FWHM 2.4 at: fx = -0.5 exactly, 0 and just under +0.5; the frame's
    corner, half outside, fully outside; one masked pixel, every pixel masked, all but one pixel masked; an rms of 0, NaN
    and inf; a NaN pixel; positions that are not finite; then generic ones up to 65."""
    n = 96
    rng = np.random.default_rng(21)
    jj, ii = np.mgrid[0:n, 0:n]
    img = 20.0 + rng.normal(0.0, 4.0, (n, n))
    rms = (4.0 * (1.0 + 0.004 * ii)).astype(np.float32)
    mask = np.zeros((n, n), np.int32)
    named = [('fx-minus-half', 20.5, 14.21), ('fx-zero', 38.0, 14.37), ('fx-under-half', np.nextafter(56.5, 0.0), 14.13),
             ('fy-zero', 74.31, 14.0), ('corner', 0.21, 0.32), ('half-outside', -0.43, 25.31), ('top-edge', 50.71, 95.45),
             ('fully-outside', -20.31, 10.23), ('far-outside', 500.7, -900.1), ('huge', 1.0e300, 3.3),
             ('one-masked', 14.31, 40.62), ('all-masked', 40.41, 42.73), ('one-left', 66.23, 42.31),
             ('rms-zero', 14.63, 68.21), ('rms-nan', 36.32, 70.71), ('rms-inf', 58.73, 69.41), ('nan-pixel', 80.23, 70.81),
             ('x-nan', np.nan, 20.0), ('y-inf', 20.0, np.inf)]
    gaussians(img, [(x, y, 2.0e3) for _, x, y in named if np.isfinite(x) and np.isfinite(y) and abs(x) < 1e6])
    mask[41, 15] |= BIT8
    mask[40, 13] |= BIT1                                   # not a bad bit
    pad = 10 if half <= 12 else 13                         # wider than the largest circle (R = half - 3.5)
    mask[43 - pad:43 + pad + 1, 40 - pad:40 + pad + 1] |= BIT8
    mask[42 - pad:42 + pad + 1, 66 - pad:66 + pad + 1] |= BIT8
    mask[42, 66] = 0                                       # the one pixel left of 'one-left'
    rms[68, 15] = 0.0
    rms[71, 36] = np.nan
    rms[69, 59] = np.inf
    img[71, 80] = np.nan
    x = [s[1] for s in named]
    y = [s[2] for s in named]
    k = 65 - len(named)
    x += list(rng.uniform(10.0, 86.0, k))
    y += list(rng.uniform(10.0, 86.0, k))
    names = tuple(s[0] for s in named) + tuple(f'generic{i}' for i in range(k))
    return Fits(img.astype(np.float32), rms, mask, np.array(x), np.array(y), model_gaussian(half), names)


FIT_CASES = [(6.0, 0, True, True), (6.0, 1, True, True), (1.0, 0, True, True), (8.5, 1, True, True),
             (6.0, 0, False, True), (6.0, 1, False, False), (6.0, 1, True, False)]     # (R, fit_sky, with rms, with mask)
# (R = 1 with a sky term is left out: two parameters on three to five pixels of nearly equal profile is a fit the float64
# and the extended run of the restatement themselves disagree on)
