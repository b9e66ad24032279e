"""Small scenes for the photometric calibration (tests/test_photcal_ref.py asserts their conditions on the reference
alone, tests/test_photcal_gpu.py runs the kernels on them).  numpy only; every scene is built once and shared."""
import functools
from typing import NamedTuple

import numpy as np

BAD_BITS = 198589                # BAD_SUM of the package (zuds/constants.py:45)
BIT8 = 1 << 8                    # SATURATED: one of the bad bits
BIT1 = 1 << 1                    # CONTAINS SEXTRACTOR DETECTION: not a bad bit
FWHM = 2.4
K_FWHM = 2.3548200450309493
SATURATE = 50000.0
NX, NY = 96, 80                  # deliberately not square


class Growth(NamedTuple):
    img: np.ndarray
    rms: np.ndarray
    mask: np.ndarray
    x: np.ndarray
    y: np.ndarray
    radii: tuple
    annulus: tuple
    saturate: float
    nsky_min: int
    names: tuple


def gaussians(img, items, fwhm=FWHM):
    s = fwhm / K_FWHM
    jj, ii = np.mgrid[0:img.shape[0], 0:img.shape[1]]
    for x, y, f in items:
        if np.isfinite(x) and np.isfinite(y):
            img += f / (2 * np.pi * s * s) * np.exp(-0.5 * ((ii - x) ** 2 + (jj - y) ** 2) / (s * s))
    return img


def _base(seed, noise=4.0):
    rng = np.random.default_rng(seed)
    jj, ii = np.mgrid[0:NY, 0:NX]
    img = 150.0 + 0.05 * ii - 0.03 * jj + rng.normal(0.0, noise, (NY, NX))          # a tilted sky with noise
    rms = (noise * (1.0 + 0.002 * ii)).astype(np.float32)
    return rng, img, rms


@functools.lru_cache(maxsize=None)
def growth_main():
    """Seven radii, annulus 12 .. 18: centres on a pixel centre, a pixel corner and generic fractions; boxes clipped by
    each edge; an annulus alone clipped; bad, saturated and NaN pixels inside particular apertures; NaN, inf and bad
    pixels in an annulus; a position that is not finite, one far outside the frame."""
    rng, img, rms = _base(11)
    stars = [('centre', 48.0, 40.0), ('corner', 30.5, 30.5), ('generic', 60.37, 45.81),
             ('clip-left', 5.3, 40.2), ('clip-right', 91.6, 38.7), ('clip-bottom', 47.2, 3.9), ('clip-top', 52.8, 76.4),
             ('annulus-clipped', 14.2, 41.3), ('bad-in-1', 22.3, 60.6), ('bad-in-ref', 70.4, 25.2),
             ('saturated', 35.6, 52.3), ('nan-in-3', 64.7, 57.2), ('nan-position', np.nan, 20.0),
             ('inf-position', 30.0, np.inf), ('far-outside', 400.5, -300.25), ('just-outside', -3.2, 40.0)]
    gaussians(img, [(x, y, 3.0e4) for _, x, y in stars])
    mask = np.zeros((NY, NX), np.int32)
    mask[61, 22] |= BIT8                 # 0.5 px from bad-in-1: inside aperture 1 (r = 1)
    mask[25, 78] |= BIT8                 # 7.6 px from bad-in-ref: inside r = 10 only
    mask[10:14, 40:60] |= BIT1           # a bit that is not bad: seen by nobody
    img[52, 36] = 60000.0                # the peak of `saturated`
    img[59, 66] = np.nan                 # nearest point 1.53 px from nan-in-3: touches r = 2 and up, not r = 1.5
    img[26, 48] = np.nan                 # in the annulus of `centre` (14 px)
    img[53, 50] = np.inf                 # the same annulus (13.2 px)
    mask[55, 48] |= BIT8                 # the same annulus (15 px)
    img[30, 16] = -np.inf                # annulus of `corner` (14.5 px)
    rms[46, 63] = np.inf                 # nearest point 2.13 px from `generic`: its errors are NaN from r = 3 on
    rms[30, 35] = np.nan                 # nearest point 4.0 px from `corner`: NaN from r = 5 on
    x = np.array([s[1] for s in stars])
    y = np.array([s[2] for s in stars])
    return Growth(img.astype(np.float32), rms, mask, x, y, (1.0, 1.5, 2.0, 3.0, 5.0, 7.0, 10.0), (12.0, 18.0), SATURATE,
                  50, tuple(s[0] for s in stars))


@functools.lru_cache(maxsize=None)
def growth_sky():
    """One radius, annulus 5 .. 8, stars 24 px apart: a constant annulus (sigma 0, nothing clipped), an annulus that is
    entirely bad (nsky 0), one with few usable pixels (below nsky_min), a cosmic ray that takes two clipping rounds, ties,
    and plain ones whose usable counts are even and odd."""
    rng, img, rms = _base(12, noise=1.0)
    pos = {'plain': (12.0, 12.0), 'constant': (36.0, 12.0), 'all-bad': (60.0, 12.0), 'few': (84.0, 12.0),
           'cosmic': (12.3, 36.4), 'ties': (36.5, 36.5), 'odd': (60.2, 36.7), 'even': (84.0, 36.0),
           'half-ties': (12.0, 62.0), 'plain2': (36.1, 61.8)}
    gaussians(img, [(x, y, 5.0e3) for x, y in pos.values()])
    mask = np.zeros((NY, NX), np.int32)
    jj, ii = np.mgrid[0:NY, 0:NX]

    def ring(name, r0=5.0, r1=8.0):
        x, y = pos[name]
        d2 = (ii - x) ** 2 + (jj - y) ** 2
        return (d2 >= r0 * r0) & (d2 < r1 * r1)
    img[ring('constant')] = 151.25
    mask[ring('all-bad')] |= BIT8
    few = ring('few')
    mask[few & (ii > 79)] |= BIT8                              # leaves the left edge of the ring
    c = ring('cosmic')
    cj, ci = np.nonzero(c)
    order = np.argsort((ci - 12.3) * 7 + (cj - 36.4) * 3)
    # a bright hit and a graded halo: the halo inflates the first MAD, so its faint end goes only in the second round
    img[cj[order[:3]], ci[order[:3]]] += 500.0
    img[cj[order[3:15]], ci[order[3:15]]] += np.linspace(3.2, 5.5, 12)
    t = ring('ties')
    img[t] = np.round(img[t])                                  # integers: many equal values
    h = ring('half-ties')
    hj, hi = np.nonzero(h)
    img[hj[::2], hi[::2]] = 150.5                              # half of the ring at one value: the MAD may be 0 with outliers
    e, o = ring('even'), ring('odd')
    for r, want in ((e, 0), (o, 1)):
        j, i = np.nonzero(r)
        if (r.sum() & 1) != want:
            mask[j[0], i[0]] |= BIT8
    names = tuple(pos)
    x = np.array([pos[k][0] for k in names])
    y = np.array([pos[k][1] for k in names])
    return Growth(img.astype(np.float32), None, mask, x, y, (3.0,), (5.0, 8.0), 0.0, 50, names)


@functools.lru_cache(maxsize=None)
def growth_rout20():
    """Eight radii and the largest annulus, 14 .. 20, on a 128 x 100 frame."""
    rng = np.random.default_rng(13)
    ny, nx = 100, 128
    jj, ii = np.mgrid[0:ny, 0:nx]
    img = 90.0 + 0.02 * ii + rng.normal(0.0, 3.0, (ny, nx))
    stars = [(40.0, 40.0), (80.5, 50.5), (100.3, 30.9), (20.2, 70.6), (64.0, 97.0)]
    s = FWHM / K_FWHM
    for x, y in stars:
        img += 2.0e4 / (2 * np.pi * s * s) * np.exp(-0.5 * ((ii - x) ** 2 + (jj - y) ** 2) / (s * s))
    rms = np.full((ny, nx), 3.0, np.float32)
    mask = np.zeros((ny, nx), np.int32)
    x, y = np.array([p[0] for p in stars]), np.array([p[1] for p in stars])
    return Growth(img.astype(np.float32), rms, mask, x, y, (1.0, 1.5, 2.0, 3.0, 5.0, 7.0, 10.0, 12.0), (14.0, 20.0), 0.0, 50,
                  tuple(f's{k}' for k in range(len(stars))))


COUNTS = (1, 2, 63, 64, 65, 257)          # one star per workgroup: 0, 1 and 2 are the counts either side of it


@functools.lru_cache(maxsize=None)
def growth_many():
    """257 positions on the main image, two small radii and annulus 5 .. 8: the star counts are its first n."""
    g = growth_main()
    rng = np.random.default_rng(14)
    x = rng.uniform(-6.0, NX + 5.0, 257)
    y = rng.uniform(-6.0, NY + 5.0, 257)
    x[:3], y[:3] = [48.0, 30.5, 60.37], [40.0, 30.5, 45.81]
    x[100], y[200] = np.nan, np.inf
    return Growth(g.img, g.rms, g.mask, x, y, (2.0, 3.0), (5.0, 8.0), SATURATE, 50, tuple(f'p{k}' for k in range(257)))


GROWTH = {'main': growth_main, 'sky': growth_sky, 'rout20': growth_rout20}


# ---- clipped median ---------------------------------------------------------------------------------------------------
# 5000: a column of exactly 64 KB of dynamic LDS (8192 padded doubles) beside the kernel's static words
CM_ROWS = (0, 1, 2, 3, 64, 65, 1023, 1024, 1025, 5000, 16384)


@functools.lru_cache(maxsize=None)
def clipmed_columns(n):
    """A (n, 9) array whose first 7 columns are used (the stride is larger than the column count): noise, noise with
    outliers that go in one round, a graded tail that takes three, ties, all NaN, +-inf and NaN sprinkled in, constants."""
    rng = np.random.default_rng(100 + n)
    a = np.full((n, 9), 12345.0)
    if n == 0:
        return a
    a[:, 0] = rng.normal(10.0, 1.0, n)
    a[:, 1] = rng.normal(-3.0, 0.5, n)
    a[::7, 1] += 40.0
    a[:, 2] = graded(n, rng)
    a[:, 3] = np.round(rng.normal(0.0, 2.0, n))
    a[:, 4] = np.nan
    a[:, 5] = rng.normal(5.0, 1.0, n)
    a[::3, 5] = np.nan
    a[1::5, 5] = np.inf
    a[2::11, 5] = -np.inf
    a[:, 6] = 2.5
    return a


def graded(n, rng):
    """Noise with a tail whose far end inflates the MAD: it goes a layer per round."""
    v = rng.normal(0.0, 1.0, n)
    k = n // 3
    if k:
        v[:k] = np.linspace(2.0, 30.0, k)
    return v


# ---- limiting magnitude -----------------------------------------------------------------------------------------------
class Maglim(NamedTuple):
    rms: np.ndarray
    mask: np.ndarray
    radius: float
    step: int


@functools.lru_cache(maxsize=None)
def maglim(name):
    shape = {'small': (50, 70), 'large': (130, 257)}[name.split('-')[0]]
    ny, nx = shape
    kind = name.split('-')[1]
    jj, ii = np.mgrid[0:ny, 0:nx]
    mask = np.zeros(shape, np.int32)
    step = 8 if name.startswith('small') else 16
    if kind == 'flat':
        return Maglim(np.full(shape, 2.5, np.float32), None, 3.0, step)
    rms = (2.0 + 0.01 * ii + 0.02 * jj).astype(np.float32)
    if kind == 'graded':
        mask[20:30, 30:45] |= BIT8          # a masked block
        mask[5:9, 5:9] |= BIT1              # not a bad bit
        rms[12, 20] = 0.0                   # a non-positive rms pixel inside an aperture box
        rms[36, 52] = -1.0
        if name.startswith('large'):
            rms[100, 200] = np.nan
            rms[68, 100] = np.inf
        return Maglim(rms, mask, 3.0, step)
    if kind == 'none':                      # every lattice point rejected
        mask[:, :] = BIT8
        return Maglim(rms, mask, 3.0, step)
    raise KeyError(name)


MAGLIM = ('small-flat', 'small-graded', 'small-none', 'large-flat', 'large-graded')


# ---- end to end -------------------------------------------------------------------------------------------------------
E2E_N = 256
E2E_ZP = (26.1, 26.3, 26.5)
E2E_NSTAR = 60


def e2e_stars():
    """(x, y on the base grid, magnitude) of 60 stars, no two nearer than 22 px, away from the frame's edge."""
    rng = np.random.default_rng(21)
    pts = []
    while len(pts) < E2E_NSTAR:
        p = rng.uniform(8.0, E2E_N - 8.0, 2)
        if all((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 > 22.0 ** 2 for q in pts):
            pts.append(p)
    pts = np.array(pts)
    mag = rng.uniform(13.5, 16.5, E2E_NSTAR)
    return pts[:, 0], pts[:, 1], mag
