"""Scenes for the seeing estimate (``k_find_stars``, ``k_star_fwhm``, ``seeing.py``): the smallest inputs at which
each part can go wrong.

Test infrastructure, numpy only.  ``tests/test_seeing_scenes.py`` asserts on the CPU what is said about a scene here
(from ``oracle/detect.py``) and that the scenes tell a slightly wrong operator from the right one;
``tests/test_seeing_gpu.py`` runs them through the kernels.

Finder scenes are ``Finder(img, bad, lo, hi, iso, border)``: integer-valued float32 pixels (but for the two
``nextafter`` peaks), so that every comparison is exact.  ``FINDER`` maps a name to the function that builds it.

Moments scenes are ``Moments(img, x, y, half)``: a float32 frame that is never square, the start pixels of the stars
and the half width of the window.  Sub-pixel centres have different fractions in x and y, so that a swapped axis
shows.  ``MOMENTS`` maps a name to its builder; ``trace`` restates ``oracle.detect.star_fwhm`` with a record of every
round, from which the preconditions are read:

* stop round.  The iteration converges linearly (each step about half the one before) and stops at the first step of
  at most 1e-8.  Two evaluations that differ in the last bits stop at the same round unless a step lands on 1e-8 to
  within rounding; one round more or less moves the FWHM by some 2.5e-9, more than the tolerance.  So no star of a
  scene may have a step within 1 % of 1e-8 at any round: the step it stops at is at most 0.99e-8, every step before
  it at least 1.01e-8.  (The step itself is good to some 1e-15, i.e. 1e-7 of the criterion.  A band that reached a
  factor of two to either side could not be met: with each step half the one before, the step before the last one
  always lies between 1e-8 and 2e-8 - 1.3e-8 for a clean star of FWHM 2.5.)
* exits.  A star that leaves through ``s0``, ``t0``, ``m2`` or ``inv`` must do so by a margin that rounding cannot
  cross: the sum that decides is exactly zero, not finite, or at least 1e-6 of the sum of the absolute terms (``inv``:
  of ``1 / s2``).
* visible window.  Where a scene is there for the extent of the window, its corner pixel must carry at least 1e-3 of
  the centre's weight at the converged ``s2`` (on a well-sampled star at ``half = 10`` it carries e^-80).

The chaotic regime (a star of FWHM 1.2 px) is not pinned: the stars here have FWHM >= 1.7 px, but for the
single hot pixel, which leaves at once through ``m2``.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

K_FWHM = 2.3548200450309493


class Finder(NamedTuple):
    img: np.ndarray
    bad: Optional[np.ndarray]
    lo: float
    hi: float
    iso: int
    border: int


class Moments(NamedTuple):
    img: np.ndarray
    x: np.ndarray
    y: np.ndarray
    half: int


# ---------------------------------------------------------------------------------------------------- finder scenes
def rules():
    """104 x 96, iso 5, border 12, lo 10, hi 1000.  ``RULES_WANT`` lists who must be found.

    * an isolated peak;
    * equal pairs side by side, stacked and on both diagonals - of the pair (77, 20), (76, 21) the first is earlier in
      raster order although it lies to the right - and a 3 x 3 plateau: the first pixel in raster order wins;
    * peaks of different heights exactly ``iso`` apart (along x, along y, and at the corner of the box, where the
      higher one stands in the border zone: it is no star itself and still hides its neighbour): only the higher one;
      ``iso + 1`` apart: both;  equal peaks ``iso`` apart along x and across the corner (dx = -iso, dy = +iso);
    * a peak equal to ``lo``, equal to ``hi`` (neither is a star: both comparisons are strict) and at ``nextafter``
      inside each (both are); a peak next to a pixel above ``hi`` (hidden by it);
    * peaks at ``border - 1``, ``border``, ``n - border - 1`` and ``n - border`` on all four sides: the inner two are in.
    """
    nx, ny = 104, 96
    img = np.zeros((ny, nx), np.float32)
    img[20, 20] = 100
    img[20, 34] = img[20, 35] = 80
    img[20, 48] = img[21, 48] = 81
    img[20, 62] = img[21, 63] = 82
    img[21, 76] = img[20, 77] = 83
    img[19:22, 89:92] = 84
    img[34, 20], img[34, 25] = 90, 91
    img[34, 40], img[34, 46] = 92, 93
    img[34, 60], img[39, 60] = 94, 95
    img[34, 76], img[40, 76] = 96, 97
    img[34, 88], img[39, 93] = 98, 99
    img[48, 20] = 10
    img[48, 34] = np.nextafter(np.float32(10), np.float32(np.inf))
    img[48, 48] = 1000
    img[48, 62] = np.nextafter(np.float32(1000), np.float32(-np.inf))
    img[62, 20], img[62, 22] = 500, 2000
    img[76, 34] = img[76, 39] = 70
    img[76, 60] = img[81, 55] = 71
    for k, (x, y) in enumerate(((11, 55), (12, 69), (nx - 12, 55), (nx - 13, 69),
                                (27, 11), (41, 12), (27, ny - 12), (41, ny - 13))):
        img[y, x] = 200 + k
    return Finder(img, None, 10.0, 1000.0, 5, 12)


RULES_WANT = sorted([(20, 20), (34, 20), (48, 20), (62, 20), (77, 20), (89, 19), (25, 34), (40, 34), (46, 34),
                     (60, 39), (76, 34), (76, 40), (34, 48), (62, 48), (34, 76), (60, 76),
                     (12, 69), (91, 69), (41, 12), (41, 83)])


def poison():
    """96 x 96, iso 5, border 12, lo 10, hi 3e38; 17 peaks of distinct heights on a 14-pixel lattice, 100 + 10 k at
    cell k.  ``POISON_WANT`` / ``POISON_WANT_NOMAP`` list who must be found with and without the bad-pixel map.

    * cells 0-3: a bad pixel at each far corner of the box (dx = +-5, dy = +-5): no star; cells 4-7: at +-6: a star;
    * cells 8-11: a NaN at the corners (5, 5) and (-5, -5): no star; at 6: a star;
    * cell 12: a +inf neighbour (larger: no star); cell 13: a -inf neighbour (smaller, and not NaN: a star);
    * cell 14: a +inf peak: not below ``hi``, so no star, and it hides cell 15, which stands 4 px from it;
    * cell 16: a bad pixel on the peak itself."""
    n = 96
    img = np.zeros((n, n), np.float32)
    bad = np.zeros((n, n), bool)
    cells = [(20 + 14 * (k % 5), 20 + 14 * (k // 5)) for k in range(17)]
    for k, (x, y) in enumerate(cells):
        img[y, x] = 100 + 10 * k
    for k, (dx, dy) in enumerate(((5, 5), (-5, -5), (5, -5), (-5, 5), (6, 6), (-6, -6), (6, -6), (-6, 6))):
        x, y = cells[k]
        bad[y + dy, x + dx] = True
    for k, d in ((8, 5), (9, -5), (10, 6), (11, -6)):
        x, y = cells[k]
        img[y + d, x + d] = np.nan
    img[cells[12][1] + 2, cells[12][0] - 3] = np.inf
    img[cells[13][1] - 2, cells[13][0] + 3] = -np.inf
    x14, y14 = cells[14]
    img[y14, x14] = np.inf
    img[y14 + 4, x14 - 4] = 250                                      # "cell 15": its own lattice cell stays empty
    img[cells[15][1], cells[15][0]] = 0
    bad[cells[16][1], cells[16][0]] = True
    return Finder(img, bad, 10.0, 3.0e38, 5, 12)


def _cells(*ks):
    return sorted((20 + 14 * (k % 5), 20 + 14 * (k // 5)) for k in ks)


POISON_WANT = _cells(4, 5, 6, 7, 10, 11, 13)
POISON_WANT_NOMAP = _cells(0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 13, 16)


def iso1(border):
    """26 x 22, iso 1: the box is the 3 x 3 neighbourhood.  Peaks on the first and last pixel that ``border`` admits
    (at ``border == iso`` the box then reaches row / column 0 and the last one), equal neighbours along x, y and both
    diagonals, a higher neighbour at distance 1 and at distance 2, and a bad pixel in the frame's corner (0, 0), which
    is in the box of (1, 1) only."""
    nx, ny = 26, 22
    img = np.zeros((ny, nx), np.float32)
    bad = np.zeros((ny, nx), bool)
    b = border
    img[b, b], img[b, nx - b - 1], img[ny - b - 1, b], img[ny - b - 1, nx - b - 1] = 50, 51, 52, 53
    img[b - 1, 8], img[8, b - 1], img[ny - b, 12], img[12, nx - b] = 54, 55, 56, 57
    img[10, 6] = img[10, 7] = 60
    img[10, 11] = img[11, 11] = 61
    img[14, 6] = img[15, 7] = 62
    img[15, 11] = img[14, 12] = 63
    img[6, 15], img[6, 16] = 64, 65
    img[10, 15], img[10, 17] = 66, 67
    bad[0, 0] = True
    return Finder(img, bad, 10.0, 1000.0, 1, b)


def iso32(border):
    """230 x 200, iso 32: the box is 65 x 65.  A peak on each of the four corner pixels that ``border`` admits - at
    ``border == iso`` their boxes reach pixel 0 and the last pixel of the frame, where a bad pixel sits - a peak with
    a higher pixel at the far corner of its box (dx = dy = 32: hidden) and one with a higher pixel at 33 (both stand).
    No other two peaks are within 32 px of each other."""
    nx, ny = 230, 200
    img = np.zeros((ny, nx), np.float32)
    bad = np.zeros((ny, nx), bool)
    b = border
    img[b, b], img[ny - b - 1, nx - b - 1] = 50, 51
    img[b, nx - b - 1], img[ny - b - 1, b] = 52, 53
    bad[0, 0] = bad[ny - 1, nx - 1] = True
    img[60, 100], img[92, 132] = 60, 61
    img[120, 70], img[153, 103] = 63, 64
    return Finder(img, bad, 10.0, 1000.0, 32, b)


def seam(nx):
    """``nx`` x 40, iso 1, border 1: single peaks at x = 254 .. 257 and 510 .. 512 (those that the frame holds) and
    equal pairs across x = 254|255, 255|256 (the seam between two 256-thread blocks), 256|257 and 511|512, one
    feature every third row.  At nx = 257 and 513 the last block holds one thread."""
    ny = 40
    img = np.zeros((ny, nx), np.float32)
    feats = [(254,), (255,), (256,), (257,), (510,), (511,), (512,), (254, 255), (255, 256), (256, 257), (511, 512)]
    for k, xs in enumerate(feats):
        for x in xs:
            if x < nx:
                img[2 + 3 * k, x] = 100 + k
    return Finder(img, None, 10.0, 1000.0, 1, 1)


def tiny(nx, ny, iso, border):
    """A frame of 2 border - 1, 2 border or 2 border + 1 pixels on a side: none, none, or exactly one pixel is a
    candidate.  Every pixel is above ``lo`` and the values fall off from the middle pixel, so that the one candidate,
    where there is one, is a star."""
    y, x = np.mgrid[:ny, :nx]
    img = (900 - np.abs(x - border) - np.abs(y - border)).astype(np.float32)
    return Finder(img, None, 10.0, 1000.0, iso, border)


def cap():
    """84 x 60, iso 5, border 12: 40 peaks of distinct heights, 8 px apart, for the overflow contract."""
    img = np.zeros((60, 84), np.float32)
    for k in range(40):
        img[14 + 8 * (k // 8), 14 + 8 * (k % 8)] = 100 + k
    return Finder(img, None, 10.0, 1000.0, 5, 12)


FINDER = {'rules': rules, 'poison': poison, 'cap': cap,
          'iso1-border1': functools.partial(iso1, 1), 'iso1-border3': functools.partial(iso1, 3),
          'iso32-border32': functools.partial(iso32, 32), 'iso32-border40': functools.partial(iso32, 40)}
for _nx in (255, 256, 257, 513):
    FINDER[f'seam-{_nx}'] = functools.partial(seam, _nx)
for _iso, _b in ((5, 12), (1, 1)):
    for _dx in (-1, 0, 1):
        for _dy in (-1, 0, 1):
            FINDER[f'tiny-b{_b}-{2 * _b + _dx}x{2 * _b + _dy}'] = functools.partial(tiny, 2 * _b + _dx, 2 * _b + _dy,
                                                                                   _iso, _b)


# --------------------------------------------------------------------------------------------------- moments scenes
def gaussians(nx, ny, items, base=0.0):
    """float64 frame: ``base`` plus, for every (cx, cy, peak, fwhm), a pixel-centre sampled circular Gaussian."""
    y, x = np.mgrid[:ny, :nx]
    img = np.full((ny, nx), base, np.float64)
    for cx, cy, amp, fwhm in items:
        s = fwhm / K_FWHM
        img += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * s * s))
    return img


def _starts(items):
    return (np.array([int(round(c[0])) for c in items], np.int32),
            np.array([int(round(c[1])) for c in items], np.int32))


INTERIOR = [(30.31, 28.77, 9000.0, 1.7), (71.0, 30.0, 7000.0, 2.5), (109.62, 31.43, 8000.0, 4.2),
            (40.18, 75.66, 6000.0, 8.0), (90.61, 72.24, 5000.0, 2.5), (120.45, 80.87, 4000.0, 1.7)]


def stars_interior():
    """150 x 110, half 10: stars of FWHM 1.7, 2.5, 4.2 and 8 well inside the frame, started on their peak pixel; the
    last two are started one pixel off it, along x and along y."""
    img = gaussians(150, 110, INTERIOR).astype(np.float32)
    x, y = _starts(INTERIOR)
    x[4] += 1
    y[5] -= 1
    return Moments(img, x, y, 10)


EDGE = [(2.31, 35.64, 9000.0, 1.7), (87.42, 33.17, 7000.0, 2.5), (45.28, 1.83, 8000.0, 4.2),
        (44.63, 67.71, 6000.0, 8.0), (1.72, 2.39, 5000.0, 2.5), (88.19, 1.34, 5500.0, 4.2),
        (2.58, 68.12, 6500.0, 8.0), (87.66, 67.41, 7500.0, 1.7)]


def stars_clipped():
    """90 x 70, half 10: a star at each edge and in each corner, within 3 px of it, so that the window loses up to
    8 columns, 8 rows, or both."""
    img = gaussians(90, 70, EDGE).astype(np.float32)
    x, y = _starts(EDGE)
    return Moments(img, x, y, 10)


def stars_outside():
    """The frame of ``stars_clipped`` on a pedestal of 20, with start pixels outside it: windows that still hold a
    star (they find it, through a window that is not the one of ``stars_clipped``), windows that touch the frame with
    one column or row of the pedestal (x or y does not vary: a finite answer from the other axis, after 25 rounds),
    and windows with no pixel at all, up to 10^6 px away (NaN, the centroid is the start pixel).  No window holds one
    column of a star: that is the chaotic regime.  None holds a single pixel away from the start either: whether
    ``(w i) / w`` gives back ``i`` to the last bit, and with it whether ``m2`` is 0 or 1e-30, hangs on the last bit
    of the exponential."""
    img = gaussians(90, 70, EDGE, base=20.0).astype(np.float32)
    pos = [(-1, 35), (-4, 36), (-10, 20), (-11, 36), (90, 33), (93, 33), (99, 50), (100, 33), (45, -2), (20, -10),
           (45, -11), (44, 70), (44, 79), (70, 79), (44, 80), (-3, -2), (-11, -11), (92, 72),
           (100, 80), (-1000000, 35), (1000000, 35), (45, -1000000), (45, 1000000), (-1000000, 1000000),
           (1000000, -1000000)]
    return Moments(img, np.array([p[0] for p in pos], np.int32), np.array([p[1] for p in pos], np.int32), 10)


def flat(half):
    """A constant 44 x 34 frame: the answer is a function of the window alone (FWHM 4.186 for the full window at
    half = 2), so a window that loses or gains a pixel shows in the first digits.  Started in the interior, at every
    edge and in every corner, and one pixel inside each of them."""
    nx, ny = 44, 34
    img = np.full((ny, nx), 100.0, np.float32)
    pos = [(20, 15), (0, 15), (nx - 1, 16), (21, 0), (22, ny - 1), (0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1),
           (1, 14), (nx - 2, 1), (2, ny - 2)]
    return Moments(img, np.array([p[0] for p in pos], np.int32), np.array([p[1] for p in pos], np.int32), half)


def broad(half):
    """A frame of 3 half + 40 by 3 half + 20 pixels with Gaussians of FWHM 1.18 half (sigma = half / 2): one whose
    window is whole, one at the left edge, and one 1.4 times as wide in the far corner.  The weight at the window's corner is above 1e-3,
    so every pixel of the (2 half + 1)^2 window counts: 3969, 4225 and 16641 of them, 63, 67 and 261 per lane."""
    nx, ny = 3 * half + 40, 3 * half + 20
    f = 1.18 * half
    items = [(half + 8.37, half + 4.71, 5000.0, f), (3.24, 2 * half + 9.58, 4000.0, f),
             (nx - 4.46, ny - 2.81, 3000.0, 1.4 * f)]
    img = gaussians(nx, ny, items).astype(np.float32)
    x, y = _starts(items)
    return Moments(img, x, y, half)


def exits():
    """130 x 100, half 10, on a zero background:

    0. a single hot pixel: ``m2`` = 0 in round 1, NaN, the centroid is the pixel;
    1. a negative star: ``s0`` < 0 in round 1, NaN, the centroid is the start pixel;
    2. an empty window: ``s0`` = 0;
    3. +1000 and -980 two pixels apart, started between them: ``s0`` > 0 sends the centroid 99 px away, to x = 1,
       where every weight underflows: ``t0`` = 0, NaN, and that far centroid is reported;
    4. a bowl that rises from its middle (100 + r^2 / 2): the measured second moment exceeds the weight's, ``inv`` < 0
       in round 1, NaN;
    5. a star with a NaN pixel at the corner of its window: ``s0`` is NaN;
    6. a star with a +inf pixel in its window: the centroid is inf / inf, everything is NaN;
    7. two equal stars of FWHM 2.5, 5 px apart, started on the left one: the criterion is met in round 25, the last
       one there is;
    8. a faint star of FWHM 2.5 in a bowl that rises around it (2 r^2): two rounds measure the star, the weight
       widens, the bowl takes over and ``inv`` turns negative in round 3: the width of round 2 is kept;
    9. the pair of 7, 4 px apart: the weight widens to hold both and creeps to its fixed point (steps of 3e-6 when
       round 25 ends it)."""
    nx, ny = 130, 100
    img = np.zeros((ny, nx), np.float64)
    yy, xx = np.mgrid[:ny, :nx]
    img[15, 15] = 1000.0
    img -= gaussians(nx, ny, [(45.3, 15.6, 3000.0, 2.5)])
    img[15, 99], img[15, 101] = 1000.0, -980.0
    r2 = (xx - 20) ** 2 + (yy - 50) ** 2
    img[r2 <= 15 ** 2 * 2] = (100.0 + 0.5 * r2)[r2 <= 15 ** 2 * 2]
    img += gaussians(nx, ny, [(60.4, 50.7, 4000.0, 2.5), (95.3, 50.2, 4000.0, 2.5)])
    img[61, 70] = np.nan
    img[47, 98] = np.inf
    img += gaussians(nx, ny, [(25.3, 84.6, 3000.0, 2.5), (30.3, 84.6, 3000.0, 2.5)])
    box = (np.abs(xx - 70) <= 14) & (np.abs(yy - 82) <= 14)
    r2 = (xx - 70.3) ** 2 + (yy - 82.4) ** 2
    img[box] += (2.0 * r2)[box]
    img += gaussians(nx, ny, [(70.3, 82.4, 300.0, 2.5)])
    img += gaussians(nx, ny, [(105.3, 84.6, 3000.0, 2.5), (109.3, 84.6, 3000.0, 2.5)])
    pos = [(15, 15), (45, 16), (75, 15), (100, 15), (20, 50), (60, 51), (95, 50), (25, 85), (70, 82), (105, 85)]
    return Moments(img.astype(np.float32), np.array([p[0] for p in pos], np.int32),
                   np.array([p[1] for p in pos], np.int32), 10)


EXITS_WANT = ('m2', 's0', 's0', 't0', 'inv', 's0', 't0', 'done', 'inv', 'cap')

MOMENTS = {'stars-interior': stars_interior, 'stars-clipped': stars_clipped, 'stars-outside': stars_outside,
           'exits': exits}
for _h in (2, 3, 10):
    MOMENTS[f'flat-half{_h}'] = functools.partial(flat, _h)
for _h in (31, 32, 64):
    MOMENTS[f'broad-half{_h}'] = functools.partial(broad, _h)
# the scenes that are there for the extent of the window (the corner-weight precondition holds on their finite stars)
WINDOW_SCENES = tuple(k for k in MOMENTS if k.startswith(('flat', 'broad')))


class Trace(NamedTuple):
    fwhm: float
    cx: float
    cy: float
    exit: str             # 'done', 'cap', 's0', 't0', 'm2' or 'inv'
    rounds: int           # rounds begun
    steps: tuple          # |ns2 - s2| / ns2 of every round that got that far
    margin: float         # of the deciding sum at an exit through s0 / t0 / m2 / inv (inf: exactly 0, or not finite)
    s2: float             # the last weight sigma^2
    corner: float         # weight of the clipped window's farthest corner relative to the centroid's, at the last s2


def trace(img, x, y, half=10, maxit=25):
    """``oracle.detect.star_fwhm`` once more, keeping a record of every round (the window is clipped to the frame and
    empty where it misses it).  ``tests/test_seeing_scenes.py`` holds its three numbers to the oracle's, bit for bit."""
    img = np.asarray(img, dtype=np.float64)
    ny, nx = img.shape
    j0, j1 = max(y - half, 0), min(y + half + 1, ny)
    i0, i1 = max(x - half, 0), min(x + half + 1, nx)
    j1, i1 = max(j1, j0), max(i1, i0)
    jj, ii = np.mgrid[j0:j1, i0:i1]
    I = img[j0:j1, i0:i1]
    cx, cy, s2 = float(x), float(y), 4.0
    out, why, steps, margin, it = np.nan, 'cap', [], np.nan, 0

    def rel(total, terms):
        if not np.isfinite(total) or total == 0:
            return np.inf
        return abs(total) / np.abs(terms).sum()

    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for it in range(1, maxit + 1):
            w = np.exp(-0.5 * ((ii - cx) ** 2 + (jj - cy) ** 2) / s2) * I
            s0 = w.sum()
            if not s0 > 0:
                why, margin = 's0', rel(s0, w)
                break
            cx, cy = (w * ii).sum() / s0, (w * jj).sum() / s0
            w = np.exp(-0.5 * ((ii - cx) ** 2 + (jj - cy) ** 2) / s2) * I
            t0 = w.sum()
            if not t0 > 0:
                why, margin = 't0', rel(t0, w)
                break
            m2 = 0.5 * ((w * (ii - cx) ** 2).sum() + (w * (jj - cy) ** 2).sum()) / t0
            if not m2 > 0:
                why, margin = 'm2', rel(m2, m2 if m2 != 0 else 1.0)
                break
            inv = 1.0 / m2 - 1.0 / s2
            if not inv > 0:
                why, margin = 'inv', rel(inv, 1.0 / s2)
                break
            ns2 = 1.0 / inv
            steps.append(abs(ns2 - s2) / ns2)
            done = abs(ns2 - s2) <= 1e-8 * ns2
            s2 = ns2
            out = K_FWHM * np.sqrt(s2)
            if done:
                why = 'done'
                break
        corner = np.nan
        if I.size:      # the corner of the clipped window that is farthest from the centroid
            far = max((c - cx) ** 2 for c in (i0, i1 - 1)) + max((c - cy) ** 2 for c in (j0, j1 - 1))
            corner = float(np.exp(-0.5 * far / s2))
    return Trace(out, cx, cy, why, it, tuple(steps), margin, s2, corner)


def stop_round_is_safe(t):
    """The stop-round precondition on one trace (module docstring)."""
    return not any(0.99e-8 <= s <= 1.01e-8 for s in t.steps)


def is_tame(t):
    """No step after the second one reaches 1: in the chaotic regime they run to 1e+1 .. 1e+24."""
    return all(s < 1.0 for s in t.steps[2:])


def exit_is_safe(t):
    return t.exit in ('done', 'cap') or t.margin >= 1e-6


# ------------------------------------------------------------------------------------------------ end-to-end fields
TRUTH = 2.4


def lattice_field():
    """260 x 260: a 19 x 19 lattice of stars of FWHM 2.4, 12 px apart, 361 in all - more than ``NMAX`` = 300 - with
    sub-pixel offsets and distinct heights (peaks 400 .. 20000), on a sloped background with noise 3; a bad block over
    four stars and a saturated blob on a fifth.  Returns (img, bad, saturate)."""
    rng = np.random.default_rng(41)
    n = 260
    gx, gy = np.meshgrid(22 + 12 * np.arange(19), 22 + 12 * np.arange(19))
    cx = gx.ravel() + rng.uniform(-0.4, 0.4, 361)
    cy = gy.ravel() + rng.uniform(-0.4, 0.4, 361)
    peak = rng.permutation(np.geomspace(400.0, 20000.0, 361))
    img = gaussians(n, n, list(zip(cx, cy, peak, np.full(361, TRUTH))))
    yy, xx = np.mgrid[:n, :n]
    img += 150.0 + 0.05 * xx + 0.03 * yy + rng.normal(0.0, 3.0, (n, n))
    bad = np.zeros((n, n), bool)
    bad[88:104, 112:128] = True
    img[200:207, 140:147] = 60000.0
    return img.astype(np.float32), bad, 50000.0


def sparse_field(equal=False):
    """200 x 180: 30 stars of FWHM 2.4 on a flat background of 100 with noise 2, peaks 1500 .. 12000 (distinct), for
    the loop that doubles the threshold when the list is full; ``equal``: every star on a pixel centre with a peak of 5500 instead,
    so that no threshold keeps a part of them (the thresholds are 30 noise sigmas times a power of two: some 3840,
    then 7680)."""
    rng = np.random.default_rng(43)
    nx, ny = 200, 180
    gx, gy = np.meshgrid(25 + 30 * np.arange(6), 25 + 30 * np.arange(5))
    cx = gx.ravel() + rng.uniform(-0.4, 0.4, 30)
    cy = gy.ravel() + rng.uniform(-0.4, 0.4, 30)
    peak = rng.permutation(np.geomspace(1500.0, 12000.0, 30))
    if equal:
        cx, cy, peak = gx.ravel().astype(np.float64), gy.ravel().astype(np.float64), np.full(30, 5500.0)
    img = gaussians(nx, ny, list(zip(cx, cy, peak, np.full(30, TRUTH))))
    img += 100.0 + rng.normal(0.0, 2.0, (ny, nx))
    return img.astype(np.float32)


# ------------------------------------------------------------------------------------------------------ tolerances
# tests/measure_seeing_tolerance.py: against 50 digits the float64 oracle is off by at most 2.69e-15 (FWHM, relative)
# and 8.89e-13 px (centroid) on the moments scenes above.  8 x that, rounded up to one digit; the ceilings are the
# suite's rtol 1e-9 / atol 1e-8 (tests/test_detect_gpu.py), which hold under the stop-round precondition alone.
RTOL_FW = 3e-14
ATOL_C = 8e-12
