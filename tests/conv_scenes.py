"""Scenes for the convolution of the subtraction (helpers, no tests).

``scene()`` of test_subtract_gpu.py blurs the template with an isotropic Gaussian and carries a constant template
noise of 0.5: the fitted kernel is symmetric up to noise, and the template's share of the noise plane is a hundredth
of the science's.  A convolution that reads its taps mirrored or transposed moves few pixels of such a difference
image, and no error in the variance plane moves any pixel of the noise image beyond the tolerance.

``asymmetric()`` has neither symmetry.  The science frame is the template convolved with a kernel that slides, along
x, from one elongated, rotated, off-centre Gaussian to another, and the template noise is 3.0 times a log-normal
factor drawn per pixel: every tap of K^2 meets another variance, and the template term of the noise plane is a fifth
of the science term instead of a two-hundredth. tests/test_conv_scenes.py proves on the CPU, with the oracle alone, that a mirrored, a transposed
and a shifted tap table each move most pixels of both products; tests/test_convolution_gpu.py runs the scenes through
every instance of the GPU convolution.

``case(hwk)``: the frame and the fit settings of kernel half width ``hwk``, sized so that the first column of regions
ends in a block one pixel wide and the region height leaves a block one row short.  ``oracle(hwk)`` is the oracle's
answer to it, computed once per process.
"""
import functools

import numpy as np
from scipy.ndimage import convolve

from oracle import hotpants as ohp
from test_subtract_gpu import COMMON
from util import synth

# (sigma_major, sigma_minor, angle / rad, dx, dy) of the two ends of the sliding kernel
KA = (1.3, 0.6, 0.5, +0.45, -0.30)
KB = (0.7, 1.2, -0.4, -0.30, +0.40)
KHW = 6                      # 13 x 13 taps

_subtract = ohp.subtract     # (the GPU tests put oracle() in its place for compare())


def skewed_gaussian(smaj, smin, angle, dx, dy, hw=KHW):
    """Unit-sum Gaussian on (2 hw + 1)^2 taps, indexed [v + hw, u + hw]: axes ``smaj`` along ``angle`` and ``smin``
    across it, centred on (dx, dy)."""
    v, u = np.mgrid[-hw:hw + 1, -hw:hw + 1].astype(np.float64)
    c, s = np.cos(angle), np.sin(angle)
    a = (u - dx) * c + (v - dy) * s
    b = -(u - dx) * s + (v - dy) * c
    k = np.exp(-0.5 * ((a / smaj) ** 2 + (b / smin) ** 2))
    return k / k.sum()


def asymmetric(nx, ny, seed, nstars=120, nbad=3):
    """(sci, srms, ref, rrms, bpm) like ``test_subtract_gpu.scene``: the same sky, stars, pixel noise and bad patches;
    science = 1.3 ((1 - t) ref (x) Ka + t ref (x) Kb) + 20 with t = x / (nx - 1); srms a constant 3.0;
    rrms = 3.0 exp(N(0, 0.5)) per pixel, from a generator of its own."""
    s = synth()
    rng = np.random.default_rng(seed)
    ref = np.full((ny, nx), 150.0)
    xs = rng.uniform(10, nx - 10, nstars)
    ys = rng.uniform(10, ny - 10, nstars)
    fl = np.exp(rng.uniform(np.log(3e3), np.log(8e4), nstars))
    s.add_stars(ref, xs, ys, fl, 2.0)
    a = convolve(ref, skewed_gaussian(*KA), mode='nearest')       # (true convolution, as the oracle's apply)
    b = convolve(ref, skewed_gaussian(*KB), mode='nearest')
    t = np.arange(nx, dtype=np.float64)[None, :] / (nx - 1.0)
    sci = 1.3 * ((1 - t) * a + t * b) + 20.0
    ref = ref + rng.normal(0, 0.5, ref.shape)
    sci = sci + rng.normal(0, 3.0, sci.shape)
    bpm = np.zeros((ny, nx), np.uint8)
    for _ in range(nbad):
        bx, by = rng.integers(20, nx - 20), rng.integers(20, ny - 20)
        bpm[by:by + 3, bx:bx + 3] = 1
    rrms = 3.0 * np.exp(np.random.default_rng(7919 + seed).normal(0.0, 0.5, (ny, nx)))
    return (sci.astype(np.float32), np.full((ny, nx), 3.0, np.float32), ref.astype(np.float32),
            rrms.astype(np.float32), bpm)


def settings(hwk, **over):
    kw = dict(r=hwk + 0.7, rss=2 * hwk + 1.2, nsx=3, nsy=3, nrx=2, nry=1, ko=1, bgo=1, **COMMON)
    kw.update(over)
    return kw


def reach(hwk):
    """Half width of the box a substamp centre keeps free: hwk + int(rss)."""
    return hwk + int(2 * hwk + 1.2)


def floor_size(hwk):
    hw = reach(hwk)
    return max(2 * hw + 200, 260), max(2 * hw + 180, 240)


def frame_size(hwk):
    """Smallest (nx, ny) at or above ``floor_size`` whose first region column (nrx = 2: nx // 2 wide) ends in a block
    one pixel wide and whose height leaves the last block row one row short."""
    step = 2 * hwk + 1
    nx, ny = floor_size(hwk)
    while (nx // 2) % step != 1:
        nx += 1
    while ny % step != step - 1:
        ny += 1
    return nx, ny


@functools.lru_cache(maxsize=None)
def case(hwk):
    nx, ny = frame_size(hwk)
    return asymmetric(nx, ny, seed=100 + hwk), settings(hwk)


def run(data, kw):
    sci, srms, ref, rrms, bpm = data
    return _subtract(sci, ref, srms, rrms, bpm, **kw)


@functools.lru_cache(maxsize=None)
def oracle(hwk):
    """(diff, noise, info) of oracle.hotpants.subtract on ``case(hwk)``; both forms of a half width share it."""
    return run(*case(hwk))


# ---- ragged and exact blocks: (name) -> region grid and the residues of the region sizes modulo the block ----------
# 'thirds': nrx = 3, nry = 2 on a width of 3 w + 1 and a height of 2 h + 1 with w and h multiples of the block: region
#           sizes of residue 0 and 1 on both axes, the last column and row of regions larger than the others (the launch
#           grid is sized by them; the workgroups beyond the smaller regions return early).
# 'halves': nrx = nry = 2 on 2 w + 1 by 2 h + 1 with w and h one short of a multiple: residues STEP - 1 and 0.
LAYOUTS = ('thirds', 'halves')


def layout_size(hwk, layout):
    step = 2 * hwk + 1
    hw = reach(hwk)
    # (a region of 2 hw + 70 or more on a side: the corner regions, which lose a border of hw to the substamp boxes,
    # still find the four stamps that a first-order kernel's three spatial terms need to be determined)
    side = -(-max(2 * hw + 70, 110) // step) * step
    if layout == 'thirds':
        return 3 * side + 1, 2 * side + 1, dict(nrx=3, nry=2, nsx=3, nsy=3)
    return 2 * side - 1, 2 * side - 1, dict(nrx=2, nry=2, nsx=3, nsy=3)


@functools.lru_cache(maxsize=None)
def ragged(hwk, layout):
    nx, ny, grid = layout_size(hwk, layout)
    return asymmetric(nx, ny, seed=200 + hwk, nstars=nx * ny // 350), settings(hwk, **grid)


def residues(nx, ny, kw):
    """Sets of (x1 - x0) % STEP and (y1 - y0) % STEP over the regions of a layout."""
    step = 2 * int(kw['r']) + 1
    regs = ohp.regions(nx, ny, kw['nrx'], kw['nry'])
    return {(r[1] - r[0]) % step for r in regs}, {(r[3] - r[2]) % step for r in regs}


@functools.lru_cache(maxsize=None)
def ragged_oracle(hwk, layout):
    return run(*ragged(hwk, layout))


# ---- non-finite template noise ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nonfinite(hwk=6):
    """``case(hwk)`` with NaN and +inf in ``rrms`` at a dozen good pixels: four within ``hwk`` of the boundary between
    the two regions, four within ``hwk`` of the frame edge (in the filled border or on its rim: the first unfilled
    pixels read them), four in the interior.  None lies in a substamp of any candidate centre (the
    noise maps enter the fit only through a stamp's mean variance; this scene is about the convolution)."""
    (sci, srms, ref, rrms, bpm), kw = case(hwk)
    ny, nx = ref.shape
    p = ohp.params(**kw)
    ok = ohp.valid_mask(sci.astype(np.float64), ref.astype(np.float64), bpm, p)
    taken = np.zeros((ny, nx), bool)
    for reg in ohp.regions(nx, ny, kw['nrx'], kw['nry']):
        for cands in ohp.find_substamps(ref.astype(np.float64), ok, reg, p):
            for cx, cy in cands:
                taken[cy, cx] = True
    free = ok & ~ohp.box_any(taken, int(kw['rss']))
    xb = nx // 2
    want = [(xb - 1, ny // 3), (xb, ny // 3 + 9), (xb - hwk, 2 * ny // 3), (xb + hwk - 1, ny // 2),
            (2, ny // 4), (nx - 1 - hwk, 3 * ny // 4), (nx // 4, hwk - 1), (3 * nx // 4, ny - 2),
            (nx // 5, ny // 2), (nx // 5 + 1, ny // 2), (4 * nx // 5, ny // 3), (nx // 3, 4 * ny // 5)]
    rrms = rrms.copy()
    for i, (x, y) in enumerate(want):
        while not free[y, x]:           # (slide down the column to a pixel outside every substamp)
            y += 1
        rrms[y, x] = np.nan if i % 2 == 0 else np.inf
    return (sci, srms, ref, rrms, bpm), kw


@functools.lru_cache(maxsize=None)
def nonfinite_oracle(hwk=6):
    return run(*nonfinite(hwk))


@functools.lru_cache(maxsize=None)
def normalized_oracle(hwk=6):
    data, kw = case(hwk)
    return run(data, dict(kw, normalize=1))


# ---- the wrong kernels of tests/test_conv_scenes.py -----------------------------------------------------------------
MUTATIONS = {
    'flip': lambda k: k[::-1, ::-1],
    'transpose': lambda k: k.T,
    'roll': lambda k: np.roll(k, 1, axis=1),
}


def moved(base, mutant, sci):
    """Fractions of the unfilled pixels of ``diff`` and of ``noise`` that differ between two oracle runs by more than
    ten times the limits of ``test_subtract_gpu.compare``."""
    (d0, n0, _), (d1, n1, _) = base, mutant
    good = d0 != 1e-30
    assert np.array_equal(good, d1 != 1e-30)
    s = sci.astype(np.float64)
    dlim = 1e-5 * (np.abs(s) + np.abs(s - d0)) + 1e-4
    nlim = 2e-5 * np.abs(n0) + 1e-5
    return (float((np.abs(d1 - d0) > 10 * dlim)[good].mean()), float((np.abs(n1 - n0) > 10 * nlim)[good].mean()))
