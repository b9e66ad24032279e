"""Scenes for the CLEAN tests: the smallest inputs at which each part of the operator can go wrong.

Test infrastructure.  Every scene is (img, sigma, keyword arguments of the extraction, which may carry a ``bad`` and a
``flag`` plane).  The scenes of ``PLANES`` are those of tests/deblend_scenes.py at the frame's edges and with bad, flagged
and non-finite pixels, and two of their own (``shred``, ``shred_corner``).  Moffat sources are ``amp (1 + r^2 / w^2)^-b``
with ``w = fwhm / (2 sqrt(2^(1/b) - 1))``, centres 0-based, noise ``default_rng(seed).normal``.  ``reference(name, ...)`` computes the numpy restatement once per process.
"""
import functools

import numpy as np

import clean_ref as cr
import deblend_scenes as ds


def moffats(nx, ny, items):
    y, x = np.mgrid[:ny, :nx]
    img = np.zeros((ny, nx), np.float64)
    for cx, cy, amp, fwhm, b in items:
        w = fwhm / (2.0 * np.sqrt(2.0 ** (1.0 / b) - 1.0))
        img += amp * (1.0 + ((x - cx) ** 2 + (y - cy) ** 2) / (w * w)) ** -b
    return img


HALO_SOURCES = [(80.3, 79.6, 600.0, 12.0, 1.5), (125.4, 40.7, 120.0, 2.8, 2.5), (30.2, 120.9, 40.0, 2.8, 2.5)]


def halo(seed):
    """160 x 160, noise 4: a compact galaxy and two real stars; the noise bumps on the galaxy's halo are what CLEAN folds
    back, the galaxy and both stars are what it keeps."""
    img = moffats(160, 160, HALO_SOURCES) + np.random.default_rng(seed).normal(0.0, 4.0, (160, 160))
    return img.astype(np.float32), np.full((160, 160), 4.0, np.float32), {}


def halo_pair():
    """``halo(2)`` with a pair of stars 6 px apart: deblending splits the pair (FLAGS bit 2, one PARENT_NUMBER), CLEAN
    folds the halo's bumps and leaves both members of the pair alone: neither star is the other's shred."""
    pair = [(40.0, 38.0, 300.0, 2.8, 2.5), (46.0, 38.0, 220.0, 2.8, 2.5)]
    img = moffats(160, 160, HALO_SOURCES + pair) + np.random.default_rng(2).normal(0.0, 4.0, (160, 160))
    return img.astype(np.float32), np.full((160, 160), 4.0, np.float32), {}


def stars40():
    """256 x 256, noise 2: 40 stars with Moffat wings, amplitudes 10^U(1.5, 4.3).  Stars are not each other's shreds:
    nothing is absorbed."""
    rng = np.random.default_rng(5)
    x, y = rng.uniform(8, 248, 40), rng.uniform(8, 248, 40)
    amp = 10 ** rng.uniform(1.5, 4.3, 40)
    img = moffats(256, 256, [(a, b, c, 2.8, 2.5) for a, b, c in zip(x, y, amp)]) + rng.normal(0.0, 2.0, (256, 256))
    return img.astype(np.float32), np.full((256, 256), 2.0, np.float32), {}


def two_equal():
    """The same 41 x 41 float32 stamp of one star pasted twice, 44 px apart, no noise: the two objects are translates of
    each other, so their F are equal to the last bit (the smaller NUMBER counts as the larger), and neither explains the
    other."""
    stamp = moffats(41, 41, [(20.0, 20.0, 500.0, 2.8, 2.5)]).astype(np.float32)
    img = np.zeros((64, 128), np.float32)
    img[12:53, 20:61] = stamp
    img[12:53, 64:105] = stamp
    return img, np.ones((64, 128), np.float32), {}


def shapes(k):
    """No filter, DETECT_MINAREA = k, a noise plane that varies from pixel to pixel (so f - t orders otherwise than f): an
    object of exactly k pixels, a plateau (all f equal: m is a tie of every member), an object whose box is 40 x 36 (beyond
    one round of the 256 lanes and beyond 32 x 32) and a diagonal of 2 k pixels with repeated values."""
    img = np.zeros((64, 96), np.float32)
    y, x = np.mgrid[:64, :96]
    sigma = (1.0 + 0.25 * ((x + 2 * y) % 3)).astype(np.float32)
    img[2, 3:3 + k] = 20.0 + 3.0 * np.arange(k)
    img[8:14, 4:10] = 50.0
    img[20:56, 30:70] = (30.0 + 0.37 * ((x[20:56, 30:70] * 7 + y[20:56, 30:70] * 13) % 41) + 0.011 * x[20:56, 30:70]).astype(np.float32)
    for i in range(2 * k):
        img[2 + i, 94 - i] = 40.0 + (i % 3)
    return img, sigma, dict(filter=False, detect_minarea=k)


def shred(cx, cy):
    """48 x 48, no filter: a blend of two stars (2000 at (cx, cy), 1500 6 px below it), a 3 x 3 hole of bad pixels in the
    first one's wing 7 .. 9 px to its right, and beside the hole, cut off from the star by it, a shred of 3 x 2 pixels at
    1.75 (0.25 above the threshold).  Deblending at nthresh 32 splits the blend; CLEAN folds the shred into the first
    star, which then borders the hole on both sides.  ``shred(4, 4)`` sits in the frame's corner."""
    img = ds.gaussians(48, 48, [(cx, cy, 2000.0, 2.0), (cx, cy + 6, 1500.0, 2.0)]).astype(np.float32)
    bad = np.zeros((48, 48), np.uint8)
    bad[cy - 1:cy + 2, cx + 7:cx + 10] = 1
    img[cy - 1:cy + 2, cx + 10:cx + 12] = 1.75
    return img, np.ones((48, 48), np.float32), dict(filter=False, bad=bad)


SHREDS = {'shred': lambda: shred(20, 20), 'shred_corner': lambda: shred(4, 4)}
# the scenes with edges, bad pixels, flags and poison: each runs deblended at nthresh 32 and at nthresh 8
PLANES = list(ds.EDGE_SCENES) + list(ds.BAD_SCENES) + list(ds.POISON_SCENES) + list(SHREDS)
PLANES_NTHRESH = (32, 8)

SCENES = {**{name: (lambda name=name: ds.scene(name)) for name in PLANES if name not in SHREDS}, **SHREDS,
          'halo1': lambda: halo(1), 'halo2': lambda: halo(2), 'halo3': lambda: halo(3), 'halo_pair': halo_pair, 'stars40': stars40,
          'two_equal': two_equal, 'shapes1': lambda: shapes(1), 'shapes5': lambda: shapes(5), 'shapes9': lambda: shapes(9),
          'noisy_field': ds.noisy_field}
# the scenes whose full call is compared with the restatement bit for bit: test_clean_ref.py checks their gap
BITWISE = [(name, db) for name in ('halo1', 'halo2', 'halo3') for db in (False, True)] + [('noisy_field', True),
                                                                                    ('halo_pair', False), ('halo_pair', True)]


@functools.lru_cache(maxsize=None)
def scene(name):
    img, sigma, kw = SCENES[name]()
    for a in (img, sigma, kw.get('bad'), kw.get('flag')):
        if a is not None:
            a.setflags(write=False)
    return img, sigma, kw


def ref_kw(kw):
    return dict(detect_thresh=kw.get('detect_thresh', 1.5), detect_minarea=kw.get('detect_minarea', 5),
                use_filter=kw.get('filter', True), satur_level=kw.get('satur_level', 50000.0),
                aper_radius=kw.get('aper_radius', 3.0))


@functools.lru_cache(maxsize=None)
def reference(name, deblend=False, param=1.0, reverse=False):
    """``deblend``: False, True (nthresh 32) or another nthresh."""
    img, sigma, kw = scene(name)
    db = dict(nthresh=32 if deblend is True else int(deblend), mincont=0.005) if deblend else None
    return cr.clean(img, sigma, kw.get('bad'), kw.get('flag'), param=param, deblend=db, reverse=reverse, **ref_kw(kw))


TABLE_SIZES = (1, 2, 255, 256, 257, 1000)               # either side of one tile of absorbers, and several tiles
TABLE_SEED = 100


def random_table(n, seed, size=512.0):
    """A synthetic table of n rows in a size x size area (rows, F, T, m): a few bright extended objects among many faint
    compact ones, so that some are absorbed and chains form."""
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, cr.ROW)
    rows['number'] = np.arange(1, n + 1)
    rows['x_image'], rows['y_image'] = rng.uniform(1, size, n), rng.uniform(1, size, n)
    big = rng.random(n) < 0.1
    a = np.where(big, rng.uniform(3.0, 8.0, n), rng.uniform(0.6, 1.5, n))
    b = a * rng.uniform(0.5, 1.0, n)
    th = rng.uniform(-np.pi / 2, np.pi / 2, n)
    rows['x2'] = a * a * np.cos(th) ** 2 + b * b * np.sin(th) ** 2
    rows['y2'] = a * a * np.sin(th) ** 2 + b * b * np.cos(th) ** 2
    rows['xy'] = (a * a - b * b) * np.sin(th) * np.cos(th)
    rows['a_image'], rows['b_image'] = a, b
    rows['npix'] = np.maximum(5, (np.pi * a * b * rng.uniform(2.0, 4.0, n)).astype(np.int32))
    rows['first'] = rng.permutation(n).astype(np.int32)
    T = np.full(n, 6.0, np.float32)
    F = np.where(big, 10 ** rng.uniform(4.0, 6.0, n), 10 ** rng.uniform(1.8, 3.0, n)) * rows['npix'] / 10.0
    m = rng.uniform(0.5, 6.0, n).astype(np.float32)
    return rows, F, T, m
