"""Scenes for the deblending tests: the smallest inputs at which each part of the operator can go wrong.

Test infrastructure.  Every scene is (img, sigma, keyword arguments of the extraction); no scene carries a non-finite
pixel.  ``reference(name)`` computes the numpy restatement once per process (forward and reversed member order).
"""
import functools

import numpy as np

import deblend_ref as dr


def gaussians(nx, ny, items, base=0.0):
    y, x = np.mgrid[:ny, :nx]
    img = np.full((ny, nx), base, np.float64)
    for cx, cy, amp, width in items:
        img += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * width * width))
    return img


def pair(sep):
    """48 x 48, sigma = 1: amplitudes 200 and 150, width 1.1, ``sep`` pixels apart."""
    img = gaussians(48, 48, [(20, 24, 200.0, 1.1), (20 + sep, 24, 150.0, 1.1)])
    return img.astype(np.float32), np.ones((48, 48), np.float32), {}


def contrast(amp):
    """A primary of amplitude 1000 and width 2.5 with a companion of width 1.1, 12 px away."""
    img = gaussians(64, 64, [(24, 32, 1000.0, 2.5), (36, 32, float(amp), 1.1)])
    return img.astype(np.float32), np.ones((64, 64), np.float32), {}


def nested():
    """Three peaks in one component at x = 20, 25 and 34: the split of the close two survives the merge with the third."""
    img = gaussians(64, 64, [(20, 32, 300.0, 1.3), (25, 32, 250.0, 1.3), (34, 32, 200.0, 1.3)])
    return img.astype(np.float32), np.ones((64, 64), np.float32), {}


def plateaus():
    """Two mesas of 50, 8 x 10 px each, joined by a 4-row bridge of 10; integers, no filter: every tie rule decides."""
    img = np.zeros((32, 48), np.float32)
    img[10:20, 6:14] = 50.0
    img[10:20, 30:38] = 50.0
    img[13:17, 14:30] = 10.0
    return img, np.ones_like(img), dict(filter=False)


def sigma_step():
    """A 2x step in sigma across a blend: T is the threshold at the peak pixel, level 0 is still the whole object."""
    img = gaussians(56, 40, [(22, 20, 400.0, 1.6), (31, 20, 300.0, 1.6)])
    sigma = np.ones((40, 56), np.float32)
    sigma[:, 27:] = 2.0
    return img.astype(np.float32), sigma, {}


def noisy_field():
    """128 x 128, 25 stars on noise 1, fixed seed; several land in one component.  One realisation of such a field: 15
    objects before and 20 after, three parents split, one of them in four.  (The prototype the issue quotes had its own
    seed and amplitudes, which are not recorded, and gave 18 -> 24 with one parent split in six; the difference is the
    scene's, the operator is the one stated.)"""
    rng = np.random.default_rng(20261019)
    x, y = rng.uniform(8, 120, 25), rng.uniform(8, 120, 25)
    amp = 10 ** rng.uniform(1.2, 2.8, 25)
    img = gaussians(128, 128, list(zip(x, y, amp, np.full(25, 1.4)))) + rng.normal(0.0, 1.0, (128, 128))
    return img.astype(np.float32), np.ones((128, 128), np.float32), {}


def lone_star():
    """Amplitude 5000 under noise 3 on 96 x 96: the noise on its wings must not shred it."""
    rng = np.random.default_rng(5)
    img = gaussians(96, 96, [(47.3, 48.6, 5000.0, 1.5)]) + rng.normal(0.0, 3.0, (96, 96))
    return img.astype(np.float32), np.full((96, 96), 3.0, np.float32), {}


def all_above():
    """512 x 512, every pixel above the threshold, two broad peaks: one object far beyond any LDS tile."""
    img = gaussians(512, 512, [(170, 250, 400.0, 40.0), (350, 260, 300.0, 40.0)], base=10.0)
    return img.astype(np.float32), np.ones((512, 512), np.float32), dict(filter=False)


def spiral_with_knots():
    """test_extract_gpu's spiral, a bright knot at either end of the arm: long chains, one leftover pixel per round."""
    from test_extract_gpu import spiral
    arm = spiral(512)
    img = np.where(arm, 100.0, 0.0).astype(np.float32)
    img[0, 0:40] = 20000.0                                # the outer end: the arm starts along the first row
    ys, xs = np.nonzero(arm[250:262, 250:262])            # the inner end: the arm's pixels at the centre
    img[250 + ys, 250 + xs] = 20000.0
    return img, np.ones_like(img), dict(filter=False)


def edge():
    """A blend that touches the frame's left and top edges."""
    img = gaussians(40, 32, [(1, 2, 300.0, 1.3), (8, 2, 250.0, 1.3)])
    return img.astype(np.float32), np.ones((32, 40), np.float32), {}


def just_too_small():
    """Two rows with two peaks each: 9 = 2 x minarea - 1 pixels (it cannot hold two branches of minarea pixels and is not
    examined) and 11 pixels (two branches of five around one low pixel: it splits at mincont 0)."""
    img = np.zeros((24, 40), np.float32)
    img[8, 4:13] = [90, 80, 70, 60, 6, 60, 70, 80, 90]
    img[16, 4:15] = [90, 80, 70, 60, 50, 6, 50, 60, 70, 80, 90]
    return img, np.ones_like(img), dict(filter=False, detect_minarea=5, mincont=0.0)


def box(width):
    """A 32-row block of ``width`` columns above the threshold with two peaks, no filter: the bounding box has exactly
    32 x width pixels (1024: the largest that the kernel keeps in LDS; 1056: the smallest that goes to global memory)."""
    img = np.zeros((48, 56), np.float32)
    img[8:40, 10:10 + width] = 10.0 + gaussians(width, 32, [(9, 15, 300.0, 2.0), (22, 17, 240.0, 2.0)])
    return img, np.ones_like(img), dict(filter=False)


SCENES = {'pair3': lambda: pair(3), 'pair4': lambda: pair(4), 'pair5': lambda: pair(5), 'pair6': lambda: pair(6),
          'pair8': lambda: pair(8), 'contrast20': lambda: contrast(20), 'contrast60': lambda: contrast(60),
          'nested': nested, 'plateaus': plateaus, 'sigma_step': sigma_step, 'noisy_field': noisy_field,
          'lone_star': lone_star, 'all_above': all_above, 'spiral_with_knots': spiral_with_knots, 'edge': edge,
          'just_too_small': just_too_small, 'box1024': lambda: box(32), 'box1056': lambda: box(33)}


@functools.lru_cache(maxsize=None)
def scene(name):
    img, sigma, kw = SCENES[name]()
    img.setflags(write=False)
    sigma.setflags(write=False)
    return img, sigma, kw


def split_kw(kw):
    """(extraction keywords, deblending keywords) of a scene's keyword arguments."""
    ex = {k: v for k, v in kw.items() if k not in ('nthresh', 'mincont')}
    db = {k: v for k, v in kw.items() if k in ('nthresh', 'mincont')}
    return ex, db


@functools.lru_cache(maxsize=None)
def reference(name, reverse=False):
    img, sigma, kw = scene(name)
    ex, db = split_kw(kw)
    ref_kw = dict(detect_thresh=ex.get('detect_thresh', 1.5), detect_minarea=ex.get('detect_minarea', 5),
                  use_filter=ex.get('filter', True), satur_level=ex.get('satur_level', 50000.0),
                  aper_radius=ex.get('aper_radius', 3.0))
    return dr.deblend(img, sigma, reverse=reverse, **db, **ref_kw)
