"""Scenes for the stack-combine kernels with a stated census (numpy only, no GPU).

A scene is ``Scene(vals, wgts, clip_sigma, clip_ampfrac)``: float32 arrays of shape ``(n, npix)``
and the two parameters of COMBINE_TYPE CLIPPED it is meant for.  Everything that is said about a
scene here is said from ``oracle/combine.py`` in float64 (``census``); ``tests/test_combine_scenes.py``
asserts it, ``tests/test_combine_gpu.py`` runs the scenes through the kernels.

Valid counts.  Pixel p has exactly ``p % (n + 1)`` valid samples, at frames drawn at random per
pixel; ``npix = max(2 (n + 1) + 3, 515)`` (more than one 256-thread block, a ragged last wave at
every lane layout), so every count 0 .. n occurs at least twice, and at different lanes of a wave
where several lanes share a pixel.  An invalid sample carries weight 0, a negative weight or NaN by
turns, and the finite poison +-1e30 as its value.

Clip scenes.  Weights are log-uniform over 1e-4 .. 1e4.  Every pixel gets a target median m: the
centre of the parameter set itself in the even cycles of the count (p // (n + 1) even), the centre
moved by up to 5 % (of max(|centre|, 1)) in the odd ones, so that medians of both signs and exact
zeros occur.  With thr_i = clip_sigma / sqrt(w_i) + clip_ampfrac |m| the valid samples are placed
at ``m +- r thr_i``, r drawn from R_SET (the two values next to 1 with probability 1/4 each, the
others 1/10), half of them on either side of m so that m IS the median: an odd count has one sample
at m, an even count has its middle pair at m -+ h, h = r thr of the first of the two, and no other
sample closer to m than h.  A threshold that is wrong by 1e-3 therefore moves samples across it at
every count >= 2.

Margin.  No valid sample may have ``| |v - med| - thr | < 2^-18 (|v| + |med| + thr)`` (med, thr:
the oracle's, float64).  An offender is moved to 1.01 thr, i.e. away from the median, the scene is
rebuilt and checked again; the generator raises when four passes do not settle it.  (The kernel's
comparison is off by less than 5 x 2^-24 of that envelope: one rounding of |v - med|, one of the
median, an rsqrt within 2 ulp, one product, one sum.)  The tie scenes keep their values and move
the weight of an offender by 5 % instead.  The on-boundary scene is exempt by construction.
"""
import functools
from typing import NamedTuple

import numpy as np

from oracle import combine as ocombine

R_SET = np.array([0.0, 0.3, 0.9, 1 - 2.0 ** -10, 1 + 2.0 ** -10, 1.1, 3.0])
R_PROB = np.array([0.1, 0.1, 0.1, 0.25, 0.25, 0.1, 0.1])
# (clip_sigma, clip_ampfrac, centre)
PARAM_SETS = ((4.0, 0.3, 100.0),       # the reference's science coadds
              (4.0, 0.3, -100.0),      # |med|
              (2.5, 0.0, 7.0),         # the sigma term alone
              (0.0, 0.5, 33.0),        # the amplitude term alone
              (4.0, 0.3, 0.0))         # medians around and at zero
DEPTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512)
MARGIN = 2.0 ** -18
POISON = 1e30
TIE_KINDS = ('four', 'equal', 'zeros')


class Scene(NamedTuple):
    vals: np.ndarray
    wgts: np.ndarray
    clip_sigma: float
    clip_ampfrac: float


def npix_for(n):
    return max(2 * (n + 1) + 3, 515)


def lanes_per_pixel(n):
    """How many lanes of a wave share a pixel at depth n (zm_launch_combine)."""
    return 1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 8


def _validity(rng, n, npix):
    """(valid, role): pixel p has p % (n + 1) valid samples at random frames; role numbers them 0 .. count - 1 in
    random order."""
    count = np.arange(npix) % (n + 1)
    role = rng.random((n, npix)).argsort(axis=0).argsort(axis=0)
    return role < count[None], role, count


def _poison(valid, vals, wgts):
    """Invalid samples: weight 0 / negative / NaN by turns, value +-1e30 by turns."""
    n, npix = valid.shape
    turn = (np.arange(n)[:, None] + np.arange(npix)[None]) % 3
    bad_w = np.where(turn == 0, 0.0, np.where(turn == 1, -(wgts + 1.0), np.nan))
    sign = np.where((np.arange(n)[:, None] + np.arange(npix)[None] // 3) % 2 == 0, 1.0, -1.0)
    return (np.where(valid, vals, sign * POISON).astype(np.float32),
            np.where(valid, wgts, bad_w).astype(np.float32))


def census(scene):
    """What the oracle says about a scene (float64)."""
    v = scene.vals.astype(np.float64)
    w = scene.wgts.astype(np.float64)
    valid = w > 0
    med, nv = ocombine._median_valid(v, valid)
    with np.errstate(divide='ignore', invalid='ignore'):
        thr = np.where(valid, scene.clip_sigma * (1.0 / np.sqrt(np.where(valid, w, 1.0))), 0.0) + scene.clip_ampfrac * np.abs(med)[None]
        dist = np.abs(np.where(valid, v, 0.0) - med[None])
        rel = np.where(thr > 0, dist / np.where(thr > 0, thr, 1.0) - 1.0, np.inf)
    keep = valid & (dist <= thr)
    env = np.abs(np.where(valid, v, 0.0)) + np.abs(med)[None] + thr
    slack = np.where(valid, np.abs(dist - thr) - MARGIN * env, np.inf)
    nval = max(int(valid.sum()), 1)
    return dict(valid=valid, keep=keep, med=med, thr=thr, dist=dist, rel=rel, count=nv, slack=slack,
                min_margin=float(np.where(valid, np.abs(dist - thr) / np.where(env > 0, env, 1.0), np.inf).min()),
                rejected=float((valid & ~keep).sum()) / nval, kept=float(keep.sum()) / nval,
                near_in=float((valid & (rel <= 0) & (rel > -2e-3)).sum()) / nval,
                near_out=float((valid & (rel > 0) & (rel < 2e-3)).sum()) / nval)


def _frozen(scene):
    scene.vals.setflags(write=False)
    scene.wgts.setflags(write=False)
    return scene


@functools.lru_cache(maxsize=None)
def clip_scene(n, clip_sigma, clip_ampfrac, center, seed=0, npix=None):
    """Built once per argument set and shared between the tests, read-only."""
    npix = npix_for(n) if npix is None else npix
    rng = np.random.default_rng([seed, n, npix])
    valid, role, count = _validity(rng, n, npix)
    even = (count % 2 == 0)[None]
    w = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), (n, npix))).astype(np.float32).astype(np.float64)
    exact = ((np.arange(npix) // (n + 1)) % 2 == 0)
    m = np.where(exact, center, center + 0.05 * max(abs(center), 1.0) * rng.uniform(-1, 1, npix))
    m = m.astype(np.float32).astype(np.float64)
    # side of the median: even count - roles 0, 2, .. below, 1, 3, .. above; odd count - role 0 at m, 1, 3, .. below
    side = np.where(even, np.where(role % 2 == 0, -1.0, 1.0),
                    np.where(role == 0, 0.0, np.where(role % 2 == 1, -1.0, 1.0)))
    thr = clip_sigma / np.sqrt(w) + clip_ampfrac * np.abs(m)[None]
    d = rng.choice(R_SET, (n, npix), p=R_PROB) * thr

    def build(d):
        h = np.where(valid & even & (role == 0), d, 0.0).sum(axis=0)           # half gap of the middle pair
        dd = np.where(even, np.where(role <= 1, h[None], np.maximum(d, h[None])), d)
        vals, wgts = _poison(valid, m[None] + side * dd, w)
        return Scene(vals, wgts, float(clip_sigma), float(clip_ampfrac))

    for _ in range(4):
        scene = build(d)
        c = census(scene)
        bad = c['slack'] < 0
        if not bad.any():
            return _frozen(scene)
        if (bad & (side == 0)).any():
            raise RuntimeError('clip_scene: a sample at the median sits on the threshold (threshold 0)')
        d = np.where(bad, 1.01 * c['thr'], d)
        # the second sample of a middle pair sits at the first one's distance: move the pair
        pair = np.where(bad & even & (role == 1), 1.01 * c['thr'], 0.0).max(axis=0)
        d = np.where(even & (role == 0) & (pair[None] > 0), pair[None], d)
    raise RuntimeError(f'clip_scene(n={n}, {clip_sigma}, {clip_ampfrac}, {center}): margin repair does not settle')


@functools.lru_cache(maxsize=None)
def tie_scene(n, kind, seed=0, clip_sigma=4.0, clip_ampfrac=0.3, npix=None):
    """Repeated values under the same cycle of valid counts: 'four' - values from {0, 1, 2, 3}; 'equal' - one
    value; 'zeros' - values from {-0.0, +0.0, 1}."""
    npix = npix_for(n) if npix is None else npix
    rng = np.random.default_rng([seed, n, npix, TIE_KINDS.index(kind)])
    valid, role, count = _validity(rng, n, npix)
    pool = {'four': [0.0, 1.0, 2.0, 3.0], 'equal': [42.5], 'zeros': [-0.0, 0.0, 1.0]}[kind]
    v = rng.choice(np.array(pool), (n, npix))
    w = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), (n, npix))).astype(np.float32).astype(np.float64)
    for _ in range(4):
        vals, wgts = _poison(valid, v, w)
        scene = Scene(vals, wgts, float(clip_sigma), float(clip_ampfrac))
        bad = census(scene)['slack'] < 0
        if not bad.any():
            return _frozen(scene)
        w = np.where(bad, w * 1.05, w).astype(np.float32).astype(np.float64)
    raise RuntimeError(f'tie_scene(n={n}, {kind}): margin repair does not settle')


def boundary_scene(n, npix=67):
    """|v - med| == thr in exactly representable numbers: every weight 1/16, clip_sigma 4, ampfrac 0.25, every
    sample 64 but one per pixel (frame p % n) at 96 (even pixels) or 32 (odd pixels): med = 64 for n >= 3,
    thr = 4 * 4 + 0.25 * 64 = 32 = |v - med|.  The oracle keeps the sample (<=)."""
    assert n >= 3
    vals = np.full((n, npix), 64.0, np.float32)
    p = np.arange(npix)
    vals[p % n, p] = np.where(p % 2 == 0, 96.0, 32.0)
    return Scene(vals, np.full((n, npix), 1 / 16.0, np.float32), 4.0, 0.25)


def clipped_strict(scene):
    """The oracle's CLIPPED with '<' in place of '<=' (what a kernel that drops the on-boundary sample computes)."""
    v = scene.vals.astype(np.float64)
    w = scene.wgts.astype(np.float64)
    c = census(scene)
    keep = c['valid'] & (c['dist'] < c['thr'])
    s0 = np.where(keep, w, 0.0).sum(axis=0)
    s1 = np.where(keep, w * v, 0.0).sum(axis=0)
    return np.where(s0 > 0, s1 / np.where(s0 > 0, s0, 1.0), 0.0), s0


def scaled(scene, k):
    """Values times 2^k, weights times 2^-2k: every operation of the combine commutes with it."""
    return Scene(np.ldexp(scene.vals, k).astype(np.float32), np.ldexp(scene.wgts, -2 * k).astype(np.float32),
                 scene.clip_sigma, scene.clip_ampfrac)


def reference(scene, kind):
    """(value, weight, value bound, weight bound) from the oracle in float64.

    weight: |g - r| <= n 2^-24 r (n - 1 roundings of positive terms in any order).  value (CLIPPED, WEIGHTED,
    AVERAGE): |g - r| <= (n + 3) 2^-24 sum_kept(w |v|) / sum_kept(w) - two fp32 sums of n terms, the rounding of
    the fp32 median that feeds the threshold, the division; kept = the oracle's keep set (CLIPPED) or the valid
    set, w = 1 for AVERAGE.  MEDIAN has no value bound: it is compared bit for bit."""
    n = scene.vals.shape[0]
    v = scene.vals.astype(np.float64)
    w = scene.wgts.astype(np.float64)
    val, wgt, _ = ocombine.combine(scene.vals, scene.wgts, kind, scene.clip_sigma, scene.clip_ampfrac)
    if kind == 'MEDIAN':
        return val, wgt, None, n * 2.0 ** -24 * wgt
    kept = census(scene)['keep'] if kind == 'CLIPPED' else w > 0
    ww = np.where(kept, 1.0 if kind == 'AVERAGE' else np.where(kept, w, 0.0), 0.0)
    s0 = ww.sum(axis=0)
    env = np.where(s0 > 0, (ww * np.abs(np.where(kept, v, 0.0))).sum(axis=0) / np.where(s0 > 0, s0, 1.0), 0.0)
    return val, wgt, (n + 3) * 2.0 ** -24 * env, n * 2.0 ** -24 * wgt
