"""The scenes of tests/combine_scenes.py have the power they claim - from oracle/combine.py alone, no GPU.

What tests/test_combine_gpu.py can notice depends on what its scenes hold: every valid count, samples on both
sides of the clip threshold and close to it, a margin that keeps float32 rounding from deciding a sample, and a
result that moves when the threshold is wrong by 2^-8.  Depths 1 and 2 cannot hold all of it: a lone sample is its
own median and is never rejected, and two samples are equally far from theirs, so only the first of a pair can be
placed against its threshold.  The shares are asserted from n = 3 on; at n = 2 the perturbed thresholds must still
move some pixel.  The parameter set with centre 0 has medians of 0 and +-0.05: its amplitude term is (next to) zero
by design, so a wrong clip_ampfrac is looked for in the other sets.
"""
import numpy as np
import pytest

import combine_scenes as cs
from oracle import combine as ocombine


@pytest.mark.parametrize('n', cs.DEPTHS)
def test_every_valid_count_occurs_twice_and_on_different_lanes(n):
    sc = cs.clip_scene(n, *cs.PARAM_SETS[0])
    assert sc.vals.dtype == np.float32 and sc.wgts.dtype == np.float32 and sc.vals.shape == (n, cs.npix_for(n))
    c = cs.census(sc)
    assert np.array_equal(c['count'], np.arange(cs.npix_for(n)) % (n + 1))
    assert np.bincount(c['count'], minlength=n + 1).min() >= 2
    ppw = 64 // cs.lanes_per_pixel(n)                     # pixels per wave: pixel p sits at lane position p % ppw
    for k in range(n + 1):
        assert len(set(np.nonzero(c['count'] == k)[0] % ppw)) >= 2, k
    # the three kinds of invalid weight and the poison under them
    bad = ~c['valid']
    if n >= 3:
        assert (sc.wgts[bad] == 0).any() and (sc.wgts[bad] < 0).any() and np.isnan(sc.wgts[bad]).any()
    assert np.all(np.abs(sc.vals[bad]) == np.float32(cs.POISON)) and np.isfinite(sc.vals).all()
    if n >= 2:
        assert (sc.vals[bad] > 0).any() and (sc.vals[bad] < 0).any()
    w = sc.wgts[c['valid']]
    assert w.min() >= 0.99e-4 and w.max() <= 1.01e4
    if n >= 16:
        assert w.min() < 1e-3 and w.max() > 1e3


@pytest.mark.parametrize('params', cs.PARAM_SETS, ids=str)
@pytest.mark.parametrize('n', cs.DEPTHS)
def test_clip_scene_census(n, params):
    sigma, ampfrac, center = params
    sc = cs.clip_scene(n, *params)
    c = cs.census(sc)
    # the census is the oracle's: same survivors, same result
    val, wgt, nused = ocombine.combine(sc.vals, sc.wgts, 'CLIPPED', sigma, ampfrac)
    assert np.array_equal(nused, c['keep'].sum(axis=0))
    assert (c['slack'] >= 0).all() and c['min_margin'] >= cs.MARGIN
    if n >= 3:
        assert c['rejected'] >= 0.10 and c['kept'] >= 0.05
        assert c['near_in'] >= 0.05 and c['near_out'] >= 0.05
        assert ((c['count'] > 0) & (nused == 0)).any()              # pixels whose every sample is rejected
    has = c['count'] > 0
    if center < 0:
        assert (c['med'][has] < 0).all()
    if center == 0:
        assert (c['med'][has] == 0).any() and (c['med'][has] < 0).any() and (c['med'][has] > 0).any()
    # a threshold that is wrong by 2^-8 moves the result outside the bound the GPU test applies
    _, _, vbound, _ = cs.reference(sc, 'CLIPPED')
    for wrong in ([sc._replace(clip_sigma=sigma * (1 + 2.0 ** -8))] if sigma else []) + \
                 ([sc._replace(clip_ampfrac=ampfrac * (1 + 2.0 ** -8))] if ampfrac and center else []):
        moved = np.abs(cs.reference(wrong, 'CLIPPED')[0] - val) > vbound
        assert moved.mean() >= (0.05 if n >= 3 else 0.0), (n, params)
        if n == 2:
            assert moved.any()


@pytest.mark.parametrize('kind', cs.TIE_KINDS)
@pytest.mark.parametrize('n', cs.DEPTHS)
def test_tie_scene_census(n, kind):
    sc = cs.tie_scene(n, kind)
    c = cs.census(sc)
    assert np.array_equal(c['count'], np.arange(cs.npix_for(n)) % (n + 1))
    assert (c['slack'] >= 0).all()
    v = sc.vals[c['valid']]
    pool = {'four': [0, 1, 2, 3], 'equal': [42.5], 'zeros': [0, 1]}[kind]
    assert set(np.unique(v)) <= set(pool)
    if kind == 'zeros' and n >= 3:
        assert np.signbit(v[v == 0]).any() and (~np.signbit(v[v == 0])).any()
    if kind == 'four' and n >= 8:
        # repeated values at the middle of the sorted samples, and medians between two different ones
        assert (c['med'] % 1 == 0.5).any() and (c['med'] % 1 == 0).any()
        assert c['rejected'] > 0.02


@pytest.mark.parametrize('n', [d for d in cs.DEPTHS if d >= 3])
def test_on_boundary_scene_is_on_the_boundary(n):
    sc = cs.boundary_scene(n)
    c = cs.census(sc)
    on = c['dist'] == c['thr']
    assert (on.sum(axis=0) == 1).all() and (c['thr'] == 32).all() and (c['med'] == 64).all()
    val, wgt, nused = ocombine.combine(sc.vals, sc.wgts, 'CLIPPED', sc.clip_sigma, sc.clip_ampfrac)
    assert (nused == n).all() and (wgt == n / 16.0).all()              # the oracle keeps it: <=
    sval, swgt = cs.clipped_strict(sc)
    assert (swgt == (n - 1) / 16.0).all() and (sval == 64).all() and (sval != val).all()
    _, _, vbound, wbound = cs.reference(sc, 'CLIPPED')
    assert (np.abs(sval - val) > vbound).all() and (np.abs(swgt - wgt) > wbound).all()


def test_scaling_is_exact_in_the_oracle():
    sc = cs.clip_scene(5, *cs.PARAM_SETS[0])
    for k in (-20, 20):
        s2 = cs.scaled(sc, k)
        assert np.isfinite(s2.vals).all() and (s2.wgts[sc.wgts > 0] > 0).all()
        for kind in ('MEDIAN', 'CLIPPED'):
            a = ocombine.combine(sc.vals, sc.wgts, kind, sc.clip_sigma, sc.clip_ampfrac)
            b = ocombine.combine(s2.vals, s2.wgts, kind, sc.clip_sigma, sc.clip_ampfrac)
            assert np.array_equal(np.ldexp(a[1], -2 * k), b[1]) and np.array_equal(a[2], b[2])
            np.testing.assert_allclose(np.ldexp(a[0], k), b[0], rtol=1e-15, atol=0)
