"""The combine kernels of csrc/combine.hip against oracle/combine.py: every valid count, the clip boundary, ties.

Scenes and what they hold: tests/combine_scenes.py (asserted on the CPU by tests/test_combine_scenes.py).  Every
call here hands the kernels a stack with one spare frame and, where the frame stride allows, padding behind every
frame, all of it filled with value 1e30 and weight 1e30 (a VALID sample: a kernel that reads it changes its
result), and output planes that are 256 floats longer than npix and pre-filled with a sentinel.

Bounds (derived in combine_scenes.reference and DESIGN.md, "Combine, every count and the clip boundary"); no pixel
is left out and there is no absolute term:
  validity    out_wgt > 0 equals the oracle's, exactly; no valid sample or no survivor: value 0 and weight 0
  MEDIAN      bit-equal to float32(oracle): a + b is exact in float64 and rounds once either way, 0.5 is exact
  weight      |g - r| <= n 2^-24 r
  value       |g - r| <= (n + 3) 2^-24 sum_kept(w |v|) / sum_kept(w)
A result of zero is compared by value, not by sign: the order of -0.0 and +0.0 among equal keys is not defined
(np.sort and the kernel's fminf / fmaxf network may differ), and the scenes hold both zeros.

Left out: valid samples whose value is NaN, +-inf, or so large that a + b overflows.  The resampler never emits
them with a positive weight (tests/test_nonfinite_gpu.py).  A real mask value of -1 (the "not covered" marker of
the mask fold, include/zudsmi.h) is left out too.
"""
import ctypes as C

import numpy as np
import pytest

import combine_scenes as cs
from oracle import combine as ocombine
from util import pkg

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
TAIL = 256          # (at least the 64 the output planes must be guarded by: a wide launch has up to 127 idle pixel slots behind npix)
KINDS = ('CLIPPED', 'MEDIAN', 'WEIGHTED', 'AVERAGE')
_refs = {}


def ref(scene, kind):
    """The oracle's result and the bounds, computed once per scene and kind."""
    key = (id(scene.vals), id(scene.wgts), scene.clip_sigma, scene.clip_ampfrac, kind)
    if key not in _refs:
        _refs[key] = (scene,) + cs.reference(scene, kind)         # (the scene is held: its ids stay its own)
    return _refs[key][1:]


def run_dev(engine, scene, kind, stride=None, spare=1):
    """zm_combine_stack_dev on torch tensors; returns (img, wgt) of npix elements after checking the tails."""
    import torch
    z = pkg()
    n, npix = scene.vals.shape
    stride = npix if stride is None else stride
    host = np.full((n + spare, stride, 2), 1e30, np.float32)
    host[:n, :npix, 0] = scene.vals
    host[:n, :npix, 1] = scene.wgts
    stack = torch.from_numpy(host).cuda()
    img = torch.full((npix + TAIL,), SENTINEL, dtype=torch.float32, device='cuda')
    wgt = torch.full((npix + TAIL,), SENTINEL, dtype=torch.float32, device='cuda')
    p = z.coadd_params(combine=kind, clip_sigma=scene.clip_sigma, clip_ampfrac=scene.clip_ampfrac)
    torch.cuda.synchronize()
    z._lib.check(engine.L.zm_combine_stack_dev(engine.ctx, n, stack.data_ptr(), stride, npix, C.byref(p),
                                               img.data_ptr(), wgt.data_ptr()), 'zm_combine_stack_dev')
    engine.synchronize()
    img, wgt = img.cpu().numpy(), wgt.cpu().numpy()
    assert (img[npix:] == np.float32(SENTINEL)).all() and (wgt[npix:] == np.float32(SENTINEL)).all(), \
        f'{kind} n={n} npix={npix}: written past npix'
    return img[:npix], wgt[:npix]


def same_bits(a, b):
    """Bit-equal float32, a zero compared by value."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))


def check(g_img, g_wgt, scene, kind, what):
    """The bounds of the module docstring at every pixel; returns the worst (value, weight) error in units of them."""
    val, wgt, vbound, wbound = ref(scene, kind)
    what = f'{what} {kind} n={scene.vals.shape[0]}'
    assert np.array_equal(g_wgt > 0, wgt > 0), f'{what}: validity differs at {np.nonzero((g_wgt > 0) != (wgt > 0))[0][:8]}'
    dead = wgt == 0
    assert (g_img[dead] == 0).all() and (g_wgt[dead] == 0).all(), f'{what}: a pixel without survivors is not 0 / 0'
    werr = np.abs(g_wgt.astype(np.float64) - wgt)
    wratio = float(np.max(np.where(wbound > 0, werr / np.where(wbound > 0, wbound, 1.0), np.where(werr > 0, np.inf, 0.0)), initial=0.0))
    if kind == 'MEDIAN':
        ok = same_bits(g_img, np.float32(val))
        vratio = 0.0 if ok.all() else np.inf
        detail = f'{(~ok).sum()} medians differ, first at pixel {np.argmin(ok)}: got {g_img[np.argmin(ok)]!r} ref {val[np.argmin(ok)]!r}'
    else:
        verr = np.abs(g_img.astype(np.float64) - val)
        r = np.where(vbound > 0, verr / np.where(vbound > 0, vbound, 1.0), np.where(verr > 0, np.inf, 0.0))
        vratio = float(np.max(r, initial=0.0))
        i = int(np.argmax(r)) if r.size else 0
        detail = f'worst at pixel {i}: got {g_img[i]!r} ref {val[i]!r} bound {vbound[i]:.3e}' if r.size else ''
    print(f'ratio {what}: value {vratio:.3f} weight {wratio:.3f}')
    assert vratio <= 1.0, f'{what}: value error is {vratio:.3f} of the bound; {detail}'
    assert wratio <= 1.0, f'{what}: weight error is {wratio:.3f} of the bound'
    return vratio, wratio


@pytest.mark.parametrize('n', cs.DEPTHS)
def test_clipped_every_count_at_the_threshold(engine, n):
    for params in cs.PARAM_SETS:
        scene = cs.clip_scene(n, *params)
        check(*run_dev(engine, scene, 'CLIPPED'), scene, 'CLIPPED', f'clip{params}')


@pytest.mark.parametrize('n', cs.DEPTHS)
def test_median_weighted_average_every_count(engine, n):
    for params in cs.PARAM_SETS:
        scene = cs.clip_scene(n, *params)
        check(*run_dev(engine, scene, 'MEDIAN'), scene, 'MEDIAN', f'clip{params}')
    for params in (cs.PARAM_SETS[0], cs.PARAM_SETS[4]):
        scene = cs.clip_scene(n, *params)
        for kind in ('WEIGHTED', 'AVERAGE'):
            check(*run_dev(engine, scene, kind), scene, kind, f'clip{params}')


@pytest.mark.parametrize('n', cs.DEPTHS)
def test_ties(engine, n):
    """Repeated values ({0, 1, 2, 3}, one value, {-0.0, +0.0, 1}): MEDIAN bit-equal, CLIPPED within the bounds.  In the
    scene with both zeros a zero result is compared by value, not by sign (same_bits, module docstring)."""
    for tk in cs.TIE_KINDS:
        scene = cs.tie_scene(n, tk)
        for kind in ('MEDIAN', 'CLIPPED'):
            check(*run_dev(engine, scene, kind), scene, kind, f'ties {tk}')


@pytest.mark.parametrize('n', [d for d in cs.DEPTHS if d >= 3])
def test_sample_on_the_boundary_is_kept(engine, n):
    """|v - med| == thr == 32 in exactly representable numbers (w = 1/16: the kernel's rsqrt has to give 4): kept, as
    the oracle's <= keeps it.  The weight is a sum of n sixteenths: exact."""
    scene = cs.boundary_scene(n)
    g_img, g_wgt = run_dev(engine, scene, 'CLIPPED')
    assert (g_wgt == np.float32(n / 16.0)).all(), f'n={n}: weights {np.unique(g_wgt)} for {n / 16.0}'
    check(g_img, g_wgt, scene, 'CLIPPED', 'on-boundary')


@pytest.mark.parametrize('k', [-20, 20])
@pytest.mark.parametrize('n', [5, 64, 130, 512])
def test_powers_of_two_commute(engine, n, k):
    """combine(2^k v, 2^-2k w) == (2^k value, 2^-2k weight) of the unscaled call, bit for bit: every operation of the
    kernels commutes with powers of two in the values and of four in the weights, the reciprocal square root too."""
    for params in (cs.PARAM_SETS[0], cs.PARAM_SETS[2]):
        scene = cs.clip_scene(n, *params)
        for kind in ('MEDIAN', 'CLIPPED'):
            a_img, a_wgt = run_dev(engine, scene, kind)
            b_img, b_wgt = run_dev(engine, cs.scaled(scene, k), kind)
            bad = ~same_bits(np.ldexp(a_img, k), b_img) | ~same_bits(np.ldexp(a_wgt, -2 * k), b_wgt)
            assert not bad.any(), f'{kind} n={n} k={k} {params}: {bad.sum()} pixels, first {np.argmax(bad)}'


@pytest.mark.parametrize('n', [5, 130])
def test_denormal_weights_are_valid(engine, n):
    """The only valid samples carry weights of 1e-40, a float32 denormal.  oracle/combine.py: valid when the weight
    is > 0 - they count, with their weight, in every kind."""
    rng = np.random.default_rng(n)
    npix = 70
    valid = rng.uniform(size=(n, npix)) < 0.6
    valid[:, 0] = False
    valid[1:, 1] = False
    valid[0, 1] = True
    vals = rng.normal(100, 10, (n, npix)).astype(np.float32)
    scene = cs.Scene(vals, np.where(valid, np.float32(1e-40), np.float32(0)).astype(np.float32), 4.0, 0.3)
    assert (scene.wgts[valid] > 0).all() and (scene.wgts[valid] < np.finfo(np.float32).tiny).all()
    for kind in KINDS:
        check(*run_dev(engine, scene, kind), scene, kind, 'denormal weights')


@pytest.mark.parametrize('kind', ['CLIPPED', 'WEIGHTED'])
@pytest.mark.parametrize('n', [5, 130])
def test_frame_stride_wider_than_the_frame(engine, n, kind):
    """frame_stride_px = npix + 37, the padding holds valid-looking samples (1e30, 1e30): bit-equal to the packed call."""
    scene = cs.clip_scene(n, *cs.PARAM_SETS[0])
    npix = scene.vals.shape[1]
    a = run_dev(engine, scene, kind)
    b = run_dev(engine, scene, kind, stride=npix + 37)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    check(*b, scene, kind, 'strided')


@pytest.mark.parametrize('npix', [1, 7, 9, 31, 33, 257])
@pytest.mark.parametrize('n', [5, 130, 260, 512])
def test_ragged_last_wave(engine, n, npix):
    """Pixel counts that end inside a wave and inside the group of pixels a wave holds at 2, 4 and 8 lanes per pixel:
    the result is the oracle's and nothing behind npix is written (run_dev checks the tails)."""
    rng = np.random.default_rng([n, npix])
    vals = rng.normal(50, 5, (n, npix)).astype(np.float32)
    vals[rng.uniform(size=vals.shape) < 0.05] += 400
    wgts = rng.uniform(0.01, 0.1, (n, npix)).astype(np.float32)
    wgts[rng.uniform(size=wgts.shape) < 0.3] = 0
    scene = cs.Scene(vals, wgts, 4.0, 0.3)
    assert (cs.census(scene)['slack'] >= 0).all()
    for kind in KINDS:
        check(*run_dev(engine, scene, kind), scene, kind, f'ragged npix={npix}')


@pytest.mark.parametrize('n', [5, 64, 130, 260, 512])
def test_two_runs_give_the_same_bits(engine, n):
    scene = cs.clip_scene(n, *cs.PARAM_SETS[0])
    for kind in KINDS:
        a, b = run_dev(engine, scene, kind), run_dev(engine, scene, kind)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize('n', [3, 64, 128, 512])
def test_engine_combine_stack_is_the_same_call(engine, n):
    """Engine.combine_stack (host arrays, packed stack without a spare frame) gives the bits of the direct call."""
    z = pkg()
    scene = cs.clip_scene(n, *cs.PARAM_SETS[1])
    for kind in KINDS:
        p = z.coadd_params(combine=kind, clip_sigma=scene.clip_sigma, clip_ampfrac=scene.clip_ampfrac)
        npix = scene.vals.shape[1]
        e_img, e_wgt = engine.combine_stack(scene.vals.reshape(n, 1, npix), scene.wgts.reshape(n, 1, npix), p)
        d_img, d_wgt = run_dev(engine, scene, kind)
        assert np.array_equal(e_img.ravel().view(np.uint32), d_img.view(np.uint32))
        assert np.array_equal(e_wgt.ravel().view(np.uint32), d_wgt.view(np.uint32))


# ---- masks ------------------------------------------------------------------------------------------------------
MASK_BITS = np.array([0, 1 << 30, -2 ** 31, -2, 4, 1 << 16, 0x7ffffffe, 6], np.int64)     # (bit 0 never set: an OR cannot
#                                                                                            become -1, the marker)


@pytest.mark.parametrize('with_cov', [True, False])
@pytest.mark.parametrize('npix', [1, 255, 257])
@pytest.mark.parametrize('kind', ['AND', 'OR'])
def test_mask_fold_against_the_oracle(engine, kind, npix, with_cov):
    """zm_mask_accum_dev / zm_mask_finalize_dev: 4 frames, every one of the 16 coverage subsets, bit patterns with 0,
    bit 30, the sign bit and -2; first = 1 on a dirty accumulator; cov = NULL still finalises the accumulator."""
    import torch
    z = pkg()
    rng = np.random.default_rng(npix)
    idx = np.arange(npix)
    subsets = [np.array([s]) for s in range(16)] if npix == 1 else [(idx + 5 * (idx // 16)) % 16]
    for subset in subsets:
        covered = ((subset[None] >> np.arange(4)[:, None]) & 1).astype(bool)
        masks = rng.choice(MASK_BITS, (4, npix))
        assert npix == 1 or len(set(subset)) == 16
        r_mask, r_cov = ocombine.combine_masks(masks, covered, kind)
        acc = torch.full((npix + TAIL,), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
        cov = torch.full((npix + TAIL,), SENTINEL, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        for i in range(4):
            m = torch.from_numpy(np.where(covered[i], masks[i], -1).astype(np.int32)).cuda()
            torch.cuda.synchronize()
            z._lib.check(engine.L.zm_mask_accum_dev(engine.ctx, acc.data_ptr(), m.data_ptr(), npix,
                                                    z._lib.MASKCOMB[kind], int(i == 0)), 'zm_mask_accum_dev')
            engine.synchronize()
        z._lib.check(engine.L.zm_mask_finalize_dev(engine.ctx, acc.data_ptr(), cov.data_ptr() if with_cov else None, npix),
                     'zm_mask_finalize_dev')
        engine.synchronize()
        acc, cov = acc.cpu().numpy(), cov.cpu().numpy()
        assert np.array_equal(acc[:npix], r_mask.astype(np.int32)), kind
        assert (acc[npix:] == 0x5a5a5a5a).all() and (cov[npix:] == np.float32(SENTINEL)).all()
        if with_cov:
            assert np.array_equal(cov[:npix], r_cov.astype(np.float32))
        else:
            assert (cov == np.float32(SENTINEL)).all()


def test_coadd_finalize_rule(engine):
    """zm_coadd_finalize_dev: w > 0 ? s1 / w : 0 for w in {0, -1, 1e-40, 1, NaN} (1e-40: a denormal, > 0)."""
    import torch
    z = pkg()
    npix = 300
    rng = np.random.default_rng(3)
    s0 = np.array([0, -1, 1e-40, 1, np.nan], np.float32)[np.arange(npix) % 5]
    s1 = (rng.normal(0, 1, npix) * np.where(np.arange(npix) % 2, 1e-38, 50.0)).astype(np.float32)
    with np.errstate(all='ignore'):
        want = np.where(s0 > 0, s1 / s0, np.float32(0)).astype(np.float32)
    assert np.isinf(want).any() and (np.isfinite(want) & (want != 0))[2::5].any()
    d1 = torch.cat([torch.from_numpy(s1), torch.full((TAIL,), SENTINEL)]).cuda()
    d0 = torch.from_numpy(s0).cuda()
    torch.cuda.synchronize()
    z._lib.check(engine.L.zm_coadd_finalize_dev(engine.ctx, d1.data_ptr(), d0.data_ptr(), npix), 'zm_coadd_finalize_dev')
    engine.synchronize()
    got = d1.cpu().numpy()
    assert np.array_equal(got[:npix].view(np.uint32), want.view(np.uint32)), np.nonzero(got[:npix] != want)[0][:8]
    assert (got[npix:] == np.float32(SENTINEL)).all()
