"""The independent FITS reference (tests/fits_ref.py) against the host reader on every scene of tests/fits_scenes.py,
and what the scenes can tell apart - on the CPU, before any kernel is asked."""
import os
from fractions import Fraction

import numpy as np
import pytest

import fits_ref
import fits_scenes
from util import pkg

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SCENES = fits_scenes.scenes()


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).ravel().tolist()


def _check_against_host_reader(block, path, what):
    """fits.read of the file against the reference's reading of the same bytes: every pixel."""
    ref = fits_ref.Block.from_bytes(block)
    data = pkg().fits.read(path)[0]
    assert data.shape == ref.shape, what
    if data.dtype.kind in 'iu':
        # physical values exact
        exact = ref.exact()
        assert all(x.denominator == 1 for x in exact), what
        assert [int(v) for v in data.ravel().tolist()] == [int(x) for x in exact], what
    elif data.dtype == np.float64:
        # an unscaled BITPIX -64 block: the bits of the file
        assert not ref.scaled and ref.bitpix == -64, what
        assert np.ascontiguousarray(data).view(np.uint64).ravel().tolist() == ref.stored, what
    else:
        assert data.dtype == np.float32, what
        want, any_nan = ref.want_f32()
        got = _bits32(data)
        for i in any_nan:
            assert got[i] & 0x7fffffff > 0x7f800000, (what, i)
            got[i] = fits_ref.NAN_ANY
        assert got == want, (what, [i for i in range(ref.n) if got[i] != want[i]][:5])
    # ... and as a float32 plane, which is what the device route hands on
    if data.dtype != np.float32:
        want, any_nan = ref.want_f32()
        with np.errstate(all='ignore'):
            got = _bits32(data.astype(np.float32))
        for i in any_nan:
            assert got[i] & 0x7fffffff > 0x7f800000, (what, i)
            got[i] = fits_ref.NAN_ANY
        assert got == want, (what, [i for i in range(ref.n) if got[i] != want[i]][:5])


@pytest.mark.parametrize('scene', SCENES, ids=repr)
def test_reference_reads_what_the_host_reader_reads(scene, tmp_path):
    if not scene.host:
        # stored + BZERO leaves int64, the type of the host reader's integer plane: no host value to compare with
        assert any(not -2 ** 63 <= x < 2 ** 63 for x in scene.ref.exact())
        return
    p = str(tmp_path / 'scene.fits')
    with open(p, 'wb') as f:
        f.write(scene.block)
    _check_against_host_reader(scene.block, p, scene.name)


@pytest.mark.parametrize('name', ['astropy_f32.fits', 'astropy_i16.fits', 'astropy_u8.fits'])
def test_reference_reads_the_astropy_files(name):
    p = os.path.join(GOLD, name)
    with open(p, 'rb') as f:
        _check_against_host_reader(f.read(), p, name)


def test_fused_and_two_rounding_scalings_differ_on_the_scenes():
    s = fits_scenes.by_name('scaled16_0.1_-3').ref
    two, _ = s.want_f32()
    fused, _ = s.want_f32(s.fused())
    diff = [i for i in range(s.n) if two[i] != fused[i]]
    assert len(diff) >= 1
    assert [s.stored[i] for i in diff] == [30] and two[diff[0]] == 0 and fused[diff[0]] != 0
    t = fits_scenes.by_name(f'scaled16_{1 / 3!r}_{2 / 3!r}').ref
    n = sum(a != b for a, b in zip(t.want_int('i32'), t.want_int('i32', t.fused())))
    assert n >= 10000, n


@pytest.mark.parametrize('kind', ['i32', 'i16', 'u8'])
def test_wrap_and_saturate_differ_on_every_clipping_scene(kind):
    for name, kinds in fits_scenes.CLIP_SCENES.items():
        if kind not in kinds:
            continue
        r = fits_scenes.by_name(name).ref
        n = sum(a != b for a, b in zip(r.want_int(kind), r.want_int(kind, clip='wrap')))
        assert n >= 1, (name, kind)
    # the exact integer path has its own clipping scenes: the conventions and the ends of wider types
    for name in ('edges_bp64', 'convention_bp32') + (('edges_bp32', 'convention_bp16') if kind != 'i32' else ()):
        r = fits_scenes.by_name(name).ref
        assert r.int_exact
        assert sum(a != b for a, b in zip(r.want_int(kind), r.want_int(kind, clip='wrap'))) >= 1, (name, kind)


def test_a_conversion_through_fp64_differs_on_the_bitpix_64_scene():
    r = fits_scenes.by_name('edges_bp64').ref
    direct, _ = r.want_f32()
    double = [fits_ref.f32_bits_of_float(float(s)) for s in r.stored]
    assert sum(a != b for a, b in zip(direct, double)) >= 1


@pytest.mark.parametrize('scene', SCENES, ids=repr)
def test_float32_plane_is_within_the_derived_bound_of_the_exact_value(scene):
    """|two-rounding value - exact| <= 2^-53 (|bscale * stored| + |exact|), derived: with u = 2^-53 a correctly
    rounded operation errs by at most u / (1 + u) of its exact result (no underflow here).  The product p = bscale *
    stored gives e1 <= u / (1 + u) |p|; the sum of fl(p) and bzero has the exact result exact + e1, so
    e2 <= u / (1 + u) (|exact| + e1), and e1 + e2 <= u / (1 + u) ((1 + u) |p| + |exact|) <= u (|p| + |exact|).
    (BITPIX 64: fl(stored) rounds beyond 2^53.  With BSCALE 1 that rounding takes the product's place in the
    argument; the scaled BITPIX 64 scene keeps |stored| < 2^53, asserted.)  The float32 plane adds at most half a
    float32 spacing.  Every pixel; where the exact value is not finite the plane holds the same infinity, or a NaN."""
    r = scene.ref
    if r.bitpix == 64 and r.bscale != 1.0:
        assert all(float(s) == s for s in r.stored)
    exact = r.exact()
    two = r.two_rounding()
    bits, any_nan = r.want_f32()
    best = r.want_f32_correctly_rounded()
    bs = Fraction(r.bscale)
    u = Fraction(1, 2 ** 53)
    for i, x in enumerate(exact):
        if isinstance(x, str):
            if x == 'nan':
                assert bits[i] & 0x7fffffff > 0x7f800000
            else:
                assert bits[i] == (0x7f800000 if x == '+inf' else 0xff800000)
            continue
        assert i not in any_nan
        got = fits_ref.exact_of_bits(bits[i], -32)
        if r.is_int and not r.scaled or (r.bitpix == -32 and not r.scaled):
            assert bits[i] & 0x7fffffff == best[i] & 0x7fffffff          # one rounding from the exact value (or none)
        if isinstance(got, str):                                         # overflow of float32: only beyond FLT_MAX + half a spacing
            assert abs(x) >= Fraction(2) ** 128 - Fraction(2) ** 103
            continue
        prod = abs(bs * (Fraction(r.stored[i]) if r.is_int else fits_ref.exact_of_bits(r.stored[i], r.bitpix)))
        bound = u * (prod + abs(x)) if r.scaled else 0
        if r.bitpix == 64 and not r.scaled:
            assert got == fits_ref.exact_of_bits(best[i], -32)
            continue
        assert abs(Fraction(two[i]) - x) <= bound, (scene.name, i)
        # half a spacing at the exact value, or at the result when the result went up to a power of two
        half = max(fits_ref.f32_spacing(x), fits_ref.f32_spacing(got)) / 2
        assert abs(got - x) <= bound + half, (scene.name, i, r.stored[i])
