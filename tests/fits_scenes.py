"""FITS data blocks for tests/test_fits_ref.py and tests/test_fits_decode_gpu.py: the smallest blocks at which a
decode can go wrong.  Every block is raw bytes - ``fits.header_block`` followed by the packed stored values - so
the stored values are chosen directly; the largest has 65 536 pixels (every int16), most have a few hundred."""
import functools
import random
import struct

import fits_ref
from util import pkg

LENGTHS = (1, 255, 256, 257, 1551)          # one block of 256 threads and its neighbours, several blocks
SCALINGS = ((0.1, -3), (1 / 3, 2 / 3), (1.0000001, 32768), (0.01, 327.68), (1, 0.5), (-2.5, 1e4))
_PACK = {8: '>B', 16: '>h', 32: '>i', 64: '>q', -32: '>I', -64: '>Q'}     # float blocks are packed as bit patterns
_INT_RANGE = {8: (0, 255), 16: (-2 ** 15, 2 ** 15 - 1), 32: (-2 ** 31, 2 ** 31 - 1), 64: (-2 ** 63, 2 ** 63 - 1)}


def f32(x):
    """bits of the float32 nearest to the Python float x"""
    return struct.unpack('>I', struct.pack('>f', x))[0]


def f64(x):
    return struct.unpack('>Q', struct.pack('>d', x))[0]


class Scene(object):
    def __init__(self, name, bitpix, stored, bscale=1, bzero=0, shape=None, host=True):
        self.name, self.bitpix, self.bscale, self.bzero = name, bitpix, bscale, bzero
        self.host = host            # False: a physical value leaves int64, which the host reader's integer plane cannot hold
        self.stored = list(stored)
        self.shape = tuple(shape) if shape else (len(self.stored),)
        self.n = len(self.stored)
        self.raw = b''.join(struct.pack(_PACK[bitpix], v) for v in self.stored)
        extra = []
        if bscale != 1 or bzero != 0:
            extra = [('BSCALE', bscale, ''), ('BZERO', bzero, '')]
        self.header = pkg().fits.header_block(self.shape, bitpix, extra=extra)
        self.block = self.header + self.raw + b'\0' * (-len(self.raw) % 2880)

    @functools.cached_property
    def ref(self):
        """The independent reading of the block's own bytes, header included."""
        r = fits_ref.Block.from_bytes(self.block)
        assert r.n == self.n and r.shape == self.shape and r.stored == self.stored
        return r

    def __repr__(self):
        return self.name


def _random_stored(rng, bitpix, n):
    if bitpix > 0:
        lo, hi = _INT_RANGE[bitpix]
        return [rng.randint(lo, hi) for _ in range(n)]
    if bitpix == -32:
        return [f32(rng.gauss(0, 1e3)) for _ in range(n)]
    return [f64(rng.gauss(0, 1e3)) for _ in range(n)]


def _int_edges(bitpix):
    lo, hi = _INT_RANGE[bitpix]
    e = [lo, hi, 0, 1, lo + 1, hi - 1]
    if bitpix > 8:
        e += [-1, 255, 256, -129, 32767, 32768, -32768, -32769]
    else:
        e += [127, 128]
    return [v for v in e if lo <= v <= hi]


# float32 / float64 special values as bit patterns
F32_SPECIALS = [0x7fc00000, 0xffc00000, 0x7fc12345, 0xffedcba9,      # quiet NaNs, both signs, payloads
                0x7f800001, 0xff800001, 0x7fa55aa5, 0xffbfffff,      # signalling NaNs, both signs, payloads
                0x7f800000, 0xff800000, 0x00000000, 0x80000000,      # +-inf, +-0
                0x00000001, 0x80000001, 0x007fffff, 0x807fffff,      # smallest / largest subnormal
                0x00800000, 0x7f7fffff, 0xff7fffff, 0x3f800000]      # FLT_MIN, +-FLT_MAX, 1
F64_SPECIALS = [0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000012345678, 0xfffedcba98765432,
                0x7ff0000000000001, 0xfff0000000000001, 0x7ff4000000000abc, 0xfff7ffffffffffff,
                0x7ff0000000000000, 0xfff0000000000000, 0x0000000000000000, 0x8000000000000000,
                0x0000000000000001, 0x800fffffffffffff, 0x7fefffffffffffff, 0xffefffffffffffff]


def _f64_for_f32_edges():
    """float64 values at the edges of float32: overflow, underflow to subnormal and to zero, rounding ties."""
    flt_max = (2.0 - 2.0 ** -23) * 2.0 ** 127
    v = [flt_max, -flt_max,
         flt_max + 2.0 ** 102,                # half a spacing above FLT_MAX: a tie that rounds to 2^128 = inf
         flt_max + 2.0 ** 102 - 2.0 ** 75,    # just below it: stays FLT_MAX
         -(flt_max + 2.0 ** 102), 1e39, -1e39, 1e300,
         2.0 ** -126, 2.0 ** -126 - 2.0 ** -150,          # rounds up to FLT_MIN (tie, even) ...
         2.0 ** -127, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149,   # subnormal results; ties to even: 2 and 2
         2.0 ** -149, 0.75 * 2.0 ** -149, 2.0 ** -150,    # 2^-150 is the tie between 0 and the smallest subnormal: 0
         2.0 ** -150 + 2.0 ** -200, -2.0 ** -150, 2.0 ** -151, -1e-300, 1e-46, 3e-39, -3e-39]
    # exact ties between neighbouring float32 values: lower neighbour even (stays) and odd (goes up), both signs
    for m, e in ((0x800000, 0), (0x800001, 0), (0xfffffe, 5), (0xffffff, 5), (0x9abcde, -20), (0x9abcdf, -20),
                 (0xffffff, 127 - 23)):
        tie = (m + 0.5) * 2.0 ** (e - 23)
        v += [tie, -tie, tie + tie * 2.0 ** -52, tie - tie * 2.0 ** -52]
    return [f64(x) for x in v]


CLIP_VALUES = [-1.0, -0.5, 255.5, 256.0, 32767.5, -32769.0, 3e9, -3e9, float('nan'), float('inf'), float('-inf'),
               -0.0, 0.999, 254.999, 32767.0, -32768.0, -32768.5, 2147483647.0, 2147483648.0, -2147483648.0,
               -2147483649.0, 2147483647.5, 1e19, -1e19, 1e300]


@functools.lru_cache(maxsize=None)
def scenes():
    rng = random.Random(20261021)
    out = []

    # lengths, every BITPIX, unscaled; one 3-D block
    for bitpix in (8, 16, 32, 64, -32, -64):
        for n in LENGTHS:
            out.append(Scene(f'len{n}_bp{bitpix}', bitpix, _random_stored(rng, bitpix, n)))
    out.append(Scene('cube_bp16', 16, _random_stored(rng, 16, 30), shape=(2, 3, 5)))
    out.append(Scene('cube_bp-32_scaled', -32, _random_stored(rng, -32, 30), 0.1, -3, shape=(2, 3, 5)))

    # integer blocks: the ends of the type and of every narrower output type
    for bitpix in (8, 16, 32, 64):
        st = _int_edges(bitpix) + _random_stored(rng, bitpix, 300)
        if bitpix == 64:
            for b in (2 ** 24, 2 ** 53):
                st += [s * (b + d) for s in (1, -1) for d in (-1, 0, 1)]
            st += [2 ** 63 - 1, -(2 ** 63 - 1), 3 * 10 ** 9, -3 * 10 ** 9, 2 ** 31, -2 ** 31 - 1]
            # just above a float32 tie, by less than fp64 resolves: through fp64 they land ON the tie and go to even
            st += [s * v for s in (1, -1) for v in (2 ** 53 + 2 ** 29 + 1, 2 ** 60 + 2 ** 36 + 1, 2 ** 62 + 2 ** 38 + 255)]
        out.append(Scene(f'edges_bp{bitpix}', bitpix, st))

    # the unsigned / signed-byte conventions
    for bitpix, bzero in ((16, 32768), (32, 2147483648), (8, -128)):
        out.append(Scene(f'convention_bp{bitpix}', bitpix, _int_edges(bitpix) + _random_stored(rng, bitpix, 300),
                         1, bzero))
    out.append(Scene('convention_bp16_float_card', 16, _int_edges(16) + _random_stored(rng, 16, 100), 1.0, 32768.0))

    # real scalings on every int16 stored value
    every16 = list(range(-32768, 32768))
    for bscale, bzero in SCALINGS:
        out.append(Scene(f'scaled16_{bscale!r}_{bzero!r}', 16, every16, bscale, bzero))
    out.append(Scene('scaled32_0.1_-3', 32, _int_edges(32) + [30, -30, 29, 31] + _random_stored(rng, 32, 1500), 0.1, -3))
    out.append(Scene('scaled-32_0.1_-3', -32, [f32(30.0), f32(-30.0)] + F32_SPECIALS + _random_stored(rng, -32, 1500),
                     0.1, -3))
    out.append(Scene('scaled8_0.1_-3', 8, list(range(256)), 0.1, -3))
    out.append(Scene('scaled64_thirds', 64, _int_edges(32) + _random_stored(rng, 32, 500), 1 / 3, 2 / 3))
    out.append(Scene('scaled-64_0.1_-3', -64, F64_SPECIALS + _random_stored(rng, -64, 500), 0.1, -3))

    # float blocks: special values
    out.append(Scene('special_bp-32', -32, F32_SPECIALS + _random_stored(rng, -32, 50)))
    out.append(Scene('special_bp-64', -64, F64_SPECIALS + _f64_for_f32_edges() + _random_stored(rng, -64, 50)))

    # integer outputs that must clip: float blocks, and scaled blocks that reach the same values
    out.append(Scene('clip_bp-32', -32, [f32(v) for v in CLIP_VALUES if abs(v) < 1e38 or v != v or abs(v) == float('inf')]))
    out.append(Scene('clip_bp-64', -64, [f64(v) for v in CLIP_VALUES]))
    out.append(Scene('clip_bp-32_scaled', -32, [f32(v) for v in CLIP_VALUES if not abs(v) > 1e38] +
                     [f32(float('nan')), f32(float('inf')), f32(float('-inf'))], 2, 0.5))
    # 0.5 * stored: -1.0 -0.5 255.5 256.0 32767.5 -32769.0 and the ends of int32 halved
    out.append(Scene('clip_bp32_half', 32, [-2, -1, 511, 512, 65535, -65538, 65534, -65536, -65537, 2 ** 31 - 1, -2 ** 31],
                     0.5, 0))
    out.append(Scene('clip_bp32_threehalves', 32, [2 ** 31 - 1, -2 ** 31, 1431655765, 1431655764, -1431655765, -1431655766,
                                                    170, 171, 21845, 21846, -21846, -21847, 0, -1], 1.5, 0.25))
    # 2 * stored: +-3e9 and beyond int32 on both sides
    out.append(Scene('clip_bp32_twice', 32, [1500000000, -1500000000, 2 ** 30, -2 ** 30 - 1, 2 ** 30 - 1, 2 ** 31 - 1,
                                              -2 ** 31, 128, -1], 2, 0))
    out.append(Scene('clip_bp64_exact', 64, [3 * 10 ** 9, -3 * 10 ** 9, 2 ** 63 - 1, -2 ** 63 + 7, 255, 256, -1, 32768, -32769,
                                              2 ** 31, 2 ** 31 - 1, -2 ** 31 - 1, 2 ** 32 + 5, -2 ** 32 + 7], 1, -7))
    # stored + BZERO beyond int64 on either side, and the unsigned 64-bit convention
    out.append(Scene('clip_bp64_below', 64, [-2 ** 63, -2 ** 63 + 6, -2 ** 63 + 7, 0, 7, 2 ** 63 - 1], 1, -7, host=False))
    out.append(Scene('clip_bp64_above', 64, [2 ** 63 - 1, 2 ** 63 - 7, 2 ** 63 - 8, 0, -7, -2 ** 63], 1, 7, host=False))
    out.append(Scene('convention_bp64', 64, [-2 ** 63, -2 ** 63 + 255, -2 ** 63 + 256, -2 ** 63 + 2 ** 31 - 1, -2 ** 63 + 2 ** 31,
                                             -1, 0, 2 ** 63 - 1], 1, 9223372036854775808, host=False))
    return tuple(out)


def by_name(name):
    return next(s for s in scenes() if s.name == name)


# the scenes on which an integer plane must clip, and the output kinds whose range each one leaves (half an int32 fits int32)
_ALL = ('i32', 'i16', 'u8')
CLIP_SCENES = {'clip_bp-32': _ALL, 'clip_bp-64': _ALL, 'clip_bp-32_scaled': _ALL, 'clip_bp32_half': ('i16', 'u8'),
               'clip_bp32_threehalves': _ALL, 'clip_bp32_twice': _ALL, 'clip_bp64_exact': _ALL}
