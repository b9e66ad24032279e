"""An independent FITS data-block decoder / encoder: the expectation of tests/test_fits_ref.py and
tests/test_fits_decode_gpu.py.

Plain Python: ``int.from_bytes``, ``struct`` and ``fractions.Fraction``; no numpy, nothing of
``zuds-pipeline_amd/fits.py`` and nothing of the kernel.  It restates the contract written above
``zm_fits_decode_dev`` / ``zm_fits_encode_dev`` in include/zudsmi.h:

* the physical value of a pixel is ``Fraction(bzero) + Fraction(bscale) * Fraction(stored)``, exact (bscale and
  bzero are the doubles the header's text parses to);
* a float32 plane of an unscaled BITPIX -32 block is the 32 bits of the file; of an unscaled integer block the
  correctly rounded float32 of the integer; of anything else the float32 nearest to the fp64 value
  ``fl(fl(bscale * fl(stored)) + bzero)`` ("two roundings"; ``fl(stored)`` only rounds for BITPIX 64);
* an integer plane truncates that fp64 value toward zero and saturates at the ends of its type, NaN gives 0; an
  unscaled integer block, and BSCALE 1 with an integer BZERO of magnitude <= 2^63, stay in exact integers.

Float values travel as bit patterns (ints): NaN payloads, -0.0 and subnormals are never passed through a host
float conversion that could change them.  A NaN that an arithmetic operation or a float64 -> float32 conversion
produces has no defined payload: it is reported as ``NAN_ANY`` and listed in ``any_nan`` for the caller.
"""
import math
import struct
from fractions import Fraction

NAN_ANY = 0x7fc00000
INT_RANGE = {'i32': (-2 ** 31, 2 ** 31 - 1), 'i16': (-2 ** 15, 2 ** 15 - 1), 'u8': (0, 255)}
KINDS = ('f32', 'i32', 'u8', 'i16')


# ---- the header: only the cards that describe the array ------------------------------------------------------
def parse(block):
    """(bitpix, shape, bscale, bzero, data offset) of the bytes of a primary HDU.  bscale / bzero are Python
    numbers as the card's text parses (int or float)."""
    cards = {}
    off = 0
    done = False
    while not done:
        for i in range(off, off + 2880, 80):
            card = block[i:i + 80].decode('ascii')
            key = card[:8].strip()
            if key == 'END':
                done = True
                break
            if card[8:10] != '= ' or key not in ('BITPIX', 'NAXIS', 'NAXIS1', 'NAXIS2', 'NAXIS3', 'BSCALE', 'BZERO'):
                continue
            text = card[10:].split('/')[0].strip()
            try:
                cards[key] = int(text)
            except ValueError:
                cards[key] = float(text)
        off += 2880
    shape = tuple(cards[f'NAXIS{i}'] for i in range(cards['NAXIS'], 0, -1))
    return cards['BITPIX'], shape, cards.get('BSCALE', 1), cards.get('BZERO', 0), off


def stored_values(raw, bitpix, n):
    """The n stored values of a big-endian data block: ints for an integer BITPIX (unsigned for 8), the IEEE bit
    patterns (ints) for -32 / -64."""
    size = abs(bitpix) // 8
    assert len(raw) >= n * size
    signed = bitpix > 8
    return [int.from_bytes(raw[i * size:(i + 1) * size], 'big', signed=signed) for i in range(n)]


# ---- IEEE bit patterns <-> exact values -----------------------------------------------------------------------
def _fields(bits, bitpix):
    ebits, mbits = (8, 23) if bitpix == -32 else (11, 52)
    sign = bits >> (ebits + mbits)
    e = (bits >> mbits) & ((1 << ebits) - 1)
    m = bits & ((1 << mbits) - 1)
    return sign, e, m, ebits, mbits


def is_nan_bits(bits, bitpix):
    _, e, m, ebits, _ = _fields(bits, bitpix)
    return e == (1 << ebits) - 1 and m != 0


def float_of_bits(bits, bitpix):
    """The Python float (fp64) with the value of a float32 / float64 bit pattern; exact (every float32 is an fp64).
    Not for NaN payloads: those stay bit patterns."""
    if bitpix == -32:
        return struct.unpack('>f', bits.to_bytes(4, 'big'))[0]
    return struct.unpack('>d', bits.to_bytes(8, 'big'))[0]


def exact_of_bits(bits, bitpix):
    """Fraction of a finite bit pattern, or 'nan' / '+inf' / '-inf'."""
    sign, e, m, ebits, mbits = _fields(bits, bitpix)
    bias = (1 << (ebits - 1)) - 1
    if e == (1 << ebits) - 1:
        return 'nan' if m else ('-inf' if sign else '+inf')
    if e == 0:
        v = Fraction(m) * Fraction(2) ** (1 - bias - mbits)
    else:
        v = Fraction((1 << mbits) | m) * Fraction(2) ** (e - bias - mbits)
    return -v if sign else v


def f32_bits_of_exact(x):
    """Bits of the float32 nearest to the Fraction x, ties to even, overflow to inf; zero is +0.

    The two float32 neighbours of |x| are lo * ulp and (lo + 1) * ulp with ulp the spacing of float32 in the binade
    of |x| (2^-149 below 2^-126).  |x| = (lo + r / D) * ulp with 0 <= r < D in integers, so comparing |x| - lo ulp
    with (lo + 1) ulp - |x| is comparing 2 r with D: the exact comparison of x with its neighbours, never a cast."""
    if x == 0:
        return 0
    sign = 0x80000000 if x < 0 else 0
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()                  # 2^(e - 1) < |x| < 2^(e + 1)
    if (n << max(-e, 0)) < (d << max(e, 0)):             # |x| < 2^e
        e -= 1
    e = max(e, -126)
    k = e - 23                                           # ulp = 2^k
    N, D = (n << -k, d) if k < 0 else (n, d << k)
    lo, r = divmod(N, D)
    if 2 * r > D or (2 * r == D and (lo & 1)):
        lo += 1
    if lo == 1 << 24:
        lo >>= 1
        e += 1
    if e > 127:
        return sign | 0x7f800000
    if lo < 1 << 23:                                     # subnormal (e == -126) or zero
        return sign | lo
    return sign | ((e + 127) << 23) | (lo - (1 << 23))


def f32_bits_of_float(v):
    """Bits of the float32 nearest to the fp64 value v: one rounding.  NaN -> NAN_ANY."""
    if v != v:
        return NAN_ANY
    if v in (math.inf, -math.inf):
        return 0x7f800000 | (0x80000000 if v < 0 else 0)
    if v == 0:
        return 0x80000000 if math.copysign(1.0, v) < 0 else 0
    b = f32_bits_of_exact(Fraction(v))
    return b | 0x80000000 if (v < 0 and b == 0) else b   # a negative value that rounds to zero is -0.0


def f32_spacing(x):
    """Spacing of float32 around the Fraction x (of the binade that holds |x|)."""
    if x == 0:
        return Fraction(2) ** -149
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()
    if (n << max(-e, 0)) < (d << max(e, 0)):
        e -= 1
    return Fraction(2) ** (max(e, -126) - 23)


# ---- a block -------------------------------------------------------------------------------------------------
class Block(object):
    """One data block with its scaling: every derived plane is a list with one entry per pixel, in file order."""

    def __init__(self, raw, bitpix, n, bscale=1, bzero=0):
        self.bitpix, self.n = bitpix, n
        self.bscale, self.bzero = float(bscale), float(bzero)
        self.scaled = self.bscale != 1.0 or self.bzero != 0.0
        self.is_int = bitpix > 0
        self.stored = stored_values(raw, bitpix, n)
        # the integer path of the contract: exact integers
        self.int_exact = (self.is_int and self.bscale == 1.0 and math.isfinite(self.bzero)
                          and self.bzero == math.floor(self.bzero) and abs(self.bzero) <= 2.0 ** 63)

    @classmethod
    def from_bytes(cls, block):
        bitpix, shape, bscale, bzero, off = parse(block)
        n = 1
        for s in shape:
            n *= s
        b = cls(block[off:off + n * abs(bitpix) // 8], bitpix, n, bscale, bzero)
        b.shape = shape
        return b

    # -- the exact physical value
    def exact(self):
        """Per pixel: Fraction, or 'nan' / '+inf' / '-inf' (float blocks; bscale != 0 in every scene, so an
        infinity keeps the sign of bscale * stored)."""
        bs, bz = Fraction(self.bscale), Fraction(self.bzero)
        if self.is_int:
            return [bz + bs * s for s in self.stored]
        out = []
        for bits in self.stored:
            x = exact_of_bits(bits, self.bitpix)
            if isinstance(x, str):
                if x != 'nan' and bs < 0:
                    x = '+inf' if x == '-inf' else '-inf'
                out.append(x)
            else:
                out.append(bz + bs * x)
        return out

    # -- fp64 evaluations
    def _fl_stored(self):
        if self.is_int:
            return [float(s) for s in self.stored]        # correctly rounded; rounds only beyond 2^53 (BITPIX 64)
        return [float_of_bits(b, self.bitpix) for b in self.stored]

    def two_rounding(self):
        """fl(fl(bscale * fl(stored)) + bzero) in Python floats (fp64, no contraction); fl(stored) when unscaled."""
        v = self._fl_stored()
        if not self.scaled:
            return v
        bs, bz = self.bscale, self.bzero
        out = []
        for s in v:
            t = bs * s
            out.append(t + bz)
        return out

    def fused(self):
        """fl(bzero + bscale * fl(stored)): ONE rounding, what a fused multiply-add gives.  The candidate the scenes
        must tell from two_rounding()."""
        if not self.scaled:
            return self._fl_stored()
        bs, bz = Fraction(self.bscale), Fraction(self.bzero)
        out = []
        for s in self._fl_stored():
            if s != s or s in (math.inf, -math.inf):
                out.append(self.bscale * s + self.bzero)
            else:
                x = bz + bs * Fraction(s)
                out.append(float(x) if x != 0 else self.bscale * s + self.bzero)    # Fraction -> float rounds correctly
        return out

    # -- the planes of the contract
    def want_f32(self, values=None):
        """(bits per pixel, set of pixels whose value is a NaN of no defined payload)."""
        if values is None:
            if self.bitpix == -32 and not self.scaled:
                return list(self.stored), set()
            if self.is_int and not self.scaled:
                return [f32_bits_of_exact(Fraction(s)) for s in self.stored], set()
            values = self.two_rounding()
        bits = [f32_bits_of_float(v) for v in values]
        return bits, {i for i, v in enumerate(values) if v != v}

    def want_f32_correctly_rounded(self):
        """The float32 nearest to the exact value (None where it is not finite): the yardstick of the error bound."""
        return [None if isinstance(x, str) else f32_bits_of_exact(x) for x in self.exact()]

    def want_int(self, kind, values=None, clip='saturate'):
        """``clip='wrap'`` is the candidate that keeps the low bits instead (two's complement), the other one the
        scenes must tell apart; NaN and infinities wrap to 0 there."""
        lo, hi = INT_RANGE[kind]
        span = hi - lo + 1

        def fit(i):
            if clip == 'saturate':
                return min(max(i, lo), hi)
            return (i - lo) % span + lo
        if values is None and self.int_exact:
            bz = int(self.bzero)
            return [fit(s + bz) for s in self.stored]
        if values is None:
            values = self.two_rounding()
        out = []
        for v in values:
            if v != v:
                out.append(0)
            elif v in (math.inf, -math.inf):
                out.append((hi if v > 0 else lo) if clip == 'saturate' else 0)
            else:
                out.append(fit(int(v)))                   # int() of a float truncates toward zero, exactly
        return out


# ---- the encoder ---------------------------------------------------------------------------------------------
def encode(values, in_kind):
    """Big-endian bytes of a plane.  in_kind 0: float32 given as bit patterns -> BITPIX -32; 1: int32 -> 32;
    2: uint8 -> 8; 3: int32 values within -32768 .. 32767 -> BITPIX 16."""
    fmt = {0: '>I', 1: '>i', 2: '>B', 3: '>h'}[in_kind]
    return b''.join(struct.pack(fmt, v) for v in values)
