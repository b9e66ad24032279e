"""Small scenes for the fake-source injection (tests/test_inject_ref.py asserts their conditions on the restatement alone,
tests/test_inject_gpu.py runs the kernel on them, tests/measure_inject_tolerance.py sets the tolerances on them).  numpy
only; every scene is built once and shared.  Frames are 96 x 80 at most.

In the scenes that are compared by the pixel rule no pixel is written twice (asserted in tests/test_inject_ref.py): the
float32 value a write starts from is then the scene's own, whatever the kernel did before.  Overlaps are the business of
the exact scenes, whose every sum is exact in float32 or rounds by a planted tie."""
import functools
from typing import NamedTuple

import numpy as np

from psf_scenes import BIT1, BIT8, model_gaussian

NX, NY = 96, 80
GAIN = 1.5
SLOT = 18                        # half width of the largest box (half 15): the slots below keep such boxes apart
SLOTS = [(19, 19), (57, 19), (19, 57), (57, 57)]
NAN_PAYLOAD = np.array([0x7FC12345], np.uint32).view(np.float32)[0]


class Scene(NamedTuple):
    name: str
    img: np.ndarray
    rms: np.ndarray
    mask: np.ndarray
    x: np.ndarray
    y: np.ndarray
    flux: np.ndarray
    model: np.ndarray
    half: int
    gain: float
    core_radius: float
    names: tuple
    unwritten: tuple             # (y, x) of planted special values no fake may write
    written: tuple               # (y, x) of planted special values under a footprint


def _planes(seed):
    rng = np.random.default_rng(seed)
    jj, ii = np.mgrid[0:NY, 0:NX]
    img = (100.0 + 0.05 * ii - 0.03 * jj + rng.normal(0.0, 5.0, (NY, NX))).astype(np.float32)
    rms = (5.0 * (1.0 + 0.004 * ii)).astype(np.float32)
    return img, rms, np.zeros((NY, NX), np.int32)


def _core(half):
    return 2.0 if half == 1 else 6.0


def model_dyadic():
    """3 x 3, unit sum, every entry a power of two: at integer positions P is the model itself."""
    return np.array([[0.0625, 0.125, 0.0625], [0.125, 0.25, 0.125], [0.0625, 0.125, 0.0625]])


@functools.lru_cache(maxsize=None)
def interior(half):
    """Four fakes in the four slots: fx = fy = 0 exactly; fx = -0.5 exactly; fx one ulp below 0.5 with fy = -0.5; a negative
    flux at fx = 0.25, fy = 0.  Around the first: a bad pixel just OUTSIDE the core radius ((c, 1): c^2 + 1 > c^2), a pixel
    with a bit that is not bad inside it, a NaN with a payload and a -0.0 at the box's corners, where its profile is 0.
    Around the fourth: a bad pixel just INSIDE the core radius ((c, 0) from fx = 0.25: (c - 0.25)^2 < c^2).  The rms
    plane holds a 0, a negative value, a NaN and an inf under the second footprint."""
    img, rms, mask = _planes(300 + half)
    c = int(_core(half))
    m = half + 3
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = SLOTS
    fakes = [('phase-zero', float(x0), float(y0), 4.0e4), ('fx-minus-half', x1 - 0.5, y1 + 0.3, 2.5e4),
             ('fx-ulp-below-half', float(np.nextafter(x2 + 0.5, 0.0)), y2 - 0.5, 3.0e4), ('negative', x3 + 0.25, float(y3), -2.0e4)]
    mask[y0 + 1, x0 + c] |= BIT8
    mask[y0, x0 + 1] |= BIT1
    mask[y3, x3 + c] |= BIT8
    img[y0 + m, x0 + m] = NAN_PAYLOAD
    img[y0 - m, x0 - m] = np.float32(-0.0)
    rms[y1, x1] = 0.0
    rms[y1, x1 - 1] = -3.0
    rms[y1 + 1, x1] = np.nan
    rms[y1 - 1, x1 - 1] = np.inf
    return Scene(f'interior-{half}', img, rms, mask, *(np.array([f[k] for f in fakes]) for k in (1, 2, 3)), model_gaussian(half),
                 half, GAIN, _core(half), tuple(f[0] for f in fakes), ((y0 + m, x0 + m), (y0 - m, x0 - m)), ())


@functools.lru_cache(maxsize=None)
def edges(half):
    """A fake in the middle over a NaN, an inf and a -0.0 pixel; boxes cut at each edge and at two corners (placed as for
    the largest box, so that none meets another); boxes wholly outside; x, y and flux that are not finite; a flux of 0 in
    the middle of everything."""
    img, rms, mask = _planes(400 + half)
    fakes = [('over-specials', 48.31, 40.27, 3.0e4), ('left', 2.3, 40.4, 2.0e4), ('right', NX - 3.4, 40.1, 2.0e4),
             ('bottom', 48.2, 1.7, 2.0e4), ('top', 48.6, NY - 2.6, 2.0e4), ('corner-low', 1.2, 1.4, 2.0e4),
             ('corner-high', NX - 1.5, NY - 1.3, -2.0e4),
             # the box's last column is the frame's first (its profile is 0 there: CLIPPED, nothing written), and one further
             ('inside-by-one', -(half + 3.0), 10.0, 1.0e4), ('outside-by-one', -(half + 4.0), 10.0, 1.0e4),
             ('outside-left', -(half + 3) - 0.6, 10.3, 1.0e4), ('outside-far', 500.7, -900.1, 1.0e4), ('huge', 1.0e300, 3.3, 1.0e4),
             ('x-nan', np.nan, 20.0, 1.0e4), ('y-inf', 20.0, np.inf, 1.0e4), ('flux-nan', 30.0, 30.0, np.nan),
             ('flux-inf', 30.0, 30.0, -np.inf), ('flux-zero', 48.0, 40.0, 0.0)]
    img[40, 48] = np.nan
    img[41, 48] = np.inf
    img[40, 49] = np.float32(-0.0)
    mask[40, 47] |= BIT8                                  # inside the core of 'over-specials' and of 'flux-zero'
    return Scene(f'edges-{half}', img, rms, mask, *(np.array([f[k] for f in fakes]) for k in (1, 2, 3)), model_gaussian(half),
                 half, GAIN, _core(half), tuple(f[0] for f in fakes), (), ((40, 48), (41, 48), (40, 49)))


@functools.lru_cache(maxsize=None)
def counts():
    """65 fakes of half 1 on a lattice of pitch 10 (boxes of 9: one layer), each at a random phase and flux."""
    img, rms, mask = _planes(500)
    rng = np.random.default_rng(501)
    spots = [(5 + 10 * a, 5 + 10 * b) for b in range(8) for a in range(9)]
    pick = rng.permutation(len(spots))[:65]
    x = np.array([spots[k][0] for k in pick]) + rng.uniform(-0.5, 0.5, 65)
    y = np.array([spots[k][1] for k in pick]) + rng.uniform(-0.5, 0.5, 65)
    flux = rng.uniform(5.0e3, 5.0e4, 65) * np.where(rng.uniform(size=65) < 0.2, -1.0, 1.0)
    return Scene('counts', img, rms, mask, x, y, flux, model_gaussian(1), 1, GAIN, 2.0, tuple(f's{k}' for k in range(65)), (), ())


def _exact(name, base, fakes):
    img = np.full((40, 64), base, np.float32)
    x, y, f = (np.array([t[k] for t in fakes], dtype=np.float64) for k in (0, 1, 2))
    return Scene(name, img, np.ones((40, 64), np.float32), np.zeros((40, 64), np.int32), x, y, f, model_dyadic(), 1, 0.0, 2.0,
                 tuple(f'f{k}' for k in range(len(fakes))), (), ())


# a - b - c at integer positions with the dyadic model: the boxes (9 px) of a and b and of b and c share pixels, those of a
# and c do not; a and b also share written pixels.  Fluxes are powers of two on a plane of zeros: every sum is exact.
_A, _B, _C = (20.0, 20.0, 1024.0), (22.0, 21.0, 64.0), (30.0, 20.0, 4096.0)
CHAIN_ORDERS = {'abc': (_A, _B, _C), 'bac': (_B, _A, _C), 'acb': (_A, _C, _B), 'cba': (_C, _B, _A)}
CHAIN_LAYERS = {'abc': (1, 2, 3), 'bac': (1, 2, 2), 'acb': (1, 1, 2), 'cba': (1, 2, 3)}


@functools.lru_cache(maxsize=None)
def chain(order):
    return _exact(f'chain-{order}', 0.0, CHAIN_ORDERS[order])


@functools.lru_cache(maxsize=None)
def same_position():
    """Two fakes on one position and a third on top of both, plane of zeros: exact sums."""
    return _exact('same-position', 0.0, ((31.0, 17.0, 512.0), (31.0, 17.0, -128.0), (32.0, 18.0, 2048.0)))


@functools.lru_cache(maxsize=None)
def order_matters(reverse):
    """A plane of ones and two fakes on one position whose centre pixel gets 2^-24 and 2^-23: 1 + 2^-24 is a tie that
    rounds to 1, then + 2^-23 gives 1 + 2^-23; the other way round 1 + 2^-23 + 2^-24 is a tie that rounds to 1 + 2^-22."""
    a, b = (25.0, 15.0, 2.0 ** -22), (25.0, 15.0, 2.0 ** -21)
    return _exact(f'order-{"ba" if reverse else "ab"}', 1.0, (b, a) if reverse else (a, b))


def tolerance_scenes():
    """The scenes compared by the pixel rule."""
    return [interior(h) for h in (1, 12, 15)] + [edges(h) for h in (1, 12, 15)] + [counts()]


def exact_scenes():
    return [chain(o) for o in CHAIN_ORDERS] + [same_position(), order_matters(False), order_matters(True)]
