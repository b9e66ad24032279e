"""An aperture reference that shares no formula with ``oracle/photometry.py`` or ``csrc/photometry.hip``.

The product and its oracle both evaluate the circle / pixel overlap as a signed sum of four quarter-box areas, each a
closed form in sqrt and asin.  Here the same area is the integral of the chord height across the box,

    A = int_{max(x0, -r)}^{min(x1, r)} max(0, min(y1, s(u)) - max(y0, -s(u))) du,      s(u) = sqrt(r^2 - u^2),

with u = r sin(theta), so that s = r cos(theta) and the integrand is a trigonometric polynomial of degree 2 between the
angles where s(u) meets |y0| or |y1|.  The range is cut at those angles and each piece gets a fixed 48-point
Gauss-Legendre rule (exact for such a piece up to rounding).  The integrand is a positive weight times a clamped height:
the result is never negative, and a wrongly placed cut costs the square of its displacement, so an edge that is within
rounding of tangent to the circle loses nothing here (the closed form loses r^2 sqrt(eps) there).
``tests/test_aperture_ref.py`` holds this file against a 50-digit evaluation by a third route.

The bounding box is photutils' ``BoundingBox.from_float(x - r, x + r, y - r, y + r)`` as its documentation defines it:
pixel i covers [i - 0.5, i + 0.5], the box is [floor(x - r + 0.5), ceil(x + r + 0.5)) and it is clipped to the frame.
Flags are the OR of the mask over that box (not the circle); sums are ``math.fsum`` of float64 products, so summation
order is not a variable.  A pixel that is not finite makes the sum it enters NaN wherever in the box it lies (the
reference multiplies the cutout by the weights and sums: 0 * NaN = NaN), DESIGN.md "Forced aperture photometry".

numpy only.
"""
import math

import numpy as np

NGL = 48
_GX, _GW = np.polynomial.legendre.leggauss(NGL)
_CHUNK = 1 << 15          # boxes per quadrature call: 5 pieces x 48 nodes x 8 B each

EPS = float(np.finfo(np.float64).eps)
RADII = (0.3, 0.5, math.sqrt(0.5), 1.2, 3.0, 7.5, 30.0, 200.0, 511.0)
# Two regimes of the closed form (oracle and kernel alike), both measured against this file, never against each other.
# The closed form takes sqrt(r^2 - u^2) and asin(u / r), which turn a rounding of u into eps / sqrt(2 (1 - u / r)) of the
# angle.  Near-tangent: a u within TANGENT_REL r of r (edges_near_tangent says when); the amplification is sqrt(eps) at
# most, the derived bound 4 r^2 sqrt(eps).  Generic: every other pixel; the amplification is below 707 there and the
# limit is GENERIC_C eps r^2 per pixel fraction, GENERIC_C = max(64, 4 x the worst oracle - reference difference of
# tests/test_aperture_ref.py in units of eps r^2).  That worst is 96.9 (r = 200; 67.9 at r = 511, 46.7 at r = 30, below
# 20 for r <= 7.5): large apertures have the pixels that come close to the border of the regime.
GENERIC_C = 388.0
TANGENT_REL = 1e-6


def generic_limit(r):
    return GENERIC_C * EPS * r * r


def tangent_limit(r):
    return 4.0 * r * r * math.sqrt(EPS)


def pixel_edges(i, j, xc, yc):
    """Edges of pixel (i, j) seen from the centre (xc, yc), formed as the kernel forms them: ``i - 0.5 - xc`` (the
    half is exact, the difference is rounded once)."""
    i, j, xc, yc = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (i, j, xc, yc)))
    return i - 0.5 - xc, i + 0.5 - xc, j - 0.5 - yc, j + 0.5 - yc


def edges_near_tangent(x0, x1, y0, y1, r):
    """True where the closed form's ill-conditioned corner is in reach: sqrt(r^2 - u^2) and asin(u / r) are taken at
    a u within TANGENT_REL * r of r.  u is an edge (it lies that close to tangent to the circle) or the end
    sqrt(r^2 - e^2) of the chord along an edge e (it passes within sqrt(2 TANGENT_REL) r = 1.4e-3 r of the centre)."""
    e = np.abs(np.stack(np.broadcast_arrays(x0, x1, y0, y1)))
    chord = np.sqrt(np.maximum(r * r - e * e, 0.0))
    return (np.minimum(np.abs(r - e), np.where(e < r, r - chord, np.inf)) <= TANGENT_REL * r).any(axis=0)


def near_tangent(dx, dy, r):
    """The same for the unit pixel centred (dx, dy) from the circle's centre."""
    return edges_near_tangent(*pixel_edges(dx, dy, 0.0, 0.0), r)


def edges_limit(x0, x1, y0, y1, r):
    return np.where(edges_near_tangent(x0, x1, y0, y1, r), tangent_limit(r), generic_limit(r))


# circle centres relative to a pixel centre: the pixel centre, a corner, two edge midpoints
SPECIAL_CENTRES = [(0.0, 0.0), (0.5, 0.5), (0.5, 0.0), (0.0, 0.5)]
# centres built so that an edge is a hair from tangent when r is an integer or a half-integer
TANGENT_CENTRES = [(1e-9, 0.0), (0.5 - 1e-9, 0.5), (0.0, -1e-9), (0.5, 0.5 + 1e-9), (3e-13, 0.5 - 2e-12)]


def ring_cases(r, centres, rng, nfill=200):
    """Pixel offsets (dx, dy) from the circle's centre: every pixel with |d - r| < 1.5 and ``nfill`` more from the
    interior and from beyond, for each centre (given relative to a pixel centre)."""
    n = int(math.ceil(r)) + 3
    g = np.arange(-n, n + 1, dtype=np.float64)
    dxs, dys = [], []
    for cx, cy in centres:
        dx, dy = np.meshgrid(g - cx, g - cy)
        ring = np.abs(np.hypot(dx, dy) - r) < 1.5
        rest = np.flatnonzero(~ring.ravel())
        sel = ring.ravel().copy()
        sel[rng.choice(rest, min(nfill, rest.size), replace=False)] = True
        dxs.append(dx.ravel()[sel])
        dys.append(dy.ravel()[sel])
    return np.concatenate(dxs), np.concatenate(dys)


def _quad(x0, x1, y0, y1, r):
    """The integral above for flat arrays of boxes that the circle's outline crosses."""
    a = np.maximum(x0, -r)
    b = np.minimum(x1, r)
    ta = np.arcsin(np.clip(a / r, -1.0, 1.0))
    tb = np.arcsin(np.clip(b / r, -1.0, 1.0))
    tb = np.maximum(tb, ta)
    cuts = [ta]
    for yy in (y0, y1):
        k = np.arccos(np.minimum(np.abs(yy) / r, 1.0))      # s(u) = |yy| at theta = +-k; k = 0 when the edge is outside
        cuts += [np.clip(-k, ta, tb), np.clip(k, ta, tb)]
    cuts.append(tb)
    t = np.sort(np.stack(cuts, axis=0), axis=0)              # 6 x n: five pieces, some of length 0
    lo, hi = t[:-1], t[1:]
    half = 0.5 * (hi - lo)
    th = (0.5 * (hi + lo))[..., None] + half[..., None] * _GX          # 5 x n x NGL
    s = r * np.cos(th)
    h = np.minimum(y1[None, :, None], s) - np.maximum(y0[None, :, None], -s)
    f = np.maximum(h, 0.0) * s
    return ((f * _GW).sum(axis=-1) * half).sum(axis=0)


def overlap_area(x0, x1, y0, y1, r):
    """Area of circle(r, centre 0) within [x0, x1] x [y0, y1] (x0 <= x1, y0 <= y1), arrays of one shape.
    A box wholly inside gives its own area, a box wholly outside (touching included) exactly 0."""
    x0, x1, y0, y1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (x0, x1, y0, y1)))
    shape = x0.shape
    x0, x1, y0, y1 = (v.ravel() for v in (x0, x1, y0, y1))
    r = float(r)
    fx, fy = np.maximum(np.abs(x0), np.abs(x1)), np.maximum(np.abs(y0), np.abs(y1))      # farthest corner
    nx, ny = np.clip(0.0, x0, x1), np.clip(0.0, y0, y1)                                  # nearest point of the box
    inside = fx * fx + fy * fy <= r * r
    outside = nx * nx + ny * ny >= r * r
    out = np.where(inside, (x1 - x0) * (y1 - y0), 0.0)
    todo = np.flatnonzero(~inside & ~outside)
    for c in range(0, todo.size, _CHUNK):
        i = todo[c:c + _CHUNK]
        out[i] = _quad(x0[i], x1[i], y0[i], y1[i], r)
    return out.reshape(shape)


def edges_fraction(x0, x1, y0, y1, r):
    """Fraction of a unit pixel with these edges that lies inside the circle: exactly 1 for a pixel wholly inside,
    exactly 0 for one wholly outside, never negative."""
    area = overlap_area(x0, x1, y0, y1, r)
    fx, fy = np.maximum(np.abs(x0), np.abs(x1)), np.maximum(np.abs(y0), np.abs(y1))
    return np.where(fx * fx + fy * fy <= float(r) * float(r), 1.0, area)


def pixel_fraction(dx, dy, r):
    """The same for the unit pixel centred (dx, dy) from the circle's centre."""
    return edges_fraction(*pixel_edges(dx, dy, 0.0, 0.0), r)


def boxes(x, y, r, nx, ny):
    """Clipped bounding boxes [i0, i1) x [j0, j1) as int64 arrays, and which positions have one.  A position that is
    not finite, or whose box misses the frame, has none."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ok = np.isfinite(x) & np.isfinite(y)
    with np.errstate(invalid='ignore', over='ignore'):
        i0 = np.clip(np.floor(x - r + 0.5), 0, nx)      # clipped while still float: 1e300 has no int
        i1 = np.clip(np.ceil(x + r + 0.5), 0, nx)
        j0 = np.clip(np.floor(y - r + 0.5), 0, ny)
        j1 = np.clip(np.ceil(y + r + 0.5), 0, ny)
    i0, i1, j0, j1 = (np.where(ok, v, 0).astype(np.int64) for v in (i0, i1, j0, j1))
    ok &= (i1 > i0) & (j1 > j0)
    return i0, i1, j0, j1, ok


def aperture_sums(data, rms, mask, x, y, r, with_terms=False):
    """(flux, fluxerr, flags) at 0-based positions; rms and mask may be None (fluxerr 0, flags 0).
    ``with_terms`` adds what the tests' error bounds are made of, one row per quantity and a column per position:
    the allowance for the fractions, sum |data| * (the limit of each pixel's regime), over the box; sum |data * frac|;
    the same two for rms^2; the number of pixels in the box."""
    data = np.asarray(data)
    ny, nx = data.shape
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    y = np.atleast_1d(np.asarray(y, dtype=np.float64))
    n = x.size
    r = float(r)
    flux, err, flags = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    terms = np.zeros((5, n))
    if not (r > 0 and math.isfinite(r)):
        return (flux, err, flags, terms) if with_terms else (flux, err, flags)
    m32 = None if mask is None else np.asarray(mask).astype(np.int32)
    i0, i1, j0, j1, ok = boxes(x, y, r, nx, ny)
    old = np.seterr(invalid='ignore', over='ignore')          # non-finite pixels are handled by hand below
    for k in np.flatnonzero(ok):
        sl = (slice(j0[k], j1[k]), slice(i0[k], i1[k]))
        edges = pixel_edges(np.arange(i0[k], i1[k])[None, :], np.arange(j0[k], j1[k])[:, None], x[k], y[k])
        frac = edges_fraction(*edges, r).ravel()
        lim = edges_limit(*edges, r).ravel() if with_terms else 0.0
        d = data[sl].astype(np.float64).ravel()
        fin = np.isfinite(d)
        flux[k] = math.fsum(d * frac) if fin.all() else np.nan
        terms[0, k], terms[1, k], terms[4, k] = (np.abs(d) * lim)[fin].sum(), np.abs(d * frac)[fin].sum(), d.size
        if rms is not None:
            v = np.asarray(rms)[sl].astype(np.float64).ravel() ** 2
            fin = np.isfinite(v)
            err[k] = math.sqrt(math.fsum(v * frac)) if fin.all() else np.nan
            terms[2, k], terms[3, k] = (v * lim)[fin].sum(), (v * frac)[fin].sum()
        if m32 is not None:
            flags[k] = np.bitwise_or.reduce(m32[sl], axis=None)
    np.seterr(**old)
    return (flux, err, flags, terms) if with_terms else (flux, err, flags)


def sums_bounds(terms):
    """(flux bound, variance bound) per position from ``with_terms``: what the fractions may be off by, plus n
    roundings of a float64 sum of n products whose absolute values add up to sum |data * frac|."""
    alw, sfrac, valw, vfrac, n = terms
    return alw + n * EPS * sfrac, valw + (n + 4) * EPS * vfrac
