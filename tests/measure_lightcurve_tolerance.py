"""Prints what the bound on ``x`` and ``y`` of tests/test_lightcurve_gpu.py is taken from: over exactly the joined pairs of
its scenes (tests/lightcurve_ref.py: the six frames, the batch of three, the count scenes), the error in pixels of

* the host's ``zm_wcs_sky2pix`` (``WCS.all_world2pix``: what stood between the planes and the aperture kernel before), and
* the float64 oracle (``oracle/wcs.py``: ``sky2pix``),

each against an extended-precision evaluation of the same map (mpmath at 50 digits when it imports, else
numpy.longdouble), and the bound the GPU is held to: POS_TOL_PX = 4 x the larger of the two, rounded up to the next
power of two.  No GPU needed (the host's sky2pix is plain C):  python tests/measure_lightcurve_tolerance.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import lightcurve_ref as lr  # noqa: E402


def _tpv_terms(x, y, r):
    """The TPV monomials of indices 0 .. 16 (axis 1; axis 2 swaps x and y)."""
    return [1, x, y, r, x * x, x * y, y * y, x ** 3, x * x * y, x * y * y, y ** 3, r ** 3, x ** 4, x ** 3 * y, x * x * y * y,
            x * y ** 3, y ** 4]


def exact_sky2pix(ow, ra, dec):
    """1-based pixel positions in extended precision."""
    pv1, pv2 = (np.asarray(ow.pv1), np.asarray(ow.pv2)) if ow.has_pv else (None, None)
    if ow.has_pv:
        assert not pv1[17:].any() and not pv2[17:].any()
    try:
        import mpmath as mp
        mp.mp.dps = 50
        F, how = mp.mpf, 'mpmath, 50 digits'
        sin, cos, sqrt, pi = mp.sin, mp.cos, mp.sqrt, mp.pi
    except ImportError:
        F, how = np.longdouble, 'numpy.longdouble'
        sin, cos, sqrt, pi = np.sin, np.cos, np.sqrt, np.longdouble(np.pi)
    d2r = pi / 180
    a0, d0 = F(float(ow.crval[0])) * d2r, F(float(ow.crval[1])) * d2r
    east = (-sin(a0), cos(a0), F(0))
    north = (-sin(d0) * cos(a0), -sin(d0) * sin(a0), cos(d0))
    pole = (cos(d0) * cos(a0), cos(d0) * sin(a0), sin(d0))
    cd = [[F(float(v)) for v in row] for row in np.asarray(ow.cd)]
    det = cd[0][0] * cd[1][1] - cd[0][1] * cd[1][0]
    xs, ys = [], []
    for a, d in zip(np.asarray(ra, dtype=np.float64), np.asarray(dec, dtype=np.float64)):
        a, d = F(float(a)) * d2r, F(float(d)) * d2r
        v = (cos(d) * cos(a), cos(d) * sin(a), sin(d))
        c = sum(p * q for p, q in zip(v, pole))
        xi = sum(p * q for p, q in zip(v, east)) / c / d2r
        eta = sum(p * q for p, q in zip(v, north)) / c / d2r
        u, w = xi, eta
        if ow.has_pv:
            p1, p2 = [F(float(t)) for t in pv1[:17]], [F(float(t)) for t in pv2[:17]]
            f = lambda p, x, y: sum(pk * tk for pk, tk in zip(p, _tpv_terms(x, y, sqrt(x * x + y * y))))
            h = F(10) ** -20
            for _ in range(40):
                r1, r2 = f(p1, u, w) - xi, f(p2, w, u) - eta
                j11, j12 = (f(p1, u + h, w) - f(p1, u - h, w)) / (2 * h), (f(p1, u, w + h) - f(p1, u, w - h)) / (2 * h)
                j21, j22 = (f(p2, w, u + h) - f(p2, w, u - h)) / (2 * h), (f(p2, w + h, u) - f(p2, w - h, u)) / (2 * h)
                dj = j11 * j22 - j12 * j21
                du, dw = (r1 * j22 - r2 * j12) / dj, (r2 * j11 - r1 * j21) / dj
                u, w = u - du, w - dw
                if abs(du) < F(10) ** -30 and abs(dw) < F(10) ** -30:
                    break
            else:
                raise AssertionError('the extended-precision TPV inverse did not converge')
        xs.append(float((cd[1][1] * u - cd[0][1] * w) / det + F(float(ow.crpix[0]))))
        ys.append(float((-cd[1][0] * u + cd[0][0] * w) / det + F(float(ow.crpix[1]))))
    return np.array(xs), np.array(ys), how


def scenes():
    """(name, product WCS, oracle WCS, ra, dec of its joined pairs) of every scene whose positions the GPU test compares."""
    out = []
    for name in lr.FRAMES:
        w, ow, ra, dec, _ = lr.frame_scene(name)
        _, idx = lr.membership([ow], ra, dec)
        out.append((name, w, ow, ra[idx], dec[idx]))
    ws, ows, _, ra, dec = lr.batch_scene()
    off, idx = lr.membership(ows, ra, dec)
    for k, (w, ow) in enumerate(zip(ws, ows)):
        j = idx[off[k]:off[k + 1]]
        out.append((f'batch[{k}]', w, ow, ra[j], dec[j]))
    for n in (63, 64, 65, 300):
        w, ow, ra, dec = lr.count_scene(n)
        _, idx = lr.membership([ow], ra, dec)
        out.append((f'count{n}', w, ow, ra[idx], dec[idx]))
    return out


def main():
    worst = 0.0
    for name, w, ow, ra, dec in scenes():
        ex, ey, how = exact_sky2pix(ow, ra, dec)
        hx, hy = w.all_world2pix(ra, dec, 1)
        ox, oy = ow.sky2pix(ra, dec)
        e_h = max(np.abs(hx - ex).max(), np.abs(hy - ey).max())
        e_o = max(np.abs(ox - ex).max(), np.abs(oy - ey).max())
        worst = max(worst, e_h, e_o)
        print(f'{name:<9} {ra.size:>4} pairs: host zm_wcs_sky2pix {e_h:.3e} px, float64 oracle {e_o:.3e} px   (against {how})')
    k = 1.0
    while k / 2 >= 4 * worst:
        k /= 2
    print(f'largest {worst:.3e} px; x 4 = {4 * worst:.3e}; next power of two = 2^{int(np.log2(k))} = {k:.3e} px; '
          f'tests/lightcurve_ref.py holds POS_TOL_PX = 2^{int(np.log2(lr.POS_TOL_PX))} = {lr.POS_TOL_PX:.3e} px '
          f'(tests/test_abi.py grants the host round trip 1e-7 px)')


if __name__ == '__main__':
    main()
