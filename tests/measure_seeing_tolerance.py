"""Measures the float64 oracle's own error on the moments scenes of tests/seeing_scenes.py: the iteration of
``oracle.detect.star_fwhm`` - same window, same exits, same stopping rule - evaluated in extended precision (mpmath at
50 digits when it imports, else numpy.longdouble) on every star of every scene, and against it

* the relative error of the oracle's FWHM, and
* the absolute error of its centroid (cx, cy), in pixels,

over the stars whose answer is finite; a star that leaves through an exit must leave through the same one, in the same
round.  ``tests/test_seeing_gpu.py`` holds the kernel to 8 x the largest figure printed here, rounded up to one digit,
as long as that is below the suite's ceilings (rtol 1e-9, atol 1e-8); its docstring quotes the figures.  The weight is
evaluated as a product of a row and a column factor, exp(-dx^2 / 2 s2) exp(-dy^2 / 2 s2), which at 50 digits is the
same number and costs one exponential per row and column instead of one per pixel.
No GPU needed:  python tests/measure_seeing_tolerance.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import seeing_scenes as ss  # noqa: E402
from oracle import detect as odet  # noqa: E402

try:
    import mpmath
    mpmath.mp.dps = 50
    HOW = 'mpmath, 50 digits'
    num, exp, sqrt = mpmath.mpf, mpmath.exp, mpmath.sqrt
except ImportError:                                          # pragma: no cover
    HOW = 'numpy.longdouble'
    num, exp, sqrt = np.longdouble, np.exp, np.sqrt


def exact_star(img, x, y, half=10, maxit=25):
    """(fwhm, cx, cy, exit, round) in extended precision; fwhm is None where the oracle's is NaN.  A window with a
    pixel that is not finite is not evaluated (None for all five)."""
    ny, nx = img.shape
    j0, j1 = max(y - half, 0), min(y + half + 1, ny)
    i0, i1 = max(x - half, 0), min(x + half + 1, nx)
    j1, i1 = max(j1, j0), max(i1, i0)
    win = img[j0:j1, i0:i1]
    if not np.isfinite(win).all():
        return None, None, None, None, None
    rows = [[num(float(v)) for v in r] for r in win]
    cols, lines = [num(i) for i in range(i0, i1)], [num(j) for j in range(j0, j1)]
    cx, cy, s2 = num(x), num(y), num(4)
    out = None

    def weight(a):
        # a factor below the smallest double is zero, as it is in float64: the t0 exit of the scene ``exits``
        # (a centroid 99 px away) is that underflow
        return exp(a) if a > -745 else num(0)

    def sums(second):
        ex = [weight(-(i - cx) ** 2 / (2 * s2)) for i in cols]
        ey = [weight(-(j - cy) ** 2 / (2 * s2)) for j in lines]
        a = b = c = num(0)
        for r, j, wy in zip(rows, lines, ey):
            r0 = r1 = r2 = num(0)
            for v, i, wx in zip(r, cols, ex):
                w = wx * v
                r0 += w
                if second:
                    r2 += w * (i - cx) ** 2
                else:
                    r1 += w * i
            a += wy * r0
            if second:
                b += wy * r2
                c += wy * r0 * (j - cy) ** 2
            else:
                b += wy * r1
                c += wy * r0 * j
        return a, b, c

    for it in range(1, maxit + 1):
        s0, s1x, s1y = sums(False)
        if not s0 > 0:
            return out, cx, cy, 's0', it
        cx, cy = s1x / s0, s1y / s0
        t0, sxx, syy = sums(True)
        if not t0 > 0:
            return out, cx, cy, 't0', it
        m2 = (sxx + syy) / (2 * t0)
        if not m2 > 0:
            return out, cx, cy, 'm2', it
        inv = 1 / m2 - 1 / s2
        if not inv > 0:
            return out, cx, cy, 'inv', it
        ns2 = 1 / inv
        done = abs(ns2 - s2) <= num(1e-8) * ns2
        s2 = ns2
        out = num(ss.K_FWHM) * sqrt(s2)
        if done:
            return out, cx, cy, 'done', it
    return out, cx, cy, 'cap', maxit


def measure(name):
    """(stars with a finite answer, largest relative error of the FWHM, largest absolute error of cx / cy, stars
    that were not evaluated) on one scene; raises when an exit or a round differs."""
    sc = ss.MOMENTS[name]()
    nfin = skipped = 0
    e_fw = e_c = 0.0
    for x, y in zip(sc.x.tolist(), sc.y.tolist()):
        fw, cx, cy, why, it = exact_star(sc.img, x, y, sc.half)
        if why is None:
            skipped += 1
            continue
        t = ss.trace(sc.img, x, y, sc.half)
        o = odet.star_fwhm(sc.img, x, y, sc.half)
        if (why, it) != (t.exit, t.rounds):
            raise AssertionError(f'{name} ({x}, {y}): extended precision leaves through {why} in round {it}, '
                                 f'float64 through {t.exit} in round {t.rounds}')
        if np.isfinite(o[1]) and np.isfinite(o[2]):
            e_c = max(e_c, float(abs(num(float(o[1])) - cx)), float(abs(num(float(o[2])) - cy)))
        if fw is None:
            assert np.isnan(o[0]), (name, x, y)
            continue
        nfin += 1
        e_fw = max(e_fw, float(abs(num(float(o[0])) - fw) / fw))
    return nfin, e_fw, e_c, skipped


def round_up(v):
    """v rounded up to one significant digit."""
    if v == 0:
        return 0.0
    e = int(np.floor(np.log10(v)))
    return float(f'{np.ceil(v / 10.0 ** e - 1e-12):.0f}e{e}')


def main():
    w_fw = w_c = 0.0
    for name in ss.MOMENTS:
        nfin, e_fw, e_c, skipped = measure(name)
        w_fw, w_c = max(w_fw, e_fw), max(w_c, e_c)
        print(f'{name:<15} {nfin:>2} finite stars: FWHM {e_fw:.2e} relative, centroid {e_c:.2e} px'
              f'   ({skipped} not evaluated: a pixel that is not finite; against {HOW})', flush=True)
    print(f'largest: FWHM {w_fw:.2e} relative, centroid {w_c:.2e} px;  8 x, rounded up: rtol {round_up(8 * w_fw):.0e}, '
          f'atol {round_up(8 * w_c):.0e}  (ceilings: rtol 1e-9, atol 1e-8)')


if __name__ == '__main__':
    main()
