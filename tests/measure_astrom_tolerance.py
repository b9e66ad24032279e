"""Measures the tolerance of tests/test_astrometry_gpu.py on the test's own scenes (tests/astrom_scenes.py).

For every frame the restatement solves, the last fit (its match list and keep set) is solved three ways:

* with mpmath at 50 digits, from the fp64 inputs on: (u, v) from the pixels, the stars' gnomonic (xi, eta), the weights,
  the normal equations and their solution; the coefficients are rounded to fp64 once, at the end;
* by the restatement (``numpy.linalg.lstsq`` on the weighted design matrix);
* by fp64 normal equations (``numpy.linalg.solve`` on A^T W A), which is what the kernel does, in another order of sums.

A header's deviation is what the test measures: the largest sky separation from the 50-digit header on a 9 x 9 grid of
pixels (``astrom_ref.grid_separation``, which carries the rounding of the fp64 evaluation of both sides), and the
difference of the rms residuals.  The bound of the test is 4 x the worst deviation of the fp64 normal equations, rounded
up to a power of two.  Run: python tests/measure_astrom_tolerance.py"""
import math
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import astrom_ref as am                                                  # noqa: E402
import astrom_scenes as sc                                               # noqa: E402
from oracle.wcs import NPV, WCS                                          # noqa: E402

mp.mp.dps = 50


def mp_gnomonic(ra, dec, ra0, dec0):
    a, d, a0, d0 = (mp.radians(mp.mpf(float(v))) for v in (ra, dec, ra0, dec0))
    cosc = mp.sin(d0) * mp.sin(d) + mp.cos(d0) * mp.cos(d) * mp.cos(a - a0)
    xi = mp.cos(d) * mp.sin(a - a0) / cosc
    eta = (mp.cos(d0) * mp.sin(d) - mp.sin(d0) * mp.cos(d) * mp.cos(a - a0)) / cosc
    return mp.degrees(xi), mp.degrees(eta)


def wcs_from(w, c1, c2, s, ncoef):
    pv1, pv2 = np.zeros(NPV), np.zeros(NPV)
    for k in range(ncoef):
        deg = sum(am.EXPONENTS[k])
        pv1[am.TPV_INDEX[k]] = float(c1[k] / s ** deg)
        pv2[am.TPV_INDEX[k]] = float(c2[k] / s ** deg)
    return WCS(w.crpix, w.crval, w.cd, pv1, pv2, w.naxis)


def three_ways(w0, det, ref, r, params):
    p = dict(am.DEFAULTS, **params)
    ncoef = am.NCOEF[p['degree']]
    x, y, sd, _ = (np.asarray(v, np.float64) for v in det)
    rows = np.flatnonzero(r['used'] != 0)
    j = r['match'][rows]
    s = am.scale_of(w0)
    pixscale = 3600.0 * math.sqrt(abs(np.linalg.det(w0.cd)))
    # 50 digits
    ms = mp.mpf(s)
    A1, A2 = mp.zeros(ncoef), mp.zeros(ncoef)
    b1, b2 = mp.zeros(ncoef, 1), mp.zeros(ncoef, 1)
    rows_mp = []
    for i, k in zip(rows, j):
        dx, dy = mp.mpf(float(x[i])) - mp.mpf(float(w0.crpix[0])), mp.mpf(float(y[i])) - mp.mpf(float(w0.crpix[1]))
        a = (mp.mpf(float(w0.cd[0, 0])) * dx + mp.mpf(float(w0.cd[0, 1])) * dy) / ms
        b = (mp.mpf(float(w0.cd[1, 0])) * dx + mp.mpf(float(w0.cd[1, 1])) * dy) / ms
        xi, eta = mp_gnomonic(ref[0][k], ref[1][k], w0.crval[0], w0.crval[1])
        wt = 1 / ((mp.mpf(float(sd[i])) * mp.mpf(pixscale)) ** 2 + mp.mpf(float(ref[2][k])) ** 2)
        f1 = [a ** e * b ** g for e, g in am.EXPONENTS[:ncoef]]
        f2 = [b ** e * a ** g for e, g in am.EXPONENTS[:ncoef]]
        rows_mp.append((f1, f2, xi, eta))
        for u in range(ncoef):
            b1[u] += wt * f1[u] * xi
            b2[u] += wt * f2[u] * eta
            for v in range(ncoef):
                A1[u, v] += wt * f1[u] * f1[v]
                A2[u, v] += wt * f2[u] * f2[v]
    c1, c2 = mp.lu_solve(A1, b1), mp.lu_solve(A2, b2)
    exact = wcs_from(w0, c1, c2, ms, ncoef)
    e1 = [3600 * (sum(c1[u] * f1[u] for u in range(ncoef)) - xi) for f1, _, xi, _ in rows_mp]
    e2 = [3600 * (sum(c2[u] * f2[u] for u in range(ncoef)) - eta) for _, f2, _, eta in rows_mp]
    rms_exact = (float(mp.sqrt(sum(v * v for v in e1) / len(e1))), float(mp.sqrt(sum(v * v for v in e2) / len(e2))))
    # fp64 normal equations
    dx, dy = x[rows] - w0.crpix[0], y[rows] - w0.crpix[1]
    a = (w0.cd[0, 0] * dx + w0.cd[0, 1] * dy) / s
    b = (w0.cd[1, 0] * dx + w0.cd[1, 1] * dy) / s
    sxi, seta, _ = am.gnomonic(ref[0][j], ref[1][j], w0.crval[0], w0.crval[1])
    wt = 1.0 / ((sd[rows] * pixscale) ** 2 + ref[2][j] ** 2)
    F1, F2 = am.design(a, b, ncoef), am.design(b, a, ncoef)
    n1 = np.linalg.solve(F1.T @ (F1 * wt[:, None]), F1.T @ (wt * sxi))
    n2 = np.linalg.solve(F2.T @ (F2 * wt[:, None]), F2.T @ (wt * seta))
    ne = wcs_from(w0, n1, n2, s, ncoef)
    r1, r2 = 3600.0 * (F1 @ n1 - sxi), 3600.0 * (F2 @ n2 - seta)
    rms_ne = (float(np.sqrt(np.mean(r1 ** 2))), float(np.sqrt(np.mean(r2 ** 2))))
    return dict(sep_ne=am.grid_separation(exact, ne), sep_ref=am.grid_separation(exact, r['wcs']),
                rms_ne=max(abs(rms_ne[0] - rms_exact[0]), abs(rms_ne[1] - rms_exact[1])),
                rms_ref=max(abs(r['rms'][0] - rms_exact[0]), abs(r['rms'][1] - rms_exact[1])))


def main():
    worst = dict(sep_ne=0.0, sep_ref=0.0, rms_ne=0.0, rms_ref=0.0)
    for name in sorted(sc.SCENES):
        (wcs_list, dets, ref, params), res = sc.reference(name)
        for f, r in enumerate(res):
            if r['status'] not in (am.OK, am.NOT_CONVERGED):
                continue
            m = three_ways(am.as_tpv(wcs_list[f]), dets[f], ref, r, params)
            print(f'{name:22s} frame {f}: normal equations {m["sep_ne"]:.3e} arcsec, rms {m["rms_ne"]:.3e}; '
                  f'restatement {m["sep_ref"]:.3e} arcsec, rms {m["rms_ref"]:.3e}')
            for k in worst:
                worst[k] = max(worst[k], m[k])
    w = max(worst['sep_ne'], worst['rms_ne'])
    print(f'worst: {worst}')
    print(f'bound: 4 x {w:.3e} = {4 * w:.3e} -> 2^{math.ceil(math.log2(4 * w))} = {2.0 ** math.ceil(math.log2(4 * w)):.3e} arcsec')


if __name__ == '__main__':
    main()
