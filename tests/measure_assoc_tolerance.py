"""Prints what the bound on ``sep`` of the cross-match tests is taken from: over exactly the scenes of
tests/test_associate_gpu.py (tests/assoc_ref.py: xm_scene), the error - in units of eps64 radians - of

* the restatement's haversine separation, and
* an fp64 evaluation of the chord between unit vectors (the formula class of csrc/associate.hip, evaluated with numpy:
  no GPU, nothing of the kernel's output),

each against an extended-precision evaluation (mpmath at 50 digits when it imports, else numpy.longdouble), and the
bound the GPU is held to: SEP_K = 4 x the largest of them, rounded up to the next power of two.
No GPU needed:  python tests/measure_assoc_tolerance.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import assoc_ref as ar  # noqa: E402


def exact_sep(ra1, dec1, ra2, dec2):
    try:
        import mpmath as mp
        mp.mp.dps = 50
        out = []
        for a1, d1, a2, d2 in zip(ra1, dec1, ra2, dec2):
            a1, d1, a2, d2 = (mp.mpf(float(v)) * mp.pi / 180 for v in (a1, d1, a2, d2))
            h = mp.sin((d2 - d1) / 2) ** 2 + mp.cos(d1) * mp.cos(d2) * mp.sin((a2 - a1) / 2) ** 2
            out.append(float(2 * mp.asin(mp.sqrt(h)) * 648000 / mp.pi))
        return np.array(out), 'mpmath, 50 digits'
    except ImportError:
        L = np.longdouble
        a1, d1, a2, d2 = (np.asarray(v, L) * L(np.pi) / L(180) for v in (ra1, dec1, ra2, dec2))
        h = np.sin((d2 - d1) / 2) ** 2 + np.cos(d1) * np.cos(d2) * np.sin((a2 - a1) / 2) ** 2
        return np.asarray(2 * np.arcsin(np.sqrt(h)) * L(648000) / L(np.pi), np.float64), 'numpy.longdouble'


def chord_sep(ra1, dec1, ra2, dec2):
    def unit(ra, dec):
        a, d = ra * (np.pi / 180.0), dec * (np.pi / 180.0)
        return np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)
    x1, y1, z1 = unit(ra1, dec1)
    x2, y2, z2 = unit(ra2, dec2)
    d2 = (x2 - x1) ** 2 + (y2 - y1) ** 2 + (z2 - z1) ** 2
    return 2.0 * np.arcsin(np.minimum(1.0, 0.5 * np.sqrt(d2))) * ar.ARCSEC_PER_RAD


def main():
    worst = 0.0
    for name in ('field', 'wrap', 'ra90', 'north', 'south'):
        ra, dec, cra, cdec, r = ar.xm_scene(name)
        idx, sep = ar.crossmatch_ref(ra, dec, cra, cdec, r)
        hit = idx >= 0
        ex, how = exact_sep(ra[hit], dec[hit], cra[idx[hit]], cdec[idx[hit]])
        unit = ar.EPS64 * ar.ARCSEC_PER_RAD
        e_h = np.abs(sep[hit] - ex).max() / unit
        e_c = np.abs(chord_sep(ra[hit], dec[hit], cra[idx[hit]], cdec[idx[hit]]) - ex).max() / unit
        worst = max(worst, e_h, e_c)
        print(f'{name:<6} {int(hit.sum()):>4} matches of {ra.size:>4}: haversine restatement {e_h:6.2f} eps64 rad, '
              f'fp64 unit-vector chord {e_c:6.2f} eps64 rad   (against {how})')
    k = 1
    while k < 4 * worst:
        k *= 2
    print(f'largest {worst:.2f} eps64 rad; x 4 = {4 * worst:.2f}; next power of two = {k}; tests/assoc_ref.py holds '
          f'SEP_K = {ar.SEP_K} ({ar.SEP_TOL_ARCSEC:.3e} arcsec)')


if __name__ == '__main__':
    main()
