"""Repeats the measurement of tests/measure_assoc_tolerance.py on the scenes of tests/test_cone_gpu.py
(tests/cone_ref.py: scene): over every (query, row) pair within 30 arcsec, the error - in units of eps64 radians - of

* the restatement's haversine separation, and
* an fp64 evaluation of the chord between unit vectors (the formula class of csrc/skyindex.hip, evaluated with numpy:
  no GPU, nothing of the kernel's output),

each against an extended-precision evaluation (mpmath at 50 digits when it imports, else numpy.longdouble).  The cone
tests hold ``sep`` to ``assoc_ref.SEP_TOL_ARCSEC`` (SEP_K = 16 eps64 radians), which was taken as 4 x the largest error
measured on the cross-match scenes; if the largest error printed here ever exceeded 4, that bound would have to be looked
at again - not widened silently.
No GPU needed:  python tests/measure_cone_tolerance.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import assoc_ref as ar  # noqa: E402
import cone_ref as cr  # noqa: E402
from measure_assoc_tolerance import chord_sep, exact_sep  # noqa: E402


def main():
    worst = 0.0
    unit = ar.EPS64 * ar.ARCSEC_PER_RAD
    for name in cr.SCENES:
        ra, dec, cra, cdec = cr.scene(name)
        sep = ar.separation(ra, dec, cra, cdec)
        i, j = np.nonzero(np.isfinite(sep) & (sep <= cr.R_KNN))
        if i.size > 4000:                                 # (mpmath is slow: an evenly spread subset of the pairs)
            pick = np.linspace(0, i.size - 1, 4000).astype(np.int64)
            i, j = i[pick], j[pick]
        ex, how = exact_sep(ra[i], dec[i], cra[j], cdec[j])
        e_h = np.abs(sep[i, j] - ex).max(initial=0.0) / unit
        e_c = np.abs(chord_sep(ra[i], dec[i], cra[j], cdec[j]) - ex).max(initial=0.0) / unit
        worst = max(worst, e_h, e_c)
        print(f'{name:<10} {i.size:>5} pairs within {cr.R_KNN:g} arcsec: haversine restatement {e_h:6.2f} eps64 rad, '
              f'fp64 unit-vector chord {e_c:6.2f} eps64 rad   (against {how})')
    print(f'largest {worst:.2f} eps64 rad (revisit the bound above 4); tests/assoc_ref.py holds SEP_K = {ar.SEP_K} '
          f'({ar.SEP_TOL_ARCSEC:.3e} arcsec)')


if __name__ == '__main__':
    main()
