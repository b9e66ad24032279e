"""Where the tolerances of tests/inject_ref.py come from: the restatement alone, run twice on the scenes of
tests/inject_scenes.py - in float64 (what the GPU is held to) and with every tap, product and sum in numpy.longdouble.  Each
constant is 4 x the largest difference seen, rounded up to a power of two.  Nothing the GPU produced enters these numbers.
The script also counts the pixels on which the float32 planes of the two runs differ: the pixel rule's cap on near-tie
pixels presumes that there are none, and tests/test_inject_ref.py asserts it.

    python tests/measure_inject_tolerance.py           (a few seconds)
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inject_ref as ir         # noqa: E402
import inject_scenes as isc     # noqa: E402
from psf_scenes import BAD_BITS  # noqa: E402

LD = np.longdouble


def pow2_up(v):
    return 2.0 ** math.ceil(math.log2(4.0 * v)) if v > 0 else 0.0


def run(sc, T):
    return ir.inject(sc.img, sc.x, sc.y, sc.flux, sc.model, rms=sc.rms, mask=sc.mask, bad_bits=BAD_BITS, gain=sc.gain,
                     core_radius=sc.core_radius, T=T)


def measure_scene(sc):
    """dict(inj, sum_rel, rms_rel, disagree) of one scene."""
    a, b = run(sc, ir.F64), run(sc, LD)
    assert np.array_equal(a['flags'], b['flags']) and np.array_equal(a['nwrites'], b['nwrites'])
    assert np.array_equal(a['rms_nwrites'], b['rms_nwrites'])
    w = (b['nwrites'] > 0) & np.isfinite(b['base'])
    scale = np.abs(b['base'].astype(LD)) + np.abs(b['v'])
    inj = float(np.max(np.abs(a['v'].astype(LD) - b['v'])[w] / scale[w])) if w.any() else 0.0
    s64, sld = a['out_sum'].astype(LD), b['out_sum']
    ok = np.isfinite(sld) & (sld != 0)
    assert np.array_equal(np.isnan(s64), np.isnan(sld))
    sum_rel = float(np.max(np.abs(s64 - sld)[ok] / np.abs(sld[ok]))) if ok.any() else 0.0
    r = b['rms_nwrites'] > 0
    rms_rel = float(np.max(np.abs(a['rms_want'].astype(LD) - b['rms_want'])[r] / b['rms_want'][r])) if r.any() else 0.0
    same = ir.same_bits(a['img'], b['img']) & ir.same_bits(a['rms'], b['rms'])
    return dict(inj=inj, sum_rel=sum_rel, rms_rel=rms_rel, disagree=int((~same).sum()))


def measure():
    seen = dict(inj=0.0, sum_rel=0.0, rms_rel=0.0)
    disagree = {}
    for sc in isc.tolerance_scenes():
        m = measure_scene(sc)
        print(f'{sc.name}: flux P {m["inj"]:.3e} of |img| + |flux P|, out_sum rel {m["sum_rel"]:.3e}, rms rel {m["rms_rel"]:.3e}, '
              f'{m["disagree"]} pixel(s) on which the two precisions disagree')
        for k in seen:
            seen[k] = max(seen[k], m[k])
        disagree[sc.name] = m['disagree']
    return seen, disagree


CONSTANTS = (('INJ_TOL', 'inj'), ('SUM_RTOL', 'sum_rel'), ('RMS_TOL', 'rms_rel'))


def main():
    seen, disagree = measure()
    print('MEASURED =', {k: float(f'{v:.3e}') for k, v in seen.items()})
    for name, key in CONSTANTS:
        t = pow2_up(seen[key])
        print(f'{name} = 2.0 ** {int(math.log2(t)) if t else "-inf"}    (4 x {seen[key]:.3e} rounded up; inject_ref has '
              f'2.0 ** {int(math.log2(getattr(ir, name)))})')
    print('pixels on which float64 and longdouble disagree:', disagree)
    return seen, disagree


if __name__ == '__main__':
    main()
