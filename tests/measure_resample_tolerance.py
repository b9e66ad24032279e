"""Measures the tolerances of tests/test_resample_geometry_gpu.py on the test's own scenes (tests/resample_scenes.py).

The kernels do not evaluate the inverse map per pixel: they take fp64 lattice nodes every 16 output pixels, subtract
the origin of the tile's bounding box, round to fp32 and interpolate bilinearly in fp32.  ``resample_scenes.emulated_positions``
does the same in numpy float32; this script feeds those positions to ``oracle.resample.resample`` and prints, per scene,

* delta0: the largest distance of an emulated position from the exact one (covered pixels, the tile geometries of all
  three kernels), in pixels;
* the largest deviation of the LANCZOS3 values and weights from the exact-position oracle, in units of the existing
  bounds (2e-5 |ref| + 2e-5 std(img) for values, 5e-5 |ref| for weights);
* the bound that follows: 1 (the existing bound) where the deviation stays at or below 1, else 4 x the deviation.  The
  factor covers what the emulation leaves out: the fp32 tap table (2.4e-7 per tap), 36 fp32 products and one
  contraction difference between numpy and the device.

It measures the design against the reference and does not look at the GPU.  The last block is ``BOUNDS`` of
tests/resample_scenes.py, rounded up to three digits.

A second table answers where the fp32 tile-relative positions stop holding the existing bound: the geometry of
``coarser_2x`` (TAN, turned by 0.2 degrees, the same dither) at output pixels 1 to 8 times the input's, a 136 x 100
output each.  The footprint of a 64 x 32 tile is 64 x the factor wide, so the ulp of a position doubles at factors 2
and 4.  Run: python tests/measure_resample_tolerance.py"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np                                                       # noqa: E402

import resample_scenes as rs                                             # noqa: E402
from oracle import resample as oresample                                 # noqa: E402
from util import synth, to_oracle_wcs                                    # noqa: E402


def round_up(v, digits=3):
    if v == 0.0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(v)) - digits + 1)
    return float(f'{math.ceil(v / q) * q:.{digits}g}')


def scale_sweep(factors=(1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0), onx=136, ony=100):
    s = synth()
    print(f'\n{"factor":>6s} {"footprint [px]":>15s} {"delta0 [px]":>12s} {"values":>9s}')
    for k in factors:
        nx, ny = int(onx * k) + 24, int(ony * k) + 24
        win = s.ztf_wcs(nx, ny, dx=rs.SCALE_DITHER[0], dy=rs.SCALE_DITHER[1], rot_deg=0.2, tpv=False)
        wout = s.ztf_wcs(onx, ony, tpv=False)
        wout.cd = wout.cd * k
        f = s.make_frame(nx, ny, 4500, win, nstars=max(40, nx * ny // 900), nbad=nx * ny // 300)
        px, py = oresample.positions(to_oracle_wcs(wout), to_oracle_wcs(win), onx, ony)
        ex, ey = rs.emulate_map(win, wout)
        r_img, r_wgt, _ = oresample.resample(f['img'], f['wgt'], px, py)
        e_img, e_wgt, _ = oresample.resample(f['img'], f['wgt'], ex, ey)
        both = (r_wgt > 0) & (e_wgt > 0)
        cov = oresample.coverage(px, py, nx, ny)
        d0 = max(np.abs(ex - px)[cov].max(), np.abs(ey - py)[cov].max())
        tol = rs.RTOL * np.abs(r_img[both]) + rs.ATOL * float(np.std(f['img']))
        print(f'{k:6.1f} {64 * k + 8:15.0f} {d0:12.3e} {(np.abs(e_img - r_img)[both] / tol).max():9.3f}')


def main():
    rows = []
    print(f'{"scene":20s} {"delta0 [px]":>12s} {"values":>9s} {"weights":>9s} {"bound v":>9s} {"bound w":>9s}')
    for name in rs.SCENES:
        d0, dv, dw = rs.emulation(name)
        bv, bw = rs.bound_for(dv), rs.bound_for(dw)
        rows.append((name, round_up(d0), round_up(bv) if bv > 1 else 1.0, round_up(bw) if bw > 1 else 1.0))
        print(f'{name:20s} {d0:12.3e} {dv:9.3f} {dw:9.3f} {bv:9.3f} {bw:9.3f}')
    print('\nBOUNDS = {')
    for name, d0, bv, bw in rows:
        key = f"'{name}':"
        print(f'    {key:21s} ({d0!r}, {bv!r}, {bw!r}),')
    print('}')
    scale_sweep()


if __name__ == '__main__':
    main()
