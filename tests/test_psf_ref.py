"""The float64 restatement of the PSF photometry (tests/psf_ref.py) held to known answers, the conditions of the scenes
(tests/psf_scenes.py), the tolerance constants held to tests/measure_psf_tolerance.py, and the CPU side of psf.py
(settings, the model file, the header's section).  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import measure_psf_tolerance as mt
import psf_ref as pr
import psf_scenes as ps
from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_taps_sum_to_one_and_zero_is_the_identity():
    for d in (1e-12, 0.1, 0.5, 0.75, float(np.nextafter(1.0, 0.0))):
        t, k = pr.taps(d)
        assert list(k) == [-2, -1, 0, 1, 2, 3] and abs(t.sum() - 1.0) < 4e-16
    t, k = pr.taps(0.0)
    assert list(t) == [1.0] and list(k) == [0]
    seq = np.random.default_rng(0).normal(size=20)
    M, foot, out = pr.interp_matrix(np.arange(20.0), 20)
    assert np.array_equal(M @ seq, seq) and foot.sum() == 20 and not out.any()
    M, foot, out = pr.interp_matrix([1.5, 9.25, 17.5], 20)
    assert list(out) == [True, False, True] and list(foot.sum(1)) == [5, 6, 5]


def test_the_cutout_of_a_constant_image_is_the_constant():
    img = np.full((40, 48), 7.0, np.float32)
    c = pr.cutouts(img, [20.3, 24.0], [19.6, 18.5], [1.0, 1.0], [2.0, 3.0], 5)
    assert np.allclose(c[0], 3.0, rtol=0, atol=1e-14) and np.allclose(c[1], 2.0, rtol=0, atol=1e-14)
    c = pr.cutouts(img, [6.3], [19.6], [0.0], [1.0], 5)             # floor(x) - 5 - 2 = -1: the first column only
    assert np.isnan(c[0][:, 0]).all() and np.isfinite(c[0][:, 1:]).all()


def test_a_fit_of_a_profile_plus_a_constant_returns_both():
    model = ps.model_gaussian(12)
    x, y = 30.37, 28.81
    P = pr.fit(np.zeros((64, 64), np.float32), [x], [y], model, 6.0, 0)          # (for the pixel set only)
    i, j, ixd, iyd, fx, fy, _ = pr.circle_pixels(x, y, 6.0)
    Mx, _, _ = pr.interp_matrix(np.arange(-7, 8) - fx + 12, 25)
    My, _, _ = pr.interp_matrix(np.arange(-7, 8) - fy + 12, 25)
    prof = My @ model @ Mx.T
    img = np.zeros((64, 64))
    img[int(iyd) - 7:int(iyd) + 8, int(ixd) - 7:int(ixd) + 8] = 1234.5 * prof
    img += 17.25
    img32 = img.astype(np.float32)
    f = pr.fit(img32, [x], [y], model, 6.0, 1)
    assert P['npix'][0] == f['npix'][0] == i.size and f['flags'][0] == 0
    # the image is float32: a P + b holds to 2^-24 of a pixel value, and the fit returns a and b to that
    assert abs(f['flux'][0] - 1234.5) < 1e-3 and abs(f['sky'][0] - 17.25) < 1e-5
    assert f['chi2'][0] < i.size * (40.0 * 2.0 ** -24) ** 2
    f0 = pr.fit((img - 17.25).astype(np.float32), [x], [y], model, 6.0, 0)
    assert abs(f0['flux'][0] - 1234.5) < 1e-3 and f0['sky'][0] == 0.0


def test_with_uniform_noise_the_error_is_sigma_over_the_root_of_the_sum_of_squares():
    model = ps.model_gaussian(12)
    x, y, sigma = 31.3, 33.7, 2.5
    i, j, ixd, iyd, fx, fy, _ = pr.circle_pixels(x, y, 6.0)
    Mx, _, _ = pr.interp_matrix(i.astype(float) - fx + 12, 25)
    My, _, _ = pr.interp_matrix(j.astype(float) - fy + 12, 25)
    P = np.einsum('pa,ab,pb->p', My, model, Mx)
    img = np.random.default_rng(3).normal(0.0, sigma, (64, 64)).astype(np.float32)
    f = pr.fit(img, [x], [y], model, 6.0, 0, rms=np.full((64, 64), sigma, np.float32))
    assert abs(f['err'][0] - sigma / math.sqrt((P * P).sum())) < 1e-12
    assert abs(f['cover'][0] - 1.0) < 1e-15


def test_singular_and_flag_rules():
    s = ps.fit_main()
    f = pr.fit(s.img, s.x, s.y, s.model, 6.0, 1, rms=s.rms, mask=s.mask, bad_bits=ps.BAD_BITS)
    fl = dict(zip(s.names, f['flags']))
    npx = dict(zip(s.names, f['npix']))
    assert fl['fx-zero'] == 0 and fl['corner'] == pr.CLIPPED and fl['one-masked'] == pr.BAD
    assert fl['fully-outside'] == fl['huge'] == pr.CLIPPED | pr.SINGULAR and npx['far-outside'] == 0
    assert fl['all-masked'] == pr.BAD | pr.LOWCOVER | pr.SINGULAR and npx['all-masked'] == 0
    assert fl['one-left'] == pr.BAD | pr.LOWCOVER | pr.SINGULAR and npx['one-left'] == 1
    assert fl['rms-zero'] == fl['rms-nan'] == fl['rms-inf'] == pr.BADRMS and fl['nan-pixel'] == pr.NONFINITE
    assert fl['x-nan'] == fl['y-inf'] == pr.BADPOS
    sing = (f['flags'] & (pr.SINGULAR | pr.BADPOS)) != 0
    for k in ('flux', 'err', 'chi2', 'sky', 'cover'):
        assert np.array_equal(np.isnan(f[k]), sing), k
    f0 = pr.fit(s.img, s.x, s.y, s.model, 6.0, 0, rms=s.rms, mask=s.mask, bad_bits=ps.BAD_BITS)
    assert dict(zip(s.names, f0['flags']))['one-left'] == pr.BAD | pr.LOWCOVER           # one pixel fits one parameter
    with pytest.raises(ValueError):
        pr.fit(s.img, s.x, s.y, s.model, 8.6, 0)


def test_scene_conditions():
    """Not a tolerance: every pixel centre lies at least 1e-9 px from every fit circle and from the model's support
    radius, so npix, flags and supports are exact."""
    s = ps.fit_main()
    for R in sorted({c[0] for c in ps.FIT_CASES}):
        f = pr.fit(s.img, s.x, s.y, s.model, R, 0)
        assert f['margin'].min() >= ps.MARGIN, (R, s.names[int(np.argmin(f['margin']))])
    for half, r in ((3, 3.0), (4, 3.5), (12, 10.0)):
        jj, ii = np.mgrid[-half:half + 1, -half:half + 1]
        d = np.abs(np.sqrt(ii * ii + jj * jj) - r)
        # on the circle itself only where both squares are whole numbers: that comparison is exact
        assert d[d > 0].min() >= ps.MARGIN and float(r * r).is_integer() or d.min() >= ps.MARGIN
    g = ps.cutout_edges(12)
    c = pr.cutouts(g.img, g.x, g.y, g.sky, g.norm, 12, mask=g.mask, bad_bits=ps.BAD_BITS)
    nn = dict(zip(g.names, np.isnan(c).reshape(len(g.names), -1).sum(1)))
    assert nn['dx-zero'] == nn['dx-half'] == nn['dx-ulp-below-one'] == nn['generic'] == nn['dy-zero'] == 0
    assert nn['dx-zero-beside-bad-column'] == 0 and nn['off-frame-one-tap-left'] == 25
    assert nn['bad-under-one-tap'] == 6 and nn['nan-pixel'] == 36
    for k in ('norm-nan', 'norm-inf', 'norm-zero', 'norm-negative', 'sky-nan', 'x-nan', 'y-inf'):
        assert nn[k] == 625, k
    g = ps.model_floor()
    for floor, want in ((3, 3), (4, 0)):
        m, nu, _ = pr.build_model(g.img, g.x, g.y, g.sky, g.norm, half=4, norm_radius=3.5, clip_iter=0, min_stars_pixel=floor,
                                  mask=g.mask, bad_bits=ps.BAD_BITS)
        assert nu[4 + 1, 4 + 2] == 0 and m[4 + 1, 4 + 2] == 0.0
        assert nu[4 - 1, 4 + 1] == 2 and m[4 - 1, 4 + 1] == 0.0
        assert nu[4 + 2, 4 - 1] == 3 and (m[4 + 2, 4 - 1] != 0.0) == (want == 3)
        assert abs(m.sum() - 1.0) < 1e-15 and m[0, 0] == 0.0 and nu[0, 0] == 5


def test_phase_floor_and_error_ratio_as_measured():
    """Noiseless Gaussians through the operator's two interpolations: recovered / true flux over the sub-pixel phase per
    FWHM, printed and held to what measure_psf_tolerance.py printed (psf_ref.PHASE_FLOOR, to the 1e-4 it is written with);
    the error ratio to the r = 3 aperture is printed (motivation, no promise)."""
    for fwhm in (1.6, 2.0, 2.4, 3.0):
        lo, hi, med = mt.phase_floor(fwhm)
        ratio = mt.error_ratio(fwhm)
        print(f'FWHM {fwhm}: recovered / true {lo:.4f} .. {hi:.4f} (median {med:.4f}); error / r = 3 aperture error {ratio:.3f}')
        assert abs(lo - pr.PHASE_FLOOR[fwhm][0]) <= 1e-4 and abs(hi - pr.PHASE_FLOOR[fwhm][1]) <= 1e-4
        assert 0.98 < lo and hi < 1.01 and ratio < 1.0


def test_tolerance_constants_are_the_measuring_scripts():
    """The whole measurement again (a few seconds): every constant is 4 x the largest float64 - longdouble difference,
    rounded up to a power of two, and the figures written beside them are the ones measured."""
    seen = mt.measure()
    for name, key in mt.CONSTANTS:
        print(f'{name}: measured {seen[key]:.3e}, recorded {pr.MEASURED[key]:.3e}, constant 2^{int(math.log2(getattr(pr, name)))}')
        assert getattr(pr, name) == mt.pow2_up(seen[key]), name
        assert abs(seen[key] - pr.MEASURED[key]) <= 1e-3 * pr.MEASURED[key], name


def test_settings_and_model_file(tmp_path):
    z = pkg()
    p = z.psf
    st = p.psf_settings({'-PSF_HALF': '10', 'FIT_RADIUS': 5, '-ANNULUS': '20,30'})
    assert (st['psf_half'], st['fit_radius'], st['annulus'], st['norm_radius'], st['min_stars']) == (10, 5.0, (20.0, 30.0), 10.0, 10)
    assert (st['sn_min'], st['nmax'], st['min_stars_pixel'], st['fit_sky']) == (50.0, 1000, 3, 0)
    with pytest.raises(ValueError, match='not a key'):
        p.psf_settings({'-SEEING': 2})
    with pytest.raises(ValueError, match='3.5'):
        p.psf_settings({'-FIT_RADIUS': 9})
    with pytest.raises(ValueError, match='PSF_HALF'):
        p.psf_settings({'-PSF_HALF': 16})
    m = p.PSFModel(ps.model_gaussian(12) * (1.0 + 1e-16), cards={'PSFCOR': -0.0123456789012345, 'PSFCORUN': 1.5e-3, 'PSFNSTAR': 41,
                                                                  'PSFHALF': 12, 'PSFFITR': 6.0, 'PSFFWHM': 2.41, 'ZMPSF': True})
    path = m.save(tmp_path / 'sci.psf.fits')
    back = p.PSFModel.from_file(path)
    assert back.data.tobytes() == m.data.tobytes() and back.half == 12 and back.cards == m.cards and back.n_used is None
    assert z.fits.read_header(path)[0]['BITPIX'] == -64
    with pytest.raises(ValueError):
        p.PSFModel(np.zeros((4, 4)))


def test_the_header_declares_the_entry_points_and_the_constants():
    z = pkg()
    L = z._lib
    text = open(os.path.join(ROOT, 'include', 'zudsmi.h')).read()
    sec = text[text.index('PSF photometry: star model and batched fits'):text.index('alert packets: cone searches')]
    for name in ('zm_psf_build', 'zm_psf_build_dev', 'zm_psf_photometry', 'zm_psf_photometry_dev', 'zm_psf_photometry_batch_dev'):
        assert f'int {name}(' in sec and name in L.exported_symbols()
    defs = dict(re.findall(r'#define (ZM_[A-Z0-9_]+) ([0-9]+)', sec))
    assert int(defs['ZM_PSF_HALF_MAX']) == L.PSF_HALF_MAX == pr.HALF_MAX
    for k in ('BAD', 'NONFINITE', 'BADRMS', 'CLIPPED', 'LOWCOVER', 'SINGULAR', 'BADPOS'):
        assert int(defs[f'ZM_PSF_{k}']) == getattr(L, f'PSF_{k}') == getattr(pr, k) == z.psf.PSF_FLAGS[k]


def test_struct_layout_of_zm_psf_image(tmp_path):
    """zm_psf_image against a probe compiled from the header itself, and its first fields against zm_lc_image."""
    import ctypes as C
    import subprocess
    z = pkg()
    cls = z._lib.zm_psf_image
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zudsmi.h"', 'int main(void) {',
             '  printf(". %zu\\n", sizeof(zm_psf_image));']
    for field, _ in cls._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(zm_psf_image, {field}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines) + '\n')
    exe = tmp_path / 'probe'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        field, value = line.split()
        assert int(value) == (C.sizeof(cls) if field == '.' else getattr(cls, field).offset), field
        seen += 1
    assert seen == len(cls._fields_) + 1
    for field, _ in z._lib.zm_lc_image._fields_:
        assert getattr(cls, field).offset == getattr(z._lib.zm_lc_image, field).offset
