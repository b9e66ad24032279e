"""Where the tolerances of tests/psf_ref.py come from: the restatement alone, run twice on the scenes of
tests/psf_scenes.py - in float64 (what the GPU is held to) and with every sum, tap and solve in numpy.longdouble.  Each
constant is 4 x the largest difference seen, rounded up to a power of two.  Nothing the GPU produced enters these numbers.
The script also prints the phase floor of the operator per FWHM (noiseless Gaussians, model built from and evaluated on
them: two interpolations) and the error of a fit against that of the r = 3 aperture.

    python tests/measure_psf_tolerance.py           (a few seconds)
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psf_ref as pr            # noqa: E402
import psf_scenes as ps         # noqa: E402

LD = np.longdouble


def pow2_up(v):
    return 2.0 ** math.ceil(math.log2(4.0 * v)) if v > 0 else 0.0


def worst_abs(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float(np.max(np.abs(a - b)[fin])) if fin.any() else 0.0


def worst_rel(a, b, sel=None):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    fin = np.isfinite(a) & np.isfinite(b) & (b != 0)
    if sel is not None:
        fin &= sel
    return float(np.max(np.abs(a - b)[fin] / np.abs(b[fin]))) if fin.any() else 0.0


def card_scenes():
    """``PSFCOR`` / ``PSFCORUN`` of the restatement (``psf_ref.cards``) in both precisions on: the frame of the end-to-end
    test (60 stars, rms plane) and the 65 stars of ``cutout_many`` (no rms plane), each with and without a sky term.
    Returns (largest difference of a card, the float64 cards per case)."""
    nt, g = ps.night_planes(), ps.cutout_many()
    cases = {'night': (nt['img'], nt['x'], nt['y'], np.full(60, 200.0), nt['flux'], nt['rms'], nt['mask']),
             'many': (g.img, g.x, g.y, g.sky, g.norm, None, g.mask)}
    worst, seen = 0.0, {}
    for name, (img, x, y, sky, norm, rms, mask) in cases.items():
        for fit_sky in (0, 1):
            c = {T: pr.cards(img, x, y, sky, norm, fit_sky, rms=rms, mask=mask, bad_bits=ps.BAD_BITS, T=T) for T in (pr.F64, LD)}
            assert c[pr.F64]['PSFNSTAR'] == c[LD]['PSFNSTAR'] and np.array_equal(c[pr.F64]['used'], c[LD]['used'])
            d = max(abs(float(LD(c[pr.F64][k]) - c[LD][k])) for k in ('PSFCOR', 'PSFCORUN'))
            print(f'cards {name} sky {fit_sky}: PSFCOR {float(c[pr.F64]["PSFCOR"]):.6f} PSFCORUN {float(c[pr.F64]["PSFCORUN"]):.6f} '
                  f'of {c[pr.F64]["PSFNSTAR"]} stars, largest difference {d:.3e}')
            worst = max(worst, d)
            seen[(name, fit_sky)] = c[pr.F64]
    return worst, seen


def phase_floor(fwhm, nphase=9):
    """min / max / median of recovered / true flux over the sub-pixel phase: a model built from 12 noiseless Gaussians at
    scattered phases, fitted (R = 6, no sky) to single noiseless Gaussians on a lattice of phases."""
    rng = np.random.default_rng(int(fwhm * 10))
    xs, ys = rng.uniform(20, 108, 12), rng.uniform(20, 108, 12)
    xs, ys = xs[np.argsort(xs)], ys
    img = pr.gaussian_image(128, 128, xs, ys, np.full(12, 1.0e5), fwhm)
    # the flux of each star in the reference aperture (r = 10) from the same subsampled sum for all
    norm = np.array([pr.aperture_sum(pr.gaussian_image(128, 128, [x], [y], [1.0e5], fwhm), x, y, 10.0)[0] for x, y in zip(xs, ys)])
    model, _, _ = pr.build_model(img.astype(np.float32), xs, ys, np.zeros(12), norm, half=12, norm_radius=10.0, clip_iter=0,
                                 min_stars_pixel=1)
    ratios = []
    for a in range(nphase):
        for b in range(nphase):
            x, y = 32.0 + (a + 0.5) / nphase - 0.5, 32.0 + (b + 0.5) / nphase - 0.5
            one = pr.gaussian_image(64, 64, [x], [y], [1.0e5], fwhm)
            f = pr.fit(one.astype(np.float32), [x], [y], model, 6.0, 0)
            ref = pr.aperture_sum(one, x, y, 10.0)[0]
            ratios.append(float(f['flux'][0]) / ref)
    return min(ratios), max(ratios), float(np.median(ratios))


def error_ratio(fwhm):
    """err of a fit with uniform noise / err of the r = 3 aperture scaled to the same flux fraction."""
    model = ps.model_gaussian(12, fwhm)
    img = np.zeros((64, 64), np.float32)
    f = pr.fit(img, [32.3], [31.6], model, 6.0, 0, rms=np.ones((64, 64), np.float32))
    one = pr.gaussian_image(64, 64, [32.3], [31.6], [1.0], fwhm)
    inside, frac = pr.aperture_sum(one, 32.3, 31.6, 3.0)
    ap_err = math.sqrt(float((frac * frac).sum())) / inside            # error of the aperture flux corrected to the total
    return float(f['err'][0]) / ap_err


def measure():
    """The largest float64 - longdouble difference per constant, printed per scene."""
    seen = dict(model=0.0, flux_rel=0.0, flux_abs=0.0, err_rel=0.0, chi2_rel=0.0, card=0.0)
    for half in (1, 12, 15):
        g = ps.cutout_edges(half)
        a = pr.cutouts(g.img, g.x, g.y, g.sky, g.norm, half, mask=g.mask, bad_bits=ps.BAD_BITS)
        b = pr.cutouts(g.img, g.x, g.y, g.sky, g.norm, half, mask=g.mask, bad_bits=ps.BAD_BITS, T=LD)
        d = worst_abs(a, b)
        print(f'cutout_edges half {half}: largest difference {d:.3e}')
        seen['model'] = max(seen['model'], d)
    for g, kw in ((ps.cutout_many(), dict(norm_radius=3.0, clip_sigma=3.0, clip_iter=5, min_stars_pixel=3)),
                  (ps.model_floor(), dict(norm_radius=3.5, clip_sigma=3.0, clip_iter=0, min_stars_pixel=3))):
        ma, na, ca = pr.build_model(g.img, g.x, g.y, g.sky, g.norm, half=g.half, mask=g.mask, bad_bits=ps.BAD_BITS, **kw)
        mb, nb, cb = pr.build_model(g.img, g.x, g.y, g.sky, g.norm, half=g.half, mask=g.mask, bad_bits=ps.BAD_BITS, T=LD, **kw)
        assert np.array_equal(na, nb)
        d = max(worst_abs(ma, mb), worst_abs(ca, cb))
        print(f'model of {len(g.x)} stars, half {g.half}: largest difference {d:.3e}')
        seen['model'] = max(seen['model'], d)
    s = ps.fit_main()
    for R, fit_sky, with_rms, with_mask in ps.FIT_CASES:
        kw = dict(rms=s.rms if with_rms else None, mask=s.mask if with_mask else None, bad_bits=ps.BAD_BITS)
        a = pr.fit(s.img, s.x, s.y, s.model, R, fit_sky, **kw)
        b = pr.fit(s.img, s.x, s.y, s.model, R, fit_sky, T=LD, **kw)
        assert np.array_equal(a['flags'], b['flags']) and np.array_equal(a['npix'], b['npix'])
        with np.errstate(invalid='ignore'):
            big = np.abs(b['flux']) >= b['err']
        fr = max(worst_rel(a['flux'], b['flux'], big), worst_rel(a['sky'], b['sky'], big))
        fa = worst_abs(np.where(big, np.nan, a['flux']), np.where(big, np.nan, b['flux']))
        er = max(worst_rel(a['err'], b['err']), worst_rel(a['cover'], b['cover']))
        cr = worst_abs(a['chi2'] / b['chi2_scale'].astype(pr.F64), b['chi2'] / b['chi2_scale'])
        print(f'fit R {R} sky {fit_sky} rms {with_rms} mask {with_mask}: flux rel {fr:.3e} abs {fa:.3e}, err rel {er:.3e}, '
              f'chi2 rel {cr:.3e}, margin {a["margin"].min():.3e}')
        for k, v in (('flux_rel', fr), ('flux_abs', fa), ('err_rel', er), ('chi2_rel', cr)):
            seen[k] = max(seen[k], v)
    seen['card'], _ = card_scenes()
    return seen


CONSTANTS = (('MODEL_TOL', 'model'), ('FLUX_RTOL', 'flux_rel'), ('FLUX_ATOL', 'flux_abs'), ('ERR_RTOL', 'err_rel'),
             ('CHI2_RTOL', 'chi2_rel'), ('CARD_TOL', 'card'))


def main():
    seen = measure()
    print('MEASURED =', {k: float(f'{v:.3e}') for k, v in seen.items()})
    for name, key in CONSTANTS:
        t = pow2_up(seen[key])
        print(f'{name} = 2.0 ** {int(math.log2(t)) if t else "-inf"}    (4 x {seen[key]:.3e} rounded up; psf_ref has '
              f'2.0 ** {int(math.log2(getattr(pr, name)))})')
    floor = {}
    for fwhm in (1.6, 2.0, 2.4, 3.0):
        lo, hi, med = phase_floor(fwhm)
        floor[fwhm] = (round(lo, 4), round(hi, 4))
        print(f'phase floor FWHM {fwhm}: recovered / true flux {lo:.4f} .. {hi:.4f}, median {med:.4f}; '
              f'error ratio to the r = 3 aperture {error_ratio(fwhm):.3f}')
    print('PHASE_FLOOR =', floor)
    return seen, floor


if __name__ == '__main__':
    main()
