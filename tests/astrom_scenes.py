"""The scenes of tests/test_astrometry_gpu.py, shared with tests/measure_astrom_tolerance.py so that the tolerance is
measured on exactly what the test runs.  ``SCENES[name]()`` returns ``(wcs_list, detections, ref, params)`` for
``astrom_ref.solve`` / ``scamp.solve``; ``reference(name)`` solves a scene with the restatement once and keeps it.

Every scene is small: the sizes are the smallest at which the kernels take another path - more rows than a wave (65),
more than a workgroup (300), frames of different sizes in one batch, an empty frame."""
import functools

import numpy as np

import astrom_ref as am

MIN_RADIUS_MARGIN, MIN_CLIP_MARGIN, MIN_VOTE_MARGIN = 1e-3, 1e-6, 1e-9


def _one(w0, det, ref, **params):
    return [w0], [det], ref, params


def empty():
    base = am.tan_header(naxis=(256, 256))
    _, ref, _ = am.scene(base, 30, 1)
    return _one(base, tuple(np.zeros(0) for _ in range(4)), ref)


def _few(n):
    base = am.tan_header(crval=(40.0, -12.0), naxis=(256, 256))
    det, ref, _ = am.scene(base, n, 11, nunrelated=4)
    return _one(am.perturbed(base, dpix=(0.4, -0.3)), det, ref, degree=1, match=0)


def exactly_enough():
    return _few(6)


def one_too_few():
    return _few(5)


def rows_65():
    base = am.tan_header(crval=(150.0, 20.0), naxis=(512, 512), scale=1.0, angle=30.0)
    truth = am.tpv_truth(base, 65)
    det, ref, _ = am.scene(truth, 65, 65, nspurious=6, nunrelated=20, noutliers=5)
    return _one(am.perturbed(base, dpix=(5.3, -3.6), angle=0.01), det, ref, degree=2)


def rows_300():
    base = am.tan_header(crval=(211.0, 33.0), naxis=(1024, 1024), scale=1.01, angle=12.0)
    truth = am.tpv_truth(base, 300)
    det, ref, _ = am.scene(truth, 300, 300, nspurious=30, nunrelated=80, noutliers=5)
    return _one(am.perturbed(base, dpix=(17.3, -9.6), angle=0.02, scale=1.0002), det, ref)


def batch_of_three():
    base = am.tan_header(crval=(10.0, 5.0), naxis=(512, 512))
    a, ref_a, _ = am.scene(base, 70, 21, nunrelated=10)
    b, ref_b, _ = am.scene(base, 130, 22, nunrelated=10)
    ref = tuple(np.concatenate([u, v]) for u, v in zip(ref_a, ref_b))
    # (the two frames look at the same sky through different headers; each finds its own stars among both lists)
    nothing = tuple(np.zeros(0) for _ in range(4))
    return ([am.perturbed(base, dpix=(3.0, 2.0)), base, am.perturbed(base, dpix=(-4.4, 1.7), angle=0.01)], [a, nothing, b], ref,
            dict(degree=2))


def stars_far_away():
    base = am.tan_header(crval=(80.0, 45.0), naxis=(256, 256))
    det, ref, _ = am.scene(base, 40, 31)
    rng = np.random.default_rng(31)
    far_ra = np.concatenate([rng.uniform(0, 360, 300), [260.0, 260.0]])             # the last two: the antipode
    far_dec = np.concatenate([rng.uniform(-90, 30, 300), [-45.0, -44.9]])
    ref = (np.concatenate([far_ra[:150], ref[0], far_ra[150:]]), np.concatenate([far_dec[:150], ref[1], far_dec[150:]]),
           np.full(ref[0].size + far_ra.size, 0.01))
    return _one(am.perturbed(base, dpix=(2.2, 1.1)), det, ref, degree=1)


def _shifted(pixels):
    base = am.tan_header(crval=(120.0, -30.0), naxis=(512, 512))
    det, ref, _ = am.scene(base, 60, 41)
    return _one(am.perturbed(base, dpix=(pixels, 0.0)), det, ref, degree=1)


def shift_inside_window():
    return _shifted(58.7)                                   # P = 60 arcsec at 1 arcsec per pixel, bins of 1 arcsec


def shift_outside_window():
    return _shifted(63.2)


def two_equal_peaks():
    base = am.tan_header(crval=(200.0, 10.0), naxis=(256, 256))
    det, ref, _ = am.scene(base, 30, 51)
    # every star twice: where it is, and 20.3 x 7.4 pixels away
    x, y = base.sky2pix(ref[0], ref[1])
    ra2, dec2 = base.pix2sky(x + 20.3, y + 7.4)
    ref = (np.concatenate([ref[0], ra2]), np.concatenate([ref[1], dec2]), np.concatenate([ref[2], ref[2]]))
    return _one(base, det, ref, degree=1)


def _degree(degree, tpv_in):
    base = am.tan_header(crval=(33.0, 61.0), naxis=(512, 512), angle=-20.0)
    truth = am.tpv_truth(base, 100 + degree)
    det, ref, _ = am.scene(truth, 90, 60 + degree, nspurious=5, nunrelated=12, noutliers=3)
    w0 = am.perturbed(truth if tpv_in else base, dpix=(6.1, 4.4), keep_pv=tpv_in)
    return _one(w0, det, ref, degree=degree)


def across_ra_zero():
    base = am.tan_header(crval=(359.99, 12.0), naxis=(512, 512))
    det, ref, _ = am.scene(base, 70, 71, nunrelated=10)
    assert (ref[0] > 359.9).any() and (ref[0] < 0.1).any()
    return _one(am.perturbed(base, dpix=(-7.0, 3.0)), det, ref, degree=2)


def near_the_pole():
    base = am.tan_header(crval=(77.0, 89.5), naxis=(512, 512))
    det, ref, _ = am.scene(base, 70, 72, nunrelated=10)
    return _one(am.perturbed(base, dpix=(4.1, -6.2)), det, ref, degree=2)


def duplicate_stars():
    base = am.tan_header(crval=(300.0, -5.0), naxis=(256, 256))
    det, ref, _ = am.scene(base, 40, 81)
    dup = np.array([3, 7, 7, 20])
    ref = tuple(np.concatenate([v, v[dup]]) for v in ref)   # exact copies behind the originals: the lowest index wins
    return _one(am.perturbed(base, dpix=(1.0, 1.0)), det, ref, degree=1)


def nonfinite_rows():
    base = am.tan_header(crval=(15.0, 15.0), naxis=(256, 256))
    det, ref, _ = am.scene(base, 50, 91)
    x, y, sd, snr = (v.copy() for v in det)
    x[4], y[9], sd[17], snr[23], x[30] = np.nan, np.inf, np.nan, -np.inf, np.inf
    ra, dec, sig = (v.copy() for v in ref)
    ra[5], dec[6] = np.nan, np.inf                          # a star that is not finite is matched by nothing
    return _one(am.perturbed(base, dpix=(2.0, -2.0)), (x, y, sd, snr), (ra, dec, sig), degree=1)


def a_row_returns():
    """A big outlier pulls the first fit, the pull pushes a mild outlier next to it over the clip bound; the second
    fit, without the two, is back at the truth, where the mild one is inside the bound: it returns."""
    base = am.tan_header(crval=(170.0, 40.0), naxis=(512, 512))
    (x, y, sd, snr), ref, _ = am.scene(base, 100, 95)
    corner = np.argsort(np.hypot(x - 512.0, y - 512.0))[:2]
    # sd = 0.05 px and sig = 0.01 arcsec: chi2 = (d / 0.051)^2; the bound is 18 while the reduced chi2 is below 1
    x[corner[0]] += 0.051 * 14.0                            # chi2 ~ 196 at the truth
    x[corner[1]] -= 0.051 * 4.0                             # chi2 ~ 16 at the truth: inside, but not while pulled
    return _one(am.perturbed(base, dpix=(1.4, 0.3)), (x, y, sd, snr), ref, degree=1)


def vote_skipped():
    base = am.tan_header(crval=(95.0, 27.0), naxis=(512, 512))
    truth = am.tpv_truth(base, 97)
    det, ref, _ = am.scene(truth, 80, 97, nunrelated=10)
    return _one(am.perturbed(base, dpix=(0.7, -0.5)), det, ref, degree=3, match=0)


def top_of_the_list():
    """More detections than MATCH_NMAX: only the brightest vote (ties in snr: the lowest row)."""
    base = am.tan_header(crval=(250.0, -40.0), naxis=(512, 512))
    (x, y, sd, snr), ref, _ = am.scene(base, 120, 99, nspurious=10)
    snr[10:40] = 77.0                                       # a run of equal keys across the cut
    return _one(am.perturbed(base, dpix=(9.0, 9.0)), (x, y, sd, snr), ref, degree=1, match_nmax=48)


def fine_bins():
    """The largest vote the library takes: P / q = 100, 201 x 201 bins, which leave room in LDS for about 120 detections at
    a time - fewer than vote here, so the detections pass through LDS in pieces."""
    base = am.tan_header(crval=(60.0, 25.0), naxis=(512, 512))
    det, ref, _ = am.scene(base, 150, 103, nspurious=8, nunrelated=15)
    return _one(am.perturbed(base, dpix=(33.37, -41.21)), det, ref, degree=1, match_resol=0.6)


def one_round():
    """max_rounds = 1: a first round cannot repeat an earlier one, so the frame ends NOT_CONVERGED with its solution."""
    (wl, dets, ref, params) = _degree(1, False)
    return wl, dets, ref, dict(params, max_rounds=1)


def singular():
    """Eight detections on CRPIX itself and one star on CRVAL: u = v = 0 for every row, so the second pivot is exactly
    zero in the normal equations and the design matrix has rank 1 for the restatement."""
    base = am.tan_header(crval=(140.0, 30.0), naxis=(256, 256))
    n = 8
    det = (np.full(n, base.crpix[0]), np.full(n, base.crpix[1]), np.full(n, 0.05), np.linspace(20.0, 90.0, n))
    return _one(base, det, (np.array([140.0]), np.array([30.0]), np.array([0.01])), degree=1, match=0)


SCENES = dict(fine_bins=fine_bins, one_round=one_round, singular=singular, empty=empty, exactly_enough=exactly_enough, one_too_few=one_too_few, rows_65=rows_65, rows_300=rows_300,
              batch_of_three=batch_of_three, stars_far_away=stars_far_away, shift_inside_window=shift_inside_window,
              shift_outside_window=shift_outside_window, two_equal_peaks=two_equal_peaks, across_ra_zero=across_ra_zero,
              near_the_pole=near_the_pole, duplicate_stars=duplicate_stars, nonfinite_rows=nonfinite_rows,
              a_row_returns=a_row_returns, vote_skipped=vote_skipped, top_of_the_list=top_of_the_list)
for _d in (1, 2, 3):
    for _t in (False, True):
        SCENES[f'degree{_d}_{"tpv" if _t else "tan"}'] = functools.partial(_degree, _d, _t)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(scene, [restatement's result per frame]); the margins of every frame are asserted here, once."""
    wcs_list, dets, ref, params = SCENES[name]()
    res = am.solve(wcs_list, dets, ref, **params)
    for f, r in enumerate(res):
        assert r['min_radius_margin'] >= MIN_RADIUS_MARGIN, (name, f, 'radius', r['min_radius_margin'])
        assert r['min_clip_margin'] >= MIN_CLIP_MARGIN, (name, f, 'clip', r['min_clip_margin'])
        assert r['min_vote_margin'] >= MIN_VOTE_MARGIN, (name, f, 'vote', r['min_vote_margin'])
    return (wcs_list, dets, ref, params), res
