"""The restatement of the astrometric refit (tests/astrom_ref.py) pinned on planted truth: a degree-3 TPV sky seen
through a header that is off by (17.3, -9.6) pixels, 0.02 degrees and 1.0002 in scale, with detections that have no
star, stars that have no detection and five detections moved by one pixel.  Without noise the solver has to come back
to the truth to about 1e-10 arcsec (fp64 at a condition number of ~1e4 on values of ~0.1 degree) and reject exactly the
five.

The five are rejected only where the clip can see them.  The bound is 2 * 9 * max(1, sum chi2 / (2 (n - ncoef))); with
five equal outliers among n noiseless rows the largest chi2 is sum / 5, so it passes the bound unless
2 (n - ncoef) > 90: n >= 56 at degree 3.  The smallest scene here therefore has 80 stars."""
import numpy as np
import pytest

import astrom_ref as am


def planted(nstars, seed):
    base = am.tan_header(crval=(211.0, 33.0), naxis=(1024, 1024), scale=1.01, angle=12.0)
    truth = am.tpv_truth(base, seed)
    det, ref, out = am.scene(truth, nstars, seed, nspurious=nstars // 8, nunrelated=nstars // 4, noutliers=5)
    w0 = am.perturbed(base, dpix=(17.3, -9.6), angle=0.02, scale=1.0002)
    return truth, w0, det, ref, out


@pytest.mark.parametrize('nstars', [80, 200, 1000])
def test_planted_truth_is_recovered(nstars):
    truth, w0, det, ref, out = planted(nstars, seed=nstars)
    assert am.grid_separation(truth, w0) > 15.0                         # the header is off by many cross-id radii
    r = am.solve_frame(w0, *det, *ref)
    assert r['status'] == am.OK and 2 <= r['rounds'] <= 3
    assert am.grid_separation(truth, r['wcs']) < 1e-9
    assert max(r['rms']) < 1e-9
    assert r['nmatch'] == nstars and r['nused'] == nstars - 5
    unused = np.flatnonzero((r['match'] >= 0) & (r['used'] == 0))
    assert np.array_equal(unused, out)
    assert np.hypot(*r['shift']) > 15.0 and r['vote_peak'] >= nstars // 2 and 2 * r['vote_runner_up'] < r['vote_peak']
    # CRPIX, CRVAL and CD are the header's own: the solution is in the PV terms
    assert np.array_equal(r['wcs'].cd, w0.cd) and np.array_equal(r['wcs'].crpix, w0.crpix)
    assert r['wcs'].pv1[3] == 0.0 and r['wcs'].pv1[11] == 0.0 and not r['wcs'].pv1[12:].any()


def test_lower_degrees_and_a_skipped_vote():
    base = am.tan_header(naxis=(512, 512))
    det, ref, _ = am.scene(base, 60, 3)
    for degree in (1, 2, 3):
        r = am.solve_frame(am.perturbed(base, dpix=(4.0, 3.0)), *det, *ref, degree=degree)
        assert r['status'] == am.OK and am.grid_separation(base, r['wcs']) < 1e-9
    r = am.solve_frame(am.perturbed(base, dpix=(4.0, 3.0)), *det, *ref, match=0)    # 5 pixels off and no vote: no match
    assert r['status'] == am.TOO_FEW and r['wcs'].crpix[0] == base.crpix[0] + 4.0
    r = am.solve_frame(am.perturbed(base, dpix=(0.6, -0.4)), *det, *ref, match=0)
    assert r['status'] == am.OK and r['vote_peak'] == 0 and am.grid_separation(base, r['wcs']) < 1e-9


def test_statuses():
    base = am.tan_header(naxis=(256, 256))
    det, ref, _ = am.scene(base, 30, 5)
    r = am.solve_frame(am.perturbed(base, dpix=(70.0, 0.0)), *det, *ref)           # outside the vote's window
    assert r['status'] in (am.AMBIGUOUS, am.TOO_FEW) and r['wcs'].pv1[0] == 0.0
    r = am.solve_frame(base, *[v[:5] for v in det], *ref, degree=1)                # 5 rows < 2 * 3
    assert r['status'] == am.AMBIGUOUS
    r = am.solve_frame(base, *[v[:5] for v in det], *ref, degree=1, match=0)
    assert r['status'] == am.TOO_FEW and r['nmatch'] <= 5
    empty = tuple(np.zeros(0) for _ in range(4))
    r = am.solve_frame(base, *empty, *ref)
    assert r['status'] == am.AMBIGUOUS and r['match'].size == 0
    x, y, sd, snr = (v.copy() for v in det)
    x[3] = np.nan
    sd[7] = np.inf
    r = am.solve_frame(base, x, y, sd, snr, *ref, degree=2)
    assert r['status'] == am.OK and r['match'][3] == -1 and r['match'][7] == -1 and r['nmatch'] == 28
