"""``tests/cuts_ref.py`` (the numpy restatement the candidate-cut kernel is held to) against the independent overlap
reference ``tests/aperture_ref.py``, on hand-made cases, and the margins of the synthetic fields the GPU tests use."""
import numpy as np
import pytest

import aperture_ref as aref
import cuts_ref as cref

from util import pkg

BAD = cref.BAD_SUM
OTHER = 1 << 20


def test_bad_sum_is_the_package_s():
    assert cref.BAD_SUM == pkg().BAD_SUM


def flat(ny=64, nx=64, rms=2.0):
    rng = np.random.default_rng(0)
    img = rng.normal(0, 2.0, (ny, nx)).astype(np.float32)
    return img, np.full((ny, nx), rms, np.float32), np.zeros((ny, nx), np.int32)


def test_sums_agree_with_the_independent_overlap_reference():
    """BPMCUT and RMSCUT x area against the quadrature of aperture_ref.py, to its own derived bounds."""
    for seed in cref.SEEDS:
        img, rms, mask, x, y = cref.field(seed, BAD, OTHER)
        bad = (mask & BAD) != 0
        bsum, rsum = cref.aperture_sums(rms, bad, x, y)
        for plane, got in ((rms, rsum), (bad.astype(np.float32), bsum)):
            ref, _, _, terms = aref.aperture_sums(plane, None, None, x, y, cref.RADIUS, with_terms=True)
            bound, _ = aref.sums_bounds(terms)
            assert (np.abs(got - ref) <= bound + 1e-300).all(), float(np.abs(got - ref).max())


def test_lone_bad_pixel_inside_on_and_outside_the_circle():
    img, rms, mask = flat()
    # aperture centre (0-based) = (x, y) unchanged: a candidate at X_IMAGE = 30 has its aperture about pixel 30
    x, y = np.array([30.0]), np.array([30.0])
    for (i, j), want in (((30, 30), 1.0), ((33, 28), 1.0), ((36, 30), None), ((30, 24), None), ((37, 30), 0.0),
                         ((35, 35), 0.0), ((44, 30), 0.0)):
        m = mask.copy()
        m[j, i] = BAD & -BAD
        m[5, 5] = OTHER                                         # a bit that is not bad never counts
        c = cref.candidate_cuts(img, rms, m, x, y, BAD)
        ref = aref.pixel_fraction(i - 30.0, j - 30.0, cref.RADIUS)
        assert abs(c['BPMCUT'][0] - ref) < 1e-12
        if want is None:
            assert 0.4 < c['BPMCUT'][0] < 0.6 and c['GOODCUT'][0] == 0          # the circle cuts the pixel in half
        elif want == 1.0:
            assert abs(c['BPMCUT'][0] - 1.0) < 1e-12 and c['GOODCUT'][0] == 0
        else:
            assert abs(c['BPMCUT'][0]) < 1e-12
    # a mask bit outside bad_bits inside the aperture
    m = mask.copy()
    m[30, 30] = OTHER
    c = cref.candidate_cuts(img, rms, m, x, y, BAD)
    assert c['BPMCUT'][0] == 0 and c['GOODCUT'][0] == 1


def test_rmscut_and_medcut():
    img, rms, mask = flat()
    rms[20:44, 20:44] = 5.0
    mask[0:32] = BAD & -BAD                       # the bad half does not enter the median
    rms[0:32, 0:10] = 100.0
    c = cref.candidate_cuts(img, rms, mask, [32.0, 54.0], [38.0, 54.0], BAD)
    assert c['MEDCUT'] == pytest.approx(1.1 * 2.0)
    assert c['RMSCUT'][1] == pytest.approx(2.0, rel=1e-12) and c['RMSCUT'][0] > c['MEDCUT']
    med = float(np.median(img))
    assert c['IMMED'] == med
    assert c['IMSIG'] == pytest.approx(1.48 * float(np.median(np.abs(img - np.float32(med)))), rel=1e-12)


def test_dipole_at_the_cutout_edge_and_in_the_surround_ring():
    img, rms, mask = flat()
    x, y = np.array([31.0]), np.array([31.4])              # cutout centre (0-based) (30, 30): columns 25 .. 35
    def neg(pairs):
        a = img.copy()
        for (i, j), v in pairs:
            a[j, i] = v
        return int(cref.candidate_cuts(a, rms, mask, x, y, BAD)['NEGPIX'][0])
    assert neg([]) == 0
    assert neg([((30, 30), -60.0), ((31, 30), 70.0)]) == 1
    assert neg([((35, 30), -60.0), ((36, 30), 70.0)]) == 1            # negative at the edge, positive in the ring
    assert neg([((36, 30), -60.0), ((35, 30), 70.0)]) == 0            # negative in the ring: not looked at
    assert neg([((35, 35), -60.0), ((36, 36), 70.0)]) == 1            # the ring's corner
    assert neg([((36, 30), -60.0), ((37, 30), 70.0)]) == 0            # both outside
    assert neg([((35, 30), -60.0), ((37, 30), 70.0)]) == 0            # not neighbours
    assert neg([((30, 30), -60.0)]) == 0 and neg([((30, 30), 70.0)]) == 0
    # half to even: X_IMAGE = 30.5 rounds to 30, 31.5 to 32
    x[0] = 30.5
    assert neg([((34, 30), -60.0), ((35, 30), 70.0)]) == 1            # centre 29: edge column 34
    x[0] = 31.5
    assert neg([((36, 30), -60.0), ((37, 30), 70.0)]) == 1            # centre 31: edge column 36


def test_positions_near_and_beyond_the_frame_edges():
    img, rms, mask = flat(40, 48)
    img[0, 0], img[0, 1] = -60.0, 70.0
    img[39, 47], img[38, 46] = -60.0, 70.0
    x = np.array([1.0, 3.5, 47.0, 44.9, 20.0, 20.0, 48.0, -30.0, 1e300, np.nan, np.inf, 20.0])
    y = np.array([1.0, 20.0, 20.0, 38.0, 2.0, 39.5, 40.0, 10.0, 10.0, 10.0, 10.0, -np.inf])
    c = cref.candidate_cuts(img, rms, mask, x, y, BAD)
    ref, _, _ = aref.aperture_sums(rms, None, None, x, y, cref.RADIUS)
    np.testing.assert_allclose(c['RMSCUT'] * cref.AREA, ref, rtol=1e-12, atol=1e-12)
    assert (c['RMSCUT'][:7] > 0).all() and (c['RMSCUT'][:7] < 2.0).all()          # truncated apertures
    assert (c['RMSCUT'][7:] == 0).all() and (c['BPMCUT'][7:] == 0).all() and (c['NEGPIX'][7:] == 0).all()
    assert c['NEGPIX'][:7].tolist() == [1, 0, 0, 1, 0, 0, 1]


@pytest.mark.parametrize('seed', cref.SEEDS)
def test_the_gpu_fields_leave_no_row_undecided(seed):
    """The rows a decision test may leave out - RMSCUT within the aperture pin of MEDCUT, BPMCUT in (0, 1e-9] - from
    the restatement alone: none for the committed seeds (the cap, were a seed not to be found, is 1 % of rows)."""
    img, rms, mask, x, y = cref.field(seed, BAD, OTHER)
    c = cref.candidate_cuts(img, rms, mask, x, y, BAD)
    near, tiny = cref.undecided(c)
    assert near.mean() == 0 and tiny.mean() == 0
    # no aperture holds a bad pixel it merely grazes by rounding, from either side of zero
    assert ((c['BPMCUT'] == 0) | (np.abs(c['BPMCUT']) > 1e-3)).all()
    # and the field has what it is for: every outcome of every cut
    assert c['NEGPIX'].sum() >= 5 and (c['BPMCUT'] > 0.1).sum() >= 6 and (c['RMSCUT'] > c['MEDCUT']).sum() >= 4
    assert 0.5 < c['GOODCUT'].mean() < 0.95
