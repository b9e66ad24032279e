"""``zm_candidate_cuts_dev`` (``csrc/detect.hip: k_candidate_cuts``) and ``filterobjects.pixel_cuts_dev``: the three
pixel cuts of the candidate filter on planes in HBM, against the numpy restatement ``tests/cuts_ref.py`` and against
the host-pointer route ``pixel_cuts`` on copies of the same planes."""
import ctypes as C

import numpy as np
import pytest

import cuts_ref as cref
from util import pkg

pytestmark = pytest.mark.gpu
OTHER = 1 << 20


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def raw_cuts(engine, img, rms, mask, x, y, bad_bits):
    """The C entry point itself: (bpmcut, rmscut, negpix, stats[3])."""
    z = pkg()
    d = [dev(img.astype(np.float32)), dev(rms.astype(np.float32)), dev(mask.astype(np.int32))]
    ny, nx = img.shape
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    n = x.size
    b, r, neg, st = np.full(n, -7.0), np.full(n, -7.0), np.full(n, -7, np.int32), np.full(3, -7.0)
    import torch
    torch.cuda.synchronize()
    z._lib.check(engine.L.zm_candidate_cuts_dev(engine.ctx, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                int(bad_bits), nx, ny, n, x.ctypes.data, y.ctypes.data, b.ctypes.data,
                                                r.ctypes.data, neg.ctypes.data, st.ctypes.data), 'zm_candidate_cuts_dev')
    return b, r, neg, st


@pytest.mark.parametrize('seed', cref.SEEDS)
def test_cuts_equal_the_restatement(engine, seed):
    z = pkg()
    BAD = z.BAD_SUM
    img, rms, mask, x, y = cref.field(seed, BAD, OTHER)
    want = cref.candidate_cuts(img, rms, mask, x, y, BAD)
    b, r, neg, st = raw_cuts(engine, img, rms, mask, x, y, BAD)
    assert np.array_equal(neg, want['NEGPIX'])
    # the select is exact: the statistics are Engine.median_mad's on the same planes, formed as pixel_cuts forms them
    med, _ = engine.median_mad(rms, ((mask & BAD) != 0).astype(np.int32))
    immed, immad = engine.median_mad(img)
    assert st[0] == 1.1 * med and st[1] == immed and st[2] == 1.48 * (immad / 1.4826)
    assert (st[0], st[1], st[2]) == (want['MEDCUT'], want['IMMED'], want['IMSIG'])
    np.testing.assert_allclose(b, want['BPMCUT'], rtol=cref.PIN_RTOL, atol=cref.PIN_ATOL)
    np.testing.assert_allclose(r * cref.AREA, want['RMSCUT'] * cref.AREA, rtol=cref.PIN_RTOL, atol=cref.PIN_ATOL)
    # decisions: on every row the restatement does not call undecided (none, tests/test_cuts_ref.py)
    near, tiny = cref.undecided(want)
    assert not near.any() and not tiny.any()
    import torch
    got = z.pixel_cuts_dev(engine, dev(img), dev(rms), dev(mask), x, y, bad_bits=BAD)
    assert np.array_equal(got['GOODCUT'], want['GOODCUT']) and got['GOODCUT'].dtype == np.uint8
    assert np.array_equal(got['BPMCUT'], b) and np.array_equal(got['RMSCUT'], r) and got['MEDCUT'] == st[0]
    assert np.array_equal(got['NEGPIX'], neg)


@pytest.mark.parametrize('seed', cref.SEEDS)
def test_cuts_equal_the_host_route(engine, seed):
    """``pixel_cuts`` (host pointers: two aperture calls, two selects, zm_negpix_test) on copies of the same planes:
    integers and GOODCUT identical; the largest float difference is printed (the two routes sum the same products in
    the same order, so anything but 0 would be FMA contraction, and the aperture pin would be its bound)."""
    z = pkg()
    BAD = z.BAD_SUM
    img, rms, mask, x, y = cref.field(seed, BAD, OTHER)
    host = z.pixel_cuts(img.copy(), rms.copy(), (mask & BAD) != 0, x, y, engine=engine)
    got = z.pixel_cuts_dev(engine, dev(img), dev(rms), dev(mask), x, y, bad_bits=BAD)
    assert np.array_equal(got['NEGPIX'], host['NEGPIX']) and np.array_equal(got['GOODCUT'], host['GOODCUT'])
    assert got['MEDCUT'] == host['MEDCUT']
    db = float(np.abs(got['BPMCUT'] - host['BPMCUT']).max())
    dr = float(np.abs(got['RMSCUT'] - host['RMSCUT']).max() * cref.AREA)
    print(f'seed {seed}: largest |BPMCUT| difference {db!r}, largest |RMSCUT x area| difference {dr!r}')
    np.testing.assert_allclose(got['BPMCUT'], host['BPMCUT'], rtol=cref.PIN_RTOL, atol=cref.PIN_ATOL)
    np.testing.assert_allclose(got['RMSCUT'] * cref.AREA, host['RMSCUT'] * cref.AREA, rtol=cref.PIN_RTOL,
                               atol=cref.PIN_ATOL)


def test_no_candidates_returns_at_once(engine):
    z = pkg()
    img, rms, mask, _, _ = cref.field(cref.SEEDS[0])
    b, r, neg, st = raw_cuts(engine, img, rms, mask, np.zeros(0), np.zeros(0), z.BAD_SUM)
    assert b.size == 0 and (st == -7.0).all()                      # nothing written
    # pixel_cuts_dev still answers with the dict of pixel_cuts: MEDCUT from the select alone
    got = z.pixel_cuts_dev(engine, dev(img), dev(rms), dev(mask), [], [])
    host = z.pixel_cuts(img, rms, (mask & z.BAD_SUM) != 0, [], [], engine=engine)
    assert got['GOODCUT'].size == 0 and got['NEGPIX'].size == 0 and got['MEDCUT'] == host['MEDCUT'] > 0
    assert got.keys() == host.keys() and all(np.asarray(got[k]).dtype == np.asarray(host[k]).dtype for k in got)
    # planes that are not on the engine's GPU never reach the kernel
    import torch
    with pytest.raises(ValueError, match="on the engine's GPU"):
        z.pixel_cuts_dev(engine, torch.from_numpy(img), dev(rms), dev(mask), [5.0], [5.0])
    # null planes are refused whatever the count
    assert engine.L.zm_candidate_cuts_dev(engine.ctx, None, None, None, 1, 8, 8, 0, None, None, None, None, None, None) != 0


def test_positions_that_are_not_finite_or_far_outside(engine):
    z = pkg()
    img, rms, mask, _, _ = cref.field(cref.SEEDS[1])
    ny, nx = img.shape
    x = np.array([np.nan, 30.0, np.inf, -np.inf, 1e300, -1e300, 3e9, -3e9, 1e5, 40.0, nx + 7.0, -6.6, 50.0])
    y = np.array([30.0, np.nan, 30.0, 30.0, 30.0, 30.0, 30.0, -3e9, 1e5, 1e18, 30.0, 30.0, 50.0])
    b, r, neg, st = raw_cuts(engine, img, rms, mask, x, y, z.BAD_SUM)
    assert (b[:12] == 0).all() and (r[:12] == 0).all() and (neg[:12] == 0).all()
    want = cref.candidate_cuts(img, rms, mask, x, y, z.BAD_SUM)
    assert np.array_equal(neg, want['NEGPIX']) and r[12] > 0
    np.testing.assert_allclose(r * cref.AREA, want['RMSCUT'] * cref.AREA, rtol=cref.PIN_RTOL, atol=cref.PIN_ATOL)


def test_a_frame_smaller_than_the_cutout(engine):
    z = pkg()
    rng = np.random.default_rng(3)
    img = rng.normal(0, 2.0, (16, 16)).astype(np.float32)
    rms = rng.uniform(1.9, 2.1, (16, 16)).astype(np.float32)
    mask = np.zeros((16, 16), np.int32)
    mask[3, 4] = 1
    mask[10, 10] = OTHER
    img[7, 7], img[7, 8] = -50.0, 60.0
    img[0, 15], img[1, 15] = -50.0, 60.0
    x = np.array([8.0, 1.0, 16.0, 12.3, -2.0, 20.0, 8.5])
    y = np.array([8.0, 1.0, 16.0, 3.3, 8.0, 20.0, 15.5])
    want = cref.candidate_cuts(img, rms, mask, x, y, z.BAD_SUM)
    b, r, neg, st = raw_cuts(engine, img, rms, mask, x, y, z.BAD_SUM)
    assert np.array_equal(neg, want['NEGPIX']) and neg[0] == 1
    assert (st[0], st[1], st[2]) == (want['MEDCUT'], want['IMMED'], want['IMSIG'])
    np.testing.assert_allclose(b, want['BPMCUT'], rtol=cref.PIN_RTOL, atol=cref.PIN_ATOL)
    np.testing.assert_allclose(r * cref.AREA, want['RMSCUT'] * cref.AREA, rtol=cref.PIN_RTOL, atol=cref.PIN_ATOL)
    host = z.pixel_cuts(img, rms, (mask & z.BAD_SUM) != 0, x, y, engine=engine)
    assert np.array_equal(neg, host['NEGPIX'])


@pytest.mark.parametrize('shape', [(16, 16), (1100, 1024)])
def test_a_frame_whose_every_pixel_is_bad_raises(engine, shape):
    """The select has nothing to take a median of: the entry point says so (both forms of the select: the three-pass
    one below a megapixel, the bracketed one above)."""
    z = pkg()
    rng = np.random.default_rng(4)
    img = rng.normal(0, 2.0, shape).astype(np.float32)
    rms = np.full(shape, 2.0, np.float32)
    mask = np.full(shape, 1 << 4, np.int32)
    with pytest.raises(z.ZMError, match='every pixel is masked'):
        raw_cuts(engine, img, rms, mask, np.array([8.0]), np.array([8.0]), z.BAD_SUM)
    # the same planes with a bit that is not bad: fine
    mask[:] = OTHER
    b, r, neg, st = raw_cuts(engine, img, rms, mask, np.array([8.0]), np.array([8.0]), z.BAD_SUM)
    assert b[0] == 0 and st[0] == 1.1 * 2.0
