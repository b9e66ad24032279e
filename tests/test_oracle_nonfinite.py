"""The oracle's rule for non-finite pixels and extreme weights (oracle/resample.py, oracle/background.py
docstrings), pinned with hand-placed pixels whose flagged footprint is known in closed form.

Resample: a NaN / +inf / -inf value is a bad input pixel (value 0, variance BIGVAR), with or without a weight map,
for every kernel; an output is bad when a non-zero tap lands on a bad pixel or when its interpolated variance is
>= BADVAR_TEST.  Background: a mesh sample needs |p| < BIG and a weight above WEIGHT_THRESH."""
import numpy as np
import pytest

from oracle import background as oback
from oracle import resample as ores

NX, NY = 40, 30
POISON = [np.nan, np.inf, -np.inf]


def field(seed=1):
    rng = np.random.default_rng(seed)
    return rng.normal(100.0, 5.0, (NY, NX)), np.full((NY, NX), 0.04)


def grid(dx=0.0, dy=0.0):
    yo, xo = np.mgrid[0:NY, 0:NX].astype(np.float64)
    return xo + dx, yo + dy


def bad_of(kind, img, wgt, px, py):
    o, w, _ = ores.resample(img, wgt, px, py, kind)
    assert np.isfinite(o).all() and np.isfinite(w).all()
    assert np.all(o[w == 0] == 0)
    return w == 0


def covered(kind, px, py):
    return ores.coverage(px, py, NX, NY, kind)


@pytest.mark.parametrize('value', POISON)
@pytest.mark.parametrize('with_w', [True, False])
@pytest.mark.parametrize('kind', [ores.LANCZOS3, ores.BILINEAR, ores.NEAREST])
def test_identity_flags_the_poisoned_pixel_alone(kind, with_w, value):
    img, wgt = field()
    img[12, 17] = value
    px, py = grid()
    bad = bad_of(kind, img, wgt if with_w else None, px, py)
    want = np.zeros((NY, NX), bool)
    want[12, 17] = True
    assert np.array_equal(bad, want)


@pytest.mark.parametrize('value', POISON)
@pytest.mark.parametrize('with_w', [True, False])
@pytest.mark.parametrize('kind,cols', [(ores.LANCZOS3, (14, 20)), (ores.BILINEAR, (16, 18)), (ores.NEAREST, (16, 17))])
def test_half_pixel_shift_flags_the_non_zero_tap_footprint(kind, cols, with_w, value):
    """px = x + 0.5: floor x, taps x - 2 .. x + 3 (LANCZOS3), x, x + 1 (BILINEAR), nearest x + 1; a delta along y.
    A bad pixel in column 17 reaches the outputs of columns 14..19, 16..17 and 16 of its own row."""
    img, wgt = field()
    img[12, 17] = value
    px, py = grid(dx=0.5)
    bad = bad_of(kind, img, wgt if with_w else None, px, py)
    want = ~covered(kind, px, py)
    want[12, cols[0]:cols[1]] = True
    assert np.array_equal(bad, want)


@pytest.mark.parametrize('kind', [ores.LANCZOS3, ores.BILINEAR])
def test_a_non_finite_pixel_adds_nothing_to_its_neighbours(kind):
    """Outside the footprint a poisoned frame gives the values and weights of the frame whose pixel has weight 0."""
    img, wgt = field(3)
    rng = np.random.default_rng(4)
    px, py = grid(dx=0.3)
    py = py + rng.uniform(0.1, 0.9, py.shape)
    zero = wgt.copy()
    for (y, x), v in zip([(5, 9), (14, 30), (22, 3)], POISON):
        img[y, x] = v
        zero[y, x] = 0.0
    clean = np.where(np.isfinite(img), img, 0.0)
    a = ores.resample(img, wgt, px, py, kind)
    b = ores.resample(clean, zero, px, py, kind)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # without a weight map the same pixels are the only bad ones
    c = ores.resample(img, None, px, py, kind)
    assert np.array_equal(c[1] == 0, b[1] == 0)


@pytest.mark.parametrize('w,good', [(np.nan, False), (np.inf, False), (-1.0, False), (0.0, False), (1e-30, False),
                                    (1.5e-30, False), (1e-20, False), (1e-16, False), (1e-13, True), (1e-12, True)])
@pytest.mark.parametrize('kind', [ores.LANCZOS3, ores.BILINEAR, ores.NEAREST])
def test_weight_thresholds_at_identity(kind, w, good):
    """An identity alignment hands a pixel's own variance 1 / w to its output: bad at or below WEIGHT_THRESH, and bad
    at or above BADVAR_TEST = 1e14 (weights up to 1e-14), as the device decides; a weight of +inf is a variance of 0,
    which is not > 0."""
    img, wgt = field()
    wgt[12, 17] = w
    px, py = grid()
    o, ow, _ = ores.resample(img, wgt, px, py, kind)
    assert np.isfinite(o).all() and np.isfinite(ow).all()
    assert (ow[12, 17] > 0) == good
    if good:
        assert ow[12, 17] == pytest.approx(w, rel=1e-12) and o[12, 17] == img[12, 17]
    others = np.ones((NY, NX), bool)
    others[12, 17] = False
    assert (ow[others] > 0).all()


def test_weights_near_the_variance_test_follow_the_interpolated_variance():
    """Half-pixel shift, LANCZOS3 (taps ~ 0.02, -0.13, 0.61, 0.61, -0.13, 0.02): a weight of 1e-13 is a variance of 1e13.
    Under a positive tap the output variance stays below 1e14 (good), under a negative one it is negative (bad).
    A weight of 1e-16 pushes every output of the footprint to or beyond the test."""
    img, wgt = field()
    px, py = grid(dx=0.5)
    t = ores.lanczos3_taps(0.5)
    for w, want in ((1e-13, t < 0), (1e-16, np.ones(6, bool))):
        ww = wgt.copy()
        ww[12, 17] = w
        dbg = {}
        _, ow, _ = ores.resample(img, ww, px, py, ores.LANCZOS3, debug=dbg)
        # output column x has its tap k = 17 - x + 2 (x = 14..19 -> k = 5..0) on the pixel
        got = ow[12, 14:20] == 0
        assert np.array_equal(got, want[::-1]), (w, got)
        v = dbg['vacc'][12, 14:20]
        assert np.array_equal((v <= 0) | (v >= ores.BADVAR_TEST), got)


def mesh_field(seed=7):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:96, 0:128]
    img = 180.0 + 0.02 * xx + rng.normal(0.0, 6.0, yy.shape)
    return img, np.full(img.shape, 0.03)


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf, -1e30, 1e30])
def test_mesh_samples_exclude_non_finite_and_big_values(value):
    """A pixel with |p| >= BIG is not a sample: the mesh maps equal those of the frame whose pixel has weight 0,
    the first pixel of a mesh (the device's moment pivot) included."""
    img, wgt = mesh_field()
    zero = wgt.copy()
    for y, x in [(0, 0), (0, 32), (17, 45), (40, 100), (95, 127)]:
        img[y, x] = value
        zero[y, x] = 0.0
    b1, s1 = oback.mesh_maps(img, wgt, 32)
    b2, s2 = oback.mesh_maps(np.where(zero > 0, img, 0.0), zero, 32)
    assert np.array_equal(b1, b2) and np.array_equal(s1, s2)
    assert (b1 > -oback.BIG).all() and np.isfinite(b1).all() and np.isfinite(s1).all()
    # no weight map: the same meshes, the same statistics
    b3, s3 = oback.mesh_maps(img, None, 32)
    b4, s4 = oback.mesh_maps(np.where(zero > 0, img, 0.0), zero, 32)
    assert np.array_equal(b3, b4) and np.array_equal(s3, s4)


def test_a_mesh_with_too_few_samples_is_filled():
    """BACK_MINGOODFRAC: a 32 x 32 mesh needs 512 samples.  512 finite pixels keep it, 511 make it a bad mesh whose
    value comes from its neighbours; an all-NaN mesh likewise.  Nothing non-finite leaves."""
    img, wgt = mesh_field(8)
    for nnan, good in ((512, True), (513, False), (1024, False)):
        im = img.copy()
        f = im[32:64, 32:64].reshape(-1)
        f[:nnan] = np.nan
        im[32:64, 32:64] = f.reshape(32, 32)
        back, sigm = oback.mesh_maps(im, wgt, 32)
        assert (back[1, 1] > -oback.BIG) == good
        bkg, rms, m, s, bo, so = oback.background(im, wgt, 32)
        assert np.isfinite(bkg).all() and np.isfinite(rms).all() and np.isfinite([m, s]).all()
        assert abs(bo[1, 1] - 181.0) < 3.0
