"""numpy restatement of the candidate cuts (``zm_candidate_cuts_dev``; ``zuds/filterobjects.py:83-195``).

Composed of pieces that have their own pins: the exact circle / pixel overlap of ``oracle.photometry`` (held to
``tests/aperture_ref.py``), the dipole test ``oracle.detect.negpix`` and numpy medians.  Positions are SExtractor's
``X_IMAGE`` / ``Y_IMAGE`` (1-based); the r = 6 aperture takes them unchanged, as the reference hands them to photutils,
the dipole test subtracts the 1.

numpy only; also holds the synthetic field the GPU tests use, so that the CPU suite can check its margins.
"""
import numpy as np

from oracle import detect as odet
from oracle import photometry as ophot

RADIUS = 6.0
AREA = np.pi * RADIUS ** 2
# the aperture kernel's pin (tests/test_photometry_gpu.py): sums agree to rtol 1e-10, atol 1e-9
PIN_RTOL, PIN_ATOL = 1e-10, 1e-9
# the package's BAD_SUM (zuds/constants.py:45), restated so that this file needs numpy only
BAD_SUM = sum(1 << b for b in (0, 2, 3, 4, 5, 7, 8, 9, 10, 16, 17))


def frame_stats(img, rms, mask, bad_bits):
    """(medcut, immed, imsig) as ``pixel_cuts`` states them: 1.1 x the median rms of the good pixels; the median of the
    image; 1.48 x (sigma / 1.4826) with sigma = 1.4826 x MAD, medians in float32 as numpy takes them."""
    img = np.asarray(img, dtype=np.float32)
    rms = np.asarray(rms, dtype=np.float32)
    good = (np.asarray(mask) & bad_bits) == 0
    r = rms[good & ~np.isnan(rms)]
    v = img[~np.isnan(img)]
    medcut = 1.1 * float(np.median(r))
    med = np.median(v)
    mad = np.median(np.abs(v - med))
    immed = float(med)
    imsig = 1.48 * ((1.4826 * float(mad)) / 1.4826)
    return medcut, immed, imsig


def aperture_sums(rms, bad, x, y):
    """(sum of the bad-pixel map, sum of the rms map) over the r = 6 aperture at (x, y) taken as 0-based positions."""
    zero = np.zeros(np.shape(rms))
    rsum, _, _ = ophot.aperture_photometry(rms, zero, None, x, y, RADIUS)
    bsum, _, _ = ophot.aperture_photometry(np.asarray(bad, dtype=np.float64), zero, None, x, y, RADIUS)
    return bsum, rsum


def negpix(img, x, y, immed, imsig):
    """``oracle.detect.negpix``; a position that is not finite has no cutout (0)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.zeros(x.size, np.int32)
    ok = np.flatnonzero(np.isfinite(x) & np.isfinite(y))
    if ok.size:
        out[ok] = odet.negpix(img, x[ok], y[ok], immed, imsig)
    return out


def candidate_cuts(img, rms, mask, x, y, bad_bits):
    """dict(BPMCUT, RMSCUT, MEDCUT, NEGPIX, GOODCUT, IMMED, IMSIG)."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    y = np.atleast_1d(np.asarray(y, dtype=np.float64))
    bad = (np.asarray(mask) & bad_bits) != 0
    medcut, immed, imsig = frame_stats(img, rms, mask, bad_bits)
    bsum, rsum = aperture_sums(np.asarray(rms, dtype=np.float32), bad, x, y)
    neg = negpix(img, x, y, immed, imsig)
    rmscut = rsum / AREA
    good = (bsum <= 0) & (rmscut <= medcut) & (neg == 0)
    return dict(BPMCUT=bsum, RMSCUT=rmscut, MEDCUT=medcut, NEGPIX=neg, GOODCUT=good.astype(np.uint8),
                IMMED=immed, IMSIG=imsig)


def undecided(cuts):
    """Rows whose decision the pin does not settle: ``RMSCUT`` within the aperture pin of ``MEDCUT`` (compared as sums,
    RMSCUT x area), or a ``BPMCUT`` in (0, 1e-9] (the closed-form overlap leaves 1e-15 on pixels outside the circle).
    Returns the two boolean arrays."""
    rsum, msum = cuts['RMSCUT'] * AREA, cuts['MEDCUT'] * AREA
    near = np.abs(rsum - msum) <= PIN_ATOL + PIN_RTOL * abs(msum)
    tiny = (cuts['BPMCUT'] > 0) & (cuts['BPMCUT'] <= 1e-9)
    return near, tiny


# the seeds the GPU tests use (tests/test_cuts_ref.py asserts that none of their rows is undecided)
SEEDS = (11, 12, 13)


def field(seed, bad_bits=BAD_SUM, other_bits=1 << 20, ny=240, nx=256, nrand=120):
    """A synthetic difference image with its noise and mask planes and candidate positions (1-based):
    random positions, positions within 6 px of each frame edge and beyond it, candidates with a bad pixel planted
    inside / across / outside their aperture, with a dipole inside their cutout, at its edge and in the surround
    ring, and inside a noisy patch.  Bad pixels elsewhere are kept 16 px away from every aperture centre, so that no
    aperture holds one it merely grazes by rounding.  ``other_bits``: mask bits that are not bad, sprinkled everywhere.
    Returns (img, rms, mask, x, y)."""
    rng = np.random.default_rng(seed)
    img = rng.normal(0.0, 3.0, (ny, nx)).astype(np.float32)
    rms = (3.0 * (1.0 + 0.05 * rng.uniform(-1, 1, (ny, nx)))).astype(np.float32)
    lowbit = bad_bits & -bad_bits                                  # one bad bit
    mask = np.zeros((ny, nx), np.int32)
    mask[rng.uniform(size=(ny, nx)) < 0.02] |= other_bits
    sprinkle = rng.uniform(size=(ny, nx)) < 0.01
    x = rng.uniform(8.0, nx - 8.0, nrand)
    y = rng.uniform(8.0, ny - 8.0, nrand)
    edge = np.array([[1.0, 60.3], [4.6, 100.0], [nx - 0.5, 80.2], [nx - 5.2, 33.0], [70.4, 1.2], [120.0, 5.9],
                     [99.1, ny - 0.3], [140.8, ny - 4.4], [2.2, 2.9], [nx - 1.0, ny - 2.0], [-3.0, 50.0],
                     [nx + 5.5, 90.0], [60.0, -4.9], [77.7, ny + 6.4], [-20.0, -20.0], [0.5, 0.5]])
    x = np.concatenate([x, edge[:, 0]])
    y = np.concatenate([y, edge[:, 1]])
    # clear the sprinkle around every aperture centre (the aperture sits at (x, y) taken as 0-based)
    jj, ii = np.mgrid[0:ny, 0:nx]
    for xc, yc in zip(x, y):
        sprinkle[(np.abs(ii - xc) <= 16) & (np.abs(jj - yc) <= 16)] = False
    mask[sprinkle] |= lowbit
    # planted, on the first random candidates
    k = 0
    for dx, dy in ((0.0, 0.0), (3.0, -2.0), (-4.0, 1.0), (4.2, 4.2), (0.0, 6.0), (-6.0, 0.0)):   # inside, across
        i, j = int(round(x[k] + dx)), int(round(y[k] + dy))
        mask[j, i] |= bad_bits if k % 2 else lowbit
        k += 1
    for dx, dy in ((-1, 0), (4, 3), (5, -5), (-5, 5), (6, 0), (0, -6), (6, 6)):                    # dipoles
        # cutout centre (0-based) is round(x) - 1; offsets of 5 are its edge, of 6 the surround ring (positive partner)
        cx, cy = int(np.round(x[k])) - 1, int(np.round(y[k])) - 1
        if abs(dx) == 6 or abs(dy) == 6:
            i, j = cx + dx, cy + dy                                  # the positive pixel in the ring ...
            img[j, i] = 80.0
            img[j - np.sign(dy) if dy else j, i - np.sign(dx) if dx else i] = -70.0       # ... its partner at the edge
        else:
            img[cy + dy, cx + dx] = -70.0
            img[cy + dy, cx + dx + (1 if dx <= 0 else -1)] = 80.0
        k += 1
    for _ in range(4):                                                                          # noisy patches
        i, j = int(x[k]), int(y[k])
        rms[max(j - 12, 0):j + 13, max(i - 12, 0):i + 13] *= 2.0
        k += 1
    # a lone positive and a lone negative spike: no dipole
    img[int(np.round(y[k])) - 1, int(np.round(x[k])) - 1] = 90.0
    img[int(np.round(y[k + 1])) - 1, int(np.round(x[k + 1])) - 1] = -90.0
    return img, rms, mask, x, y
