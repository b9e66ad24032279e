"""Scenes for the MASK_TYPE tests: the smallest inputs at which each part of the masked second pass can go wrong.

Test infrastructure.  The measure call takes its rows and its segmentation map from the caller, so most scenes are
hand-built: Gaussians (centres 0-based) on faint noise, a map painted by hand, and rows taken from the map's members
(``rows_from_map``: barycentre and moments of the image values over each label, float64; FWHM_IMAGE where given).  A scene
is a dict: img, sigma (float32), bad (uint8 or None), seg (int32), rows (numpy array of dtype ``ROW``, the fields of
zm_object) and kw (keyword arguments of the restatement: aper_radius, kron_fact, kron_min).  ``deblended`` takes rows and
map from a deblending extraction: ``tests/deblend_ref.py`` on the CPU (for the census), ``zm_extract_deblend`` itself in
the GPU tests.
"""
import functools

import numpy as np

import measure_ref as mr

# the fields of zm_object (include/zudsmi.h) in their order; the ctypes mirror gives the same numpy dtype
ROW = np.dtype([('number', 'i4'), ('npix', 'i4'), ('xmin', 'i4'), ('xmax', 'i4'), ('ymin', 'i4'), ('ymax', 'i4'),
                ('flags', 'i4'), ('flags_weight', 'i4'), ('imaflags_iso', 'i4'), ('first', 'i4'), ('nthresh', 'i4'),
                ('pad_', 'i4'), ('x_image', 'f8'), ('y_image', 'f8'), ('x2', 'f8'), ('y2', 'f8'), ('xy', 'f8'),
                ('a_image', 'f8'), ('b_image', 'f8'), ('theta_image', 'f8'), ('elongation', 'f8'), ('fwhm_image', 'f8'),
                ('flux_iso', 'f8'), ('flux_max', 'f8'), ('peak', 'f8'), ('flux_aper', 'f8'), ('fluxerr_aper', 'f8'),
                ('x_world', 'f8'), ('y_world', 'f8')])

NAMES = ['alone', 'pair', 'corner', 'both_foreign', 'bad_column', 'wide_window_small_kron', 'deblended']
CLEAN_SCENES = ['alone']             # no foreign and no bad pixel at all


def gaussians(nx, ny, items, noise=0.02, seed=7):
    """items: (x, y, flux, fwhm)."""
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    img = np.random.default_rng(seed).normal(0.0, noise, (ny, nx))
    for x, y, flux, fw in items:
        s = fw / 2.35482
        img += flux * np.exp(-0.5 * ((xx - x) ** 2 + (yy - y) ** 2) / (s * s)) / (2.0 * np.pi * s * s)
    return img.astype(np.float32), np.ones((ny, nx), np.float32)


def rows_from_map(img, seg, fwhm=None):
    """One row per label 1 .. max(seg) from the image values over the label's pixels.  ``fwhm``: {number: FWHM_IMAGE};
    without one a row has fwhm_image = 0 and the window takes sqrt((x2 + y2) / 2)."""
    n = int(seg.max())
    rows = np.zeros(n, ROW)
    for k in range(1, n + 1):
        y, x = np.nonzero(seg == k)
        v = img[y, x].astype(np.float64)
        v = np.where(np.isfinite(v), v, 0.0)
        S = v.sum()
        xb, yb = (v * x).sum() / S, (v * y).sum() / S
        x2, y2, xy = (v * (x - xb) ** 2).sum() / S, (v * (y - yb) ** 2).sum() / S, (v * (x - xb) * (y - yb)).sum() / S
        if x2 * y2 - xy * xy < 0.00694:
            x2, y2 = x2 + 1.0 / 12.0, y2 + 1.0 / 12.0
        a, b, th = mr.ellipse(x2, y2, xy, thin=False)
        r = rows[k - 1]
        r['number'], r['npix'] = k, len(x)
        r['xmin'], r['xmax'], r['ymin'], r['ymax'] = x.min() + 1, x.max() + 1, y.min() + 1, y.max() + 1
        r['x_image'], r['y_image'], r['x2'], r['y2'], r['xy'] = xb + 1.0, yb + 1.0, x2, y2, xy
        r['a_image'], r['b_image'], r['theta_image'], r['elongation'] = a, b, th, a / b
        r['fwhm_image'] = (fwhm or {}).get(k, 0.0)
        r['flux_iso'], r['flux_max'], r['peak'] = S, v.max(), v.max()
        r['first'] = int(y[0]) * seg.shape[1] + int(x[0])
        r['x_world'] = r['y_world'] = np.nan
    return rows


def objects(rows, ext=None):
    """The restatement's object dicts of ``rows`` (a ROW array); ``ext``: rows with errx2 / erry2 / errxy for the window's
    fallback."""
    out = []
    for k, r in enumerate(rows):
        o = dict(number=int(r['number']), xc=float(r['x_image']) - 1.0, yc=float(r['y_image']) - 1.0, x2=float(r['x2']),
                 y2=float(r['y2']), xy=float(r['xy']), fwhm=float(r['fwhm_image']), a=float(r['a_image']),
                 b=float(r['b_image']), theta=float(r['theta_image']))
        if ext is not None:
            o.update(errx2=float(ext['errx2'][k]), erry2=float(ext['erry2'][k]), errxy=float(ext['errxy'][k]))
        out.append(o)
    return out


def paint_nearest(img, centres, level=1.5):
    """Pixels above ``level`` within 9 px of a centre, labelled by the nearest centre (1-based in the order given)."""
    ny, nx = img.shape
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    d = np.stack([np.hypot(xx - x, yy - y) for x, y in centres])
    seg = (np.argmin(d, axis=0) + 1).astype(np.int32)
    seg[~((img > level) & (d.min(axis=0) < 9.0))] = 0
    return seg


def _scene(img, sigma, seg, bad=None, fwhm=None, **kw):
    return dict(img=img, sigma=sigma, bad=bad, seg=np.ascontiguousarray(seg, np.int32), rows=rows_from_map(img, seg, fwhm), kw=kw)


def alone():
    """40 x 40: one Gaussian, nothing foreign, nothing bad: both mask types must give the unmasked call's bits."""
    img, sigma = gaussians(40, 40, [(19.3, 20.6, 2500.0, 3.5)])
    return _scene(img, sigma, paint_nearest(img, [(19.3, 20.6)]), fwhm={1: 3.5})


def pair():
    """48 x 40: two Gaussians 6 px apart, the map split where the nearer centre changes: each lies inside the other's
    aperture, Kron ellipse and window."""
    c = [(20.3, 19.6, 3000.0, 3.2), (26.3, 20.2, 1800.0, 3.2)]
    img, sigma = gaussians(48, 40, c)
    return _scene(img, sigma, paint_nearest(img, [q[:2] for q in c]), fwhm={1: 3.2, 2: 3.2})


def corner():
    """40 x 40: an object 4 px from the corner with a neighbour on its inner side: the neighbour's mirrors fall off the
    frame (lost under CORRECT as well); the neighbour's own foreign pixels have mirrors in the frame."""
    c = [(4.2, 3.7, 2500.0, 3.0), (10.4, 6.1, 1500.0, 3.0)]
    img, sigma = gaussians(40, 40, c)
    return _scene(img, sigma, paint_nearest(img, [q[:2] for q in c]), fwhm={1: 3.0, 2: 3.0})


def both_foreign():
    """64 x 64: an object with two painted foreign blocks that are each other's mirrors about its centre (lost under
    CORRECT), and a third block whose mirror is clean (replaced)."""
    img, sigma = gaussians(64, 64, [(32.3, 31.6, 6000.0, 5.0)])
    seg = paint_nearest(img, [(32.3, 31.6)])
    seg[30:34, 36:39] = 2            # mirror of x 36 .. 38 about 32.3 is x 27 .. 29 (floor(64.6 - i + 0.5)), y 30 .. 33 -> 30 .. 33
    seg[30:34, 27:30] = 3
    seg[36:38, 30:35] = 4            # mirror rows 25 .. 27: clean
    img[30:34, 36:39] += 40.0
    img[30:34, 27:30] += 25.0
    img[36:38, 30:35] += 30.0
    return _scene(img, sigma, seg, fwhm={1: 5.0})


def bad_column():
    """56 x 48: a bad column and two NaN pixels (and one pixel with sigma = 0) through an object: its own bad pixels are
    replaced by their mirrors; nothing is foreign."""
    img, sigma = gaussians(56, 48, [(28.4, 24.3, 5000.0, 4.5)])
    seg = paint_nearest(img, [(28.4, 24.3)])
    bad = np.zeros(img.shape, np.uint8)
    bad[:, 30] = 1
    img[22, 26], img[27, 27] = np.nan, np.inf
    sigma[25, 25] = 0.0
    return _scene(img, sigma, seg, bad=bad, fwhm={1: 4.5})


def wide_window_small_kron():
    """72 x 64: object 1 has FWHM_IMAGE 7.1 (window radius 12 px: a box of 26 x 26 > 256 elements, the stride loop);
    object 2 is 7 pixels with moments near 0.3 (a Kron box under 64 elements: a part-filled wave).  Each has foreign and
    bad pixels in its footprints; the aperture radius is 2.5."""
    img, sigma = gaussians(72, 64, [(30.4, 31.7, 9000.0, 7.1), (55.3, 20.6, 60.0, 1.3), (36.6, 35.2, 900.0, 2.5),
                                    (57.4, 22.7, 40.0, 1.3)])
    seg = np.zeros(img.shape, np.int32)
    yy, xx = np.mgrid[0:64, 0:72]
    seg[(np.hypot(xx - 30.4, yy - 31.7) < 7.5)] = 1
    seg[(np.abs(xx - 55) + np.abs(yy - 21) <= 1) | ((xx == 56) & (yy == 20)) | ((xx == 54) & (yy == 20))] = 2
    seg[np.hypot(xx - 36.6, yy - 35.2) < 2.2] = 3
    seg[(np.abs(xx - 57) <= 1) & (np.abs(yy - 23) <= 1) & (seg == 0)] = 4
    bad = np.zeros(img.shape, np.uint8)
    bad[28, 20:24] = 1
    bad[19, 55] = 1
    return _scene(img, sigma, seg, bad=bad, fwhm={1: 7.1, 2: 1.3, 3: 2.5, 4: 1.3}, aper_radius=2.5)


DEBLENDED_SOURCES = [(14.3, 12.6, 900.0, 2.6), (40.7, 15.2, 2500.0, 3.4), (46.2, 16.9, 1900.0, 3.2), (75.1, 20.4, 1500.0, 3.0),
                     (22.2, 40.8, 3000.0, 4.0), (52.5, 44.3, 1200.0, 2.8), (58.1, 46.0, 1000.0, 2.8), (82.6, 50.3, 800.0, 2.6),
                     (12.4, 66.7, 1500.0, 3.0), (36.6, 68.2, 2200.0, 3.6), (64.3, 70.1, 700.0, 2.6), (88.2, 72.9, 1300.0, 3.0)]


def deblended_planes():
    """96 x 80: a dozen Gaussians, two pairs of them about 6 px apart under one detection footprint."""
    return gaussians(96, 80, DEBLENDED_SOURCES, seed=11)


def rows_of_table(tab, objs):
    """ROW array of an extraction table (restatement columns) and the objects ``measure_ref.objects_of`` made of it."""
    rows = np.zeros(len(tab), ROW)
    for k, o in enumerate(objs):
        r = rows[k]
        r['number'], r['npix'] = o['number'], tab['ISOAREA_IMAGE'][k]
        r['xmin'], r['xmax'], r['ymin'], r['ymax'] = (tab[c][k] for c in ('XMIN_IMAGE', 'XMAX_IMAGE', 'YMIN_IMAGE', 'YMAX_IMAGE'))
        r['x_image'], r['y_image'], r['x2'], r['y2'], r['xy'] = o['xc'] + 1.0, o['yc'] + 1.0, o['x2'], o['y2'], o['xy']
        r['a_image'], r['b_image'], r['theta_image'], r['fwhm_image'] = o['a'], o['b'], o['theta'], o['fwhm']
        r['flags'] = tab['FLAGS'][k]
    return rows


def deblended():
    """The CPU form: rows and map of tests/deblend_ref.py (what zm_extract_deblend is pinned to)."""
    import deblend_ref as dr
    img, sigma = deblended_planes()
    base = dr.deblend(img, sigma)
    base.update(img=img, sigma=sigma)
    assert base['nsplit'] >= 1, 'the scene is meant to hold a deblended pair'
    return dict(img=img, sigma=sigma, bad=None, seg=np.ascontiguousarray(base['segm'], np.int32),
                rows=rows_of_table(base['table'], mr.objects_of(base)), kw={})


@functools.lru_cache(maxsize=None)
def scene(name):
    return globals()[name]()
