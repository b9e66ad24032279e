"""numpy restatement of the source extractor (csrc/extract.hip; DESIGN.md "Source extraction").

Test infrastructure, imported like ``util.py``.  The operator is a chosen convention (there is no SExtractor to compare
with); this file states it a second time, independently of the HIP code, and ``test_extract_ref.py`` holds it against
things that are not ours (``scipy.ndimage.label``, analytic Gaussians).

``extract(..., reverse=True)`` evaluates every float64 sum in the opposite order: the difference between the two is the
size of a summation-order effect, which the GPU tests derive their bounds from.
"""
import numpy as np

from oracle import photometry as ophot

COLUMNS = [('NUMBER', 'i4'), ('X_IMAGE', 'f8'), ('Y_IMAGE', 'f8'), ('X_WORLD', 'f8'), ('Y_WORLD', 'f8'),
           ('XMIN_IMAGE', 'i4'), ('XMAX_IMAGE', 'i4'), ('YMIN_IMAGE', 'i4'), ('YMAX_IMAGE', 'i4'),
           ('ISOAREA_IMAGE', 'i4'), ('A_IMAGE', 'f8'), ('B_IMAGE', 'f8'), ('THETA_IMAGE', 'f8'), ('ELONGATION', 'f8'),
           ('FWHM_IMAGE', 'f8'), ('FLUX_ISO', 'f8'), ('FLUX_MAX', 'f8'), ('FLUX_APER', 'f8'), ('FLUXERR_APER', 'f8'),
           ('FLAGS', 'i4'), ('FLAGS_WEIGHT', 'i4'), ('IMAFLAGS_ISO', 'i4')]
FLOAT_COLUMNS = [n for n, t in COLUMNS if t == 'f8' and not n.endswith('WORLD')]
INT_COLUMNS = [n for n, t in COLUMNS if t == 'i4']

KERNEL = ((1, 2, 1), (2, 4, 2), (1, 2, 1))          # default.conv, times 16


def bad_pixels(img, sigma, bad=None):
    b = ~np.isfinite(img) | ~np.isfinite(sigma) | ~(sigma > 0)
    if bad is not None:
        b |= np.asarray(bad) != 0
    return b


def filter_image(img, badmap):
    """3 x 3 filter, float32, taps in row-major order, 1 / 16 last; bad and outside pixels enter as 0."""
    ny, nx = img.shape
    pad = np.zeros((ny + 2, nx + 2), np.float32)
    pad[1:-1, 1:-1] = np.where(badmap, np.float32(0), img)
    acc = np.zeros((ny, nx), np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for r in range(3):
            for d in range(3):
                acc = acc + np.float32(KERNEL[r][d]) * pad[r:r + ny, d:d + nx]
        return acc * np.float32(0.0625)


def label8(fg):
    """For every foreground pixel the smallest linear index of its 8-connected component; -1 elsewhere.

    Runs of foreground pixels per row, union-find over runs that touch in adjacent rows."""
    fg = np.asarray(fg, bool)
    ny, nx = fg.shape
    pad = np.zeros((ny, nx + 2), np.int8)
    pad[:, 1:-1] = fg
    d = np.diff(pad, axis=1)
    ys, xs = np.nonzero(d == 1)                      # row-major: runs in raster order; xs = first column
    _, xe = np.nonzero(d == -1)                      # one past the last column
    nrun = len(ys)
    out = np.full((ny, nx), -1, np.int64)
    if nrun == 0:
        return out
    parent = list(range(nrun))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    xs_l, xe_l = xs.tolist(), xe.tolist()
    row0 = np.searchsorted(ys, np.arange(ny + 1)).tolist()
    for y in range(1, ny):
        i, iend, j, jend = row0[y - 1], row0[y], row0[y], row0[y + 1]
        while i < iend and j < jend:
            if xs_l[i] <= xe_l[j] and xe_l[i] >= xs_l[j]:       # columns overlap once either run is widened by one
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            if xe_l[i] < xe_l[j]:
                i += 1
            else:
                j += 1
    root = np.array([find(a) for a in range(nrun)])
    first = ys.astype(np.int64) * nx + xs               # first pixel of every run; of a root run: of the component
    out[fg] = np.repeat(first[root], xe - xs)
    return out


def segment(labels, minarea):
    """(segmentation map int32, first pixel of every kept object, npix) from label8's output."""
    lab = labels.ravel()
    idx = np.flatnonzero(lab >= 0)
    roots, counts = np.unique(lab[idx], return_counts=True)     # ascending = raster order of the first pixel
    keep = counts >= minarea
    number = np.zeros(len(roots), np.int32)
    number[keep] = np.arange(1, keep.sum() + 1, dtype=np.int32)
    seg = np.zeros(lab.shape, np.int32)
    seg[idx] = number[np.searchsorted(roots, lab[idx])]
    return seg.reshape(labels.shape), roots[keep], counts[keep]


def _sum(a, reverse):
    a = np.asarray(a, np.float64)
    return float(np.sum(a[::-1] if reverse else a))


def extract(img, sigma, bad=None, flag=None, detect_thresh=1.5, detect_minarea=5, use_filter=True, satur_level=50000.0,
            aper_radius=3.0, reverse=False, wcs=None):
    """dict(filtered, fg, segm, table, first).  ``wcs``: an object with all_pix2world(x, y, 1), or None (NaN)."""
    img = np.ascontiguousarray(img, np.float32)
    sigma = np.ascontiguousarray(sigma, np.float32)
    ny, nx = img.shape
    badmap = bad_pixels(img, sigma, bad)
    filt = filter_image(img, badmap) if use_filter else img
    with np.errstate(invalid='ignore', over='ignore'):
        thr = np.float32(detect_thresh) * sigma
        fg = ~badmap & (filt > thr)
    seg, first, npix = segment(label8(fg), detect_minarea)
    n = len(first)
    tab = np.zeros(n, dtype=COLUMNS)
    flat = seg.ravel()
    members = np.flatnonzero(flat)
    order = np.argsort(flat[members], kind='stable')     # raster order inside every object
    members = members[order]
    bounds = np.searchsorted(flat[members], np.arange(1, n + 2))
    badpad = np.zeros((ny + 2, nx + 2), bool)
    badpad[1:-1, 1:-1] = badmap
    near_bad = np.zeros((ny, nx), bool)
    for dy in range(3):
        for dx in range(3):
            near_bad |= badpad[dy:dy + ny, dx:dx + nx]
    fl_flat = None if flag is None else np.asarray(flag).astype(np.int32).ravel()
    ffilt, fimg, fthr = filt.ravel(), img.ravel(), thr.ravel()
    for k in range(n):
        p = members[bounds[k]:bounds[k + 1]]
        y, x = np.divmod(p, nx)
        xmin, xmax, ymin, ymax = x.min(), x.max(), y.min(), y.max()
        v = ffilt[p].astype(np.float64)
        dx, dy = (x - xmin).astype(np.float64), (y - ymin).astype(np.float64)
        S = _sum(v, reverse)
        xb, yb = _sum(v * dx, reverse) / S, _sum(v * dy, reverse) / S
        x2 = _sum(v * dx * dx, reverse) / S - xb * xb
        y2 = _sum(v * dy * dy, reverse) / S - yb * yb
        xy = _sum(v * dx * dy, reverse) / S - xb * yb
        if x2 * y2 - xy * xy < 0.00694:
            x2 += 1.0 / 12.0
            y2 += 1.0 / 12.0
        pm, dm = 0.5 * (x2 + y2), 0.5 * (x2 - y2)
        rt = np.sqrt(dm * dm + xy * xy)
        A, B = np.sqrt(pm + rt), np.sqrt(max(pm - rt, 0.0))
        r = tab[k]
        r['NUMBER'] = k + 1
        r['X_IMAGE'], r['Y_IMAGE'] = xmin + xb + 1.0, ymin + yb + 1.0
        r['XMIN_IMAGE'], r['XMAX_IMAGE'], r['YMIN_IMAGE'], r['YMAX_IMAGE'] = xmin + 1, xmax + 1, ymin + 1, ymax + 1
        r['ISOAREA_IMAGE'] = len(p)
        r['A_IMAGE'], r['B_IMAGE'] = A, B
        r['THETA_IMAGE'] = 0.5 * np.degrees(np.arctan2(2.0 * xy, x2 - y2))
        with np.errstate(divide='ignore'):
            r['ELONGATION'] = np.float64(A) / np.float64(B)
        ipk = int(np.argmax(ffilt[p]))                   # first pixel in raster order of the largest value
        peak = ffilt[p][ipk]
        t = max(fthr[p[ipk]], np.float32(0.5) * peak)    # float32
        nt = int(np.count_nonzero(ffilt[p] >= t))
        r['FWHM_IMAGE'] = np.sqrt(4.0 * np.log(2.0) * nt / (np.pi * np.log(np.float64(peak) / np.float64(t)))) \
            if peak > t else 0.0
        r['FLUX_ISO'] = _sum(fimg[p], reverse)
        r['FLUX_MAX'] = fimg[p].max()
        r['IMAFLAGS_ISO'] = 0 if fl_flat is None else np.bitwise_or.reduce(fl_flat[p])
        r['FLAGS_WEIGHT'] = int(near_bad.ravel()[p].any())
        flags = 4 if (fimg[p] >= np.float32(satur_level)).any() else 0
        if xmin == 0 or ymin == 0 or xmax == nx - 1 or ymax == ny - 1:
            flags |= 8
        xc, yc = r['X_IMAGE'] - 1.0, r['Y_IMAGE'] - 1.0
        rad = float(aper_radius)
        # bit 16: the circle leaves the frame (pixel i covers [i - 0.5, i + 0.5]) or reaches a bad pixel (the point of the
        # pixel's square nearest to the centre lies inside the radius)
        if xc - rad < -0.5 or xc + rad > nx - 0.5 or yc - rad < -0.5 or yc + rad > ny - 0.5:
            flags |= 16
        i0, i1, j0, j1 = ophot.bbox(xc, yc, rad)
        i0, i1, j0, j1 = max(i0, 0), min(i1, nx), max(j0, 0), min(j1, ny)
        if i0 < i1 and j0 < j1:
            jj, ii = np.mgrid[j0:j1, i0:i1]
            ddx = np.maximum(np.abs(ii - xc) - 0.5, 0.0)
            ddy = np.maximum(np.abs(jj - yc) - 0.5, 0.0)
            if (badmap[j0:j1, i0:i1] & (ddx * ddx + ddy * ddy < rad * rad)).any():
                flags |= 16
            # the aperture sums of oracle/photometry.py (same fractions, same pixels), in the order asked for
            frac = ophot.overlap_fraction(ii - 0.5 - xc, ii + 0.5 - xc, jj - 0.5 - yc, jj + 0.5 - yc, rad)
            with np.errstate(invalid='ignore', over='ignore'):
                r['FLUX_APER'] = _sum((img[j0:j1, i0:i1].astype(np.float64) * frac).ravel(), reverse)
                r['FLUXERR_APER'] = np.sqrt(_sum((sigma[j0:j1, i0:i1].astype(np.float64) ** 2 * frac).ravel(), reverse))
        r['FLAGS'] = flags
    if wcs is not None and n:
        tab['X_WORLD'], tab['Y_WORLD'] = wcs.all_pix2world(tab['X_IMAGE'], tab['Y_IMAGE'], 1)
    else:
        tab['X_WORLD'] = tab['Y_WORLD'] = np.nan
    return dict(filtered=filt, fg=fg, segm=seg, table=tab, first=first, bad=badmap)


def order_bounds(fwd, rev, margin=10.0):
    """Per float column: ``margin`` x the largest difference between the restatement's forward and reversed summation
    order - the size of an order effect on this input, nothing else."""
    out = {}
    for c in FLOAT_COLUMNS:
        a, b = fwd[c], rev[c]
        ok = np.isfinite(a) & np.isfinite(b)
        out[c] = margin * float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0
    return out


# Columns whose last step is a library function that is not correctly rounded, so that two correct implementations
# differ on identical inputs.  The allowance is per row, in units of the spacing of the row's own value:
#   THETA_IMAGE = 0.5 * atan2(2 xy, x2 - y2) * (180 / pi).  glibc documents atan2 to 1 ulp and numpy its float64 SIMD
#     loops to 4 ulp: the two results are at most 5 ulp apart; the product with 180 / pi rounds once on either side
#     (half an ulp each; the factor 0.5 is exact): 6 ulp.
#   FWHM_IMAGE = sqrt(4 ln2 n / (pi ln(peak / t))).  peak / t is one IEEE division of the same floats on both sides; the
#     two logarithms are at most 1 + 4 = 5 ulp apart; numerator and denominator take two roundings each on either side
#     (4 ulp in all), the quotient one each (1 ulp): a relative difference of 10 ulp under the root, which halves it,
#     plus the root's own rounding on either side: 6 ulp.
# Every other column ends in +, -, *, / or sqrt, which IEEE 754 rounds correctly: the same sums give the same bits, and
# the order bound stands alone.
LIBM_ULPS = {'THETA_IMAGE': 6, 'FWHM_IMAGE': 6}


def libm_allowance(column, values):
    """Per-row allowance (array) for a column of LIBM_ULPS; zeros for every other column."""
    v = np.abs(np.asarray(values, np.float64))
    return LIBM_ULPS.get(column, 0) * np.spacing(np.where(np.isfinite(v), v, 0.0))
