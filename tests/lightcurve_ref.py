"""A restatement of the footprint join and the batched forced photometry that shares no formula with
``csrc/lightcurve.hip``, and the scenes the GPU tests run.

Membership goes the way q3c goes: the four corners of a footprint and the source are projected gnomonically about the
image centre (float64), where great circles are straight lines, and a planar crossing-number test decides - no edge
planes, no orientation sign.  A source in the far hemisphere of the centre is outside.  Sky -> pixel is ``oracle/wcs.py``
(``sky2pix``), apertures are ``tests/aperture_ref.py``.

A crossing-number test and a plane-sign test may disagree about a source that lies on an edge to within rounding.
``edge_distance_arcsec`` gives the angular distance of every source to the nearest edge of every footprint, and
``assert_clear`` holds every scene to 1e-3 arcsec - float64 rounding is some 1e-10 arcsec, so the band is a condition on
the scenes, not a tolerance: membership is then compared exactly, every pair.

numpy and the oracle only.
"""
import numpy as np

import aperture_ref as ar
from util import synth, to_oracle_wcs

D2R = np.pi / 180.0
ARCSEC_PER_RAD = 648000.0 / np.pi
EDGE_BAND_ARCSEC = 1e-3
RADIUS = 3.0                      # APERTURE_RADIUS

# |x - oracle| and |y - oracle| of the batch, pixels: tests/measure_lightcurve_tolerance.py measures the host's
# zm_wcs_sky2pix and the float64 oracle against a 50-digit evaluation on exactly these scenes; the bound is 4 x the larger
# of the two, rounded up to a power of two (the factor: a device sin / cos / FMA contraction that differs from the host's).
# Measured: 9.877e-11 px (the frame across RA 0; 2.2e-11 .. 3.7e-11 elsewhere), x 4 = 3.95e-10, so 2^-31 = 4.66e-10 px -
# far below the 1e-7 px tests/test_abi.py grants the host's round trip.
POS_TOL_PX = 2.0 ** -31


def unit(ra, dec):
    a, d = np.asarray(ra, dtype=np.float64) * D2R, np.asarray(dec, dtype=np.float64) * D2R
    return np.stack([np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)], axis=-1)


def corners(ow):
    """[4, 2] (ra, dec) of the centres of the corner pixels, WCS.calc_footprint's order."""
    nx, ny = ow.naxis
    ra, dec = ow.pix2sky(np.array([1.0, 1.0, nx, nx]), np.array([1.0, ny, ny, 1.0]))
    return np.stack([ra, dec], axis=1)


def centre(ow):
    nx, ny = ow.naxis
    ra, dec = ow.pix2sky(np.array([(nx + 1) / 2.0]), np.array([(ny + 1) / 2.0]))
    return float(ra[0]), float(dec[0])


def gnomonic(ra0, dec0, ra, dec):
    """Standard coordinates (xi, eta) about (ra0, dec0), and which points lie in its hemisphere."""
    a0, d0 = ra0 * D2R, dec0 * D2R
    a, d = np.asarray(ra, dtype=np.float64) * D2R, np.asarray(dec, dtype=np.float64) * D2R
    with np.errstate(invalid='ignore', divide='ignore'):
        cosc = np.sin(d0) * np.sin(d) + np.cos(d0) * np.cos(d) * np.cos(a - a0)
        xi = np.cos(d) * np.sin(a - a0) / cosc
        eta = (np.cos(d0) * np.sin(d) - np.sin(d0) * np.cos(d) * np.cos(a - a0)) / cosc
    return xi, eta, cosc > 0


def crossing_number(px, py, qx, qy):
    """True where (qx, qy) is inside the planar polygon (px, py): a ray towards +x crosses its outline an odd number of
    times."""
    inside = np.zeros(np.shape(qx), dtype=bool)
    n = len(px)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(n):
            j = (i + 1) % n
            straddles = (py[i] > qy) != (py[j] > qy)
            xcross = (px[j] - px[i]) * (qy - py[i]) / (py[j] - py[i]) + px[i]
            inside ^= straddles & (qx < xcross)
    return inside


def inside_corners(corner_radec, ra, dec, centre_radec=None):
    """Membership of (ra, dec) in the great-circle polygon with these corners; projection about ``centre_radec``
    (default: the direction of the corners' vector sum).  A position that is not finite is outside."""
    corner_radec = np.asarray(corner_radec, dtype=np.float64)
    if centre_radec is None:
        s = unit(corner_radec[:, 0], corner_radec[:, 1]).sum(axis=0)
        s /= np.linalg.norm(s)
        centre_radec = (np.arctan2(s[1], s[0]) / D2R, np.arcsin(s[2]) / D2R)
    cx, cy, cok = gnomonic(*centre_radec, corner_radec[:, 0], corner_radec[:, 1])
    assert cok.all()
    qx, qy, ok = gnomonic(*centre_radec, ra, dec)
    fin = np.isfinite(np.asarray(ra, dtype=np.float64)) & np.isfinite(np.asarray(dec, dtype=np.float64))
    return crossing_number(cx, cy, qx, qy) & ok & fin


def membership(ows, ra, dec):
    """(offsets int64 [nimg + 1], src_idx int32) as the join returns them."""
    ra, dec = np.asarray(ra, dtype=np.float64), np.asarray(dec, dtype=np.float64)
    lists = [np.flatnonzero(inside_corners(corners(ow), ra, dec, centre(ow))) if ra.size else np.zeros(0, np.int64)
             for ow in ows]
    offsets = np.zeros(len(ows) + 1, np.int64)
    if lists:
        offsets[1:] = np.cumsum([len(v) for v in lists])
    return offsets, (np.concatenate(lists) if lists else np.zeros(0)).astype(np.int32)


def edge_distance_arcsec(ows, ra, dec):
    """[nimg, nsrc]: the angle between each source and the nearest point of the nearest edge (an arc between two
    corners) of each footprint; NaN for a source that is not finite."""
    p = unit(ra, dec)
    out = np.empty((len(ows), p.shape[0]))
    for k, ow in enumerate(ows):
        c = corners(ow)
        v = unit(c[:, 0], c[:, 1])
        best = np.full(p.shape[0], np.inf)
        for i in range(4):
            a, b = v[i], v[(i + 1) % 4]
            n = np.cross(a, b)
            n /= np.linalg.norm(n)
            h = p @ n                                                  # sine of the distance to the great circle
            foot = p - h[:, None] * n
            between = (np.cross(a, foot) @ n >= 0) & (np.cross(foot, b) @ n >= 0)
            ends = np.minimum(np.linalg.norm(p - a, axis=1), np.linalg.norm(p - b, axis=1))
            with np.errstate(invalid='ignore'):
                d = np.where(between, np.arcsin(np.minimum(np.abs(h), 1.0)), 2.0 * np.arcsin(np.minimum(0.5 * ends, 1.0)))
            best = np.where(np.isnan(h), np.nan, np.minimum(best, d))
        out[k] = best * ARCSEC_PER_RAD
    return out


def assert_clear(ows, ra, dec):
    """The condition on a scene: no (finite) source within EDGE_BAND_ARCSEC of an edge of any footprint."""
    if len(ows) == 0 or np.size(ra) == 0:
        return
    d = edge_distance_arcsec(ows, ra, dec)
    assert not (d[np.isfinite(d)] < EDGE_BAND_ARCSEC).any(), float(np.nanmin(d))


# ---- scenes -----------------------------------------------------------------------------------------------------------
FRAMES = ('negdet', 'posdet', 'rot37', 'tpv', 'ra0', 'pole')


def frame_wcs(name):
    """The product's WCS object of a named frame (``to_oracle_wcs`` gives the oracle's)."""
    s = synth()
    if name == 'negdet':
        return s.tan_wcs(96, 80)                                       # CD = diag(-s, s)
    if name == 'posdet':
        return s.ztf_wcs(96, 80, tpv=False)                            # the ZTF CD matrix: det > 0
    if name == 'rot37':
        return s.ztf_wcs(130, 70, dx=3.25, dy=-2.5, rot_deg=37.0, tpv=False)
    if name == 'tpv':
        return s.ztf_wcs(96, 80, dx=-1.75, dy=2.25, rot_deg=0.3, tpv=True)
    if name == 'ra0':
        return s.tan_wcs(130, 70, crval=(0.0031, 12.0))                # 130 px of 1 arcsec across RA 0
    if name == 'pole':
        return s.tan_wcs(96, 80, crval=(40.0, 89.9992))                # the pole lies 3 px from CRPIX
    raise KeyError(name)


def planted_pixels(nx, ny):
    """1-based pixel positions 1.5 px inside and 1.5 px outside the polygon through the corner-pixel centres
    ([1, nx] x [1, ny]) along each edge and beside each corner, 0.25 px inside along each edge (clipped boxes), and
    whether each is inside."""
    xs, ys = [], []
    for t in (0.11, 0.37, 0.5, 0.83):
        ex, ey = 1.0 + t * (nx - 1.0), 1.0 + t * (ny - 1.0)
        for off in (1.5, -1.5, 0.25):
            xs += [ex, ex, 1.0 + off, nx - off]
            ys += [1.0 + off, ny - off, ey, ey]
    for cx, sx in ((1.0, 1.0), (float(nx), -1.0)):
        for cy, sy in ((1.0, 1.0), (float(ny), -1.0)):
            for ox in (1.5, -1.5):
                for oy in (1.5, -1.5):
                    xs.append(cx + sx * ox)
                    ys.append(cy + sy * oy)
    x, y = np.array(xs), np.array(ys)
    return x, y, (x > 1.0) & (x < nx) & (y > 1.0) & (y < ny)


def frame_scene(name, seed=5, nrandom=40):
    """(product WCS, oracle WCS, ra, dec, planted-inside flags or None per source) of a named frame: the planted
    positions, ``nrandom`` inside and ``nrandom`` within two frame widths around."""
    w = frame_wcs(name)
    ow = to_oracle_wcs(w)
    nx, ny = ow.naxis
    rng = np.random.default_rng(seed)
    px, py, pin = planted_pixels(nx, ny)
    ix, iy = rng.uniform(4.0, nx - 3.0, nrandom), rng.uniform(4.0, ny - 3.0, nrandom)
    ox, oy = rng.uniform(-nx, 2.0 * nx, 3 * nrandom), rng.uniform(-ny, 2.0 * ny, 3 * nrandom)
    far = (ox < -2.0) | (ox > nx + 3.0) | (oy < -2.0) | (oy > ny + 3.0)
    x = np.concatenate([px, ix, ox[far]])
    y = np.concatenate([py, iy, oy[far]])
    known = np.concatenate([pin, np.ones(nrandom, bool), np.zeros(int(far.sum()), bool)])
    order = rng.permutation(x.size)
    ra, dec = ow.pix2sky(x[order], y[order])
    return w, ow, ra, dec, known[order]


def make_planes(nx, ny, seed, rms=True, mask=True):
    """(img float32, rms float32 or None, mask int32 or None): noise on a sky, a few stars, sparse flag bits."""
    rng = np.random.default_rng(seed)
    img = rng.normal(3.0, 2.0, (ny, nx))
    yy, xx = np.mgrid[0:ny, 0:nx]
    for _ in range(6):
        cx, cy, f = rng.uniform(0, nx), rng.uniform(0, ny), rng.uniform(200, 4000)
        img += f * np.exp(-0.5 * ((xx - cx) ** 2 + (yy - cy) ** 2) / 0.9 ** 2)
    r = rng.uniform(1.0, 3.0, (ny, nx)).astype(np.float32) if rms else None
    m = None
    if mask:
        m = np.zeros((ny, nx), np.int32)
        hit = rng.uniform(size=(ny, nx)) < 0.02
        m[hit] = 1 << rng.integers(0, 17, int(hit.sum()))
    return img.astype(np.float32), r, m


def batch_scene(seed=21, nsrc=220):
    """Three overlapping frames of different sizes in one batch - 96 x 80 (all planes), 130 x 70 (rms None), 71 x 37
    (mask None) - and sources over their union, some outside all."""
    s = synth()
    ws = [s.ztf_wcs(96, 80, tpv=True), s.ztf_wcs(130, 70, dx=11.5, dy=-4.25, rot_deg=12.0, tpv=True),
          s.ztf_wcs(71, 37, dx=-9.0, dy=6.5, rot_deg=-25.0, tpv=False)]
    ows = [to_oracle_wcs(w) for w in ws]
    planes = [make_planes(96, 80, seed), make_planes(130, 70, seed + 1, rms=False), make_planes(71, 37, seed + 2, mask=False)]
    rng = np.random.default_rng(seed + 3)
    x, y = rng.uniform(-40.0, 136.0, nsrc), rng.uniform(-30.0, 110.0, nsrc)
    ra, dec = ows[0].pix2sky(x, y)
    return ws, ows, planes, ra, dec


def count_scene(n, seed=9):
    """One 96 x 80 TPV frame with exactly ``n`` sources inside among others outside, interleaved."""
    w = synth().ztf_wcs(96, 80, dx=0.5, dy=-0.75, rot_deg=1.0, tpv=True)
    ow = to_oracle_wcs(w)
    rng = np.random.default_rng(seed + n)
    x = np.concatenate([rng.uniform(3.0, 94.0, n), rng.uniform(100.0, 300.0, n // 2 + 3)])
    y = np.concatenate([rng.uniform(3.0, 78.0, n), rng.uniform(-200.0, 200.0, n // 2 + 3)])
    order = rng.permutation(x.size)
    ra, dec = ow.pix2sky(x[order], y[order])
    return w, ow, ra, dec


def photometry(ows, planes, ra, dec, offsets, src_idx, xy=None):
    """Per pair: (x, y) 0-based from the oracle's sky2pix - or the ``xy`` handed in - and ``aperture_sums`` there with
    the terms of its bounds: dict(x, y, flux, fluxerr, flags, terms)."""
    n = int(offsets[-1])
    out = dict(x=np.zeros(n), y=np.zeros(n), flux=np.zeros(n), fluxerr=np.zeros(n), flags=np.zeros(n, np.int32),
               terms=np.zeros((5, n)))
    for k, (ow, (img, rms, mask)) in enumerate(zip(ows, planes)):
        a, b = int(offsets[k]), int(offsets[k + 1])
        if a == b:
            continue
        idx = src_idx[a:b]
        if xy is None:
            x, y = ow.sky2pix(ra[idx], dec[idx])
            x, y = x - 1.0, y - 1.0
        else:
            x, y = xy[0][a:b], xy[1][a:b]
        f, e, fl, t = ar.aperture_sums(img, rms, mask, x, y, RADIUS, with_terms=True)
        out['x'][a:b], out['y'][a:b], out['flux'][a:b], out['fluxerr'][a:b], out['flags'][a:b] = x, y, f, e, fl
        out['terms'][:, a:b] = t
    return out
