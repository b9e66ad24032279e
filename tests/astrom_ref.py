"""The astrometric refit ("Astrometric refit") restated in float64 numpy, independently of
csrc/astrometry.hip:

* star positions in the tangent plane by the textbook trigonometric form of the gnomonic projection, not by dot products
  with the frame's axes;
* the vote as a dense histogram of every (star, detection) pair (``np.add.at``);
* cross-identification by brute force with the haversine formula (``assoc_ref.separation``);
* the fit by ``numpy.linalg.lstsq`` (SVD) on the weighted design matrix, one axis at a time, each in its own basis - not
  normal equations, and not one matrix for both axes.

Decisions that hang on a comparison of reals can differ between two correct implementations when the two sides are
nearly equal.  The restatement records how near they came: ``min_radius_margin`` (any separation against the cross-id
radius), ``min_clip_margin`` (any chi2 against the clip bound) and ``min_vote_margin`` (any pair's offset against the
edges of its bin and of the window), each relative and over all rounds.  A test compares discrete results exactly only
on scenes whose margins it has asserted."""
import numpy as np

from assoc_ref import separation
from oracle.wcs import NPV, WCS

STATUS = ('OK', 'TOO_FEW', 'AMBIGUOUS', 'SINGULAR', 'NOT_CONVERGED')
OK, TOO_FEW, AMBIGUOUS, SINGULAR, NOT_CONVERGED = range(5)
DEFAULTS = dict(position_maxerr=60.0, match_resol=0.0, crossid_radius=2.0, clip_nsigma=3.0, degree=3, match=1,
                match_nmax=1024, max_rounds=8, max_clip=10)
TPV_INDEX = (0, 1, 2, 4, 5, 6, 7, 8, 9, 10)
EXPONENTS = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3))
NCOEF = {1: 3, 2: 6, 3: 10}


def gnomonic(ra, dec, ra0, dec0):
    """(xi, eta) in degrees and ``front`` (the point lies before the tangent plane)."""
    a, d = np.radians(np.asarray(ra, np.float64)), np.radians(np.asarray(dec, np.float64))
    a0, d0 = np.radians(ra0), np.radians(dec0)
    with np.errstate(invalid='ignore', divide='ignore'):
        cosc = np.sin(d0) * np.sin(d) + np.cos(d0) * np.cos(d) * np.cos(a - a0)
        xi = np.cos(d) * np.sin(a - a0) / cosc
        eta = (np.cos(d0) * np.sin(d) - np.sin(d0) * np.cos(d) * np.cos(a - a0)) / cosc
    return np.degrees(xi), np.degrees(eta), np.isfinite(cosc) & (cosc > 0.0)


def as_tpv(w):
    """A copy of ``w`` in TPV form (a TAN header gets the identity polynomial)."""
    return WCS(w.crpix, w.crval, w.cd, w.pv1.copy(), w.pv2.copy(), w.naxis)


def scale_of(w):
    nx, ny = w.naxis
    xs = np.array([0.5, 0.5, nx + 0.5, nx + 0.5]) - w.crpix[0]
    ys = np.array([0.5, ny + 0.5, 0.5, ny + 0.5]) - w.crpix[1]
    u = w.cd[0, 0] * xs + w.cd[0, 1] * ys
    v = w.cd[1, 0] * xs + w.cd[1, 1] * ys
    return float(max(np.abs(u).max(), np.abs(v).max()))


def _rel(a, b):
    return np.abs(a - b) / b


def vote(w, x, y, snr, ok, ref_ra, ref_dec, P, q, nmax, margins):
    """(peak, runner_up, shift_xi, shift_eta) of stage 1."""
    rows = np.flatnonzero(ok)
    rows = rows[np.argsort(-snr[rows], kind='stable')][:nmax]          # ties: the lowest row
    nb = int(np.floor(2.0 * P / q + 0.5)) + 1
    hist = np.zeros((nb, nb), np.int64)
    if rows.size and ref_ra.size:
        dxi, deta = w.pix2plane(x[rows], y[rows])
        sxi, seta, front = gnomonic(ref_ra, ref_dec, w.crval[0], w.crval[1])
        sxi, seta = sxi[front] * 3600.0, seta[front] * 3600.0
        dx = sxi[None, :] - (dxi * 3600.0)[:, None]
        dy = seta[None, :] - (deta * 3600.0)[:, None]
        near = (np.abs(dx) <= 1.5 * P) & (np.abs(dy) <= 1.5 * P)
        if near.any():
            margins['vote'] = min(margins['vote'], float(np.min(_rel(np.abs(dx[near]), P))), float(np.min(_rel(np.abs(dy[near]), P))))
        take = (np.abs(dx) <= P) & (np.abs(dy) <= P)
        fx, fy = (dx[take] + P) / q + 0.5, (dy[take] + P) / q + 0.5
        if fx.size:
            edge = min(np.min(np.abs(fx - np.round(fx))), np.min(np.abs(fy - np.round(fy))))
            margins['vote'] = min(margins['vote'], float(edge))
        np.add.at(hist, (np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)), 1)
    pad = np.pad(hist, 1)
    S = sum(pad[1 + dr:1 + dr + nb, 1 + dc:1 + dc + nb] for dr in (-1, 0, 1) for dc in (-1, 0, 1))
    k = int(np.argmax(S))                                               # the first of equals in (row, column) order
    pr, pc = divmod(k, nb)
    peak = int(S[pr, pc])
    out = S.copy()
    out[max(pr - 2, 0):pr + 3, max(pc - 2, 0):pc + 3] = 0
    runner = int(out.max())
    sx = sy = 0
    for r in range(max(pr - 1, 0), min(pr + 2, nb)):
        for c in range(max(pc - 1, 0), min(pc + 2, nb)):
            sx += int(hist[r, c]) * c
            sy += int(hist[r, c]) * r
    if peak == 0:
        return 0, runner, 0.0, 0.0
    return peak, runner, float(sx) * q / float(peak) - P, float(sy) * q / float(peak) - P


def design(a, b, ncoef):
    return np.stack([a ** p * b ** r for p, r in EXPONENTS[:ncoef]], axis=1)


def solve_frame(w0, x, y, sd, snr, ref_ra, ref_dec, ref_sig, **kw):
    """One frame.  Returns a dict: ``wcs`` (oracle WCS), ``status``, ``shift``, ``vote_peak``, ``vote_runner_up``,
    ``nmatch``, ``nused``, ``rounds``, ``rms``, ``chi2``, ``match`` (int32), ``used`` (uint8), ``returned`` (how often a row that
    a fit had rejected was taken back by the next) and the three margins."""
    p = dict(DEFAULTS, **kw)
    x, y, sd, snr = (np.asarray(v, np.float64) for v in (x, y, sd, snr))
    ref_ra, ref_dec, ref_sig = (np.asarray(v, np.float64) for v in (ref_ra, ref_dec, ref_sig))
    n, ncoef = x.size, NCOEF[p['degree']]
    P, R = float(p['position_maxerr']), float(p['crossid_radius'])
    q = float(p['match_resol']) or R / 2.0
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(sd) & np.isfinite(snr)
    margins = dict(vote=np.inf, radius=np.inf, clip=np.inf)
    w = as_tpv(w0)
    res = dict(wcs=w0, status=NOT_CONVERGED, shift=(0.0, 0.0), vote_peak=0, vote_runner_up=0, nmatch=0, nused=0, rounds=0,
               rms=(0.0, 0.0), chi2=0.0, match=np.full(n, -1, np.int32), used=np.zeros(n, np.uint8), returned=0)

    def done(**more):
        res.update(more)
        res.update(min_vote_margin=margins['vote'], min_radius_margin=margins['radius'], min_clip_margin=margins['clip'])
        return res

    if p['match']:
        peak, runner, sx, sy = vote(w, x, y, snr, ok, ref_ra, ref_dec, P, q, int(p['match_nmax']), margins)
        res.update(vote_peak=peak, vote_runner_up=runner)
        if peak < 2 * ncoef or runner * 2 >= peak:
            return done(status=AMBIGUOUS)
        res['shift'] = (sx, sy)
        w.pv1[0] += sx / 3600.0
        w.pv2[0] += sy / 3600.0

    s = scale_of(w)
    pixscale = 3600.0 * np.sqrt(abs(np.linalg.det(w.cd)))
    dx, dy = x - w.crpix[0], y - w.crpix[1]
    with np.errstate(invalid='ignore'):
        a = (w.cd[0, 0] * dx + w.cd[0, 1] * dy) / s
        b = (w.cd[1, 0] * dx + w.cd[1, 1] * dy) / s
    sxi, seta, _ = gnomonic(ref_ra, ref_dec, w.crval[0], w.crval[1])
    rows = np.flatnonzero(ok)
    prev = None
    for rnd in range(1, int(p['max_rounds']) + 1):
        match = np.full(n, -1, np.int32)
        if rows.size and ref_ra.size:
            ra, dec = w.pix2sky(x[rows], y[rows])
            sep = separation(ra, dec, ref_ra, ref_dec)
            fin = np.isfinite(sep)
            if fin.any():
                margins['radius'] = min(margins['radius'], float(np.min(_rel(sep[fin], R))))
            sep = np.where(fin & (sep <= R), sep, np.inf)
            j = np.argmin(sep, axis=1)                                   # the first of equals
            hit = np.isfinite(sep[np.arange(rows.size), j])
            match[rows[hit]] = j[hit]
        m = match >= 0
        jm = np.where(m, match, 0)
        wt = np.where(m, 1.0 / ((sd * pixscale) ** 2 + ref_sig[jm] ** 2), 0.0) if ref_sig.size else np.zeros(n)
        tx, ty = (sxi[jm], seta[jm]) if ref_sig.size else (np.zeros(n), np.zeros(n))
        keep = m.copy()
        status, fits = OK, 0
        c1 = c2 = None
        while True:
            nk = int(keep.sum())
            if nk < 2 * ncoef:
                status = TOO_FEW
                break
            sw = np.sqrt(wt[keep])
            A1, A2 = design(a[keep], b[keep], ncoef), design(b[keep], a[keep], ncoef)
            c1, _, r1, _ = np.linalg.lstsq(A1 * sw[:, None], tx[keep] * sw, rcond=None)
            c2, _, r2, _ = np.linalg.lstsq(A2 * sw[:, None], ty[keep] * sw, rcond=None)
            if r1 < ncoef or r2 < ncoef:
                status = SINGULAR
                break
            fits += 1
            e1 = 3600.0 * (design(a, b, ncoef) @ c1 - tx)
            e2 = 3600.0 * (design(b, a, ncoef) @ c2 - ty)
            chi = wt * (e1 * e1 + e2 * e2)
            chi2 = float(chi[keep].sum())
            rms = (float(np.sqrt(np.mean(e1[keep] ** 2))), float(np.sqrt(np.mean(e2[keep] ** 2))))
            if fits >= int(p['max_clip']):
                break
            bound = 2.0 * float(p['clip_nsigma']) ** 2 * max(1.0, chi2 / (2.0 * (nk - ncoef)))
            margins['clip'] = min(margins['clip'], float(np.min(_rel(chi[m], bound))))
            new = m & (chi <= bound)
            if np.array_equal(new, keep):
                break
            res['returned'] += int((new & ~keep).sum())               # rows rejected by an earlier fit that are back
            keep = new
        res.update(match=match, used=keep.astype(np.uint8), nmatch=int(m.sum()), nused=int(keep.sum()), rounds=rnd)
        if status != OK:
            return done(status=status, wcs=w0, rms=(0.0, 0.0), chi2=0.0)
        pv1, pv2 = np.zeros(NPV), np.zeros(NPV)
        for k in range(ncoef):
            deg = sum(EXPONENTS[k])
            pv1[TPV_INDEX[k]] = c1[k] / s ** deg
            pv2[TPV_INDEX[k]] = c2[k] / s ** deg
        w = WCS(w.crpix, w.crval, w.cd, pv1, pv2, w.naxis)
        res.update(wcs=w, rms=rms, chi2=chi2)
        state = (match.tobytes(), keep.tobytes())
        if prev is not None and state == prev:
            return done(status=OK)
        prev = state
    return done(status=NOT_CONVERGED)


def solve(wcs_list, detections, ref, **kw):
    """Every frame of a call: ``detections`` is a list of (x, y, sd, snr), ``ref`` is (ra, dec, sig)."""
    return [solve_frame(w, *d, *ref, **kw) for w, d in zip(wcs_list, detections)]


def grid_separation(wa, wb, n=9):
    """Largest sky separation (arcsec) between two headers on an n x n grid of pixels over NAXIS."""
    gx, gy = np.meshgrid(np.linspace(1.0, wa.naxis[0], n), np.linspace(1.0, wa.naxis[1], n))
    ra1, de1 = wa.pix2sky(gx.ravel(), gy.ravel())
    ra2, de2 = wb.pix2sky(gx.ravel(), gy.ravel())
    a = separation(ra1, de1, ra2, de2)
    return float(np.max(np.diagonal(a)))


# ---- scenes -----------------------------------------------------------------------------------------------------------
def tan_header(crval=(150.0, 20.0), naxis=(512, 512), scale=1.0, angle=0.0, crpix=None):
    """A TAN header with ``scale`` arcsec pixels, east to the left, rotated by ``angle`` degrees."""
    t = np.radians(angle)
    cd = (scale / 3600.0) * np.array([[-np.cos(t), np.sin(t)], [np.sin(t), np.cos(t)]])
    if crpix is None:
        crpix = ((naxis[0] + 1) / 2.0, (naxis[1] + 1) / 2.0)
    return WCS(crpix, crval, cd, naxis=naxis)


def tpv_truth(w, seed, amplitude=2e-2):
    """``w`` with a random degree-3 distortion: terms of degree d change the edge of the field by about
    ``amplitude`` pixels."""
    rng = np.random.default_rng(seed)
    s = scale_of(w)
    px = abs(np.linalg.det(w.cd)) ** 0.5
    pv1, pv2 = np.zeros(NPV), np.zeros(NPV)
    pv1[1] = pv2[1] = 1.0
    for k in range(3, 10):
        deg = sum(EXPONENTS[k])
        pv1[TPV_INDEX[k]] = rng.uniform(-1, 1) * amplitude * px / s ** deg
        pv2[TPV_INDEX[k]] = rng.uniform(-1, 1) * amplitude * px / s ** deg
    return WCS(w.crpix, w.crval, w.cd, pv1, pv2, w.naxis)


def perturbed(w, dpix=(0.0, 0.0), angle=0.0, scale=1.0, keep_pv=False):
    """The header an observer would have: CRPIX off by ``dpix``, CD turned by ``angle`` degrees and stretched."""
    t = np.radians(angle)
    rot = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    return WCS(w.crpix + np.asarray(dpix), w.crval, scale * (rot @ w.cd), w.pv1 if keep_pv and w.has_pv else None,
               w.pv2 if keep_pv and w.has_pv else None, w.naxis)


def scene(truth, nstars, seed, nspurious=0, nunrelated=0, noutliers=0, outlier_px=1.0, sd=0.05, sig=0.01, margin=8.0,
          min_sep=12.0):
    """Stars planted through ``truth``: returns (x, y, sd, snr), (ra, dec, sig) and the rows of the outliers.  Stars
    keep ``min_sep`` pixels from each other so that no detection has two candidates; ``nspurious`` detections have
    no star, ``nunrelated`` stars no detection, ``noutliers`` detections are moved by ``outlier_px`` pixels."""
    rng = np.random.default_rng(seed)
    nx, ny = truth.naxis
    pts = []
    while len(pts) < nstars + nspurious + nunrelated:
        c = np.array([rng.uniform(margin, nx - margin), rng.uniform(margin, ny - margin)])
        if all(np.hypot(*(c - o)) >= min_sep for o in pts):
            pts.append(c)
    pts = np.array(pts).reshape(-1, 2)
    stars, spur, unrel = pts[:nstars], pts[nstars:nstars + nspurious], pts[nstars + nspurious:]
    x = np.concatenate([stars[:, 0], spur[:, 0]])
    y = np.concatenate([stars[:, 1], spur[:, 1]])
    sky = np.concatenate([stars, unrel])
    ra, dec = truth.pix2sky(sky[:, 0], sky[:, 1])
    out = rng.choice(nstars, noutliers, replace=False) if noutliers else np.zeros(0, np.int64)
    ang = rng.uniform(0, 2 * np.pi, noutliers)
    x[out] += outlier_px * np.cos(ang)
    y[out] += outlier_px * np.sin(ang)
    p = rng.permutation(x.size)
    inv = np.empty_like(p)
    inv[p] = np.arange(p.size)
    snr = rng.uniform(10.0, 500.0, x.size)
    return (x[p], y[p], np.full(x.size, sd), snr[p]), (ra, dec, np.full(ra.size, sig)), np.sort(inv[out])
