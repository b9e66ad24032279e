"""numpy restatement of the extractor's second pass (csrc/extract_measure.hip; DESIGN.md "The wide table").

Test infrastructure, imported like ``extract_ref.py``.  The operator is a chosen convention; this file states it a
second time, independently of the HIP code, and ``test_measure_ref.py`` holds it against things that are not ours
(analytic Gaussians, the same scene on a finer grid).

``reverse=True`` evaluates every float64 sum in the opposite order.  Besides the values, every object carries what the
GPU tests derive their bounds from: the sums of absolute terms behind every quotient, the pixels nearest to a
threshold, the steps of the window's iteration.
"""
import numpy as np

from oracle import photometry as ophot

EPS = np.finfo(np.float64).eps
WIN_ITER, WIN_STEP2 = 16, 1e-8
FRAC_RTOL, FRAC_ATOL = 1e-10, 1e-9                  # the pin of the aperture overlap (tests/test_photometry_gpu.py)

INT_FIELDS = ['npix_auto', 'nskip_auto', 'flags_auto', 'flags_win', 'niter_win']
FLOAT_FIELDS = ['kron_radius', 'flux_auto', 'fluxerr_auto', 'mag_auto', 'magerr_auto', 'sigma_win', 'xwin_image',
                'ywin_image', 'x2win', 'y2win', 'xywin', 'errx2win', 'erry2win', 'errxywin', 'awin_image', 'bwin_image',
                'thetawin_image', 'errawin_image', 'errbwin_image', 'errthetawin_image', 'errx2', 'erry2', 'errxy']


def _sum(a, reverse):
    a = np.asarray(a, np.float64).ravel()
    return float(np.sum(a[::-1] if reverse else a))


def ellipse(x2, y2, xy, thin=True):
    """A, B, THETA (degrees) of second moments, as the extractor takes them (the 1/12 rule with ``thin``)."""
    if thin and x2 * y2 - xy * xy < 0.00694:
        x2, y2 = x2 + 1.0 / 12.0, y2 + 1.0 / 12.0
    pm, dm = 0.5 * (x2 + y2), 0.5 * (x2 - y2)
    rt = np.sqrt(dm * dm + xy * xy)
    return np.sqrt(pm + rt), np.sqrt(max(pm - rt, 0.0)), 0.5 * np.degrees(np.arctan2(2.0 * xy, x2 - y2))


def _clip(v, n):
    if not v > 0.0:
        return 0
    return n if v >= n else int(v)


def _r2(o, ii, jj):
    dx, dy = ii - o['xc'], jj - o['yc']
    return o['cxx'] * dx * dx + o['cyy'] * dy * dy + o['cxy'] * dx * dy


def kron(img, sigma, badmap, o, kron_fact=2.5, kron_min=3.5, reverse=False):
    """The *_AUTO values of one object ``o`` (dict: xc, yc 0-based, x2, y2, xy)."""
    ny, nx = img.shape
    D = o['x2'] * o['y2'] - o['xy'] ** 2
    o = dict(o, cxx=o['y2'] / D, cyy=o['x2'] / D, cxy=-2.0 * o['xy'] / D)
    sx, sy = np.sqrt(o['x2']), np.sqrt(o['y2'])
    i0, i1 = _clip(np.floor(o['xc'] - 6.0 * sx), nx), _clip(np.ceil(o['xc'] + 6.0 * sx) + 1.0, nx)
    j0, j1 = _clip(np.floor(o['yc'] - 6.0 * sy), ny), _clip(np.ceil(o['yc'] + 6.0 * sy) + 1.0, ny)
    out = dict(near=np.inf)
    s0 = s1 = 0.0
    if i0 < i1 and j0 < j1:
        jj, ii = np.mgrid[j0:j1, i0:i1].astype(np.float64)
        r2 = _r2(o, ii, jj)
        out['near'] = float(np.abs(r2 - 36.0).min() / 36.0)
        m = (r2 <= 36.0) & ~badmap[j0:j1, i0:i1]
        v = img[j0:j1, i0:i1].astype(np.float64)[m]
        t = np.sqrt(np.maximum(r2[m], 0.0)) * v
        s0, s1 = _sum(v, reverse), _sum(t, reverse)
        out['abs0'], out['abs1'] = float(np.abs(v).sum()), float(np.abs(t).sum())
    r1 = s1 / s0 if (s0 > 0.0 and s1 > 0.0) else 0.0
    R = max(kron_fact * r1, kron_min)
    out.update(r1=r1, s0=s0, s1=s1, kron_radius=R, kron_fact=kron_fact)
    hx, hy = R * sx, R * sy

    def lim(v, n):                                       # the device's clamp to [-1, n + 1] before the int conversion
        return int(min(max(v, -1.0), n + 1.0))
    i0, i1 = max(lim(np.floor(o['xc'] - hx), nx), 0), min(lim(np.ceil(o['xc'] + hx), nx) + 1, nx)
    j0, j1 = max(lim(np.floor(o['yc'] - hy), ny), 0), min(lim(np.ceil(o['yc'] + hy), ny) + 1, ny)
    flux = var = 0.0
    npix = nskip = 0
    if i0 < i1 and j0 < j1:
        jj, ii = np.mgrid[j0:j1, i0:i1].astype(np.float64)
        r2 = _r2(o, ii, jj)
        out['near'] = min(out['near'], float(np.abs(r2 - R * R).min() / (R * R)))
        inside = r2 <= R * R
        b = badmap[j0:j1, i0:i1]
        m = inside & ~b
        npix, nskip = int(m.sum()), int((inside & b).sum())
        v = img[j0:j1, i0:i1].astype(np.float64)[m]
        s = sigma[j0:j1, i0:i1].astype(np.float64)[m]
        flux, var = _sum(v, reverse), _sum(s * s, reverse)
        out['absflux'] = float(np.abs(v).sum())
    fl = 0
    if 10 * nskip > npix + nskip:
        fl |= 1
    if o['xc'] - hx < -0.5 or o['xc'] + hx > nx - 0.5 or o['yc'] - hy < -0.5 or o['yc'] + hy > ny - 0.5:
        fl |= 2
    if r1 == 0.0:
        fl |= 4
    err = np.sqrt(var)
    out.update(flux_auto=flux, fluxerr_auto=err, npix_auto=npix, nskip_auto=nskip, flags_auto=fl,
               share=nskip / max(npix + nskip, 1),
               mag_auto=-2.5 * np.log10(flux) if flux > 0.0 else 99.0,
               magerr_auto=1.0857362 * err / flux if flux > 0.0 else 99.0)
    return out


def _win_pass(img, sigma, badmap, cx, cy, r, tw, final, reverse, cterm=0.0):
    """The sums of one pass and, per sum, the bound on what another correct evaluation of the same terms may differ by:
    sum over the terms of (FRAC_RTOL |frac| + FRAC_ATOL + cterm EPS |frac|) g |v| |geometry|."""
    ny, nx = img.shape
    n = 7 if final else 3
    i0, i1, j0, j1 = ophot.bbox(cx, cy, r)
    i0, i1, j0, j1 = max(min(max(i0, -1), nx + 1), 0), min(min(max(i1, -1), nx + 1), nx), \
        max(min(max(j0, -1), ny + 1), 0), min(min(max(j1, -1), ny + 1), ny)
    if i0 >= i1 or j0 >= j1:
        return np.zeros(n), np.zeros(n)
    jj, ii = np.mgrid[j0:j1, i0:i1].astype(np.float64)
    good = ~badmap[j0:j1, i0:i1]
    dx, dy = ii - cx, jj - cy
    frac = ophot._signed(ii + 0.5 - cx, jj + 0.5 - cy, r) - ophot._signed(ii - 0.5 - cx, jj + 0.5 - cy, r) \
        - ophot._signed(ii + 0.5 - cx, jj - 0.5 - cy, r) + ophot._signed(ii - 0.5 - cx, jj - 0.5 - cy, r)
    g = np.exp(-((dx * dx + dy * dy) / tw))
    w = frac * g
    v = np.where(good, img[j0:j1, i0:i1], 0).astype(np.float64)
    wv = w * v
    dw = (FRAC_RTOL * np.abs(frac) + FRAC_ATOL + cterm * EPS * np.abs(frac)) * g          # |delta w|
    if not final:
        terms = [wv, wv * dx, wv * dy]
        dterms = [dw * np.abs(v), dw * np.abs(v * dx), dw * np.abs(v * dy)]
    else:
        s = np.where(good, sigma[j0:j1, i0:i1], 0).astype(np.float64)
        ws = w * w * (s * s)
        dws = 2.0 * np.abs(w) * dw * (s * s)
        terms = [wv, wv * dx * dx, wv * dy * dy, wv * dx * dy, ws * dx * dx, ws * dy * dy, ws * dx * dy]
        dterms = [dw * np.abs(v), dw * np.abs(v) * dx * dx, dw * np.abs(v) * dy * dy, dw * np.abs(v * dx * dy),
                  dws * dx * dx, dws * dy * dy, dws * np.abs(dx * dy)]
    return (np.array([_sum(t[good], reverse) for t in terms]), np.array([float(t[good].sum()) for t in dterms]))


def _moments(m):
    tv = m[0]
    return np.array([2.0 * m[1] / tv, 2.0 * m[2] / tv, 2.0 * m[3] / tv,
                     4.0 * m[4] / (tv * tv), 4.0 * m[5] / (tv * tv), 4.0 * m[6] / (tv * tv)])


def window(img, sigma, badmap, o, reverse=False, cterm=0.0):
    """The windowed values of one object ``o`` (dict: xc, yc, x2, y2, xy, fwhm, a, b, theta, and errx2 / erry2 / errxy
    for the fallback).  Among the diagnostics: ``steps`` (length of every step), ``dstep`` (bound on a step's error per
    iteration), ``rho`` (the contraction factor), ``dcentre`` (bound on the final centre), ``dmom`` (bounds on the six
    moments)."""
    sw = o['fwhm'] / 2.35482 if o['fwhm'] > 0.0 else np.sqrt((o['x2'] + o['y2']) / 2.0)
    r, tw = 4.0 * sw, 2.0 * sw * sw
    cx, cy = o['xc'], o['yc']
    flags = 0 if (sw > 0.0 and r < 1e9) else 1
    niter, conv, steps, dstep, centres = 0, False, [], 0.0, []
    for it in range(WIN_ITER):
        if flags or conv:
            break
        s, d = _win_pass(img, sigma, badmap, cx, cy, r, tw, False, reverse, cterm)
        niter = it + 1
        if not s[0] > 0.0:
            flags |= 1
            break
        centres.append((cx, cy))
        stx, sty = 2.0 * s[1] / s[0], 2.0 * s[2] / s[0]
        # |delta step| <= 2 (|delta mx| + |mx / tv| |delta tv|) / tv, likewise y; the length of both
        dstep = max(dstep, 2.0 * np.hypot(d[1] + abs(s[1] / s[0]) * d[0], d[2] + abs(s[2] / s[0]) * d[0]) / s[0])
        cx, cy = cx + stx, cy + sty
        steps.append(stx * stx + sty * sty)
        conv = steps[-1] < WIN_STEP2
    if flags == 0 and not conv:
        flags |= 2
    out = dict(sigma_win=sw, niter_win=niter, steps=np.sqrt(steps))
    mom = None
    if not flags & 1:
        m, d = _win_pass(img, sigma, badmap, cx, cy, r, tw, True, reverse, cterm)
        if not m[0] > 0.0:
            flags |= 1
        else:
            mom = _moments(m)
            # contraction: the largest ratio of successive step lengths (0 with fewer than two steps).  What one pass
            # gets wrong, the passes behind it shrink (or stretch) by at most rho each: after niter passes the centre is
            # off by at most dstep (1 + rho + ... + rho^(niter - 1)), which is below dstep / (1 - rho) where rho < 1
            # and stays finite where an object's steps grew on the way or the cap of 16 passes ended the walk
            st = out['steps']
            rho = float(np.max(st[1:] / st[:-1])) if len(st) > 1 and (st[:-1] > 0).all() else 0.0
            out['rho'] = rho
            dc = dstep * float(np.sum(rho ** np.arange(niter)))
            if rho >= 0.9 or flags & 2:
                # the step ratio says little here (steps that grew on the way, a walk the cap ended).  Then the
                # object's own sensitivity: J_k, the Jacobian of one pass c -> c + step(c) at the k-th centre (finite
                # differences of 1e-5 px), carries an error on; what pass k gets wrong (at most dstep) arrives at the
                # end as J_(n-1) ... J_(k+1) times it: dc = dstep sum_k || J_(n-1) ... J_(k+1) ||_2
                def once(x, y):
                    q, _ = _win_pass(img, sigma, badmap, x, y, r, tw, False, reverse)
                    return np.array([x + 2.0 * q[1] / q[0], y + 2.0 * q[2] / q[0]])
                h, jac = 1e-5, []
                for x, y in centres:
                    f0 = once(x, y)
                    jac.append(np.column_stack([(once(x + h, y) - f0) / h, (once(x, y + h) - f0) / h]))
                prod, total = np.eye(2), 1.0
                for k in range(len(jac) - 1, 0, -1):
                    prod = prod @ jac[k]
                    total += float(np.linalg.norm(prod, 2))
                dc = dstep * total
            out['dcentre'] = dc
            # the moments: their own sums' bounds, and what moving the centre by dc along either axis does to them
            tv = m[0]
            dsum = np.array([2.0 * (d[q] + abs(m[q] / tv) * d[0]) / tv for q in (1, 2, 3)] +
                            [4.0 * (d[q] + 2.0 * abs(m[q] / tv) * d[0]) / (tv * tv) for q in (4, 5, 6)])
            if np.isfinite(dc):
                for ex, ey in ((dc, 0.0), (0.0, dc)):
                    m2, _ = _win_pass(img, sigma, badmap, cx + ex, cy + ey, r, tw, True, reverse, cterm)
                    dsum = dsum + np.abs(_moments(m2) - mom)
            out['dmom'] = dsum
    if flags & 1:
        out.update(xwin_image=o['xc'] + 1.0, ywin_image=o['yc'] + 1.0, x2win=o['x2'], y2win=o['y2'], xywin=o['xy'],
                   errx2win=o.get('errx2', np.nan), erry2win=o.get('erry2', np.nan), errxywin=o.get('errxy', np.nan),
                   awin_image=o['a'], bwin_image=o['b'], thetawin_image=o['theta'])
    else:
        a, b, th = ellipse(mom[0], mom[1], mom[2])
        out.update(xwin_image=cx + 1.0, ywin_image=cy + 1.0, x2win=mom[0], y2win=mom[1], xywin=mom[2],
                   errx2win=mom[3], erry2win=mom[4], errxywin=mom[5], awin_image=a, bwin_image=b, thetawin_image=th)
    ea, eb, eth = ellipse(out['errx2win'], out['erry2win'], out['errxywin'])
    out.update(errawin_image=ea, errbwin_image=eb, errthetawin_image=eth, flags_win=flags)
    return out


def objects_of(base, reverse=False):
    """The rows the second pass starts from, out of ``extract_ref.extract``'s result: barycentre, moments (1/12 rule
    applied) and the isophotal error moments errx2 = sum sigma^2 dx^2 / (sum f)^2 over the members."""
    seg, filt, tab = base['segm'], base['filtered'], base['table']
    sigma = base['sigma']
    ny, nx = seg.shape
    flat = seg.ravel()
    members = np.flatnonzero(flat)
    members = members[np.argsort(flat[members], kind='stable')]
    bounds = np.searchsorted(flat[members], np.arange(1, len(tab) + 2))
    out = []
    for k in range(len(tab)):
        p = members[bounds[k]:bounds[k + 1]]
        y, x = np.divmod(p, nx)
        xmin, ymin = x.min(), y.min()
        v = filt.ravel()[p].astype(np.float64)
        dx, dy = (x - xmin).astype(np.float64), (y - ymin).astype(np.float64)
        S = _sum(v, reverse)
        xb, yb = _sum(v * dx, reverse) / S, _sum(v * dy, reverse) / S
        x2 = _sum(v * dx * dx, reverse) / S - xb * xb
        y2 = _sum(v * dy * dy, reverse) / S - yb * yb
        xy = _sum(v * dx * dy, reverse) / S - xb * yb
        if x2 * y2 - xy * xy < 0.00694:
            x2, y2 = x2 + 1.0 / 12.0, y2 + 1.0 / 12.0
        xc, yc = xmin + xb + 1.0 - 1.0, ymin + yb + 1.0 - 1.0          # X_IMAGE - 1, as the device takes it
        s2 = sigma.ravel()[p].astype(np.float64) ** 2
        # sums over offsets from the box's corner (exact in any order for all but very large objects), then the shift
        ub, vb = xc - xmin, yc - ymin
        m0, mx, my = _sum(s2, reverse), _sum(s2 * dx, reverse), _sum(s2 * dy, reverse)
        mxx, myy, mxy = _sum(s2 * dx * dx, reverse), _sum(s2 * dy * dy, reverse), _sum(s2 * dx * dy, reverse)
        a, b, th = ellipse(x2, y2, xy, thin=False)
        out.append(dict(number=k + 1, xc=xc, yc=yc, x2=x2, y2=y2, xy=xy, fwhm=float(tab['FWHM_IMAGE'][k]), a=a, b=b, theta=th,
                        errx2=(mxx - 2.0 * ub * mx + ub * ub * m0) / (S * S),
                        erry2=(myy - 2.0 * vb * my + vb * vb * m0) / (S * S),
                        errxy=(mxy - ub * my - vb * mx + ub * vb * m0) / (S * S)))
    return out


def measure(base, kron_fact=2.5, kron_min=3.5, reverse=False, cterm=0.0):
    """Every object of ``extract_ref.extract``'s result ``base`` (with ``base['sigma']`` and ``base['img']`` added by the
    caller): list of dicts with INT_FIELDS, FLOAT_FIELDS and the diagnostics of ``kron`` / ``window``."""
    img, sigma, badmap = base['img'], base['sigma'], base['bad']
    rows = []
    for o in objects_of(base, reverse):
        r = dict(o)
        r.update(kron(img, sigma, badmap, o, kron_fact, kron_min, reverse))
        r.update(window(img, sigma, badmap, o, reverse, cterm))
        rows.append(r)
    return rows


def world(wcs, x_image, y_image, errx2, erry2, errxy):
    """ERRA_WORLD, ERRB_WORLD, ERRTHETA_WORLD: J C J^T with J by central differences of +-0.5 px, degrees, RA times
    cos(dec).  ``wcs``: an object with all_pix2world(x, y, 1)."""
    ra1, de1 = wcs.all_pix2world(x_image + 0.5, y_image, 1)
    ra2, de2 = wcs.all_pix2world(x_image - 0.5, y_image, 1)
    ra3, de3 = wcs.all_pix2world(x_image, y_image + 0.5, 1)
    ra4, de4 = wcs.all_pix2world(x_image, y_image - 0.5, 1)
    wrap = lambda d: (d + 180.0) % 360.0 - 180.0                        # noqa: E731
    cd = np.cos(np.radians(0.5 * (de1 + de2)))
    J = np.array([[wrap(ra1 - ra2) * cd, wrap(ra3 - ra4) * cd], [de1 - de2, de3 - de4]])
    W = J @ np.array([[errx2, errxy], [errxy, erry2]]) @ J.T
    return ellipse(W[0, 0], W[1, 1], W[0, 1], thin=False)
