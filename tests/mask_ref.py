"""numpy restatement of the masked second pass (csrc/extract_mask.hip; DESIGN.md "MASK_TYPE").

Test infrastructure, imported like ``measure_ref.py``, whose sums, boxes and bounds it uses unchanged.  For one object and
one centre the replacement step is a map of the whole frame: ``planes`` gives the value and the sigma every pixel
contributes (its own, or its mirror's) and the pixels that contribute nothing.  The Kron and windowed measurements are
then ``measure_ref``'s on those planes with the lost pixels in the place of the bad ones (position-dependent weights are
taken at the pixel itself, which is exactly what a replaced *plane* under unchanged weights says), in the same row-major
element order, with the same ``reverse`` switch.  The aperture is stated here.

Objects are dicts as ``measure_ref.objects_of`` makes them (number, xc, yc 0-based, x2, y2, xy, fwhm, a, b, theta and, for
the window's fallback, errx2 / erry2 / errxy); the segmentation map comes from the caller.
"""
import numpy as np

import measure_ref as mr
from measure_ref import EPS, FRAC_ATOL, FRAC_RTOL, WIN_ITER, WIN_STEP2, _clip, _moments, _r2, _sum, ellipse  # noqa: F401
from oracle import photometry as ophot

BLANK, CORRECT = 'blank', 'correct'
USE, REPL, LOST = 0, 1, 2
AUTO_CROWDED = 8

INT_FIELDS = mr.INT_FIELDS
FLOAT_FIELDS = [f for f in mr.FLOAT_FIELDS if f not in ('errx2', 'erry2', 'errxy')]      # (walk 3 is not restated here)
MASK_INT_FIELDS = ['nrepl_auto', 'nlost_auto', 'nap', 'nrepl_aper', 'nlost_aper', 'nrepl_win', 'nlost_win', 'crowded']
MASK_FLOAT_FIELDS = ['flux_aper', 'fluxerr_aper']


def badmap(img, sigma, bad=None):
    """The extractor's rule (mx_isbad): bad byte, non-finite img or sigma, sigma <= 0."""
    b = ~np.isfinite(img) | ~np.isfinite(sigma) | ~(np.nan_to_num(sigma, nan=0.0) > 0)
    return b if bad is None else b | (np.asarray(bad) != 0)


def unusable(bmap, seg, number):
    return bmap | ((seg != 0) & (seg != number))


def planes(img, sigma, bmap, seg, number, cx, cy, mask_type):
    """(value plane, sigma plane, lost map, how map) of object ``number`` with the replacement about (cx, cy)."""
    ny, nx = img.shape
    un = unusable(bmap, seg, number)
    how = np.where(un, LOST, USE).astype(np.int8)
    v, s = img.copy(), sigma.copy()
    if mask_type == CORRECT:
        jj, ii = np.nonzero(un)
        with np.errstate(invalid='ignore'):
            mi, mj = np.floor((2.0 * cx - ii) + 0.5), np.floor((2.0 * cy - jj) + 0.5)
        ok = np.isfinite(mi) & np.isfinite(mj)
        mi = np.clip(np.where(ok, mi, -1.0), -1.0, nx + 1.0).astype(np.int64)          # mx_int
        mj = np.clip(np.where(ok, mj, -1.0), -1.0, ny + 1.0).astype(np.int64)
        ok &= (mi >= 0) & (mi < nx) & (mj >= 0) & (mj < ny)
        ok[ok] = ~un[mj[ok], mi[ok]]
        v[jj[ok], ii[ok]] = img[mj[ok], mi[ok]]
        s[jj[ok], ii[ok]] = sigma[mj[ok], mi[ok]]
        how[jj[ok], ii[ok]] = REPL
    elif mask_type != BLANK:
        raise ValueError(mask_type)
    return v, s, how == LOST, how


def half_distance(c):
    """How far 2 c - i is from a half-integer (where the mirror's rounding flips), the same for every integer i."""
    return abs((2.0 * c) % 1.0 - 0.5)


def _lim(v, n):
    return int(min(max(v, -1.0), n + 1.0))


def kron(img, sigma, bmap, seg, o, mask_type, kron_fact=2.5, kron_min=3.5, reverse=False):
    ny, nx = img.shape
    v, s, lost, how = planes(img, sigma, bmap, seg, o['number'], o['xc'], o['yc'], mask_type)
    out = mr.kron(v, s, lost, o, kron_fact, kron_min, reverse)
    # the pixels of the Kron ellipse again, for the replaced ones (measure_ref.kron counts summed and lost ones)
    D = o['x2'] * o['y2'] - o['xy'] ** 2
    oo = dict(o, cxx=o['y2'] / D, cyy=o['x2'] / D, cxy=-2.0 * o['xy'] / D)
    R = out['kron_radius']
    hx, hy = R * np.sqrt(o['x2']), R * np.sqrt(o['y2'])
    i0, i1 = max(_lim(np.floor(o['xc'] - hx), nx), 0), min(_lim(np.ceil(o['xc'] + hx), nx) + 1, nx)
    j0, j1 = max(_lim(np.floor(o['yc'] - hy), ny), 0), min(_lim(np.ceil(o['yc'] + hy), ny) + 1, ny)
    nrepl = nlost = 0
    if i0 < i1 and j0 < j1:
        jj, ii = np.mgrid[j0:j1, i0:i1].astype(np.float64)
        inside = _r2(oo, ii, jj) <= R * R
        nrepl = int((inside & (how[j0:j1, i0:i1] == REPL)).sum())
        nlost = int((inside & (how[j0:j1, i0:i1] == LOST)).sum())
    assert nlost == out['nskip_auto']
    # ... and of the search ellipse r2 <= 36 (the sums behind the radius), which may reach further
    sx, sy = np.sqrt(o['x2']), np.sqrt(o['y2'])
    i0, i1 = _clip(np.floor(o['xc'] - 6.0 * sx), nx), _clip(np.ceil(o['xc'] + 6.0 * sx) + 1.0, nx)
    j0, j1 = _clip(np.floor(o['yc'] - 6.0 * sy), ny), _clip(np.ceil(o['yc'] + 6.0 * sy) + 1.0, ny)
    touched = nrepl + nlost
    if i0 < i1 and j0 < j1:
        jj, ii = np.mgrid[j0:j1, i0:i1].astype(np.float64)
        touched += int(((_r2(oo, ii, jj) <= 36.0) & (how[j0:j1, i0:i1] != USE)).sum())
    out['touched_auto'] = touched
    npix = out['npix_auto']
    if 10 * (nrepl + nlost) > npix + nlost:
        out['flags_auto'] |= AUTO_CROWDED
    out.update(nrepl_auto=nrepl, nlost_auto=nlost, share_crowd_auto=(nrepl + nlost) / max(npix + nlost, 1),
               half=min(half_distance(o['xc']), half_distance(o['yc'])))
    return out


def _overlap(cx, cy, r, nx, ny):
    """(i0, i1, j0, j1, frac) of the clipped box of the circle: the box rule and the overlap of measure_ref._win_pass."""
    i0, i1, j0, j1 = ophot.bbox(cx, cy, r)
    i0, i1, j0, j1 = max(min(max(i0, -1), nx + 1), 0), min(min(max(i1, -1), nx + 1), nx), \
        max(min(max(j0, -1), ny + 1), 0), min(min(max(j1, -1), ny + 1), ny)
    if i0 >= i1 or j0 >= j1:
        return i0, i0, j0, j0, np.zeros((0, 0))
    jj, ii = np.mgrid[j0:j1, i0:i1].astype(np.float64)
    frac = ophot._signed(ii + 0.5 - cx, jj + 0.5 - cy, r) - ophot._signed(ii - 0.5 - cx, jj + 0.5 - cy, r) \
        - ophot._signed(ii + 0.5 - cx, jj - 0.5 - cy, r) + ophot._signed(ii - 0.5 - cx, jj - 0.5 - cy, r)
    return i0, i1, j0, j1, frac


def _reaches(cx, cy, r, i0, i1, j0, j1):
    """("frac > 0" as the device decides it, how near the decision comes to a tie): the pixel's square reaches inside the
    circle, i.e. the point of the square nearest to the centre lies inside the radius.  The computed overlap of a pixel
    outside the circle is a rounding residue of either sign; the distance of the nearest pixel's point from the circle,
    in pixels, is what the census asks about."""
    if i0 >= i1 or j0 >= j1:
        return np.zeros((0, 0), bool), np.inf
    jj, ii = np.mgrid[j0:j1, i0:i1].astype(np.float64)
    ax, ay = np.maximum(np.abs(ii - cx) - 0.5, 0.0), np.maximum(np.abs(jj - cy) - 0.5, 0.0)
    d2 = ax * ax + ay * ay
    return d2 < r * r, float(np.abs(np.sqrt(d2) - r).min())


def window(img, sigma, bmap, seg, o, mask_type, reverse=False, cterm=0.0):
    """measure_ref.window with every pass on the planes replaced about that pass's centre; the same diagnostics, and
    ``half``: the smallest half_distance over every centre a pass used."""
    ny, nx = img.shape
    sw = o['fwhm'] / 2.35482 if o['fwhm'] > 0.0 else np.sqrt((o['x2'] + o['y2']) / 2.0)
    r, tw = 4.0 * sw, 2.0 * sw * sw
    cx, cy = o['xc'], o['yc']
    half, touched = [np.inf], [0]

    def one(x, y, final, ct=cterm):
        half[0] = min(half[0], half_distance(x), half_distance(y))
        v, s, lost, how = planes(img, sigma, bmap, seg, o['number'], x, y, mask_type)
        i0, i1, j0, j1 = _overlap(x, y, r, nx, ny)[:4]
        touched[0] += int((how[j0:j1, i0:i1] != USE).sum())              # (anywhere in the pass's clipped box)
        return mr._win_pass(v, s, lost, x, y, r, tw, final, reverse, ct)

    flags = 0 if (sw > 0.0 and r < 1e9) else 1
    niter, conv, steps, dstep, centres = 0, False, [], 0.0, []
    for it in range(WIN_ITER):
        if flags or conv:
            break
        s, d = one(cx, cy, False)
        niter = it + 1
        if not s[0] > 0.0:
            flags |= 1
            break
        centres.append((cx, cy))
        stx, sty = 2.0 * s[1] / s[0], 2.0 * s[2] / s[0]
        dstep = max(dstep, 2.0 * np.hypot(d[1] + abs(s[1] / s[0]) * d[0], d[2] + abs(s[2] / s[0]) * d[0]) / s[0])
        cx, cy = cx + stx, cy + sty
        steps.append(stx * stx + sty * sty)
        conv = steps[-1] < WIN_STEP2
    if flags == 0 and not conv:
        flags |= 2
    out = dict(sigma_win=sw, niter_win=niter, steps=np.sqrt(steps), nrepl_win=0, nlost_win=0)
    mom = None
    if not flags & 1:
        m, d = one(cx, cy, True)
        i0, i1, j0, j1, frac = _overlap(cx, cy, r, nx, ny)
        how = planes(img, sigma, bmap, seg, o['number'], cx, cy, mask_type)[3][j0:j1, i0:i1]
        pos, out['tangent_win'] = _reaches(cx, cy, r, i0, i1, j0, j1)
        out['nrepl_win'], out['nlost_win'] = int((pos & (how == REPL)).sum()), int((pos & (how == LOST)).sum())
        if not m[0] > 0.0:
            flags |= 1
        else:
            mom = _moments(m)
            st = out['steps']
            rho = float(np.max(st[1:] / st[:-1])) if len(st) > 1 and (st[:-1] > 0).all() else 0.0
            out['rho'] = rho
            dc = dstep * float(np.sum(rho ** np.arange(niter)))
            if rho >= 0.9 or flags & 2:                  # the object's own sensitivity (measure_ref.window)
                def once(x, y):
                    q, _ = one(x, y, False, 0.0)
                    return np.array([x + 2.0 * q[1] / q[0], y + 2.0 * q[2] / q[0]])
                h, jac, keep = 1e-5, [], half[0]
                for x, y in centres:
                    f0 = once(x, y)
                    jac.append(np.column_stack([(once(x + h, y) - f0) / h, (once(x, y + h) - f0) / h]))
                half[0] = keep                           # (probes beside the walk are not passes of it)
                prod, total = np.eye(2), 1.0
                for k in range(len(jac) - 1, 0, -1):
                    prod = prod @ jac[k]
                    total += float(np.linalg.norm(prod, 2))
                dc = dstep * total
            out['dcentre'] = dc
            tv = m[0]
            dsum = np.array([2.0 * (d[q] + abs(m[q] / tv) * d[0]) / tv for q in (1, 2, 3)] +
                            [4.0 * (d[q] + 2.0 * abs(m[q] / tv) * d[0]) / (tv * tv) for q in (4, 5, 6)])
            if np.isfinite(dc):
                keep = half[0]
                for ex, ey in ((dc, 0.0), (0.0, dc)):
                    m2, _ = one(cx + ex, cy + ey, True)
                    dsum = dsum + np.abs(_moments(m2) - mom)
                half[0] = keep
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
    out.update(errawin_image=ea, errbwin_image=eb, errthetawin_image=eth, flags_win=flags, half_win=half[0], touched_win=touched[0])
    return out


def aperture(img, sigma, bmap, seg, o, mask_type, radius=3.0, reverse=False):
    """The masked aperture about the barycentre: flux_aper = sum frac v', fluxerr_aper = sqrt(sum frac sigma'^2), the
    counts over the pixels the circle reaches (``_reaches``), and the overlap's pin summed over the terms (``dflux``, ``dvar``)."""
    ny, nx = img.shape
    cx, cy = o['xc'], o['yc']
    v, s, lost, how = planes(img, sigma, bmap, seg, o['number'], cx, cy, mask_type)
    i0, i1, j0, j1, frac = _overlap(cx, cy, radius, nx, ny)
    out = dict(flux_aper=0.0, fluxerr_aper=0.0, nap=0, nrepl_aper=0, nlost_aper=0, dflux=0.0, dvar=0.0, var_aper=0.0)
    if frac.size:
        h, keep = how[j0:j1, i0:i1], ~lost[j0:j1, i0:i1]
        pos, out['tangent_aper'] = _reaches(cx, cy, radius, i0, i1, j0, j1)
        out.update(nap=int(pos.sum()), nrepl_aper=int((pos & (h == REPL)).sum()), nlost_aper=int((pos & (h == LOST)).sum()))
        vv = np.where(keep, v[j0:j1, i0:i1], 0).astype(np.float64)
        ss = np.where(keep, s[j0:j1, i0:i1], 0).astype(np.float64)
        flux, var = _sum((frac * vv)[keep], reverse), _sum((frac * (ss * ss))[keep], reverse)
        pin = FRAC_RTOL * np.abs(frac) + FRAC_ATOL
        out.update(flux_aper=flux, var_aper=var, fluxerr_aper=float(np.sqrt(max(var, 0.0) if np.isfinite(var) else var)),
                   dflux=float((pin * np.abs(vv))[keep].sum()), dvar=float((pin * ss * ss)[keep].sum()))
    out['touched_aper'] = int((how[j0:j1, i0:i1] != USE).sum())
    out['share_aper'] = (out['nrepl_aper'] + out['nlost_aper']) / max(out['nap'], 1)
    out['aper_crowded'] = int(10 * (out['nrepl_aper'] + out['nlost_aper']) > out['nap'])
    return out


def measure(img, sigma, bad, seg, objs, mask_type, aper_radius=3.0, kron_fact=2.5, kron_min=3.5, reverse=False, cterm=0.0):
    """Every object of ``objs`` on the map ``seg``: list of dicts with INT_FIELDS, FLOAT_FIELDS, MASK_INT_FIELDS,
    MASK_FLOAT_FIELDS and the diagnostics."""
    img, sigma = np.ascontiguousarray(img, np.float32), np.ascontiguousarray(sigma, np.float32)
    bmap = badmap(img, sigma, bad)
    rows = []
    for o in objs:
        r = dict(o)
        r.update(kron(img, sigma, bmap, seg, o, mask_type, kron_fact, kron_min, reverse))
        r.update(window(img, sigma, bmap, seg, o, mask_type, reverse, cterm))
        r.update(aperture(img, sigma, bmap, seg, o, mask_type, aper_radius, reverse))
        r['crowded'] = int(bool(r['flags_auto'] & AUTO_CROWDED) or bool(r['aper_crowded']))
        rows.append(r)
    return rows


def census(rows):
    """What the integer results hinge on, on the restatement alone (tests/test_mask_gpu.py runs it before anything else)."""
    for r in rows:
        n = r['number']
        assert min(r['half'], r['half_win']) >= 1e-9, (n, 'a mirror at a rounding tie', r['half'], r['half_win'])
        assert r['near'] >= 1e-9, (n, 'a pixel on an ellipse edge', r['near'])
        for s in r['steps']:
            assert abs(s - 1e-4) > 1e-6 * 1e-4, (n, 'a step at the threshold', s)
        # the counts' "frac > 0": no pixel nearer to tangency than the centre is known (the window's centre ends an
        # iteration: dcentre) plus 1e-9 px
        assert r.get('tangent_aper', np.inf) >= 1e-9, (n, 'a pixel tangent to the aperture', r['tangent_aper'])
        assert r.get('tangent_win', np.inf) >= 1e-9 + 10.0 * r.get('dcentre', 0.0), (n, 'a pixel tangent to the window', r['tangent_win'])
        for k in ('share', 'share_crowd_auto', 'share_aper'):
            assert abs(r[k] - 0.10) > 1e-9, (n, k, r[k])
        for a, b, c in ((r['x2win'], r['y2win'], r['xywin']), (r['errx2win'], r['erry2win'], r['errxywin'])):
            d = a * b - c * c
            assert not np.isfinite(d) or abs(d - 0.00694) > 1e-9 * 0.00694, (n, 'determinant at the 1/12 rule', d)
