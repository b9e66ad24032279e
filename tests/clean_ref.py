"""The CLEAN pass of the source extraction, restated in numpy ("CLEAN"): the authority the GPU tests compare
zm_extract_clean and zm_clean_decide with.

Test infrastructure.  Everything a decision depends on is float64 (float32 where the operator says so), one rounded
operation each in the order DESIGN.md writes them: with ``param == 1`` the decisions are made of +, -, x, / and
comparisons alone and must agree with the kernels bit for bit on the same table.  For any other ``param`` the two sides'
``pow`` differ by a few ulp, and a full call reaches ``decide`` through rows whose sums were taken in another order:
``decide`` therefore returns the smallest relative gap of any comparison of a profile, and agreement is asked for only
where that gap exceeds ``GAP_MIN``.
"""
import numpy as np

import deblend_ref as dr
import extract_ref as xr

GAP_MIN = 1e-5
ROW = np.dtype([('number', 'i4'), ('npix', 'i4'), ('first', 'i4'), ('x_image', 'f8'), ('y_image', 'f8'), ('x2', 'f8'),
                ('y2', 'f8'), ('xy', 'f8'), ('a_image', 'f8'), ('b_image', 'f8')])
COLUMNS = xr.COLUMNS + [('PARENT_NUMBER', 'i4'), ('NMERGED', 'i4')]


def check_settings(param):
    if not (np.isfinite(param) and 0.1 <= param <= 10.0):
        raise ValueError(f'param={param!r} must be finite and lie in [0.1, 10]')


def kth_largest(values, k):
    """The k-th largest value, ties counted, by rounds of "largest value below the last one, with its multiplicity"."""
    v = np.asarray(values, np.float32)
    assert len(v) >= k >= 1
    last, seen = np.float32(np.inf), 0
    while True:
        below = v[v < last]
        best = below.max()
        seen += int(np.count_nonzero(below == best))
        if seen >= k:
            return best
        last = best


def fixed_order_sum(e, v):
    """Sum of float64 ``v`` as k_ex_measure takes it: element ``e`` (position in the row-major bounding box) belongs to
    lane e % 256 and every lane adds its elements in the order of the walk; the 64 lanes of a wave are added by xor
    shuffles over 32, 16 .. 1, the four waves as ((w0 + w1) + w2) + w3."""
    e = np.asarray(e, np.int64)
    v = np.asarray(v, np.float64)
    order = np.argsort(e, kind='stable')
    e, v = e[order], v[order]
    lanes = np.zeros(256, np.float64)
    rounds = e // 256
    for r in np.unique(rounds):
        sel = rounds == r
        lanes[e[sel] % 256] += v[sel]                     # one element per lane and round
    w = lanes.reshape(4, 64)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, idx ^ o]
    return float(((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


def object_sums(p, ffilt, fthr, nx, k, reverse=False):
    """(row fields, F, T, m) of the object with member pixels ``p`` (raster order).  ``reverse``: sums in reversed member
    order instead of the kernel's (an order effect, which no decision of a scene may depend on)."""
    y, x = np.divmod(p, nx)
    xmin, xmax, ymin = x.min(), x.max(), y.min()
    v = ffilt[p].astype(np.float64)
    dx, dy = (x - xmin).astype(np.float64), (y - ymin).astype(np.float64)
    e = (y - ymin) * (xmax - xmin + 1) + (x - xmin)
    tot = (lambda a: xr._sum(a, True)) if reverse else (lambda a: fixed_order_sum(e, a))
    S = tot(v)
    xb, yb = tot(v * dx) / S, tot(v * dy) / S
    x2 = tot(v * dx * dx) / S - xb * xb
    y2 = tot(v * dy * dy) / S - yb * yb
    xy = tot(v * dx * dy) / S - xb * yb
    if x2 * y2 - xy * xy < 0.00694:
        x2 += 1.0 / 12.0
        y2 += 1.0 / 12.0
    pm, dm = 0.5 * (x2 + y2), 0.5 * (x2 - y2)
    rt = np.sqrt(dm * dm + xy * xy)
    row = dict(npix=len(p), first=int(p.min()), x_image=xmin + xb + 1.0, y_image=ymin + yb + 1.0, x2=x2, y2=y2, xy=xy,
               a_image=np.sqrt(pm + rt), b_image=np.sqrt(max(pm - rt, 0.0)))
    ipk = int(np.argmax(ffilt[p]))                        # first pixel in raster order of the largest value
    T = fthr[p[ipk]]
    m = kth_largest(ffilt[p] - fthr[p], k)                # float32 - float32
    return row, S, np.float32(T), np.float32(m)


def model(rows, F, T, param):
    """dict(amp, alpha, cxx, cyy, cxy, ok) in float64."""
    x2, y2, xy = rows['x2'], rows['y2'], rows['xy']
    with np.errstate(all='ignore'):
        d = x2 * y2 - xy * xy
        cxx, cyy, cxy = y2 / d, x2 / d, -2.0 * xy / d
        area = np.pi * rows['a_image'] * rows['b_image']
        amp = np.asarray(F, np.float64) / (2.0 * area)
        ratio = amp / np.asarray(T, np.float32).astype(np.float64)
        g = ratio if param == 1.0 else np.power(ratio, 1.0 / param)
        alpha = (g - 1.0) * area / rows['npix'].astype(np.float64)
        ok = np.isfinite(amp) & np.isfinite(alpha) & (alpha > 0.0)
    return dict(amp=amp, alpha=alpha, cxx=cxx, cyy=cyy, cxy=cxy, ok=ok)


def decide(rows, F, T, m, param=1.0):
    """(into, root, gap): NUMBER of the absorber of every object (0: none), NUMBER at the end of its chain, and the smallest
    relative gap of the decisions: |prof - m_j| / m_j over all tested pairs, and the best absorber against the second
    best.  NUMBER is index + 1."""
    check_settings(param)
    rows = np.asarray(rows)
    n = len(rows)
    F = np.asarray(F, np.float64)
    m = np.asarray(m, np.float32)
    M = model(rows, F, T, param)
    x, y, a = rows['x_image'], rows['y_image'], rows['a_image']
    num = np.arange(n)
    into = np.zeros(n, np.int32)
    gap = np.inf
    with np.errstate(all='ignore'):
        for j in range(n):                                # absorbers i are the vector
            larger = (F > F[j]) | ((F == F[j]) & (num < j))
            dx, dy = x[j] - x, y[j] - y
            z = 10.0 * (a + a[j])
            val = 1.0 + M['alpha'] * ((M['cxx'] * dx * dx + M['cyy'] * dy * dy) + M['cxy'] * dx * dy)
            tested = larger & M['ok'] & (dx * dx + dy * dy < z * z) & (val > 1.0) & (val < 1e10)
            if not tested.any():
                continue
            prof = (M['amp'] / val if param == 1.0 else M['amp'] * np.power(val, -param))[tested]
            gap = min(gap, float(np.min(np.abs(prof - np.float64(m[j])) / np.float64(m[j]))))
            cand = prof.astype(np.float32) > m[j]
            if not cand.any():
                continue
            pc, ic = prof[cand], np.flatnonzero(tested)[cand]
            best = int(np.argmax(pc))                     # the first of a tie: the smallest NUMBER
            into[j] = ic[best] + 1
            if len(pc) > 1:
                second = np.delete(pc, best).max()
                gap = min(gap, float((pc[best] - second) / pc[best]))
    root = np.arange(1, n + 1, dtype=np.int32)
    for j in range(n):
        r, steps = j + 1, 0
        while into[r - 1]:
            r = int(into[r - 1])
            steps += 1
            assert steps <= n, 'a cycle: F grows strictly along a chain'
        root[j] = r
    return into, root, gap


def _members(seg, n):
    flat = seg.ravel()
    members = np.flatnonzero(flat)
    members = members[np.argsort(flat[members], kind='stable')]
    bounds = np.searchsorted(flat[members], np.arange(1, n + 2))
    return [members[bounds[k]:bounds[k + 1]] for k in range(n)]


def clean(img, sigma, bad=None, flag=None, param=1.0, deblend=None, reverse=False, reverse_objects=False, wcs=None, **kw):
    """dict(filtered, segm, table (with PARENT_NUMBER and NMERGED), pre = the pass before, rows, F, T, m, into, root, gap).
    ``deblend``: None or dict(nthresh=, mincont=).  ``reverse``: reversed member order in every sum;
    ``reverse_objects``: the decision on the table in reversed object order (the map must not depend on either)."""
    check_settings(param)
    k = kw.get('detect_minarea', 5)
    if deblend is not None:
        pre = dr.deblend(img, sigma, bad, flag, reverse=reverse, wcs=wcs, **deblend, **kw)
        seg1 = pre['first']['segm']
        t = pre['table']
        split = np.zeros(len(pre['first']['table']) + 1, bool)
        split[t['PARENT_NUMBER'][(t['FLAGS'] & 2) != 0]] = True
    else:
        pre = xr.extract(img, sigma, bad, flag, reverse=reverse, wcs=wcs, **kw)
        seg1 = pre['segm']
        split = np.zeros(len(pre['table']) + 1, bool)
    filt, seg0 = np.asarray(pre['filtered'], np.float32), pre['segm']
    ny, nx = seg0.shape
    n0 = len(pre['table'])
    with np.errstate(invalid='ignore', over='ignore'):
        thr = np.float32(kw.get('detect_thresh', 1.5)) * np.ascontiguousarray(sigma, np.float32)
    ffilt, fthr = filt.ravel(), thr.ravel()
    members = _members(seg0, n0)
    rows = np.zeros(n0, ROW)
    F, T, m = np.zeros(n0), np.zeros(n0, np.float32), np.zeros(n0, np.float32)
    for j, p in enumerate(members):
        r, F[j], T[j], m[j] = object_sums(p, ffilt, fthr, nx, k, reverse)
        rows[j] = tuple([j + 1] + [r[c] for c in ROW.names[1:]])
    if n0 == 0:
        into, root, gap = np.zeros(0, np.int32), np.zeros(0, np.int32), np.inf
    elif reverse_objects:
        # the same objects with their NUMBERs, visited in the other order: NUMBER (not position) breaks the ties
        into, root, gap = decide(rows, F, T, m, param)
        order = np.arange(n0)[::-1]
        i2, r2, _ = decide_permuted(rows, F, T, m, param, order)
        assert np.array_equal(i2, into) and np.array_equal(r2, root)
    else:
        into, root, gap = decide(rows, F, T, m, param)
    labels = np.full(ny * nx, -1, np.int64)
    newfirst = np.full(n0 + 1, np.iinfo(np.int64).max)
    nmerged = np.zeros(n0 + 1, np.int32)
    for j in range(n0):
        newfirst[root[j]] = min(newfirst[root[j]], rows['first'][j])
        nmerged[root[j]] += 1
    for j, p in enumerate(members):
        labels[p] = newfirst[root[j]]
    with dr._labels(labels.reshape(ny, nx)):
        out = xr.extract(img, sigma, bad, flag, reverse=reverse, wcs=wcs, **kw)
    t = out['table']
    tab = np.zeros(len(t), dtype=COLUMNS)
    for c in t.dtype.names:
        tab[c] = t[c]
    if len(t):
        parent = seg1.ravel()[out['first']]
        tab['PARENT_NUMBER'] = parent
        tab['FLAGS'] |= np.where(split[parent], 2, 0).astype(np.int32)
        tab['NMERGED'] = nmerged[root[seg0.ravel()[out['first']] - 1]]
    return dict(filtered=filt, segm=out['segm'], table=tab, pre=pre, rows=rows, F=F, T=T, m=m, into=into, root=root, gap=gap)


def decide_permuted(rows, F, T, m, param, order):
    """``decide`` on the table visited in ``order`` (a permutation of the indices), answered in the original numbering: a
    loop over pairs that takes NUMBER from the row, not from the position."""
    rows = np.asarray(rows)
    n = len(rows)
    M = model(rows, F, T, param)
    num = rows['number']
    into = np.zeros(n, np.int32)
    gap = np.inf
    with np.errstate(all='ignore'):
        for j in order:
            best, bestnum = None, 0
            for i in order:
                if not (F[i] > F[j] or (F[i] == F[j] and num[i] < num[j])) or not M['ok'][i]:
                    continue
                dx, dy = rows['x_image'][j] - rows['x_image'][i], rows['y_image'][j] - rows['y_image'][i]
                z = 10.0 * (rows['a_image'][i] + rows['a_image'][j])
                if not dx * dx + dy * dy < z * z:
                    continue
                val = 1.0 + M['alpha'][i] * ((M['cxx'][i] * dx * dx + M['cyy'][i] * dy * dy) + M['cxy'][i] * dx * dy)
                if not 1.0 < val < 1e10:
                    continue
                prof = M['amp'][i] / val if param == 1.0 else M['amp'][i] * np.power(val, -param)
                if not np.float32(prof) > np.float32(m[j]):
                    continue
                if best is None or prof > best or (prof == best and num[i] < bestnum):
                    best, bestnum = prof, int(num[i])
            into[j] = bestnum
    root = np.zeros(n, np.int32)
    for j in range(n):
        r = j + 1
        for _ in range(n + 1):
            if not into[r - 1]:
                break
            r = int(into[r - 1])
        root[j] = r
    return into, root, gap
