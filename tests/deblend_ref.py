"""numpy restatement of the multi-threshold deblending (csrc/deblend.hip; DESIGN.md "Deblending").

Test infrastructure, imported like ``extract_ref.py``, from which the filter, the 8-connected labelling and the
measurements are taken.  It follows the statement of the operator, not the kernel: the tree is built as explicit nodes
with explicit child lists and split sets, level by level from ``label8`` of every level's pixel set, and the leftover
pixels are handed out in synchronous rounds.

``reverse=True`` walks every object's members in the opposite order (level components are labelled on the flipped box,
the integer sums run backwards, the frontier of every round is visited from its other end, and the float64 sums of the
measurements are reversed as in ``extract_ref``): the map must not depend on it.
"""
from contextlib import contextmanager

import numpy as np

import extract_ref as xr

COLUMNS = xr.COLUMNS + [('PARENT_NUMBER', 'i4')]


def check_settings(nthresh, mincont):
    if int(nthresh) != nthresh or not 2 <= nthresh <= 64 or int(nthresh) & (int(nthresh) - 1):
        raise ValueError('nthresh must be a power of two in 2 .. 64')
    if not 0.0 <= mincont <= 1.0:
        raise ValueError('mincont must lie in [0, 1]')


def thresholds(P, T, nthresh):
    """u_0 .. u_(N-1): float64, log2 N square roots of P / T, then one rounded product per step."""
    g = np.float64(P) / np.float64(T)
    for _ in range(int(nthresh).bit_length() - 1):
        g = np.sqrt(g)
    u = np.empty(nthresh, np.float64)
    e = np.float64(1.0)
    u[0] = np.float64(T) * e
    for k in range(1, nthresh):
        e = e * g
        u[k] = np.float64(T) * e
    return u


def pixel_levels(f, u):
    """L(p): how many of u_1 .. u_(N-1) the pixel's value exceeds."""
    f = np.asarray(f, np.float32).astype(np.float64)
    L = np.zeros(f.shape, np.int64)
    for k in range(1, len(u)):
        L += f > u[k]
    return L


def level_components(Lbox, k, reverse=False):
    """Component id (any integer, -1 outside) of every pixel of {L >= k} in the box."""
    mask = Lbox >= k
    if reverse:
        return xr.label8(mask[::-1, ::-1])[::-1, ::-1]
    return xr.label8(mask)


def build_tree(Lbox, fbox, u, P, nthresh, mincont, minarea, reverse=False):
    """Nodes (dicts: level, pix = flat box indices, n, Q, F, children, significant) in the order they were made
    (level N - 1 first) and the index of the root."""
    m, e = np.frexp(np.float64(P))
    scale, back = np.ldexp(1.0, 32 - int(e)), np.ldexp(1.0, int(e) - 32)
    flat_f = fbox.ravel().astype(np.float64)
    q = np.trunc(flat_f * scale).astype(np.int64)
    nodes, node_of = [], np.full(Lbox.size, -1, np.int64)
    comp = None
    for k in range(nthresh - 1, -1, -1):
        if comp is None or (Lbox == k).any():                        # (a level without pixels of its own: same set)
            comp = level_components(Lbox, k, reverse).ravel()
        inside = np.flatnonzero(comp >= 0)
        if inside.size == 0:
            continue
        order = inside[np.argsort(comp[inside], kind='stable')]
        cuts = np.flatnonzero(np.diff(comp[order])) + 1
        new_of = node_of.copy()
        for pix in np.split(order, cuts):
            if reverse:
                pix = pix[::-1]
            kids = sorted(set(node_of[pix][node_of[pix] >= 0].tolist()))
            Q = int(q[pix].sum(dtype=np.int64))
            nodes.append(dict(level=k, pix=pix, n=int(pix.size), Q=Q, F=np.float64(Q) * back, children=kids))
            new_of[pix] = len(nodes) - 1
        node_of = new_of
    root = len(nodes) - 1
    assert nodes[root]['level'] == 0 and nodes[root]['n'] == int((Lbox >= 0).sum())
    rhs = np.float64(mincont) * nodes[root]['F']
    for v in nodes:
        prod = u[v['level']] * np.float64(v['n'])                    # two rounded operations: product, difference
        v['significant'] = bool(v['n'] >= minarea and (v['F'] - prod) > rhs)
    return nodes, root


def split_sets(nodes):
    """S(v) of every node, bottom up."""
    S = [None] * len(nodes)
    for i, v in enumerate(nodes):                                    # children were made before their parent
        kids = v['children']
        sig = [c for c in kids if nodes[c]['significant']]
        if len(sig) >= 2:
            S[i] = set().union(*[(S[c] if S[c] else {c}) for c in sig])
        else:
            S[i] = set().union(*[S[c] for c in kids]) if kids else set()
    return S


def grow(lab, Lbox, fbox, nthresh, reverse=False):
    """Leftover pixels: synchronous rounds, level by level.  ``lab``: int64 box, -1 = unlabelled member or outside."""
    h, w = Lbox.shape
    W = w + 2
    L = np.full((h + 2, W), -1, np.int64)
    L[1:-1, 1:-1] = Lbox
    f = np.zeros((h + 2, W), np.float32)
    f[1:-1, 1:-1] = fbox
    lb = np.full((h + 2, W), -1, np.int64)
    lb[1:-1, 1:-1] = lab
    L, f, lb = L.ravel(), f.ravel(), lb.ravel()
    offs = np.array([-W - 1, -W, -W + 1, -1, 1, W - 1, W, W + 1])
    big = np.iinfo(np.int64).max
    for k in range(nthresh - 1, -1, -1):
        # the pixels that can take a label in the first round of this level; in later rounds only the unlabelled
        # neighbours of the pixels labelled in the round before have gained a labelled neighbour
        cand = np.flatnonzero((lb < 0) & (L >= k))
        front = cand[(lb[cand[:, None] + offs[None, :]] >= 0).any(axis=1)]
        while front.size:
            if reverse:
                front = front[::-1]
            nb = front[:, None] + offs[None, :]
            labelled = lb[nb] >= 0
            fv = np.where(labelled, f[nb], -np.inf)
            best = fv.max(axis=1)
            pick = np.where(labelled & (fv == best[:, None]), nb, big).min(axis=1)   # largest f, then smallest index
            lb[front] = lb[pick]                                     # all decided before any is written
            nxt = np.unique(nb.ravel())
            front = nxt[(lb[nxt] < 0) & (L[nxt] >= k)]
    return lb.reshape(h + 2, W)[1:-1, 1:-1]


def deblend_object(members, filt, thr, nx, nthresh, mincont, minarea, reverse=False):
    """New label (smallest linear index of the sub-object) per member, or None when the object does not split."""
    ffilt = filt.ravel()
    fm = ffilt[members]
    ipk = int(np.argmax(fm))                                         # first pixel in raster order of the largest value
    P, T = fm[ipk], thr.ravel()[members[ipk]]
    u = thresholds(P, T, nthresh)
    y, x = np.divmod(members, nx)
    x0, y0 = x.min(), y.min()
    w, h = x.max() - x0 + 1, y.max() - y0 + 1
    box = (y - y0) * w + (x - x0)
    Lbox = np.full(h * w, -1, np.int64)
    Lbox[box] = pixel_levels(fm, u)
    fbox = np.zeros(h * w, np.float32)
    fbox[box] = fm
    Lbox, fbox = Lbox.reshape(h, w), fbox.reshape(h, w)
    nodes, root = build_tree(Lbox, fbox, u, P, nthresh, mincont, minarea, reverse)
    S = split_sets(nodes)
    if len(S[root]) < 2:
        return None
    lab = np.full(h * w, -1, np.int64)
    for s in sorted(S[root]):
        assert (lab[nodes[s]['pix']] < 0).all()
        lab[nodes[s]['pix']] = s
    lab = grow(lab.reshape(h, w), Lbox, fbox, nthresh, reverse).ravel()[box]
    assert (lab >= 0).all()
    out = np.empty(len(members), np.int64)
    for s in np.unique(lab):
        out[lab == s] = members[lab == s].min()
    return out


@contextmanager
def _labels(plane):
    """extract_ref.extract with its labelling step replaced by a given label plane: the measurements, flags and
    numbering are then extract_ref's own arithmetic on the deblended objects."""
    saved = xr.label8
    xr.label8 = lambda fg: plane
    try:
        yield
    finally:
        xr.label8 = saved


def deblend(img, sigma, bad=None, flag=None, nthresh=32, mincont=0.005, reverse=False, wcs=None, **kw):
    """dict(filtered, segm, table (with FLAGS bit 2 and PARENT_NUMBER), first = the first pass, nsplit)."""
    check_settings(nthresh, mincont)
    minarea = kw.get('detect_minarea', 5)
    first = xr.extract(img, sigma, bad, flag, reverse=reverse, wcs=wcs, **kw)
    filt, seg1 = np.asarray(first['filtered'], np.float32), first['segm']
    ny, nx = seg1.shape
    with np.errstate(invalid='ignore', over='ignore'):
        thr = np.float32(kw.get('detect_thresh', 1.5)) * np.ascontiguousarray(sigma, np.float32)
    labels = xr.label8(first['fg']).copy()
    flat = seg1.ravel()
    members = np.flatnonzero(flat)
    members = members[np.argsort(flat[members], kind='stable')]
    n1 = len(first['table'])
    bounds = np.searchsorted(flat[members], np.arange(1, n1 + 2))
    split = np.zeros(n1 + 1, bool)
    lflat = labels.ravel()
    for k in range(n1):
        p = members[bounds[k]:bounds[k + 1]]
        new = deblend_object(p, filt, thr, nx, nthresh, mincont, minarea, reverse)
        if new is not None:
            lflat[p] = new
            split[k + 1] = True
    with _labels(labels):
        out = xr.extract(img, sigma, bad, flag, reverse=reverse, wcs=wcs, **kw)
    t = out['table']
    tab = np.zeros(len(t), dtype=COLUMNS)
    for c in t.dtype.names:
        tab[c] = t[c]
    parent = flat[out['first']] if len(t) else np.zeros(0, np.int32)
    tab['PARENT_NUMBER'] = parent
    tab['FLAGS'] |= np.where(split[parent], 2, 0).astype(np.int32)
    return dict(filtered=filt, segm=out['segm'], table=tab, first=first, nsplit=int(split.sum()), fg=first['fg'])
