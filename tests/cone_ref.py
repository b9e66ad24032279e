"""Cone searches restated in numpy, independently of csrc/skyindex.hip: ``knn_ref`` and ``within_ref`` on
``assoc_ref.separation`` (brute force, the haversine on coordinate differences - not the chord between unit vectors the
kernels use), and the scenes tests/test_cone_gpu.py, tests/test_cone_ref.py and tests/measure_cone_tolerance.py share.

Every comparison but ``sep`` is exact, under two conditions that the restatement asserts on every scene it is given:

(a) no (query, row) pair lies in the band 0.999 r .. 1.001 r (``assoc_ref.assert_clear``): outside it the two formulas
    cannot disagree about membership;
(b) for every query, two rows within the radius are either the same position exactly (same ``ra`` and ``dec`` bits: both
    formulas give them the same distance, and the order is by row) or differ in separation by more than
    ``1000 * assoc_ref.SEP_TOL_ARCSEC``: the two formulas cannot disagree about the order.

Scenes meet both by dropping offending CATALOGUE rows when they are built (``clear_catalog``), never by leaving a query or
a slot out of a comparison."""
import numpy as np

import assoc_ref as ar

ORDER_GAP_ARCSEC = 1000 * ar.SEP_TOL_ARCSEC


def _same_position(cra, cdec, a, b):
    return cra[a].tobytes() == cra[b].tobytes() and cdec[a].tobytes() == cdec[b].tobytes()


def assert_order_clear(sep, cra, cdec, r, what='scene'):
    """Condition (b)."""
    for i in range(sep.shape[0]):
        rows = np.flatnonzero(np.isfinite(sep[i]) & (sep[i] <= r))
        if rows.size < 2:
            continue
        o = rows[np.argsort(sep[i, rows], kind='stable')]
        gap = np.diff(sep[i, o])
        for k in np.flatnonzero(gap <= ORDER_GAP_ARCSEC).tolist():
            assert _same_position(cra, cdec, o[k], o[k + 1]), \
                f'{what}: query {i}: rows {o[k]} and {o[k + 1]} are {gap[k]:.3e} arcsec apart in separation'


def _sep(ra, dec, cra, cdec, r, check, what):
    ra, dec, cra, cdec = (np.asarray(v, np.float64).reshape(-1) for v in (ra, dec, cra, cdec))
    sep = ar.separation(ra, dec, cra, cdec) if ra.size and cra.size else np.zeros((ra.size, cra.size))
    if check and sep.size:
        ar.assert_clear(sep, r, what)
        assert_order_clear(sep, cra, cdec, r, what)
    return ra, dec, cra, cdec, sep


def knn_ref(ra, dec, cat_ra, cat_dec, r, k, check=True, what='scene'):
    """(idx [n, k], sep [n, k], count [n]) of ``SkyIndex.knn``: rows within ``r`` ascending by (separation, row)."""
    ra, dec, cra, cdec, sep = _sep(ra, dec, cat_ra, cat_dec, r, check, what)
    n = ra.size
    idx = np.full((n, k), -1, np.int32)
    out = np.full((n, k), np.nan)
    count = np.zeros(n, np.int32)
    for i in range(n):
        rows = np.flatnonzero(np.isfinite(sep[i]) & (sep[i] <= r))
        count[i] = rows.size
        o = rows[np.argsort(sep[i, rows], kind='stable')][:k]            # stable: equal separations stay in row order
        idx[i, :o.size] = o
        out[i, :o.size] = sep[i, o]
    return idx, out, count


def within_ref(ra, dec, cat_ra, cat_dec, r, check=True, what='scene'):
    """(offsets int64 [n + 1], cat_idx int32) of ``SkyIndex.within``: rows within ``r``, ascending by row."""
    ra, dec, cra, cdec, sep = _sep(ra, dec, cat_ra, cat_dec, r, check, what)
    rows = [np.flatnonzero(np.isfinite(sep[i]) & (sep[i] <= r)) for i in range(ra.size)]
    offsets = np.zeros(ra.size + 1, np.int64)
    if rows:
        np.cumsum([v.size for v in rows], out=offsets[1:])
    cat_idx = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    return offsets, cat_idx


def clear_catalog(ra, dec, cra, cdec, radii):
    """Catalogue rows kept so that conditions (a) and (b) hold for the queries at every radius of ``radii``: the later row
    of an offending pair, or the row in a band, is dropped.  Rows that are not finite are kept (they match nothing).
    Returns the indices kept, ascending."""
    ra, dec, cra, cdec = (np.asarray(v, np.float64) for v in (ra, dec, cra, cdec))
    keep = np.ones(cra.size, bool)
    sep = ar.separation(ra, dec, cra, cdec)
    rmax = max(radii)
    for r in radii:
        with np.errstate(invalid='ignore'):
            keep &= ~((sep > 0.999 * r) & (sep < 1.001 * r)).any(axis=0)
    for i in range(ra.size):
        changed = True
        while changed:
            changed = False
            rows = np.flatnonzero(keep & np.isfinite(sep[i]) & (sep[i] <= rmax))
            o = rows[np.argsort(sep[i, rows], kind='stable')]
            gap = np.diff(sep[i, o])
            for k in np.flatnonzero(gap <= ORDER_GAP_ARCSEC).tolist():
                if not _same_position(cra, cdec, o[k], o[k + 1]):
                    keep[max(o[k], o[k + 1])] = False
                    changed = True
                    break
    return np.flatnonzero(keep)


# ---- scenes -----------------------------------------------------------------------------------------------------------
R_KNN, R_NAME = 30.0, 1.5
SCENES = ('field', 'counts', 'duplicates', 'wave65', 'wave300', 'cells', 'ra0', 'ra90', 'dec0', 'north', 'south', 'nonfinite')


def _cleared(ra, dec, cra, cdec, radii=(R_KNN, R_NAME)):
    k = clear_catalog(ra, dec, cra, cdec, radii)
    return ra, dec, cra[k], cdec[k]


def scene(name):
    """(ra, dec, cat_ra, cat_dec) of a scene, cleared for the radii 30 and 1.5 arcsec.  At most a few thousand rows and a
    few hundred queries."""
    seed = SCENES.index(name) + 101
    rng = np.random.default_rng(seed)
    if name == 'field':
        # a PS1-like field: 2000 rows in 0.2 deg (some tens within 30 arcsec), 200 queries, a third of them near a row
        cra, cdec = 150.0 + rng.uniform(-0.1, 0.1, 2000) / np.cos(np.radians(20.0)), 20.0 + rng.uniform(-0.1, 0.1, 2000)
        ra, dec = 150.0 + rng.uniform(-0.1, 0.1, 200) / np.cos(np.radians(20.0)), 20.0 + rng.uniform(-0.1, 0.1, 200)
        near = rng.choice(2000, 70, replace=False)
        th = rng.uniform(0, 2 * np.pi, 70)
        rho = rng.uniform(0.0, 1.3, 70)
        ra[:70], dec[:70] = ar.offset(cra[near], cdec[near], rho * np.cos(th), rho * np.sin(th))
        return _cleared(ra, dec, cra, cdec)
    if name == 'counts':
        # query q has exactly q rows within 30 arcsec, q = 0 .. 12 (around every k - 1, k, k + 1 for k <= 8), and 40
        ras, decs, cras, cdecs = [], [], [], []
        for q, nrow in enumerate(list(range(13)) + [40]):
            qa, qd = 40.0 + 0.1 * q, -5.0
            ras.append(qa)
            decs.append(qd)
            rho = 2.0 + 26.0 * (np.arange(nrow) + 0.5) / max(nrow, 1)        # distinct separations, 0.65 arcsec apart or more
            th = rng.uniform(0, 2 * np.pi, nrow)
            a, d = ar.offset(qa, qd, rho * np.cos(th), rho * np.sin(th))
            cras.append(a)
            cdecs.append(d)
        cra, cdec = np.concatenate(cras), np.concatenate(cdecs)
        p = rng.permutation(cra.size)
        return _cleared(np.array(ras), np.array(decs), cra[p], cdec[p])
    if name == 'duplicates':
        # exact duplicate rows nearest to a query: three and five copies, interleaved with other rows
        ra, dec = np.array([10.0, 200.0, 300.0]), np.array([10.0, -40.0, 0.0])
        cra = np.array([10.0001, 200.0, 10.0001, 300.0, 200.0, 10.0001, 200.0, 10.002, 200.0, 200.0, 300.001, 200.001])
        cdec = np.array([10.0001, -40.0, 10.0001, 0.0, -40.0, 10.0001, -40.0, 10.0, -40.0, -40.0, 0.0, -40.0])
        return _cleared(ra, dec, cra, cdec)
    if name in ('wave65', 'wave300'):
        # one cell holds more rows than a wave has lanes: all inside one 30 arcsec circle (radius 12: one cell or few)
        size = 65 if name == 'wave65' else 300
        rho = 12.0 * np.sqrt((np.arange(size) + 0.5) / size)
        th = rng.uniform(0, 2 * np.pi, size)
        cra, cdec = ar.offset(210.0, 33.0, rho * np.cos(th), rho * np.sin(th))
        fra, fdec = 210.0 + rng.uniform(-0.05, 0.05, 100), 33.0 + rng.uniform(-0.05, 0.05, 100)
        cra, cdec = np.concatenate([cra, fra]), np.concatenate([cdec, fdec])
        p = rng.permutation(cra.size)
        ra, dec = ar.offset(210.0, 33.0, np.array([0.0, 3.0, -20.0, 200.0]), np.array([0.0, -4.0, 15.0, 0.0]))
        return _cleared(ra, dec, cra[p], cdec[p])
    if name == 'cells':
        # rows on a ring of 25 arcsec around each query: wherever the query sits in its cell (edge 30 arcsec), the ring
        # crosses cell faces, so the matches lie in several of the 27 cells
        ras, decs, cras, cdecs = [], [], [], []
        for q in range(12):
            qa, qd = 120.0 + 0.05 * q, 45.0 + 0.013 * q
            ras.append(qa)
            decs.append(qd)
            th = np.radians(np.arange(0, 360, 30.0) + 3.0 * q)
            a, d = ar.offset(qa, qd, (25.0 - 0.7 * np.arange(12)) * np.cos(th), (25.0 - 0.7 * np.arange(12)) * np.sin(th))
            cras.append(a)
            cdecs.append(d)
        return _cleared(np.array(ras), np.array(decs), np.concatenate(cras), np.concatenate(cdecs))
    if name in ('ra0', 'ra90', 'dec0'):
        # the where cases of test_clusters_where_a_vector_component_changes_sign: a vector component changes sign
        box = dict(ra0=(0.0, 37.0, 0.01), ra90=(90.0, -20.0, 0.01), dec0=(222.0, 0.0, 0.01))[name]
        cra, cdec, _, _ = ar.scene(7, nclusters=25, nnoise=25, box=box)
        a, d = ar.offset(box[0], box[1], rng.uniform(-0.6, 0.6, 9), rng.uniform(-0.6, 0.6, 9))   # centred on the line
        cra, cdec = np.concatenate([cra, a]), np.concatenate([cdec, d])
        ra, dec = ar.offset(box[0], box[1], rng.uniform(-18, 18, 40), rng.uniform(-18, 18, 40))
        ra, dec = np.concatenate([ra, cra[:4]]), np.concatenate([dec, cdec[:4]])                # four queries exactly on a row
        if name == 'ra0':
            assert (cra > 359.99).any() and (cra < 0.01).any()
        return _cleared(ra, dec, cra, cdec)
    if name in ('north', 'south'):
        sign = 1.0 if name == 'north' else -1.0
        cra, cdec = ar.polar_cap(sign, rng.uniform(0.0, 0.9, 12), rng.uniform(0, 360, 12))      # a cluster on the pole
        a, d = ar.polar_cap(sign, rng.uniform(20.0, 400.0, 30), rng.uniform(0, 360, 30))
        cra, cdec = np.concatenate([cra, a, [0.0]]), np.concatenate([cdec, d, [sign * 90.0]])   # a row exactly on the pole
        ra, dec = ar.polar_cap(sign, rng.uniform(0.0, 60.0, 30), rng.uniform(0, 360, 30))
        ra, dec = np.concatenate([ra, [123.0]]), np.concatenate([dec, [sign * 90.0]])           # a query exactly on it too
        return _cleared(ra, dec, cra, cdec)
    if name == 'nonfinite':
        ra, dec, cra, cdec = scene('field')
        ra, dec, cra, cdec = ra[:60].copy(), dec[:60].copy(), cra.copy(), cdec.copy()
        ra[3], dec[7], ra[11], dec[12] = np.nan, np.inf, -np.inf, np.nan
        near = np.argmin(ar.separation(ra[:1], dec[:1], cra, cdec)[0])                          # the row nearest to query 0
        cra[near] = np.nan
        cdec[5], cra[9], cdec[20] = np.inf, -np.inf, np.nan
        return _cleared(ra, dec, cra, cdec)
    raise KeyError(name)
