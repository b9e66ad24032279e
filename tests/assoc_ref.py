"""Source association restated in numpy, independently of csrc/associate.hip.

* separations: brute force, O(n^2), with the haversine formula on coordinate differences - not the chord between unit
  vectors the kernels use;
* components: a plain union-find over the pairs within the radius (inclusive);
* numbering and ties as the reference's tools define them: a component of one row is noise (-1), the others are numbered
  by the rank of their smallest row (``sklearn.cluster.DBSCAN(min_samples=2)``), the best detection is the first row of
  greatest S/N (pandas ``idxmax``), the nearest catalogue entry is the first of equals (``argmin``).

The scene builder guarantees that no pair lies between 0.999 r and 1.001 r (``assert_clear``): outside that band the
two formulas cannot disagree about membership, so everything but ``sep`` is compared exactly."""
import numpy as np

ARCSEC = 3600.0


def separation(ra1, dec1, ra2, dec2):
    """Haversine separation in arcsec of every (row of 1, row of 2): shape [n1, n2]."""
    ra1, dec1 = np.asarray(ra1, np.float64)[:, None], np.asarray(dec1, np.float64)[:, None]
    ra2, dec2 = np.asarray(ra2, np.float64)[None, :], np.asarray(dec2, np.float64)[None, :]
    with np.errstate(invalid='ignore'):
        sd = np.sin(np.radians(dec2 - dec1) / 2.0)
        sr = np.sin(np.radians(ra2 - ra1) / 2.0)
        a = sd * sd + np.cos(np.radians(dec1)) * np.cos(np.radians(dec2)) * sr * sr
        return np.degrees(2.0 * np.arcsin(np.sqrt(np.minimum(a, 1.0)))) * ARCSEC


def assert_clear(sep, r, what='scene'):
    """The condition of every exact comparison: no separation between 0.999 r and 1.001 r."""
    s = sep[np.isfinite(sep)]
    bad = (s > 0.999 * r) & (s < 1.001 * r)
    assert not bad.any(), f'{what}: {int(bad.sum())} separations lie between 0.999 r and 1.001 r'


def assert_nearest_clear(sep, r, what='scene'):
    """For a cross-match: the two nearest entries in range are either exactly as far or differ by more than 1e-6 arcsec."""
    s = np.where(np.isfinite(sep) & (sep <= r), sep, np.inf)
    if s.shape[1] < 2:
        return
    part = np.sort(s, axis=1)[:, :2]
    both = np.isfinite(part[:, 1])
    gap = part[both, 1] - part[both, 0]
    assert ((gap == 0.0) | (gap > 1e-6)).all(), f'{what}: two catalogue entries are nearly, not exactly, as far'


def _find(parent, i):
    root = i
    while parent[root] != root:
        root = parent[root]
    while parent[i] != root:
        parent[i], i = root, parent[i]
    return root


def cluster_ref(ra, dec, snr, rb=None, r=2.0, check=True):
    """The arrays of ``source.cluster`` (same keys).  ``check``: assert the scene's condition on the way."""
    ra, dec, snr = (np.asarray(v, np.float64) for v in (ra, dec, snr))
    n = ra.size
    ok = np.isfinite(ra) & np.isfinite(dec) & np.isfinite(snr)
    parent = list(range(n))
    deg = np.zeros(n, np.int64)
    rows = np.flatnonzero(ok)
    for b0 in range(0, rows.size, 512):
        blk = rows[b0:b0 + 512]
        sep = separation(ra[blk], dec[blk], ra[rows], dec[rows])
        if check:
            assert_clear(sep, r)
        ii, jj = np.nonzero(sep <= r)
        for a, b in zip(blk[ii].tolist(), rows[jj].tolist()):
            if a != b:
                deg[a] += 1
                ra_, rb_ = _find(parent, a), _find(parent, b)
                if ra_ != rb_:
                    parent[max(ra_, rb_)] = min(ra_, rb_)          # the root is the smallest member
    root = np.array([_find(parent, i) for i in range(n)], dtype=np.int64)
    clustered = deg > 0
    roots = np.unique(root[clustered])                              # ascending: the rank of the smallest member
    label = np.full(n, -1, np.int32)
    label[clustered] = np.searchsorted(roots, root[clustered]).astype(np.int32)
    nsrc = roots.size
    offsets = np.zeros(nsrc + 1, np.int32)
    members, best, count, sumrb = [], np.zeros(nsrc, np.int32), np.zeros(nsrc, np.int32), np.zeros(nsrc, np.float64)
    for s in range(nsrc):
        m = np.flatnonzero(label == s)                              # ascending
        members.append(m)
        count[s] = m.size
        offsets[s + 1] = offsets[s] + m.size
        best[s] = m[np.argmax(snr[m])]                              # the first of equals
        acc = np.float64(0.0)
        if rb is not None:
            for v in np.asarray(rb, np.float64)[m]:
                acc = acc + v                                       # member order, one add at a time
        sumrb[s] = acc
    members = np.concatenate(members).astype(np.int32) if members else np.zeros(0, np.int32)
    return dict(label=label, nsrc=int(nsrc), offsets=offsets, members=members, best=best, count=count, sumrb=sumrb)


def crossmatch_ref(ra, dec, cat_ra, cat_dec, r, check=True):
    """(idx, sep) of ``source.crossmatch``."""
    ra, dec, cra, cdec = (np.asarray(v, np.float64) for v in (ra, dec, cat_ra, cat_dec))
    idx = np.full(ra.size, -1, np.int32)
    out = np.full(ra.size, np.nan)
    if cra.size == 0 or ra.size == 0:
        return idx, out
    sep = separation(ra, dec, cra, cdec)
    if check:
        assert_clear(sep, r)
        assert_nearest_clear(sep, r)
    s = np.where(np.isfinite(sep) & (sep <= r), sep, np.inf)
    j = np.argmin(s, axis=1)
    hit = np.isfinite(s[np.arange(ra.size), j])
    idx[hit] = j[hit]
    out[hit] = sep[np.arange(ra.size), j][hit]
    return idx, out


def offset(ra0, dec0, dx, dy):
    """Positions ``dx`` arcsec east and ``dy`` arcsec north of (ra0, dec0) in the tangent-plane sense; RA folded into
    [0, 360)."""
    dec = dec0 + np.asarray(dy, np.float64) / ARCSEC
    ra = ra0 + np.asarray(dx, np.float64) / ARCSEC / np.cos(np.radians(dec0))
    return np.mod(ra, 360.0), dec


def polar_cap(sign, rho, theta):
    """Positions ``rho`` arcsec from the pole of the given sign at position angles ``theta`` (degrees)."""
    return np.mod(np.asarray(theta, np.float64), 360.0), sign * (90.0 - np.asarray(rho, np.float64) / ARCSEC)


def make_clear(ra, dec, r, extra=None):
    """Rows of (ra, dec) kept so that no pair lies between 0.999 r and 1.001 r: of every offending pair the later row is
    dropped.  Returns the indices kept (ascending).  ``extra``: a second radius to clear as well."""
    keep = np.ones(ra.size, bool)
    for radius in [r] + ([extra] if extra else []):
        for b0 in range(0, ra.size, 512):
            sep = separation(ra[b0:b0 + 512], dec[b0:b0 + 512], ra, dec)
            ii, jj = np.nonzero((sep > 0.999 * radius) & (sep < 1.001 * radius))
            for a, b in zip((ii + b0).tolist(), jj.tolist()):
                if a < b and keep[a] and keep[b]:
                    keep[b] = False
    return np.flatnonzero(keep)


def scene(seed, nclusters=40, members=(2, 6), spread=0.7, nnoise=60, box=(150.0, 20.0, 0.5), r=2.0, shuffle=True):
    """A field of ``nclusters`` tight clusters (members within ``spread`` arcsec of their centre) and ``nnoise`` loose
    points in a box (ra0, dec0, side in degrees), shuffled, with S/N and rb columns.  Guaranteed clear of the band
    around ``r`` (asserted by ``cluster_ref``)."""
    rng = np.random.default_rng(seed)
    ra0, dec0, side = box
    ras, decs = [], []
    for _ in range(nclusters):
        cr, cd = ra0 + rng.uniform(-side, side) / 2, dec0 + rng.uniform(-side, side) / 2
        k = int(rng.integers(members[0], members[1] + 1))
        a, d = offset(cr, cd, rng.uniform(-spread, spread, k), rng.uniform(-spread, spread, k))
        ras.append(a)
        decs.append(d)
    ras.append(np.mod(ra0 + rng.uniform(-side, side, nnoise) / 2, 360.0))
    decs.append(dec0 + rng.uniform(-side, side, nnoise) / 2)
    ra, dec = np.concatenate(ras), np.concatenate(decs)
    if shuffle:
        p = rng.permutation(ra.size)
        ra, dec = ra[p], dec[p]
    k = make_clear(ra, dec, r)
    ra, dec = ra[k], dec[k]
    snr = rng.uniform(5.0, 50.0, ra.size)
    rb = rng.uniform(0.0, 1.0, ra.size)
    return ra, dec, snr, rb


def sklearn_labels(ra, dec, r=2.0):
    """``DBSCAN(eps=r, min_samples=2, metric='precomputed')`` on the sparse matrix of separations within ``r``, as
    nersc/makesources.py:319-339 calls it.  The pairs come from ``cKDTree.query_pairs`` on unit vectors (the reference
    gets them from astropy's ``search_around_sky``, which is the same KD-tree query), the distances from ``separation``."""
    from scipy.sparse import csr_matrix
    from scipy.spatial import cKDTree
    from sklearn.cluster import DBSCAN
    ra, dec = np.asarray(ra, np.float64), np.asarray(dec, np.float64)
    a, d = np.radians(ra), np.radians(dec)
    xyz = np.stack([np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)], axis=1)
    pairs = cKDTree(xyz).query_pairs(2.0 * np.sin(np.radians(r / ARCSEC) / 2.0), output_type='ndarray')
    idx1 = np.concatenate([pairs[:, 0], pairs[:, 1]])
    idx2 = np.concatenate([pairs[:, 1], pairs[:, 0]])
    sep = np.array([separation(ra[i:i + 1], dec[i:i + 1], ra[j:j + 1], dec[j:j + 1])[0, 0] for i, j in zip(idx1, idx2)])
    distmat = csr_matrix((sep, (idx1, idx2)), shape=(ra.size, ra.size))
    clustering = DBSCAN(eps=r, min_samples=2, metric='precomputed')
    clustering.fit(distmat)
    return clustering.labels_.astype(np.int32)


# ---- cross-match scenes shared by tests/test_associate_gpu.py and tests/measure_assoc_tolerance.py -------------------
EPS64 = float(np.finfo(np.float64).eps)
ARCSEC_PER_RAD = 648000.0 / np.pi
# sep is held to SEP_K * eps64 radians of chord, in arcsec.  tests/measure_assoc_tolerance.py prints where SEP_K comes
# from (4 x the largest error, in eps64 radians, of an fp64 evaluation against an extended-precision one over exactly
# the scenes below); tests/test_associate_gpu.py derives why that is the right order from the roundings involved.
SEP_K = 16
SEP_TOL_ARCSEC = SEP_K * EPS64 * ARCSEC_PER_RAD


def xm_scene(name):
    """(ra, dec, cat_ra, cat_dec, radius_arcsec) of a cross-match scene: every query has either one catalogue entry
    well inside the radius or none within 1.001 of it (asserted by ``crossmatch_ref``)."""
    boxes = dict(field=(150.0, 20.0, 0.5), wrap=(0.0, 0.0, 0.05), ra90=(90.0, 60.0, 0.1), north=(10.0, 89.0, 0.2),
                 south=(300.0, -89.0, 0.2))
    seed = sorted(boxes).index(name) + 31
    rng = np.random.default_rng(seed)
    r = 1.5
    ra0, dec0, side = boxes[name]
    m = 150
    cra = np.mod(ra0 + rng.uniform(-side, side, m) / 2, 360.0)
    cdec = dec0 + rng.uniform(-side, side, m) / 2
    k = make_clear(cra, cdec, 8.0)                                   # ... and thin the catalogue: no two entries within 8 arcsec
    sep = separation(cra[k], cdec[k], cra[k], cdec[k]) + 1e9 * np.eye(k.size)
    k = k[sep.min(axis=1) > 8.0]
    cra, cdec = cra[k], cdec[k]
    rho = np.where(rng.uniform(size=cra.size) < 0.7, rng.uniform(0.0, 1.4, cra.size), rng.uniform(1.7, 3.0, cra.size))
    th = rng.uniform(0, 2 * np.pi, cra.size)
    ra, dec = offset(cra, cdec, rho * np.cos(th), rho * np.sin(th))
    ra, dec = np.concatenate([ra, cra[:5]]), np.concatenate([dec, cdec[:5]])          # five queries exactly on an entry
    p = rng.permutation(ra.size)
    return ra[p], dec[p], cra, cdec, r


# ---- a three-image toy night for ``source.associate`` (tests/test_source_host.py, tests/test_source_gpu.py) ------------
def toy_night(Detection, Source):
    """Detections of three images around one known source S0 and four spots A - D, and two stars:

    * S0 (100, 10) is known, with one earlier detection of S/N 10; d0 (S/N 30) and d5 (S/N 20) lie within 2 arcsec of it;
    * A: d1, d6, d10 (S/N 8, 12, 12: the tie goes to d6), all with rb > 0.4;
    * B: d2 has rb 0.3 (gated), d7 next to it has rb 0.9 and is left alone: no source;
    * C: d3, d8; a star 1.2 arcsec from d8 (the best): vetoed;     D: d4, d9; a star 1.8 arcsec from d9: kept;
    * d11 is isolated."""
    def det(image, ra0, dec0, dx, dy, snr, rb):
        ra, dec = offset(ra0, dec0, dx, dy)
        d = Detection(ra=float(ra), dec=float(dec), image=f'img{image}', flux=float(snr) * 2.0, fluxerr=2.0)
        d.rb = rb
        return d
    S0, A, B, C, D = (100.0, 10.0), (100.01, 10.0), (100.02, 10.01), (100.03, 9.99), (100.04, 10.02)
    dets = [det(0, *S0, 0.5, 0.0, 30.0, 0.9), det(0, *A, 0.0, 0.0, 8.0, 0.9), det(0, *B, 0.0, 0.0, 5.0, 0.3),
            det(0, *C, 0.0, 0.0, 6.0, 0.8), det(0, *D, 0.0, 0.0, 7.0, 0.7),
            det(1, *S0, 0.0, 0.3, 20.0, 0.6), det(1, *A, 0.4, 0.0, 12.0, 0.5), det(1, *B, 0.2, 0.0, 9.0, 0.9),
            det(1, *C, 0.3, 0.0, 16.0, 0.75), det(1, *D, 0.0, 0.3, 17.0, 0.625),
            det(2, *A, 0.2, 0.2, 12.0, 0.75), det(2, 100.2, 10.2, 0.0, 0.0, 40.0, 0.99)]
    earlier = det(-1, *S0, 0.0, 0.0, 10.0, 0.9)
    s0 = Source(id='known0', ra=S0[0], dec=S0[1], detections=[earlier], score=0.9)
    earlier.source = s0
    sra, sdec = zip(offset(dets[8].ra, dets[8].dec, 0.0, 1.2), offset(dets[9].ra, dets[9].dec, 1.8, 0.0))
    return dets, [s0], (np.array(sra, np.float64), np.array(sdec, np.float64))


def check_toy_night(dets, out, names):
    """What ``associate`` must have made of ``toy_night`` (``names``: the calls the naming hook received)."""
    s0, a, c, d = out
    assert len(out) == 4 and names == [1, 2, 3]
    assert s0.id == 'known0' and [x.image for x in s0.detections] == ['img-1', 'img0', 'img1']
    assert (s0.ra, s0.dec) == (dets[0].ra, dets[0].dec) and s0.best_detection is dets[0]       # moved to the S/N 30 detection
    assert dets[0].source is s0 and dets[5].source is s0
    assert a.detections == [dets[1], dets[6], dets[10]] and a.best_detection is dets[6]         # the tie: the first of equals
    assert (a.id, a.ra, a.dec) == ('n1', dets[6].ra, dets[6].dec) and a.score == (0.9 + 0.5) + 0.75 and a.altdata is None
    assert dets[2].source is None and dets[7].source is None and dets[11].source is None        # the gate; alone; isolated
    assert c.detections == [dets[3], dets[8]] and c.best_detection is dets[8] and c.score == -1.0
    assert 'rejected' in c.altdata and 'star 0' in c.altdata['rejected'] and c.rejected
    assert d.detections == [dets[4], dets[9]] and d.best_detection is dets[9] and d.score == 0.7 + 0.625
    assert d.altdata is None and not d.rejected and (d.id, c.id) == ('n3', 'n2')
    for s in out:
        assert all(x.source is s for x in s.detections)
