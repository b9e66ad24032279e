"""tests/cone_ref.py against a method that does not share its formula: ``scipy.spatial.cKDTree`` on unit vectors,
``query_ball_point`` at the chord of the radius, then a sort by chord.  The restatement works on coordinate differences
(haversine) and brute force; the tree on Cartesian vectors.  Run on the scenes the GPU tests use - which also proves that
every scene satisfies the restatement's two preconditions (they are asserted inside ``knn_ref`` / ``within_ref``)."""
import numpy as np
import pytest

import assoc_ref as ar
import cone_ref as cr

RADII = (cr.R_KNN, cr.R_NAME)


def unit(ra, dec):
    a, d = np.radians(ra), np.radians(dec)
    return np.stack([np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)], axis=1)


def tree_search(ra, dec, cra, cdec, r):
    """Per query the catalogue rows within r, ordered by (chord, row), and their chords."""
    from scipy.spatial import cKDTree
    ok = np.flatnonzero(np.isfinite(cra) & np.isfinite(cdec))
    out = [(np.zeros(0, np.int64), np.zeros(0)) for _ in range(ra.size)]
    if ok.size == 0:
        return out
    cv = unit(cra[ok], cdec[ok])
    tree = cKDTree(cv)
    chord = 2.0 * np.sin(np.radians(r / ar.ARCSEC) / 2.0)
    for i in np.flatnonzero(np.isfinite(ra) & np.isfinite(dec)).tolist():
        q = unit(ra[i:i + 1], dec[i:i + 1])[0]
        rows = np.array(sorted(tree.query_ball_point(q, chord)), dtype=np.int64)
        d = np.sqrt(((cv[rows] - q) ** 2).sum(axis=1)) if rows.size else np.zeros(0)
        o = np.lexsort((ok[rows], d))
        out[i] = (ok[rows][o], d[o])
    return out


@pytest.mark.parametrize('name', cr.SCENES)
def test_restatement_agrees_with_a_kd_tree(name):
    ra, dec, cra, cdec = cr.scene(name)
    assert ra.size <= 400 and cra.size <= 4000
    for r in RADII:
        found = tree_search(ra, dec, cra, cdec, r)
        for k in (1, 3, 8):
            idx, sep, count = cr.knn_ref(ra, dec, cra, cdec, r, k, what=f'{name} at {r}')
            for i, (rows, chord) in enumerate(found):
                assert count[i] == rows.size, (name, r, i)
                # exact duplicates are as far by either formula up to rounding: compare as sets within a run of equal rows
                want = rows[:k]
                assert sorted(idx[i][idx[i] >= 0].tolist()) == sorted(want.tolist()), (name, r, k, i)
                got_sep = sep[i][:want.size]
                tree_sep = 2.0 * np.arcsin(np.minimum(1.0, chord[:k] / 2.0)) * ar.ARCSEC_PER_RAD
                assert np.abs(np.sort(got_sep) - tree_sep).max(initial=0.0) <= ar.SEP_TOL_ARCSEC, (name, r, k, i)
                assert (idx[i][want.size:] == -1).all() and np.isnan(sep[i][want.size:]).all()
                # ... and the restatement's own order: ascending separation, equal positions in row order
                assert (np.diff(got_sep) >= 0).all()
                for a, b, sa, sb in zip(idx[i][:-1], idx[i][1:], sep[i][:-1], sep[i][1:]):
                    if b >= 0 and sa == sb:
                        assert a < b
        offsets, cat_idx = cr.within_ref(ra, dec, cra, cdec, r, what=f'{name} at {r}')
        assert offsets.size == ra.size + 1 and offsets[-1] == cat_idx.size
        for i, (rows, _) in enumerate(found):
            assert np.array_equal(cat_idx[offsets[i]:offsets[i + 1]], np.sort(rows)), (name, r, i)


def test_the_scenes_hold_what_they_are_built_for():
    ra, dec, cra, cdec = cr.scene('counts')
    _, _, count = cr.knn_ref(ra, dec, cra, cdec, cr.R_KNN, 8)
    assert sorted(set(count.tolist())) == list(range(13)) + [40]                 # 0, 1, k - 1, k, k + 1 for every k <= 8, many
    ra, dec, cra, cdec = cr.scene('duplicates')
    idx, sep, count = cr.knn_ref(ra, dec, cra, cdec, cr.R_KNN, 8)
    assert idx[0][:4].tolist() == [0, 2, 5, 7] and idx[1][:6].tolist() == [1, 4, 6, 8, 9, 11] and (sep[1][:5] == 0.0).all()
    for name, size in (('wave65', 65), ('wave300', 300)):
        ra, dec, cra, cdec = cr.scene(name)
        _, _, count = cr.knn_ref(ra, dec, cra, cdec, cr.R_KNN, 1)
        assert count[0] >= size - 5 and count[0] > 64                            # (clearing may drop a few rows)
    ra, dec, cra, cdec = cr.scene('cells')
    edge = 2.0 * np.sin(np.radians(cr.R_KNN / ar.ARCSEC) / 2.0) * (1 + 1e-6)
    offsets, cat_idx = cr.within_ref(ra, dec, cra, cdec, cr.R_KNN)
    spread = [len({tuple(c) for c in np.floor(unit(cra[cat_idx[a:b]], cdec[cat_idx[a:b]]) / edge).astype(np.int64).tolist()})
              for a, b in zip(offsets[:-1], offsets[1:])]
    assert min(spread) >= 2 and max(spread) >= 4                                 # matches in several of the 27 cells
    ra, dec, cra, cdec = cr.scene('nonfinite')
    assert (~np.isfinite(ra) | ~np.isfinite(dec)).sum() == 4 and (~np.isfinite(cra) | ~np.isfinite(cdec)).sum() == 4
    for name, sign in (('north', 1.0), ('south', -1.0)):
        ra, dec, cra, cdec = cr.scene(name)
        assert (cdec == sign * 90.0).any() and (dec == sign * 90.0).any()


def test_clearing_drops_rows_not_comparisons():
    rng = np.random.default_rng(3)
    ra, dec = np.array([50.0]), np.array([5.0])
    rho = np.array([29.99, 10.0, 10.0 + 1e-9, 1.5004, 12.0])                     # in the band of 30; a near tie; in the band of 1.5
    cra, cdec = ar.offset(50.0, 5.0, rho, np.zeros(5))
    keep = cr.clear_catalog(ra, dec, cra, cdec, (30.0, 1.5))
    assert keep.tolist() == [1, 4]
    with pytest.raises(AssertionError):
        cr.knn_ref(ra, dec, cra, cdec, 30.0, 3)
    idx, _, count = cr.knn_ref(ra, dec, cra[keep], cdec[keep], 30.0, 3)
    assert idx.tolist() == [[0, 1, -1]] and count.tolist() == [2]
