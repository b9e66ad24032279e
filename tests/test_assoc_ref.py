"""tests/assoc_ref.py (the numpy restatement every association test compares with) against sklearn's DBSCAN called as
the reference calls it, and against labels sklearn gave when tests/golden/assoc_dbscan.json was written."""
import json
import os

import numpy as np
import pytest

import assoc_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'assoc_dbscan.json')


def fields():
    out = [assoc_ref.scene(1), assoc_ref.scene(2, box=(0.0, 0.0, 0.05), nclusters=30, nnoise=30),
           assoc_ref.scene(3, box=(123.0, -89.0, 0.2), nclusters=8, nnoise=8)]
    # exact duplicates and a chain whose ends are far apart
    ra, dec, snr, rb = assoc_ref.scene(4, nclusters=10, nnoise=10)
    cra, cdec = assoc_ref.offset(151.0, 21.0, 1.5 * np.arange(40), np.zeros(40))
    ra, dec = np.concatenate([ra, ra[:5], cra]), np.concatenate([dec, dec[:5], cdec])
    k = assoc_ref.make_clear(ra, dec, 2.0)
    out.append((ra[k], dec[k], np.linspace(5, 50, k.size), np.full(k.size, 0.5)))
    return out


@pytest.mark.parametrize('k', range(4))
def test_restatement_labels_as_sklearn_dbscan_does(k):
    pytest.importorskip('sklearn')
    pytest.importorskip('scipy')
    ra, dec, snr, rb = fields()[k]
    want = assoc_ref.sklearn_labels(ra, dec, 2.0)
    got = assoc_ref.cluster_ref(ra, dec, snr, rb, 2.0)
    assert want.max() >= 5 and (want < 0).any()
    assert np.array_equal(got['label'], want)
    assert got['nsrc'] == want.max() + 1
    for s in range(got['nsrc']):
        m = got['members'][got['offsets'][s]:got['offsets'][s + 1]]
        assert np.array_equal(m, np.flatnonzero(want == s)) and got['count'][s] == m.size
        assert got['best'][s] == m[np.argmax(snr[m])]


def test_restatement_matches_the_stored_sklearn_labels():
    with open(GOLDEN) as f:
        g = json.load(f)
    ra, dec, want = np.array(g['ra']), np.array(g['dec']), np.array(g['labels'], dtype=np.int32)
    assert 250 <= ra.size <= 400 and want.max() >= 40 and (want < 0).sum() >= 20
    got = assoc_ref.cluster_ref(ra, dec, np.ones(ra.size), None, g['radius_arcsec'])
    assert np.array_equal(got['label'], want)
    assert np.bincount(want[want >= 0]).max() >= 20               # the chain is one source


def test_crossmatch_restatement_rules():
    cra, cdec = np.array([10.0, 10.0, 10.0, 200.0]), np.array([1.0 / 3600, -1.0 / 3600, 1.0 / 3600, 5.0])
    idx, sep = assoc_ref.crossmatch_ref([10.0, 10.0, np.nan, 200.0], [0.0, 0.5, 0.0, 5.0 + 1.8 / 3600], cra, cdec, 1.5)
    assert list(idx) == [0, -1, -1, -1] and abs(sep[0] - 1.0) < 1e-9 and np.isnan(sep[1:]).all()
    idx, sep = assoc_ref.crossmatch_ref([200.0], [5.0 + 1.8 / 3600], cra, cdec, 2.0)
    assert list(idx) == [3] and abs(sep[0] - 1.8) < 1e-9
