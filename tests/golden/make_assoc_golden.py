"""Writes tests/golden/assoc_dbscan.json: about 300 positions and the labels sklearn's DBSCAN gives them when it is
called as the reference calls it (tests/assoc_ref.py: sklearn_labels).  Run from the repository root at a site that has
scikit-learn and scipy:  python tests/golden/make_assoc_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import assoc_ref  # noqa: E402


def build():
    # three fields: mid-latitude, across RA 0 / 360, near the north pole; tight clusters, a chain, noise
    parts = [assoc_ref.scene(11, nclusters=30, nnoise=40, box=(150.0, 20.0, 0.2)),
             assoc_ref.scene(12, nclusters=20, nnoise=20, box=(0.0, -5.0, 0.05)),
             assoc_ref.scene(13, nclusters=10, nnoise=10, box=(40.0, 89.99, 0.01))]
    ra = np.concatenate([p[0] for p in parts])
    dec = np.concatenate([p[1] for p in parts])
    cra, cdec = assoc_ref.offset(200.0, 45.0, 1.5 * np.arange(25), np.zeros(25))      # a chain at 1.5 arcsec spacing
    ra, dec = np.concatenate([ra, cra]), np.concatenate([dec, cdec])
    p = np.random.default_rng(14).permutation(ra.size)
    ra, dec = ra[p], dec[p]
    k = assoc_ref.make_clear(ra, dec, 2.0)
    return ra[k], dec[k]


if __name__ == '__main__':
    import sklearn
    ra, dec = build()
    labels = assoc_ref.sklearn_labels(ra, dec, 2.0)
    out = dict(radius_arcsec=2.0, sklearn=sklearn.__version__, ra=ra.tolist(), dec=dec.tolist(), labels=labels.tolist())
    path = os.path.join(HERE, 'assoc_dbscan.json')
    with open(path, 'w') as f:
        json.dump(out, f)
    print(path, ra.size, 'points,', int(labels.max()) + 1, 'clusters,', int((labels < 0).sum()), 'noise')
