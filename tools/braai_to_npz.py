#!/usr/bin/env python3
"""Convert the weights of a braai model from Keras' HDF5 file to the .npz that ``realbogus.load_model`` reads.

    python3 tools/braai_to_npz.py BASE          # BASE.weights.h5 -> BASE.weights.npz

Needs h5py, which is neither a dependency of this package nor installed where the package is built and tested: this
script has never been run there.  It is for a site that has the reference's ``ml/`` files and h5py.  It writes the arrays
of ``model.get_weights()`` in order (``arr_0``, ``arr_1``, ...: per layer of the file's ``layer_names`` attribute its
``weight_names``, kernel before bias) and checks them against ``BASE.architecture.json`` when that file is there.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv):
    if len(argv) != 1:
        print(__doc__, file=sys.stderr)
        return 2
    base = argv[0]
    import importlib
    rb = importlib.import_module('zuds-pipeline_amd.realbogus')
    weights = rb._weights_from_h5(base + '.weights.h5')
    if os.path.exists(base + '.architecture.json'):
        with open(base + '.architecture.json') as f:
            rb.check_weights(rb.parse_architecture(f.read()), weights)
    np.savez(base + '.weights.npz', *[np.asarray(w, dtype=np.float32) for w in weights])
    print(f'{base}.weights.npz: {len(weights)} arrays, {sum(w.size for w in weights)} values')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
