"""Record tests/golden/fit_vectors_parent.json: the digests that tests/test_fit_vectors_gram_gpu.py compares with.

Run on a GPU from a checkout and build of the commit BEFORE the rewrite of k_hp_vectors / k_hp_gram (with this script
and the test module copied in), twice, in two processes:

    python tests/golden/make_fit_vectors_golden.py a.json && python tests/golden/make_fit_vectors_golden.py b.json

and keep a.json only where ``cmp a.json b.json`` finds no difference: a scene whose two recordings differ is not
deterministic in that build and has no place in the fixture.  The pool scene is recorded from one job at a time
(``SubtractionPool(1)``); the batch of two must give the same digests in the recording build as well.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_fit_vectors_gram_gpu as t   # noqa: E402
import zuds_amd                          # noqa: E402


def main(out):
    engine = zuds_amd.get_engine(0)
    rec = {}
    for name in sorted(t.SCENES):
        data, kw, (d, n, info) = t.run_scene(engine, name)
        rec[name] = t.record(d, n, info)
        print(name, 'status', info['status'], 'niter', info['niter'], 'stamps', info['nstamps_used'], '/',
              info['nstamps_total'], 'ncoeff', info['ncoeff'], flush=True)
    assert int(rec['rejected-2x2']['info']['niter']) >= 2
    rec[t.POOL] = t.run_pool(0)
    assert t.run_pool(2) == rec[t.POOL], 'the batch of two differs from one job at a time in this build'
    print(t.POOL, [(r['info']['status'], r['info']['niter'], r['info']['nstamps_used']) for r in rec[t.POOL]])
    assert all(r['info']['status'] == 0 and r['info']['nstamps_used'] > 0 for r in rec[t.POOL])
    with open(out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main(sys.argv[1])
