"""Record tests/golden/back_cols_parent.json: the digests that tests/test_back_substitution_gpu.py compares with.

Run on a GPU from a checkout and build of the commit BEFORE the rewrite of chol_back_cols_body (with this script and the
test module copied in), twice, in two processes:

    python tests/golden/make_back_cols_golden.py a.json && python tests/golden/make_back_cols_golden.py b.json

and keep a.json only where ``cmp a.json b.json`` finds no difference: a scene whose two recordings differ is not
deterministic in that build and has no place in the fixture.  The pool scene is recorded from one job at a time
(``SubtractionPool(1)``); the batch of two must give the same digests in the recording build as well.

``--oracle`` (no GPU): every scene through oracle/hotpants.py first - each region must solve, with the unknowns the
scene is listed for; a scene that does not is taken out of the list, not recorded as a failure.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_back_substitution_gpu as t   # noqa: E402


def oracle_check():
    from oracle import hotpants as ohp
    for name in sorted(t.SCENES):
        make, kw, nunk = t.SCENES[name]
        sci, srms, ref, rrms, bpm = make()
        _, _, info = ohp.subtract(sci, ref, srms, rrms, bpm, **kw)
        regs = info['regions']
        print(name, [None if r is None else (r['niter'], r['nstamps_total'], r['nstamps_used']) for r in regs], flush=True)
        assert all(r is not None for r in regs), name
        nkp = (kw['ko'] + 1) * (kw['ko'] + 2) // 2
        assert all(r['nstamps_used'] >= nkp for r in regs), name
        if name == 'rejected-2x2':
            assert max(r['niter'] for r in regs) >= 2 and len({r['niter'] for r in regs}) > 1


def main(out):
    import zuds_amd
    engine = zuds_amd.get_engine(0)
    rec = {}
    for name in sorted(t.SCENES):
        data, kw, (d, n, info) = t.run_scene(engine, name)
        rec[name] = t.record(d, n, info)
        print(name, 'status', info['status'], 'niter', info['niter'], 'stamps', info['nstamps_used'], '/',
              info['nstamps_total'], 'ncoeff', info['ncoeff'], flush=True)
        assert info['status'] == 0 and info['ncoeff'] == t.SCENES[name][2], name
    assert int(rec['rejected-2x2']['info']['niter']) >= 2
    rec[t.POOL] = t.run_pool(0)
    assert t.run_pool(2) == rec[t.POOL], 'the batch of two differs from one job at a time in this build'
    print(t.POOL, [(r['info']['status'], r['info']['niter'], r['info']['nstamps_used'], r['info']['ncoeff'])
                   for r in rec[t.POOL]])
    assert all(r['info']['status'] == 0 and r['info']['nstamps_used'] > 0 for r in rec[t.POOL])
    with open(out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    if sys.argv[1] == '--oracle':
        oracle_check()
    else:
        main(sys.argv[1])
