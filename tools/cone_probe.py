"""Cone searches at the scale of a field catalogue: 10^6 and 10^7 rows scattered uniformly over one ZTF field (7 x 7
degrees: 5 and 50 rows per 30 arcsec circle, the density range of PS1), queried at 10^3 and 10^5 uniform positions.
Event times (the library's own timers around its launches, median of 5) of

* the index build (``zm_skyindex_create_dev``), once per catalogue,
* ``knn`` with k = 3 at 30 arcsec and ``within`` at 1.5 arcsec on the resident index, and
* the only route there was before the index: ``zm_crossmatch_dev`` on the same inputs at both radii, which returns one
  neighbour and rebuilds its cell table on every call.

Each (rows, queries) step runs in a child process under its own ``timeout``; the first step that fails stops the rest.
Writes one JSON document (default profiles/cone_probe.json).

usage: cone_probe.py [--rows 1000000 10000000] [--queries 1000 100000] [--out profiles/cone_probe.json] [--limit 240]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELD = (180.0, 30.0, 7.0)            # centre and side of the footprint, degrees
REPEATS = 5


def scatter(n, seed):
    rng = np.random.default_rng(seed)
    ra0, dec0, side = FIELD
    lo, hi = np.sin(np.radians(dec0 - side / 2)), np.sin(np.radians(dec0 + side / 2))
    width = side / np.cos(np.radians(dec0))
    return ra0 + rng.uniform(-width / 2, width / 2, n), np.degrees(np.arcsin(rng.uniform(lo, hi, n)))


def step(m, n):
    import torch
    z = importlib.import_module('zuds-pipeline_amd')
    xm = importlib.import_module('zuds-pipeline_amd.crossmatch')
    eng = z.get_engine(0)
    L, check = eng.L, z._lib.check
    cra, cdec = (torch.from_numpy(v).cuda() for v in scatter(m, 1))
    ra, dec = (torch.from_numpy(v).cuda() for v in scatter(n, 2))
    torch.cuda.synchronize()
    check(L.zm_timing_enable(eng.ctx, 1))

    def timed(scope, fn):
        out, times = None, []
        for k in range(REPEATS + 1):                      # the first call warms up: scratch allocation, code load
            check(L.zm_timing_reset(eng.ctx))
            out = fn()
            eng.synchronize()
            ms, cnt = C.c_double(), C.c_int64()
            check(L.zm_timing_read(eng.ctx, scope.encode(), C.byref(ms), C.byref(cnt)))
            if k:
                times.append(ms.value)
        return out, dict(ms=times, median_ms=float(np.median(times)))

    doc = dict(rows=m, queries=n)
    made = []

    def build():
        for ix in made:
            ix.close()
        made[:] = [xm.SkyIndex(cra, cdec, 30.0, engine=eng)]
        return made[0]
    ix, doc['index_build'] = timed('skyindex_build', build)
    doc['index'] = ix.stats()
    (idx, sep, count), doc['knn_k3_30arcsec'] = timed('cone_knn', lambda: ix.knn_dev(ra, dec, 30.0, 3))
    doc['knn_k3_30arcsec']['mean_rows_in_range'] = float(count.double().mean().cpu())
    cap = max(n, 1024)
    (off, cat_idx, npairs), doc['within_1.5arcsec'] = timed('cone_within', lambda: ix.within_dev(ra, dec, 1.5, capacity=cap))
    doc['within_1.5arcsec']['pairs'] = npairs
    for r in (30.0, 1.5):
        (xi, xs), t = timed('crossmatch', lambda: z.crossmatch_dev(ra, dec, cra, cdec, r, engine=eng))
        doc[f'crossmatch_dev_{r:g}arcsec'] = t
        if r == 30.0:                                     # k = 1 of the index is this route's answer
            doc['nearest_agrees_with_crossmatch_dev'] = bool(torch.equal(xi, idx[:, 0]))
    ix.close()
    print(json.dumps(doc))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[1000000, 10000000])
    ap.add_argument('--queries', type=int, nargs='+', default=[1000, 100000])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cone_probe.json'))
    ap.add_argument('--limit', type=int, default=240, help='seconds a step may take')
    ap.add_argument('--step', type=int, nargs=2, metavar=('ROWS', 'QUERIES'), help='run one step in this process')
    args = ap.parse_args(argv)
    if args.step:
        return step(*args.step)
    doc = dict(field_deg=FIELD, repeats=REPEATS, steps=[])
    for m in args.rows:
        for n in args.queries:
            r = subprocess.run(['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--step', str(m), str(n)],
                               capture_output=True, text=True)
            if r.returncode != 0:                         # a failure stops the rest: nothing more is started on the device
                doc['stopped'] = dict(rows=m, queries=n, returncode=r.returncode, stderr=r.stderr[-2000:])
                break
            doc['steps'].append(json.loads(r.stdout.strip().splitlines()[-1]))
        if 'stopped' in doc:
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps(doc))
    return 1 if 'stopped' in doc else 0


if __name__ == '__main__':
    sys.exit(main())
