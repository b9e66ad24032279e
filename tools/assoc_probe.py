"""Source association at the scale of a night: 10^6 synthetic detections - 10^5 sources of 2 .. 14 detections within
0.7 arcsec of their centre, plus uniform noise, over a ZTF night's footprint (a 60 x 60 degree cap) - through
``zm_associate_dev`` (end to end and per stage) and, on the same box, through ``scipy.spatial.cKDTree.query_pairs`` +
``scipy.sparse.csgraph.connected_components``.  Writes one JSON document (default profiles/assoc_probe.json).

usage: assoc_probe.py [--n 1000000] [--sources 100000] [--out profiles/assoc_probe.json] [--no-cpu]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(n, nsrc, seed=1):
    rng = np.random.default_rng(seed)
    cra = rng.uniform(150.0, 210.0, nsrc)
    cdec = np.degrees(np.arcsin(rng.uniform(np.sin(np.radians(0.0)), np.sin(np.radians(60.0)), nsrc)))
    k = rng.integers(2, 15, nsrc)
    k = (k * (0.8 * n / k.sum())).astype(np.int64).clip(2)
    own = np.repeat(np.arange(nsrc), k)
    dx, dy = rng.uniform(-0.7, 0.7, own.size) / 3600.0, rng.uniform(-0.7, 0.7, own.size) / 3600.0
    ra = np.concatenate([cra[own] + dx / np.cos(np.radians(cdec[own])), rng.uniform(150.0, 210.0, max(n - own.size, 0))])
    dec = np.concatenate([cdec[own] + dy, np.degrees(np.arcsin(rng.uniform(0.0, np.sin(np.radians(60.0)), max(n - own.size, 0))))])
    p = rng.permutation(ra.size)[:n]
    return ra[p], dec[p], rng.uniform(5, 50, p.size), rng.uniform(0, 1, p.size)


def cpu_route(ra, dec, r):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    a, d = np.radians(ra), np.radians(dec)
    xyz = np.stack([np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)], axis=1)
    pairs = cKDTree(xyz).query_pairs(2.0 * np.sin(np.radians(r / 3600.0) / 2.0), output_type='ndarray')
    t1 = time.perf_counter()
    g = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(ra.size, ra.size))
    ncomp, lab = connected_components(g, directed=False)
    t2 = time.perf_counter()
    sizes = np.bincount(lab)
    return dict(kdtree_pairs_ms=1e3 * (t1 - t0), components_ms=1e3 * (t2 - t1), total_ms=1e3 * (t2 - t0),
                npairs=int(len(pairs)), nsrc=int((sizes > 1).sum())), lab, sizes


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--sources', type=int, default=100000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'assoc_probe.json'))
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args(argv)
    import torch
    z = importlib.import_module('zuds-pipeline_amd')
    eng = z.get_engine(0)
    ra, dec, snr, rb = scene(args.n, args.sources)
    doc = dict(n=int(ra.size), sources_planted=args.sources, radius_arcsec=2.0)
    dev = [torch.from_numpy(v).cuda() for v in (ra, dec, snr, rb)]
    torch.cuda.synchronize()
    z.cluster_dev(*dev, 2.0, engine=eng)                        # warm-up: scratch allocation, code load
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = z.cluster_dev(*dev, 2.0, engine=eng)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    st = z.assoc_stats(eng)
    nsrc = int(out['nsrc'].cpu()[0])
    doc['gpu'] = dict(device_resident_ms=times, device_resident_median_ms=float(np.median(times)), nsrc=nsrc, **st,
                      mean_probe=st['probes'] / max(1, int(np.isfinite(ra).sum())))
    t0 = time.perf_counter()
    host = z.cluster(ra, dec, snr, rb, 2.0, engine=eng)
    doc['gpu']['from_host_arrays_ms'] = 1e3 * (time.perf_counter() - t0)
    # per stage: the library's own event timers around its launches
    C = importlib.import_module('ctypes')
    z._lib.check(eng.L.zm_timing_reset(eng.ctx))
    z._lib.check(eng.L.zm_timing_enable(eng.ctx, 1))
    z.cluster_dev(*dev, 2.0, engine=eng)
    torch.cuda.synchronize()
    stages = {}
    for name in ('as_build', 'as_rounds', 'as_compact'):
        ms, cnt = C.c_double(), C.c_int64()
        z._lib.check(eng.L.zm_timing_read(eng.ctx, name.encode(), C.byref(ms), C.byref(cnt)))
        stages[name + '_ms'] = ms.value
    z._lib.check(eng.L.zm_timing_enable(eng.ctx, 0))
    doc['gpu']['stages'] = stages
    if not args.no_cpu:
        cpu, lab, sizes = cpu_route(ra, dec, 2.0)
        doc['cpu'] = cpu
        same = (host['label'] >= 0) == (sizes[lab] > 1)
        doc['agree'] = bool(same.all() and cpu['nsrc'] == host['nsrc'])
        doc['gpu_over_cpu_speedup'] = cpu['total_ms'] / doc['gpu']['from_host_arrays_ms']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
