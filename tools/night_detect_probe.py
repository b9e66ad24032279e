#!/usr/bin/env python3
"""Developer probe: what detections cost in the nightly pool.

    python3 tools/night_detect_probe.py [--size NX NY] [--jobs N] [--reps R] [--out profiles/night_detect_probe.json]

On one resident subtraction it times ``filterobjects.pixel_cuts_dev`` (``zm_candidate_cuts_dev``: planes in HBM)
against the host-pointer ``pixel_cuts`` on host copies of the same planes and positions - the route every detection
took before, so the yardstick.  Then the pool's milliseconds per subtraction with ``detect`` off, on, and on with
stamps, on the same jobs in the same session; the cost of detection is stated as a fraction of the first of these.
Prints one JSON line and, with ``--out``, writes it.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, nargs=2, default=(3072, 3080), metavar=('NX', 'NY'))
    ap.add_argument('--jobs', type=int, default=12, help='subtractions per pool run')
    ap.add_argument('--frames', type=int, default=3, help='distinct science frames (reused across the jobs)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--lanes', type=int, default=3)
    ap.add_argument('--fit-batch', type=int, default=4)
    ap.add_argument('--flat-rms', action='store_true',
                    help='constant rms maps: the noise plane is then flat too, and the exact select of its median takes its '
                         'one-workgroup rescue (milliseconds) on either route')
    ap.add_argument('--out')
    args = ap.parse_args(argv)
    nm = importlib.import_module('zuds-pipeline_amd.nightly')          # (first: it sizes the hardware queues)
    import torch
    z = importlib.import_module('zuds-pipeline_amd')
    s = importlib.import_module('zuds-pipeline_amd.synth')
    devmod = importlib.import_module('zuds-pipeline_amd.device')
    nx, ny = args.size
    base = s.ztf_wcs(nx, ny, tpv=True)
    rng = np.random.default_rng(5)
    nst = int(nx * ny / 2500)
    fl = np.exp(rng.uniform(np.log(3e3), np.log(8e4), nst))
    ra, dec = base.all_pix2world(rng.uniform(-10, nx + 10, nst), rng.uniform(-10, ny + 10, nst), 0)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to('cuda:0')
    rf = s.make_frame(nx, ny, 50, base, star_sky=(ra, dec, fl), fwhm=2.0, noise=1.0, nbad=200)
    def rms_map(level, seed):
        # per-pixel scatter of a few per cent, as a map made from a weight image has it
        if args.flat_rms:
            return np.full((ny, nx), level, np.float32)
        return (level * (1.0 + 0.03 * np.random.default_rng(seed).standard_normal((ny, nx), dtype=np.float32))).astype(np.float32)
    ref = dict(img=dev(rf['img'], np.float32), rms=dev(rms_map(1.0, 90), np.float32), mask=dev(rf['mask'], np.int32),
               wcs=base, flxscale=1.0)
    pra, pdec = base.all_pix2world(rng.uniform(20, nx - 20, 100), rng.uniform(20, ny - 20, 100), 0)
    scis = []
    for i in range(args.frames):
        w = s.ztf_wcs(nx, ny, dx=rng.uniform(-6, 6), dy=rng.uniform(-6, 6), rot_deg=rng.uniform(-0.05, 0.05))
        tra, tdec = w.all_pix2world(rng.uniform(100, nx - 100, 20), rng.uniform(100, ny - 100, 20), 0)
        f = s.make_frame(nx, ny, 51 + i, w, star_sky=(np.concatenate([ra, tra]), np.concatenate([dec, tdec]),
                                                     np.concatenate([fl, np.full(20, 6e3)])), fwhm=2.4, sky=180.0, nbad=300)
        scis.append(dict(img=dev(f['img'], np.float32), rms=dev(rms_map(5.0, 91 + i), np.float32),
                         mask=dev(f['mask'], np.int32), wgt=dev(f['wgt'], np.float32), wcs=w, seeing=2.4))

    def jobs(**kw):
        return [nm.SubtractionJob(scis[k % len(scis)], ref, radec=(pra, pdec), tag=k, **kw) for k in range(args.jobs)]
    out = dict(flat_rms=bool(args.flat_rms), size=[nx, ny], jobs=args.jobs, lanes=args.lanes, fit_batch=args.fit_batch, reps=args.reps,
               device=torch.cuda.get_device_name(0))

    # 1. the cuts on one resident subtraction: device planes against the host-pointer route
    eng = z.Engine(0)
    ch = devmod.DeviceSubtraction(scis[0]['wcs'], base, engine=eng)
    sc = scis[0]
    ch.run(sc['img'], sc['rms'], sc['mask'], sc['wgt'], ref['img'], ref['rms'], ref['mask'], seeing=2.4)
    tab, nfound, _ = ch.extract()
    tab = tab[((tab['IMAFLAGS_ISO'] & z.BAD_SUM) == 0) & (tab['FLAGS_WEIGHT'] == 0)]
    x, y = np.asarray(tab['X_IMAGE'], dtype=np.float64), np.asarray(tab['Y_IMAGE'], dtype=np.float64)
    ch.stream.synchronize()
    h_img, h_rms, h_mask = (t.cpu().numpy() for t in (ch.diff, ch.noise, ch.submask))
    h_bpm = (h_mask & z.BAD_SUM) != 0

    def clock(fn):
        fn()
        ts = []
        for _ in range(max(args.reps, 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return ts
    eng.set_stream(ch.stream.cuda_stream)
    with torch.cuda.stream(ch.stream):
        t_dev = clock(lambda: z.pixel_cuts_dev(eng, ch.diff, ch.noise, ch.submask, x, y))
        t_ext = clock(lambda: ch.extract())
        t_cand = clock(lambda: ch.candidates(2.4))
    t_host = clock(lambda: z.pixel_cuts(h_img, h_rms, h_bpm, x, y, engine=eng))
    a = z.pixel_cuts_dev(eng, ch.diff, ch.noise, ch.submask, x, y)
    b = z.pixel_cuts(h_img, h_rms, h_bpm, x, y, engine=eng)
    out['cuts'] = dict(candidates=int(x.size), objects_found=int(nfound),
                       pixel_cuts_dev_ms=[round(t, 3) for t in t_dev], pixel_cuts_host_ms=[round(t, 3) for t in t_host],
                       extract_ms=[round(t, 3) for t in t_ext], candidates_ms=[round(t, 3) for t in t_cand],
                       same_decisions=bool(np.array_equal(a['GOODCUT'], b['GOODCUT']) and np.array_equal(a['NEGPIX'], b['NEGPIX'])),
                       max_abs_bpmcut_diff=float(np.abs(a['BPMCUT'] - b['BPMCUT']).max()) if x.size else 0.0,
                       max_abs_rmscut_diff=float(np.abs(a['RMSCUT'] - b['RMSCUT']).max()) if x.size else 0.0)
    del ch
    eng.close()

    # 2. the pool, same jobs, same session: detect off / on / on with stamps
    pool = nm.SubtractionPool(args.lanes, batch=args.fit_batch)
    rows = {}
    for name, kw in (('off', {}), ('detect', dict(detect=True)), ('detect_stamps', dict(detect=True, stamps=True)),
                     ('off_again', {})):
        js = jobs(**kw)
        pool.map(js, keep=False)                                   # warm: planes, scratch, plans
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pool.map(js, keep=False)
            ts.append(1e3 * (time.perf_counter() - t0) / len(js))
        rows[name] = dict(ms_per_subtraction=[round(t, 4) for t in ts], best=round(min(ts), 4))
        if kw:
            rows[name]['good_rows'] = [int((r['cat']['GOODCUT'] == 1).sum()) for r in res[:len(scis)]]
            rows[name]['rows'] = [int(len(r['cat'])) for r in res[:len(scis)]]
            rows[name]['too_many'] = int(sum(bool(r.get('too_many')) for r in res))
    pool.close()
    base_ms = min(rows['off']['best'], rows['off_again']['best'])
    out['pool'] = rows
    out['pool']['detect_cost_fraction'] = round(rows['detect']['best'] / base_ms - 1.0, 4)
    out['pool']['detect_stamps_cost_fraction'] = round(rows['detect_stamps']['best'] / base_ms - 1.0, 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(out, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
