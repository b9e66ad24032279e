"""Forced photometry of a source table on a night's resident subtractions: the route the package had before
``csrc/lightcurve.hip`` against the new one, on the same planes and the same pairs.

Workload: 64 triples (image, rms, mask) of 3072 x 3080 px resident in HBM - an 8 x 8 mosaic of ZTF-like TPV frames - and
10^5 and 10^6 synthetic sources uniform over the mosaic and a margin around it.

* ``old``: per image, the host's ``all_world2pix`` (``zm_wcs_sky2pix``: one thread, fp64) of the sources inside its
  footprint, the copy of the positions to the device and one ``zm_aperture_photometry_dev`` launch; the footprint lists
  are handed to it (the package had no join), so their cost is not in its time.
* ``new``: one ``zm_footprint_join_dev`` and one ``zm_forced_photometry_batch_dev``.

Every (route, table size) is a step that runs in a child process of its own under its own ``timeout``; the steps are
chained, and the first one that fails - a fault, a time limit, a wrong answer - ends the probe.  Times are host clocks
around work that ends in a synchronise (warm-up first, then the median of the repeats), and for the new route also the
library's own events around its launches (``lc_join``, ``lc_batch``).  The two routes' positions, sums and flags are compared.
The GPU's clock is whatever the box runs at: ratios of two routes measured in one call are what the figures are good for.

usage: lightcurve_probe.py [--out profiles/lightcurve_probe.json] [--nimg 64] [--sizes 100000,1000000] [--reps 5]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NX, NY = 3072, 3080


def mosaic(z, nimg):
    """nimg TPV frames on a grid (8 columns), a little rotated and dithered, overlapping by ~100 px."""
    s = z.synth
    rng = np.random.default_rng(4)
    ws = []
    rows = (nimg + 7) // 8
    for k in range(nimg):
        gx, gy = k % 8, k // 8
        ws.append(s.ztf_wcs(NX, NY, dx=-(gx - 3.5) * (NX - 100) + rng.uniform(-20, 20),
                            dy=-(gy - (rows - 1) / 2) * (NY - 100) + rng.uniform(-20, 20), rot_deg=rng.uniform(-0.3, 0.3), tpv=True))
    return ws


def sources(z, ws, n):
    rng = np.random.default_rng(n)
    base = z.synth.ztf_wcs(NX, NY, tpv=False)
    rows = (len(ws) + 7) // 8
    x = rng.uniform(-4.2 * NX, 4.2 * NX, n) + NX / 2
    y = rng.uniform(-(rows / 2 + 0.2) * NY, (rows / 2 + 0.2) * NY, n) + NY / 2
    return base.all_pix2world(x, y, 1)


def planes(torch, nimg):
    out = []
    g = torch.Generator(device='cuda')
    g.manual_seed(7)
    for _ in range(nimg):
        img = torch.randn((NY, NX), generator=g, device='cuda', dtype=torch.float32) * 5.0
        rms = torch.rand((NY, NX), generator=g, device='cuda', dtype=torch.float32) * 2.0 + 1.0
        mask = (torch.rand((NY, NX), generator=g, device='cuda') < 0.01).to(torch.int32) * 8
        out.append((img, rms, mask))
    torch.cuda.synchronize()
    return out


def timer(eng, z, name):
    ms, cnt = C.c_double(), C.c_int64()
    z._lib.check(eng.L.zm_timing_read(eng.ctx, name.encode(), C.byref(ms), C.byref(cnt)))
    return ms.value, cnt.value


def step(route, nsrc, nimg, reps, out):
    """One child: builds the scene, runs one route, writes its figures and a checksum of its sums."""
    import torch
    z = importlib.import_module('zuds-pipeline_amd')
    eng = z.get_engine(0)
    L, lib = eng.L, z._lib
    ws = mosaic(z, nimg)
    ra, dec = sources(z, ws, nsrc)
    pl = planes(torch, nimg)
    d_ra, d_dec = torch.from_numpy(ra).cuda(), torch.from_numpy(dec).cuda()
    wcs = (lib.zm_wcs * nimg)(*[lib.wcs_struct(w) for w in ws])
    recs = (lib.zm_lc_image * nimg)()
    for k, (img, rms, mask) in enumerate(pl):
        recs[k].img, recs[k].rms, recs[k].mask, recs[k].wcs, recs[k].nx, recs[k].ny = img.data_ptr(), rms.data_ptr(), mask.data_ptr(), wcs[k], NX, NY
    d_off = torch.zeros(nimg + 1, dtype=torch.int64, device='cuda')
    cap = 2 * nsrc
    d_idx = torch.empty(cap, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    n = C.c_int64(0)

    def join():
        lib.check(L.zm_footprint_join_dev(eng.ctx, nimg, wcs, nsrc, d_ra.data_ptr(), d_dec.data_ptr(), cap, d_off.data_ptr(),
                                          d_idx.data_ptr(), C.byref(n)), 'zm_footprint_join_dev')
        assert n.value <= cap
    join()
    eng.synchronize()
    npairs = int(n.value)
    off, idx = d_off.cpu().numpy(), d_idx[:npairs].cpu().numpy()
    res = torch.empty((4, npairs), dtype=torch.float64, device='cuda')
    flg = torch.empty(npairs, dtype=torch.int32, device='cuda')
    doc = dict(route=route, nsrc=nsrc, nimg=nimg, npairs=npairs, pairs_per_image=[int(v) for v in np.diff(off)[:4]] + ['...'])

    def new_route():
        join()
        lib.check(L.zm_forced_photometry_batch_dev(eng.ctx, nimg, recs, d_off.data_ptr(), d_idx.data_ptr(), npairs, nsrc,
                                                   d_ra.data_ptr(), d_dec.data_ptr(), 3.0, res[0].data_ptr(), res[1].data_ptr(),
                                                   res[2].data_ptr(), res[3].data_ptr(), flg.data_ptr()), 'zm_forced_photometry_batch_dev')
        eng.synchronize()

    host = dict(sky2pix=0.0)

    def old_route():
        keep = []                                                    # positions stay allocated until their kernel has run
        for k, (w, (img, rms, mask)) in enumerate(zip(ws, pl)):
            a, b = int(off[k]), int(off[k + 1])
            if a == b:
                continue
            j = idx[a:b]
            t0 = time.perf_counter()
            x, y = w.all_world2pix(ra[j], dec[j], 0)
            host['sky2pix'] += time.perf_counter() - t0
            pos = torch.from_numpy(np.ascontiguousarray(np.stack([x, y]))).cuda()
            keep.append(pos)
            torch.cuda.synchronize()
            lib.check(L.zm_aperture_photometry_dev(eng.ctx, img.data_ptr(), rms.data_ptr(), mask.data_ptr(), NX, NY, b - a,
                                                   pos[0].data_ptr(), pos[1].data_ptr(), 3.0, res[2][a:b].data_ptr(),
                                                   res[3][a:b].data_ptr(), flg[a:b].data_ptr()), 'zm_aperture_photometry_dev')
            res[0][a:b], res[1][a:b] = pos[0], pos[1]
        eng.synchronize()
        torch.cuda.synchronize()

    run = new_route if route == 'new' else old_route
    run()                                                            # warm-up: code load, scratch
    lib.check(L.zm_timing_reset(eng.ctx))
    lib.check(L.zm_timing_enable(eng.ctx, 1))
    host['sky2pix'] = 0.0
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        times.append(1e3 * (time.perf_counter() - t0))
    lib.check(L.zm_timing_enable(eng.ctx, 0))
    doc['wall_ms'] = times
    doc['wall_median_ms'] = float(np.median(times))
    if route == 'new':
        j_ms, j_n = timer(eng, z, 'lc_join')
        b_ms, b_n = timer(eng, z, 'lc_batch')
        doc['event_ms'] = dict(lc_join=j_ms / max(j_n, 1), lc_batch=b_ms / max(b_n, 1))
        doc['join_share_of_events'] = j_ms / max(j_ms + b_ms, 1e-30)
    else:
        a_ms, a_n = timer(eng, z, 'aperture')
        doc['event_ms'] = dict(aperture_all_images=a_ms / reps)
        doc['host_sky2pix_ms'] = 1e3 * host['sky2pix'] / reps
    r = res.cpu().numpy()
    doc['check'] = dict(flux=float(np.nansum(r[2])), fluxerr=float(np.nansum(r[3])), flags=int(flg.cpu().numpy().astype(np.int64).sum()),
                        max_abs_x=float(np.abs(r[0]).max()) if npairs else 0.0)
    np.save(out + '.npy', np.stack([r[0], r[1], r[2], r[3], flg.cpu().numpy().astype(np.float64)]))
    with open(out, 'w') as f:
        json.dump(doc, f)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lightcurve_probe.json'))
    ap.add_argument('--nimg', type=int, default=64)
    ap.add_argument('--sizes', default='100000,1000000')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--step', nargs=3, metavar=('ROUTE', 'NSRC', 'FILE'), help='(internal) run one step in this process')
    args = ap.parse_args(argv)
    if args.step:
        step(args.step[0], int(args.step[1]), args.nimg, args.reps, args.step[2])
        return 0
    doc = dict(tool='tools/lightcurve_probe.py', frame=[NX, NY], nimg=args.nimg, cases=[])
    with tempfile.TemporaryDirectory() as tmp:
        for nsrc in (int(v) for v in args.sizes.split(',')):
            case = dict(nsrc=nsrc)
            sums = {}
            for route in ('old', 'new'):
                part = os.path.join(tmp, f'{route}_{nsrc}.json')
                cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--nimg', str(args.nimg),
                       '--reps', str(args.reps), '--step', route, str(nsrc), part]
                rc = subprocess.call(cmd)
                if rc != 0:
                    print(f'step {route} / {nsrc} ended with status {rc}: the probe stops here', flush=True)
                    return rc
                with open(part) as f:
                    case[route] = json.load(f)
                sums[route] = np.load(part + '.npy')
            o, n = sums['old'], sums['new']
            # the routes differ in where sky -> pixel is evaluated (host / device: 1e-11 px), so sums agree to rounding, flags exactly
            case['flags_equal'] = bool(o[4].tobytes() == n[4].tobytes())
            case['max_flux_difference'] = float(np.nanmax(np.abs(o[2] - n[2]))) if o.shape[1] else 0.0
            case['max_position_difference_px'] = float(max(np.abs(o[0] - n[0]).max(), np.abs(o[1] - n[1]).max())) if o.shape[1] else 0.0
            case['old_over_new'] = case['old']['wall_median_ms'] / case['new']['wall_median_ms']
            doc['cases'].append(case)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == '__main__':
    sys.exit(main())
