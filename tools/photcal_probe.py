"""Curves of growth at the scale they are meant for: a synthetic 3072 x 3072 frame with 3000 stars, planes resident in HBM.

Two routes to the same numbers (fluxes in the six apertures and the reference aperture, each above a clipped local sky):

* ``new``: one ``zm_growth_dev`` launch (seven radii, annulus 12 .. 18), then one ``zm_clipped_median_dev`` launch over the
  six columns of magnitude differences;
* ``old``: what the package offered before - seven ``zm_aperture_photometry_dev`` launches (one per radius) and the sky of
  every star on the host: numpy's clipped median of the annulus pixels, read from a host copy of the image.

The GPU step runs in a child process under its own time limit; a child that does not end in time is killed and the
probe reports the case as not measured.  Every launch sequence is run ``--warmup`` times unrecorded, then ``--repeat``
times between two stream synchronisations; the median and the smallest wall time are kept.  Writes one JSON document
(default profiles/photcal_probe.json).

usage: photcal_probe.py [--out profiles/photcal_probe.json] [--naxis 3072] [--nstars 3000] [--repeat 20] [--limit 300]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
RADII = (1.0, 1.5, 2.0, 3.0, 5.0, 7.0, 10.0)
ANNULUS = (12.0, 18.0)


def scene(naxis, nstars, seed=5):
    """(image, rms, mask, x, y): Gaussian stars of FWHM 2.4 px on a sky with noise, a few bad pixels."""
    s = importlib.import_module('zuds-pipeline_amd.synth')
    rng = np.random.default_rng(seed)
    img = rng.normal(150.0, 4.0, (naxis, naxis))
    x, y = rng.uniform(20.0, naxis - 21.0, nstars), rng.uniform(20.0, naxis - 21.0, nstars)
    s.add_stars(img, x, y, np.exp(rng.uniform(np.log(5e3), np.log(2e5), nstars)), 2.4)
    mask = np.zeros((naxis, naxis), np.int32)
    nbad = naxis * naxis // 4700                       # 2000 bad pixels on the full frame
    mask[rng.integers(0, naxis, nbad), rng.integers(0, naxis, nbad)] = 1 << 8
    return img.astype(np.float32), np.full((naxis, naxis), 4.0, np.float32), mask, x, y


def host_sky(img, x, y, kappa=3.0, maxiter=5):
    """The clipped annulus median of every star with numpy (the host half of the old route)."""
    out = np.empty(x.size)
    r = int(ANNULUS[1]) + 1
    jj, ii = np.mgrid[-r:r + 1, -r:r + 1]
    for k in range(x.size):
        ix, iy = int(round(x[k])), int(round(y[k]))
        d2 = (ii + ix - x[k]) ** 2 + (jj + iy - y[k]) ** 2
        v = img[iy - r:iy + r + 1, ix - r:ix + r + 1][(d2 >= ANNULUS[0] ** 2) & (d2 < ANNULUS[1] ** 2)].astype(np.float64)
        for _ in range(maxiter):
            med = np.median(v)
            sig = 1.4826 * np.median(np.abs(v - med))
            keep = np.abs(v - med) <= kappa * sig
            if keep.all():
                break
            v = v[keep]
        out[k] = np.median(v)
    return out


def timed(fn, sync, warmup, repeat):
    for _ in range(warmup):
        fn()
    sync()
    t = []
    for _ in range(repeat):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), repeat=repeat)


def child(args):
    import torch
    z = importlib.import_module('zuds-pipeline_amd')
    p = z.photcal
    eng = z.get_engine(0)
    img, rms, mask, x, y = scene(args.naxis, args.nstars)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')
    d_img, d_rms, d_mask, d_x, d_y = dev(img), dev(rms), dev(mask), dev(x), dev(y)
    stream = torch.cuda.Stream('cuda:0')
    eng.set_stream(stream.cuda_stream)
    out = {}
    with torch.cuda.stream(stream):
        res = {}

        def new_growth():
            res['g'] = p.growth_curves_dev(d_img, d_x, d_y, RADII, rms=d_rms, mask=d_mask, annulus=ANNULUS, engine=eng)

        def new_medians():
            f = res['g']['flux']
            res['m'] = p.clipped_median_dev(-2.5 * torch.log10(f[:, -1:] / f[:, :-1]), engine=eng)

        out['new_growth'] = timed(new_growth, stream.synchronize, args.warmup, args.repeat)
        out['new_clipped_medians'] = timed(new_medians, stream.synchronize, args.warmup, args.repeat)
        n = x.size
        f, e = torch.empty(n, dtype=torch.float64, device='cuda:0'), torch.empty(n, dtype=torch.float64, device='cuda:0')
        fl = torch.empty(n, dtype=torch.int32, device='cuda:0')
        ny, nx = img.shape

        def old_apertures():
            for r in RADII:
                z._lib.check(eng.L.zm_aperture_photometry_dev(eng.ctx, d_img.data_ptr(), d_rms.data_ptr(), d_mask.data_ptr(), nx,
                                                              ny, n, d_x.data_ptr(), d_y.data_ptr(), r, f.data_ptr(),
                                                              e.data_ptr(), fl.data_ptr()), 'zm_aperture_photometry_dev')

        out['old_seven_aperture_launches'] = timed(old_apertures, stream.synchronize, args.warmup, args.repeat)
        stream.synchronize()
    eng.set_stream(0)
    t0 = time.perf_counter()
    sky = host_sky(img, x, y)
    out['old_host_annulus_medians'] = dict(median_ms=(time.perf_counter() - t0) * 1e3, repeat=1)
    g = {k: v.cpu().numpy() for k, v in res['g'].items()}
    out['check'] = dict(stars_with_flags_0=int((g['flags'] == 0).sum()),
                        largest_sky_difference_from_the_host_medians=float(np.nanmax(np.abs(g['sky'] - sky))),
                        apcor4=float(res['m'].cpu().numpy()[3, 0]))
    out['new_total_ms'] = out['new_growth']['median_ms'] + out['new_clipped_medians']['median_ms']
    out['old_total_ms'] = out['old_seven_aperture_launches']['median_ms'] + out['old_host_annulus_medians']['median_ms']
    print(json.dumps(out))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'photcal_probe.json'))
    ap.add_argument('--naxis', type=int, default=3072)
    ap.add_argument('--nstars', type=int, default=3000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--limit', type=float, default=300.0)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.child:
        child(args)
        return 0
    doc = dict(tool='tools/photcal_probe.py', naxis=args.naxis, nstars=args.nstars, radii=list(RADII), annulus=list(ANNULUS))
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--naxis', str(args.naxis), '--nstars', str(args.nstars),
           '--warmup', str(args.warmup), '--repeat', str(args.repeat)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        if r.returncode == 0:
            doc['measured'] = json.loads(r.stdout.strip().splitlines()[-1])
        else:
            doc['not_measured'] = f'the child ended with status {r.returncode}: {r.stderr[-500:]}'
    except subprocess.TimeoutExpired:
        doc['not_measured'] = f'the child did not end within {args.limit:g} s and was killed'
    with open(args.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
        fh.write('\n')
    print(json.dumps(doc, indent=1))
    return 0 if 'measured' in doc else 1


if __name__ == '__main__':
    sys.exit(main())
