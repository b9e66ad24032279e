"""Fake sources at the scale they are meant for, planes resident in HBM.  Two steps in one process:

* ``inject``   ``zm_inject_dev`` (``fakes.inject_dev``) of 10^3 and 10^4 fakes at random positions and phases on a 3072^2
               plane, beside the host route such a plane had before: plane to the host, the profiles added with numpy, plane
               back.  The host route here adds the MODEL AS SAMPLED, shifted to the nearest pixel (no Lanczos interpolation,
               no rms plane, no flags): it does less work than the kernel, so the comparison flatters it.
* ``recover``  ``fakes.recover_dev`` (clone, inject, subtraction, candidates, match) of 200 fakes on one science frame
               against one reference, beside a plain ``DeviceSubtraction.run`` + ``candidates`` on the same planes.

Times are host clocks around work that ends in a synchronise: one warm-up, then the median of ``--reps`` runs.  The number
of layers of each injection is printed with it (random positions overlap: one launch per layer).  No threshold is set on
any of these figures and no ratio is promised; the GPU's clock is whatever the box runs at.

usage: fakes_probe.py [--out profiles/fakes_probe.json] [--naxis 3072] [--frame 1024] [--reps 5]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gaussian_model(half=12, fwhm=2.4, norm_radius=10.0):
    s = fwhm / 2.3548200450309493
    jj, ii = np.mgrid[-half:half + 1, -half:half + 1]
    m = np.exp(-0.5 * (ii * ii + jj * jj) / (s * s))
    m[ii * ii + jj * jj > norm_radius * norm_radius] = 0.0
    return m / m.sum()


def timed(fn, reps):
    fn()                                                             # warm-up: code load, scratch
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(wall_ms=t, wall_median_ms=float(np.median(t)))


def probe_inject(z, torch, naxis, reps):
    eng = z.get_engine(0)
    stream = torch.cuda.Stream('cuda:0')
    eng.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(1)
    model = gaussian_model()
    half = 12
    base = torch.from_numpy(rng.normal(100.0, 5.0, (naxis, naxis)).astype(np.float32)).to('cuda:0')
    rms = torch.full((naxis, naxis), 5.0, dtype=torch.float32, device='cuda:0')
    dmodel = torch.from_numpy(model).to('cuda:0')
    out = {}
    for n in (1000, 10000):
        x, y = rng.uniform(20, naxis - 21, n), rng.uniform(20, naxis - 21, n)
        flux = rng.uniform(1e3, 1e4, n)
        _, nlayers = z.inject_layers(x, y, half)

        def device():
            with torch.cuda.stream(stream):
                z.inject_dev(base, x, y, flux, dmodel, rms=rms, gain=6.2, engine=eng)
            stream.synchronize()

        def host():
            with torch.cuda.stream(stream):
                plane = base.cpu().numpy()
            ix, iy = np.floor(x + 0.5).astype(int), np.floor(y + 0.5).astype(int)
            for k in range(n):
                plane[iy[k] - half:iy[k] + half + 1, ix[k] - half:ix[k] + half + 1] += (flux[k] * model).astype(np.float32)
            with torch.cuda.stream(stream):
                base.copy_(torch.from_numpy(plane))
            stream.synchronize()

        t0 = time.perf_counter()
        for _ in range(20):
            z.inject_layers(x, y, half)
        layers_ms = 1e3 * (time.perf_counter() - t0) / 20
        out[str(n)] = dict(nlayers=nlayers, layers_host_ms=layers_ms, device=timed(device, reps), host_route=timed(host, max(reps // 2, 1)))
        print(f'inject {n} fakes on {naxis}^2 ({nlayers} layers, zm_inject_layers {layers_ms:.3f} ms): zm_inject_dev '
              f'{out[str(n)]["device"]["wall_median_ms"]:.3f} ms, host route {out[str(n)]["host_route"]["wall_median_ms"]:.1f} ms', flush=True)
    eng.set_stream(0)
    return out


def probe_recover(z, torch, frame, reps):
    s = importlib.import_module('zuds-pipeline_amd.synth')
    devmod = importlib.import_module('zuds-pipeline_amd.device')
    nx = ny = frame
    base = s.ztf_wcs(nx, ny, tpv=True)
    rng = np.random.default_rng(2)
    nst = int(nx * ny / 10000)
    xs, ys = rng.uniform(-10, nx + 10, nst), rng.uniform(-10, ny + 10, nst)
    fl = np.exp(rng.uniform(np.log(3e3), np.log(8e4), nst))
    ra, dec = base.all_pix2world(xs, ys, 0)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to('cuda:0')
    rf = s.make_frame(nx, ny, 21, base, star_sky=(ra, dec, fl), fwhm=2.0, noise=1.0, nbad=20)
    w = s.ztf_wcs(nx, ny, dx=2.5, dy=-3.5, rot_deg=0.03)
    sf = s.make_frame(nx, ny, 22, w, star_sky=(ra, dec, fl), fwhm=2.4, sky=180.0, nbad=30)
    ref = dict(img=dev(rf['img'], np.float32), rms=dev(np.full((ny, nx), 1.0), np.float32), mask=dev(rf['mask'], np.int32))
    sci = dict(img=dev(sf['img'], np.float32), rms=dev(np.full((ny, nx), 5.0), np.float32), mask=dev(sf['mask'], np.int32),
               wgt=dev(sf['wgt'], np.float32))
    model = z.PSFModel(gaussian_model(), cards={'PSFFITR': 6.0})
    st = z.fake_settings(dict(N=200, MAG_MIN=15.5, MAG_MAX=19.5, MIN_SEP=15.0), psf=model)
    table = z.draw_fakes((ny, nx), w, 25.0, st)
    ch = devmod.DeviceSubtraction(w, base, engine=z.get_engine(0))
    args = (sci['img'], sci['rms'], sci['mask'], sci['wgt'], ref['img'], ref['rms'], ref['mask'])
    seen = {}

    def plain():
        ch.run(*args, seeing=2.4, nreg_side=2)
        seen['plain'] = len(ch.candidates(2.4, wcs=w)[0])
        ch.stream.synchronize()

    def recover():
        t, cat, _ = z.recover_dev(ch, *args, 2.4, table, model, run_kws=dict(nreg_side=2), candidate_kws=dict(wcs=w), gain=6.2)
        seen['fake'], seen['recovered'] = len(cat), int(t['recovered'].sum())

    out = dict(frame=frame, nfakes=200, plain=timed(plain, reps), recover=timed(recover, reps))
    out.update(rows_plain=seen['plain'], rows_fake=seen['fake'], recovered=seen['recovered'])
    print(f'recover on {frame}^2: run + candidates {out["plain"]["wall_median_ms"]:.2f} ms ({seen["plain"]} rows), recover_dev of 200 fakes '
          f'{out["recover"]["wall_median_ms"]:.2f} ms ({seen["fake"]} rows, {seen["recovered"]} recovered)', flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--naxis', type=int, default=3072)
    ap.add_argument('--frame', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args(argv)
    import torch
    z = importlib.import_module('zuds-pipeline_amd')
    res = dict(naxis=args.naxis, reps=args.reps, inject=probe_inject(z, torch, args.naxis, args.reps),
               recover=probe_recover(z, torch, args.frame, args.reps))
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
