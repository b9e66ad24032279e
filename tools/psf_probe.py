"""PSF photometry at the scale it is meant for, planes resident in HBM.  Four steps, each in a child process of its own
under its own ``timeout``; the steps are chained and the first that fails ends the probe:

* ``build``     ``zm_psf_build_dev`` for 3000 stars on a 3072^2 frame (cutouts, clipped medians, finish);
* ``psf``       ``zm_psf_photometry_batch_dev`` on the set-up of tools/lightcurve_probe.py: 64 resident triples of
                3072 x 3080 px and 10^5 sources, the pairs of one ``zm_footprint_join_dev``;
* ``aperture``  the unchanged ``zm_forced_photometry_batch_dev`` on the same pairs, beside it;
* ``numpy``     the float64 restatement (tests/psf_ref.py) on 10^3 positions: the only earlier route a PSF fit has.

Times are host clocks around work that ends in a synchronise: one warm-up, then the median of ``--reps`` runs; for the
two batch launches also the library's own events (``psf_batch``, ``lc_batch``).  No ratio is promised: the fit does 36
multiply-adds per pixel over about 113 pixels where the aperture does overlap arithmetic over about 49.  The GPU's clock
is whatever the box runs at; per-kernel counters are not collected here.

usage: psf_probe.py [--out profiles/psf_probe.json] [--naxis 3072] [--nstars 3000] [--nimg 64] [--nsrc 100000]
                    [--nref 1000] [--reps 5]"""
import argparse
import ctypes as C
import importlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
STEPS = ('build', 'psf', 'aperture', 'numpy')


def lightcurve_probe():
    spec = importlib.util.spec_from_file_location('lightcurve_probe', os.path.join(ROOT, 'tools', 'lightcurve_probe.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


def step_build(args):
    import torch
    z = importlib.import_module('zuds-pipeline_amd')
    eng = z.get_engine(0)
    rng = np.random.default_rng(5)
    n = args.naxis
    img = rng.normal(150.0, 4.0, (n, n))
    x, y = rng.uniform(20.0, n - 21.0, args.nstars), rng.uniform(20.0, n - 21.0, args.nstars)
    flux = np.exp(rng.uniform(np.log(5e3), np.log(2e5), args.nstars))
    z.synth.add_stars(img, x, y, flux, 2.4)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')
    d = [dev(img.astype(np.float32)), dev(x), dev(y), dev(np.full(args.nstars, 150.0)), dev(flux)]
    torch.cuda.synchronize()
    res = {}

    def run():
        res['m'] = z.psf.psf_build_dev(*d, half=12, norm_radius=10.0, engine=eng)
        eng.synchronize()
    doc = timed(run, args.reps)
    model = res['m'][0].cpu().numpy()
    doc.update(naxis=n, nstars=args.nstars, model_sum=float(model.sum()), model_peak=float(model.max()),
               n_used_median=float(np.median(res['m'][1].cpu().numpy())))
    return doc


def step_batch(args, route):
    import torch
    z = importlib.import_module('zuds-pipeline_amd')
    lp = lightcurve_probe()
    eng = z.get_engine(0)
    L, lib = eng.L, z._lib
    nimg, nsrc = args.nimg, args.nsrc
    ws = lp.mosaic(z, nimg)
    ra, dec = lp.sources(z, ws, nsrc)
    pl = lp.planes(torch, nimg)
    d_ra, d_dec = torch.from_numpy(ra).cuda(), torch.from_numpy(dec).cuda()
    d_model = torch.from_numpy(gaussian_model()).cuda()
    wcs = (lib.zm_wcs * nimg)(*[lib.wcs_struct(w) for w in ws])
    recs = ((lib.zm_psf_image if route == 'psf' else lib.zm_lc_image) * nimg)()
    for k, (img, rms, mask) in enumerate(pl):
        recs[k].img, recs[k].rms, recs[k].mask, recs[k].wcs, recs[k].nx, recs[k].ny = img.data_ptr(), rms.data_ptr(), mask.data_ptr(), wcs[k], lp.NX, lp.NY
        if route == 'psf':
            recs[k].model, recs[k].half = d_model.data_ptr(), 12
    d_off = torch.zeros(nimg + 1, dtype=torch.int64, device='cuda')
    cap = 2 * nsrc
    d_idx = torch.empty(cap, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    n = C.c_int64(0)
    lib.check(L.zm_footprint_join_dev(eng.ctx, nimg, wcs, nsrc, d_ra.data_ptr(), d_dec.data_ptr(), cap, d_off.data_ptr(),
                                      d_idx.data_ptr(), C.byref(n)), 'zm_footprint_join_dev')
    eng.synchronize()
    npairs = int(n.value)
    assert npairs <= cap
    res = torch.empty((7, max(npairs, 1)), dtype=torch.float64, device='cuda')
    ints = torch.empty((2, max(npairs, 1)), dtype=torch.int32, device='cuda')

    def run():
        if route == 'psf':
            lib.check(L.zm_psf_photometry_batch_dev(eng.ctx, nimg, recs, d_off.data_ptr(), d_idx.data_ptr(), npairs, nsrc,
                                                    d_ra.data_ptr(), d_dec.data_ptr(), 8, 6.0, 0, *(res[k].data_ptr() for k in range(7)),
                                                    ints[0].data_ptr(), ints[1].data_ptr()), 'zm_psf_photometry_batch_dev')
        else:
            lib.check(L.zm_forced_photometry_batch_dev(eng.ctx, nimg, recs, d_off.data_ptr(), d_idx.data_ptr(), npairs, nsrc,
                                                       d_ra.data_ptr(), d_dec.data_ptr(), 3.0, res[0].data_ptr(), res[1].data_ptr(),
                                                       res[2].data_ptr(), res[3].data_ptr(), ints[1].data_ptr()),
                      'zm_forced_photometry_batch_dev')
        eng.synchronize()
    run()
    lib.check(L.zm_timing_reset(eng.ctx))
    lib.check(L.zm_timing_enable(eng.ctx, 1))
    doc = timed(run, args.reps)
    lib.check(L.zm_timing_enable(eng.ctx, 0))
    ms, cnt = C.c_double(), C.c_int64()
    name = 'psf_batch' if route == 'psf' else 'lc_batch'
    lib.check(L.zm_timing_read(eng.ctx, name.encode(), C.byref(ms), C.byref(cnt)))
    r = res[:, :npairs].cpu().numpy()
    doc.update(nimg=nimg, nsrc=nsrc, npairs=npairs, event_ms={name: ms.value / max(cnt.value, 1)},
               check=dict(flux=float(np.nansum(r[2])), fluxerr=float(np.nansum(r[3])), finite=int(np.isfinite(r[2]).sum())))
    return doc


def step_numpy(args):
    import psf_ref as pr
    rng = np.random.default_rng(3)
    img = rng.normal(0.0, 5.0, (512, 512)).astype(np.float32)
    rms = np.full((512, 512), 5.0, np.float32)
    x, y = rng.uniform(20.0, 491.0, args.nref), rng.uniform(20.0, 491.0, args.nref)
    model = gaussian_model()
    t0 = time.perf_counter()
    f = pr.fit(img, x, y, model, 6.0, 0, rms=rms)
    ms = 1e3 * (time.perf_counter() - t0)
    return dict(npos=args.nref, wall_ms=ms, ms_per_position=ms / max(args.nref, 1), finite=int(np.isfinite(f['flux']).sum()))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'psf_probe.json'))
    ap.add_argument('--naxis', type=int, default=3072)
    ap.add_argument('--nstars', type=int, default=3000)
    ap.add_argument('--nimg', type=int, default=64)
    ap.add_argument('--nsrc', type=int, default=100000)
    ap.add_argument('--nref', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--step', nargs=2, metavar=('NAME', 'FILE'), help='(internal) run one step in this process')
    args = ap.parse_args(argv)
    if args.step:
        name, path = args.step
        doc = step_build(args) if name == 'build' else step_numpy(args) if name == 'numpy' else step_batch(args, name)
        with open(path, 'w') as f:
            json.dump(doc, f)
        return 0
    doc = dict(tool='tools/psf_probe.py', not_measured='per-kernel counters (occupancy, LDS and cache traffic) were not collected')
    with tempfile.TemporaryDirectory() as tmp:
        for name in STEPS:
            part = os.path.join(tmp, name + '.json')
            cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__)]
            for k in ('naxis', 'nstars', 'nimg', 'nsrc', 'nref', 'reps'):
                cmd += ['--' + k, str(getattr(args, k))]
            rc = subprocess.call(cmd + ['--step', name, part])
            if rc != 0:
                print(f'step {name} ended with status {rc}: the probe stops here', flush=True)
                return rc
            with open(part) as f:
                doc[name] = json.load(f)
    doc['psf_over_aperture'] = doc['psf']['wall_median_ms'] / doc['aperture']['wall_median_ms']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps(doc))
    return 0


if __name__ == '__main__':
    sys.exit(main())
