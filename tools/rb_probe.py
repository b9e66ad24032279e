#!/usr/bin/env python3
"""Developer probe: what the real / bogus score costs.

    python3 tools/rb_probe.py [--size NX NY] [--jobs N] [--reps R] [--out profiles/realbogus_probe.json]

Two steps, each a child process of its own under ``timeout`` (a step that fails or runs out of time ends the probe;
nothing more is started on the GPU):

  score  HIP-event times of ``RBModel.score_dev`` for 50 and 1000 VGG6 triplets resident in HBM, next to a float32
         torch forward of the same network (conv2d / max_pool2d / matmul) on the same GPU, and the distance from the
         arithmetic floor: 38 MFLOP per triplet at the fp32 vector rate.
  pool   milliseconds per subtraction of the nightly pool with ``detect`` + ``stamps``, the model off and on, on the
         scene of ``tools/night_detect_probe.py``; the model's cut is 0 so that every row it scores survives and the
         stamps delivered are the same.

The weights are seeded Glorot values (tests/braai_ref.py): the time does not depend on them.  Prints one JSON line
and, with ``--out``, writes it.
"""
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

FLOP_PER_TRIPLET = 2 * (61 * 61 * 16 * 27 + 59 * 59 * 16 * 144 + 27 * 27 * 32 * 144 + 25 * 25 * 32 * 288 + 1152 * 256 + 256)
FP32_VECTOR_TFLOPS = 157.3                     # MI355X, packed fp32 FMA, peak


def vgg6_model():
    import braai_ref as br
    rb = importlib.import_module('zuds-pipeline_amd.realbogus')
    size, ch, spec = br.vgg6_spec()
    weights = br.glorot_weights(size, ch, spec, 9)
    return rb.RBModel(open(br.VGG6_JSON).read(), weights, name='braai_d6_m9'), br.ref_layers(spec), weights


def step_score(args):
    import torch
    import braai_ref as br
    z = importlib.import_module('zuds-pipeline_amd')
    m, layers, weights = vgg6_model()
    eng = z.Engine(0)
    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    out = dict(device=torch.cuda.get_device_name(0), flop_per_triplet=FLOP_PER_TRIPLET, reps=args.reps)
    blocks_h, norms_h = br.make_stamps(50, 63, 3)
    for n in (50, 1000):
        blocks = torch.from_numpy(np.tile(blocks_h, (n // 50, 1, 1, 1))).to('cuda:0')
        norms = torch.from_numpy(np.tile(norms_h, (n // 50, 1))).to('cuda:0')
        x32 = (blocks / norms[:, :, None, None].to(torch.float32)).contiguous()
        torch.cuda.synchronize()

        def ours():
            return m.score_dev(blocks, norms, order=('new', 'ref', 'sub'), engine=eng, stream=stream)

        wt = [torch.from_numpy(np.asarray(w)).to('cuda:0') for w in weights]
        wt = [w.permute(3, 2, 0, 1).contiguous() if w.dim() == 4 else w for w in wt]

        def theirs():
            import torch.nn.functional as F
            t, it = x32, iter(wt)
            for l in layers:
                if l[0] == 'conv':
                    t = torch.relu(F.conv2d(t, next(it), next(it)))
                elif l[0] == 'pool':
                    t = F.max_pool2d(t, l[1], stride=l[1])
                elif l[0] == 'flatten':
                    t = t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)
                else:
                    t = t @ next(it) + next(it)
                    t = torch.relu(t) if l[1] == 'relu' else torch.sigmoid(t)
            return t

        def clock(fn):
            ts = []
            with torch.cuda.stream(stream):
                for k in range(args.reps + 2):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    r = fn()
                    b.record(stream)
                    b.synchronize()
                    if k >= 2:                       # (two warm runs: scratch, plans, the library's kernel choice)
                        ts.append(a.elapsed_time(b))
            return ts, r
        t_ours, r1 = clock(ours)
        t_torch, r2 = clock(theirs)
        floor_ms = 1e3 * n * FLOP_PER_TRIPLET / (FP32_VECTOR_TFLOPS * 1e12)
        out[f'n{n}'] = dict(score_dev_ms=[round(t, 4) for t in t_ours], torch_fp32_ms=[round(t, 4) for t in t_torch],
                            fp32_floor_ms=round(floor_ms, 4), times_the_floor=round(min(t_ours) / floor_ms, 1),
                            max_abs_diff_to_torch=float((r1 - r2.ravel()).abs().max()))
    eng.close()
    return out


def step_pool(args):
    nm = importlib.import_module('zuds-pipeline_amd.nightly')          # (first: it sizes the hardware queues)
    import torch
    s = importlib.import_module('zuds-pipeline_amd.synth')
    m, _, _ = vgg6_model()
    nx, ny = args.size
    base = s.ztf_wcs(nx, ny, tpv=True)
    rng = np.random.default_rng(5)
    nst = int(nx * ny / 2500)
    fl = np.exp(rng.uniform(np.log(3e3), np.log(8e4), nst))
    ra, dec = base.all_pix2world(rng.uniform(-10, nx + 10, nst), rng.uniform(-10, ny + 10, nst), 0)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to('cuda:0')
    rf = s.make_frame(nx, ny, 50, base, star_sky=(ra, dec, fl), fwhm=2.0, noise=1.0, nbad=200)

    def rms_map(level, seed):
        return (level * (1.0 + 0.03 * np.random.default_rng(seed).standard_normal((ny, nx), dtype=np.float32))).astype(np.float32)
    ref = dict(img=dev(rf['img'], np.float32), rms=dev(rms_map(1.0, 90), np.float32), mask=dev(rf['mask'], np.int32),
               wcs=base, flxscale=1.0)
    scis = []
    for i in range(args.frames):
        w = s.ztf_wcs(nx, ny, dx=rng.uniform(-6, 6), dy=rng.uniform(-6, 6), rot_deg=rng.uniform(-0.05, 0.05))
        tra, tdec = w.all_pix2world(rng.uniform(100, nx - 100, 20), rng.uniform(100, ny - 100, 20), 0)
        f = s.make_frame(nx, ny, 51 + i, w, star_sky=(np.concatenate([ra, tra]), np.concatenate([dec, tdec]),
                                                     np.concatenate([fl, np.full(20, 6e3)])), fwhm=2.4, sky=180.0, nbad=300)
        scis.append(dict(img=dev(f['img'], np.float32), rms=dev(rms_map(5.0, 91 + i), np.float32),
                         mask=dev(f['mask'], np.int32), wgt=dev(f['wgt'], np.float32), wcs=w, seeing=2.4))
    pool = nm.SubtractionPool(args.lanes, batch=args.fit_batch)
    rows = {}
    for name, kw in (('model_off', {}), ('model_on', dict(rb_model=m, rb_cut=0.0)), ('model_off_again', {})):
        js = [nm.SubtractionJob(scis[k % len(scis)], ref, tag=k, detect=True, stamps=True, **kw) for k in range(args.jobs)]
        res = pool.map(js, keep=False)                              # warm
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pool.map(js, keep=False)
            ts.append(1e3 * (time.perf_counter() - t0) / len(js))
        rows[name] = dict(ms_per_subtraction=[round(t, 4) for t in ts], best=round(min(ts), 4),
                          scored_rows=[int((r['cat']['rb'] != -99).sum()) for r in res[:len(scis)]],
                          good_rows=[int((r['cat']['GOODCUT'] == 1).sum()) for r in res[:len(scis)]])
    pool.close()
    base_ms = min(rows['model_off']['best'], rows['model_off_again']['best'])
    rows['model_cost_fraction'] = round(rows['model_on']['best'] / base_ms - 1.0, 4)
    return dict(size=[nx, ny], jobs=args.jobs, lanes=args.lanes, fit_batch=args.fit_batch, pool=rows)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, nargs=2, default=(3072, 3080), metavar=('NX', 'NY'))
    ap.add_argument('--jobs', type=int, default=12)
    ap.add_argument('--frames', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--lanes', type=int, default=3)
    ap.add_argument('--fit-batch', type=int, default=4)
    ap.add_argument('--step', choices=['score', 'pool'], help='(internal) run one step in this process')
    ap.add_argument('--step-timeout', type=int, default=240, help='seconds each step may take')
    ap.add_argument('--out')
    args = ap.parse_args(argv)
    if args.step:
        print('RB_PROBE ' + json.dumps(step_score(args) if args.step == 'score' else step_pool(args)), flush=True)
        return 0
    out = {}
    passed = [a for a in (argv if argv is not None else sys.argv[1:])]
    if '--out' in passed:
        k = passed.index('--out')
        del passed[k:k + 2]
    for step in ('score', 'pool'):
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--step', step] + passed
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith('RB_PROBE ')]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            print(f'rb_probe: step {step} ended with status {p.returncode}; nothing more is started', file=sys.stderr)
            return p.returncode or 1
        out[step] = json.loads(line[-1][len('RB_PROBE '):])
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(out, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
