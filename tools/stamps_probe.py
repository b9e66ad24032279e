#!/usr/bin/env python
"""Time the detection thumbnails of a resident subtraction against the whole-frame route they replace.

    python tools/stamps_probe.py [--size 3072] [--frames 8] [--steps 20] [--stamps 50] [--out FILE.json]

Builds the bench's synthetic science epoch and a reference coadded from ``--frames`` of its frames (as
tools/extract_probe.py does), runs the device-resident subtraction, then times in one process, interleaved call by call,
with HIP events on the chain's stream:

* ``stamps_ms``  (a) ``DeviceSubtraction.stamps``: difference and science frame resampled onto the reference grid under
  the ``--stamps`` seeded positions only, the reference gathered, norms, blocks and norms copied to the host;
* ``whole_ms``   (b) what the engine offered before: two ``zm_resample_dev`` calls of the whole frames onto the
  reference grid, then the crops - ONE gather per plane with index tensors made ahead of the clock (the cheapest crop
  torch offers), norms with torch, blocks and norms copied to the host;
* ``whole_resample_ms``  the two ``zm_resample_dev`` calls of (b) alone;
* ``subtract_ms``  the subtraction leg, for scale.

Medians over ``--steps`` calls after ``--warmup``; ``whole_spread_ms`` is the half width of (b)'s 16 .. 84 percentile
range, the run-to-run spread (a) is held against.  The blocks of (a) and (b) are compared bit for bit before anything
is timed.  Prints one JSON line.  For the per-kernel table run it under
``rocprofv3 --kernel-trace --stats -- python tools/stamps_probe.py --steps 5``.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3072)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--stamps', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import bench
    z = importlib.import_module('zuds-pipeline_amd')
    synth = importlib.import_module('zuds-pipeline_amd.synth')
    dev = importlib.import_module('zuds-pipeline_amd.device')
    check = z._lib.check
    device = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    eng = z.Engine(0)
    size, S, n = args.size, z.CUTOUT_SIZE, args.stamps
    base, frames = bench.make_device_frames(synth, torch, args.frames + 1, size, 2000, device, 'int16')
    sci = frames.pop()
    sci['mask'] = torch.zeros((size, size), dtype=torch.int16, device=device)
    sci['wgt'] = torch.full((size, size), float(sci['wgt'].max()), dtype=torch.float32, device=device)
    sci['rms'] = (1.0 / torch.sqrt(sci['wgt'])).to(torch.float32)
    params = z.coadd_params(combine='CLIPPED', subtract_back=True, rescale_weights=True)
    coadd = dev.DeviceCoadd(base, params, device=0, engine=eng, want_mask=True)
    sub = dev.DeviceSubtraction(sci['wcs'], base, device=0, engine=eng, stream=coadd.stream)
    stream = coadd.stream
    npx = coadd.img.numel()
    ref_rms = torch.empty_like(coadd.wgt)
    coadd.run(dev.DeviceFrames(frames, device))
    with torch.cuda.stream(stream):
        check(eng.L.zm_mask_flag_dev(eng.ctx, coadd.mask.data_ptr(), coadd.mask_wgt.data_ptr(), 0.0, 1 << 16, npx))
        check(eng.L.zm_add_scalar_dev(eng.ctx, coadd.img.data_ptr(), 150.0, npx))
        check(eng.L.zm_rms_from_weight_dev(eng.ctx, coadd.wgt.data_ptr(), None, npx, float(np.sqrt(50000.0)),
                                           ref_rms.data_ptr()))

    def subtract():
        sub.run(sci['img'], sci['rms'], sci['mask'], sci['wgt'], coadd.img, ref_rms, coadd.mask, seeing=4.0, nreg_side=3)
    subtract()
    stream.synchronize()
    rng = np.random.default_rng(50)
    ra, dec = base.all_pix2world(rng.uniform(0, size - 1, n), rng.uniform(0, size - 1, n), 0)
    x0, y0, st = z.stamp_origin(base, ra, dec, S)
    assert not st.any()
    ws, wr = z._lib.wcs_struct(sci['wcs']), z._lib.wcs_struct(base)
    fs = eng.flux_scale(sci['wcs'], base, 1.0)
    ony, onx = coadd.img.shape
    al = torch.empty((2, ony, onx), dtype=torch.float32, device=device)        # the two aligned frames of (b)
    alw = torch.empty((ony, onx), dtype=torch.float32, device=device)
    # index tensors of the crops, zero padded outside the grid
    gx = torch.from_numpy(x0.astype(np.int64))[:, None, None] + torch.arange(S)[None, None, :]
    gy = torch.from_numpy(y0.astype(np.int64))[:, None, None] + torch.arange(S)[None, :, None]
    inside = ((gx >= 0) & (gx < onx) & (gy >= 0) & (gy < ony)).to(device)
    gx, gy = gx.clamp(0, onx - 1).expand(n, S, S).to(device), gy.clamp(0, ony - 1).expand(n, S, S).to(device)

    def resample2():
        for k, plane in enumerate((sub.diff, sci['img'])):
            check(eng.L.zm_resample_dev(eng.ctx, plane.data_ptr(), None, None, C.byref(ws), C.byref(wr), 3, float(fs),
                                        al[k].data_ptr(), alw.data_ptr(), None), 'zm_resample_dev')

    def whole():
        resample2()
        three = torch.stack([al[0], al[1], coadd.img])
        blocks = torch.where(inside[None], three[:, gy, gx], torch.zeros((), device=device)).permute(1, 0, 2, 3).contiguous()
        norms = torch.sqrt((blocks.double() ** 2).sum(dim=(2, 3)))
        return blocks.cpu().numpy(), norms.cpu().numpy()

    def stamps():
        b, nrm, _, _ = sub.stamps(ra, dec, sci['img'], coadd.img)
        return b, nrm

    with torch.cuda.stream(stream):
        eng.set_stream(stream.cuda_stream)
        a_blocks, a_norms = stamps()
        b_blocks, b_norms = whole()
    same = bool(np.array_equal(a_blocks.view(np.uint32), b_blocks.view(np.uint32)))
    fn = {'stamps': stamps, 'whole': whole, 'whole_resample': resample2, 'subtract': subtract}
    times = {k: [] for k in fn}
    with torch.cuda.stream(stream):
        for it in range(args.warmup + args.steps):
            for name in ('stamps', 'whole', 'whole_resample', 'subtract'):        # interleaved: one call of each per turn
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn[name]()
                b.record(stream)
                b.synchronize()
                if it >= args.warmup:
                    times[name].append(a.elapsed_time(b))
    med = {k: float(np.median(v)) for k, v in times.items()}
    lo, hi = np.percentile(times['whole'], [16, 84])
    alo, ahi = np.percentile(times['stamps'], [16, 84])
    out = dict(size=size, frames=args.frames, steps=args.steps, stamps=n, stamp_size=S, blocks_equal=same,
               stamps_ms=round(med['stamps'], 4), stamps_ms_min=round(min(times['stamps']), 4),
               stamps_spread_ms=round(float(ahi - alo) / 2, 4),
               whole_ms=round(med['whole'], 4), whole_ms_min=round(min(times['whole']), 4),
               whole_spread_ms=round(float(hi - lo) / 2, 4), whole_resample_ms=round(med['whole_resample'], 4),
               subtract_ms=round(med['subtract'], 4), stamps_over_whole=round(med['stamps'] / med['whole'], 3),
               not_slower=bool(med['stamps'] <= med['whole'] + float(hi - lo) / 2))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
