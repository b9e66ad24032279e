#!/usr/bin/env python
"""Time the source extractor on a resident difference image of the bench's synthetic step.

    python tools/extract_probe.py [--size 3072] [--frames 8] [--steps 20] [--out FILE.json]

Builds the bench's synthetic science epoch and a reference coadded from ``--frames`` of its frames (bench.py's
``make_device_frames`` and defect mask), runs the device-resident subtraction, then times on the same stream, with HIP
events, per call:

* ``subtract_ms``  the subtraction leg (``DeviceSubtraction.run``);
* ``extract_ms``   ``DeviceSubtraction.extract`` on the resident difference, noise and mask planes (object table to the
  host included);
* ``extract_param_ms``  the same call with ``columns='param'``: the second pass (``k_ex_kron``, ``k_ex_win``) and its
  table on top; ``param_over_default`` is its ratio to ``extract_ms`` of the same run;
* ``extract_deblend_ms``  the same call with ``deblend=True`` (``k_db_tree`` and a second numbering on top);
  ``deblend_over_default`` is its ratio to ``extract_ms`` of the same run, ``objects_deblend`` what it finds;
* ``crowded_ms`` / ``crowded_deblend_ms``  both calls on a crowded field of ``--crowded-size`` px a side: 3000 stars under
  noise 1, a third of them companions 3 .. 6 px from another star (``crowded_objects`` / ``crowded_objects_deblend``);
* ``extract_clean_ms`` / ``extract_deblend_clean_ms``  the default and the deblending call with ``clean=True`` on the
  bench's epoch (every object of the pass before numbered and measured, ``k_cl_stats``, the decision, and where anything
  is absorbed a second numbering and measurement); ``objects_clean`` / ``objects_deblend_clean`` what they find;
  ``crowded_clean_ms`` / ``crowded_deblend_clean_ms`` the same on the crowded field;
* ``mask``         the masked second pass (``mask='blank' | 'correct'``: ``k_ex_kron_m``, ``k_ex_win_m``, ``k_ex_aper_m``)
  beside the unmasked ``columns='param'`` call of the same build, per scene (``epoch``: the bench's epoch, ``crowded``:
  the crowded field; each also with ``deblend=True``): ``param_ms`` the unmasked call, ``blank_ms`` / ``correct_ms`` the
  masked ones, ``*_over_param`` their ratios, ``objects`` the rows measured and ``crowded_rows`` how many of them the
  masked pass flags (FLAGS bit 1);
* ``decide_ms``    ``zm_clean_decide`` alone (model on the host, upload, ``k_cl_pairs``, ``k_cl_resolve``, two arrays back) on
  synthetic tables of 10^3, 10^4 and 10^5 rows at the surface density of the crowded field (``decide_absorbed``: how many
  rows were absorbed); the all-pairs kernel is quadratic in the rows;
* ``copy_ms``      a float4 copy (``zm_copy_probe_dev``) that moves the bytes of the planes the extractor has to touch
  at least once: image, noise, flag plane, segmentation map (4 B per pixel each) and the bad-pixel map (1 B).  The copy
  cycles through four source / destination pairs (640 MB in all at the default size), more than the 256 MB last-level
  cache holds, so that no call finds its source there from the call before;
* ``whole_frame_object_ms``  one extraction of a frame that is a single object (every pixel above the threshold): the
  worst case of the per-object walk, one workgroup over the whole bounding box.

The frame is square because the bench's synthetic frames are (``bench.make_device_frames``).

Prints one JSON line with the three clocks and the two ratios.  For the per-kernel table run it under
``rocprofv3 --kernel-trace --stats -- python tools/extract_probe.py --steps 5``.
"""
import argparse
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
    ap.add_argument('--crowded-size', type=int, default=1024)
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
    size = args.size
    base, frames = bench.make_device_frames(synth, torch, args.frames + 1, size, 2000, device, 'int16')
    sci = frames.pop()
    g = torch.Generator(device='cpu')
    g.manual_seed(77)
    bx = torch.randint(2, size - 2, (300,), generator=g)
    by = torch.randint(2, size - 2, (300,), generator=g)
    smask = torch.zeros((size, size), dtype=torch.int16)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            smask[by + dy, bx + dx] = 256
    sci['mask'] = smask.to(device)
    sci['wgt'] = torch.where(sci['mask'] != 0, 0.0, float(sci['wgt'].max())).to(torch.float32)
    sci['rms'] = torch.where(sci['wgt'] > 0, 1.0 / torch.sqrt(sci['wgt'].clamp_min(1e-20)),
                             float(np.sqrt(50000.0))).to(torch.float32)
    params = z.coadd_params(combine='CLIPPED', subtract_back=True, rescale_weights=True)
    coadd = dev.DeviceCoadd(base, params, device=0, engine=eng, want_mask=True)
    sub = dev.DeviceSubtraction(sci['wcs'], base, device=0, engine=eng, stream=coadd.stream)
    npx = coadd.img.numel()
    ref_rms = torch.empty_like(coadd.wgt)
    coadd.run(dev.DeviceFrames(frames, device))
    with torch.cuda.stream(coadd.stream):
        check(eng.L.zm_mask_flag_dev(eng.ctx, coadd.mask.data_ptr(), coadd.mask_wgt.data_ptr(), 0.0, 1 << 16, npx))
        check(eng.L.zm_add_scalar_dev(eng.ctx, coadd.img.data_ptr(), 150.0, npx))
        check(eng.L.zm_rms_from_weight_dev(eng.ctx, coadd.wgt.data_ptr(), None, npx, float(np.sqrt(50000.0)),
                                           ref_rms.data_ptr()))
    seeing = 4.0                      # bench.py --seeing default

    def subtract():
        sub.run(sci['img'], sci['rms'], sci['mask'], sci['wgt'], coadd.img, ref_rms, coadd.mask, seeing=seeing, nreg_side=3)

    found = {}

    def extract():
        tab, nfound, _ = sub.extract()
        found['n'] = nfound

    def extract_param():
        tab, nfound, _ = sub.extract(columns='param')
        found['wide'] = len(tab.dtype.names)

    def extract_deblend():
        tab, nfound, _ = sub.extract(deblend=True)
        found['deblend'] = nfound

    def extract_clean():
        tab, nfound, _ = sub.extract(clean=True)
        found['clean'] = nfound

    def extract_deblend_clean():
        tab, nfound, _ = sub.extract(deblend=True, clean=True)
        found['deblend_clean'] = nfound

    # the crowded field: 2000 stars and 1000 companions 3 .. 6 px from one of them, noise 1
    csize = args.crowded_size
    rng = np.random.default_rng(31)
    cx, cy = rng.uniform(5, csize - 5, 2000), rng.uniform(5, csize - 5, 2000)
    sep, ang = rng.uniform(3.0, 6.0, 1000), rng.uniform(0.0, 2.0 * np.pi, 1000)
    cx = np.concatenate([cx, cx[:1000] + sep * np.cos(ang)])
    cy = np.concatenate([cy, cy[:1000] + sep * np.sin(ang)])
    field = rng.normal(0.0, 1.0, (csize, csize))
    synth.add_stars(field, cx, cy, 10 ** rng.uniform(2.3, 4.0, 3000), 2.4)
    cimg = torch.from_numpy(field.astype(np.float32)).to(device)
    cone = torch.ones((csize, csize), dtype=torch.float32, device=device)

    def crowded():
        tab, found['crowded'] = eng.extract_dev(cimg.data_ptr(), cone.data_ptr(), None, None, csize, csize)

    def crowded_deblend():
        tab, found['crowded_deblend'] = eng.extract_dev(cimg.data_ptr(), cone.data_ptr(), None, None, csize, csize, deblend=True)

    def crowded_clean():
        tab, found['crowded_clean'] = eng.extract_dev(cimg.data_ptr(), cone.data_ptr(), None, None, csize, csize, clean=True)

    def crowded_deblend_clean():
        tab, found['crowded_deblend_clean'] = eng.extract_dev(cimg.data_ptr(), cone.data_ptr(), None, None, csize, csize,
                                                              deblend=True, clean=True)

    def masked_scene(call, **kw):
        """Medians of the unmasked wide call and of both masked ones on one scene."""
        res, seen = {}, {}
        for key, more in (('param', {}), ('blank', dict(mask='blank')), ('correct', dict(mask='correct'))):
            def fn():
                seen[key] = call(columns='param', **kw, **more)
            res[key + '_ms'] = round(clock(fn)[0], 4)
        res['blank_over_param'] = round(res['blank_ms'] / res['param_ms'], 2)
        res['correct_over_param'] = round(res['correct_ms'] / res['param_ms'], 2)
        res['objects'] = int(len(seen['correct']))
        res['crowded_rows'] = int((seen['correct']['FLAGS'] & 1).sum() - (seen['param']['FLAGS'] & 1).sum())
        res['replaced_rows'] = int((seen['correct']['NREPL_AUTO'] > 0).sum())
        return res

    def epoch_table(**kw):
        return sub.extract(**kw)[0]

    def crowded_table(**kw):
        return eng.extract_dev(cimg.data_ptr(), cone.data_ptr(), None, None, csize, csize, **kw)[0]

    def decide_table(n):
        """n synthetic rows at the crowded field's surface density (1505 objects on 1024 x 1024): one in ten bright and
        extended, the rest faint and compact."""
        trng = np.random.default_rng(1000 + n)
        side = csize * np.sqrt(n / 1505.0)
        rows = np.zeros(n, np.dtype(z._lib.zm_object))
        rows['number'] = np.arange(1, n + 1)
        rows['x_image'], rows['y_image'] = trng.uniform(1, side, n), trng.uniform(1, side, n)
        big = trng.random(n) < 0.1
        a = np.where(big, trng.uniform(3.0, 8.0, n), trng.uniform(0.6, 1.5, n))
        b = a * trng.uniform(0.5, 1.0, n)
        th = trng.uniform(-np.pi / 2, np.pi / 2, n)
        rows['x2'] = a * a * np.cos(th) ** 2 + b * b * np.sin(th) ** 2
        rows['y2'] = a * a * np.sin(th) ** 2 + b * b * np.cos(th) ** 2
        rows['xy'] = (a * a - b * b) * np.sin(th) * np.cos(th)
        rows['a_image'], rows['b_image'] = a, b
        rows['npix'] = np.maximum(5, (np.pi * a * b * trng.uniform(2.0, 4.0, n)).astype(np.int32))
        rows['first'] = trng.permutation(n).astype(np.int32)
        F = np.where(big, 10 ** trng.uniform(4.0, 6.0, n), 10 ** trng.uniform(1.8, 3.0, n)) * rows['npix'] / 10.0
        return rows, F, np.full(n, 6.0, np.float32), trng.uniform(0.5, 6.0, n).astype(np.float32)

    nbytes = (17 * size * size // 2) // 16 * 16
    pairs = [(torch.zeros(nbytes, dtype=torch.uint8, device=device), torch.empty(nbytes, dtype=torch.uint8, device=device))
             for _ in range(4)]
    turn = [0]

    def copy():
        src, dst = pairs[turn[0] % len(pairs)]
        turn[0] += 1
        check(eng.L.zm_copy_probe_dev(eng.ctx, src.data_ptr(), dst.data_ptr(), nbytes))

    def clock(fn):
        with torch.cuda.stream(coadd.stream):
            for _ in range(args.warmup):
                fn()
            times = []
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(coadd.stream)
                fn()
                b.record(coadd.stream)
                b.synchronize()
                times.append(a.elapsed_time(b))
        return float(np.median(times)), float(np.min(times))

    s_med, s_min = clock(subtract)
    e_med, e_min = clock(extract)
    p_med, p_min = clock(extract_param)
    d_med, d_min = clock(extract_deblend)
    cr_med, _ = clock(crowded)
    crd_med, _ = clock(crowded_deblend)
    ec_med, ec_min = clock(extract_clean)
    edc_med, edc_min = clock(extract_deblend_clean)
    crc_med, _ = clock(crowded_clean)
    crdc_med, _ = clock(crowded_deblend_clean)
    mask = dict(epoch=masked_scene(epoch_table), epoch_deblend=masked_scene(epoch_table, deblend=True),
                crowded=masked_scene(crowded_table), crowded_deblend=masked_scene(crowded_table, deblend=True))
    decide_ms, decide_absorbed = {}, {}
    keep_steps = (args.steps, args.warmup)
    for n in (1000, 10000, 100000):
        table = decide_table(n)

        def decide():
            into, _ = eng.clean_decide(*table)
            decide_absorbed[str(n)] = int((into > 0).sum())
        args.steps, args.warmup = (5, 1) if n >= 100000 else keep_steps
        decide_ms[str(n)] = round(clock(decide)[0], 4)
    args.steps, args.warmup = keep_steps
    c_med, c_min = clock(copy)
    flat = torch.full((size, size), 100.0, dtype=torch.float32, device=device)
    one = torch.ones((size, size), dtype=torch.float32, device=device)
    torch.cuda.synchronize()

    def whole():
        tab, nfound = eng.extract_dev(flat.data_ptr(), one.data_ptr(), None, None, size, size, filter=False)
        assert nfound == 1 and tab['ISOAREA_IMAGE'][0] == size * size
    args.steps, args.warmup, keep = 3, 1, (args.steps, args.warmup)
    w_med, _ = clock(whole)
    args.steps, args.warmup = keep
    out = dict(size=size, whole_frame_object_ms=round(w_med, 3), frames=args.frames, steps=args.steps, objects=found.get('n'),
               subtract_ms=round(s_med, 4), subtract_ms_min=round(s_min, 4),
               extract_ms=round(e_med, 4), extract_ms_min=round(e_min, 4),
               extract_param_ms=round(p_med, 4), extract_param_ms_min=round(p_min, 4), param_columns=found.get('wide'),
               param_over_default=round(p_med / e_med, 2),
               extract_deblend_ms=round(d_med, 4), extract_deblend_ms_min=round(d_min, 4), objects_deblend=found.get('deblend'),
               deblend_over_default=round(d_med / e_med, 2), crowded_size=csize, crowded_ms=round(cr_med, 4),
               crowded_deblend_ms=round(crd_med, 4), crowded_objects=found.get('crowded'),
               crowded_objects_deblend=found.get('crowded_deblend'),
               extract_clean_ms=round(ec_med, 4), extract_clean_ms_min=round(ec_min, 4), objects_clean=found.get('clean'),
               extract_deblend_clean_ms=round(edc_med, 4), extract_deblend_clean_ms_min=round(edc_min, 4),
               objects_deblend_clean=found.get('deblend_clean'), crowded_clean_ms=round(crc_med, 4),
               crowded_deblend_clean_ms=round(crdc_med, 4), crowded_objects_clean=found.get('crowded_clean'),
               crowded_objects_deblend_clean=found.get('crowded_deblend_clean'), decide_ms=decide_ms,
               decide_absorbed=decide_absorbed, mask=mask,
               copy_ms=round(c_med, 4), copy_bytes_per_pixel=17,
               extract_over_subtract=round(e_med / s_med, 3), extract_over_copy=round(e_med / c_med, 2))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
