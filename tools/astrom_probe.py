"""The astrometric refit at the scale it is meant for: ``zm_astrom_solve_dev`` on synthetic frames with rows resident in
HBM, and on the same box the float64 restatement (tests/astrom_ref.py) on a sample of the frames.  Two cases:

* ``stack``: 32 dithered frames of 3072 x 3072 pixels with 3000 stars each, one field, one catalogue;
* ``night``: 1000 frames of 3072 x 3072 pixels with 1000 stars each, 50 fields, one catalogue of all fields.

Every GPU step runs in a child process under its own time limit; a child that does not end in time is killed and its
case is reported as not measured.  Writes one JSON document (default profiles/astrom_probe.json) with the measured
times and the counted work: pairs tested by the vote, bytes read per fit.

usage: astrom_probe.py [--out profiles/astrom_probe.json] [--cases stack,night] [--limit 300]"""
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
CASES = dict(stack=dict(nframes=32, nfields=1, nstars=3000, naxis=3072, sample=2),
             night=dict(nframes=1000, nfields=50, nstars=1000, naxis=3072, sample=2))


def scene(nframes, nfields, nstars, naxis, seed=1, **_):
    """(headers as given to the solver, detections per frame, catalogue, field of every frame, stars per field)"""
    import astrom_ref as am
    rng = np.random.default_rng(seed)
    ras, decs, owner = [], [], []
    bases = []
    for k in range(nfields):
        base = am.tan_header(crval=(20.0 + 6.0 * (k % 10), -20.0 + 8.0 * (k // 10)), naxis=(naxis, naxis), scale=1.01)
        x, y = rng.uniform(-40, naxis + 40, int(nstars * 1.1)), rng.uniform(-40, naxis + 40, int(nstars * 1.1))
        ra, dec = base.pix2sky(x, y)
        bases.append(base)
        ras.append(ra)
        decs.append(dec)
        owner.append(np.full(ra.size, k))
    ra, dec, owner = np.concatenate(ras), np.concatenate(decs), np.concatenate(owner)
    headers, dets, field = [], [], []
    for f in range(nframes):
        k = f % nfields
        true = am.perturbed(am.tpv_truth(bases[k], 1000 + f), dpix=rng.uniform(-15, 15, 2), keep_pv=True)
        x, y = true.sky2pix(ra[owner == k], dec[owner == k])
        inside = (x > 1) & (x < naxis) & (y > 1) & (y < naxis)
        x, y = x[inside] + rng.normal(0, 0.03, inside.sum()), y[inside] + rng.normal(0, 0.03, inside.sum())
        dets.append((x, y, np.full(x.size, 0.03), rng.uniform(10, 500, x.size)))
        headers.append(am.perturbed(bases[k], dpix=true.crpix - bases[k].crpix + rng.uniform(-12, 12, 2), angle=0.01))
        field.append(k)
    return headers, dets, (ra, dec, np.full(ra.size, 0.01)), np.array(field), owner


def child(case, out):
    import torch
    import astrom_ref as am
    z = importlib.import_module('zuds-pipeline_amd')
    s = importlib.import_module('zuds-pipeline_amd.scamp')
    cfg = CASES[case]
    headers, dets, ref, field, owner = scene(**cfg)
    eng = z.get_engine(0)
    dev = torch.device('cuda', 0)
    wl = [z.WCS(w.crpix, w.crval, w.cd, naxis=w.naxis) for w in headers]
    cols = [torch.from_numpy(np.concatenate([d[k] for d in dets])).to(dev) for k in range(4)]
    offsets = np.concatenate([[0], np.cumsum([d[0].size for d in dets])]).astype(np.int32)
    rd = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in ref]
    times = []
    for _ in range(4):                                      # the first call allocates the context's scratch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, infos = s.solve_dev(wl, offsets, *cols, *rd, engine=eng)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    status = {}
    for i in infos:
        status[i['status']] = status.get(i['status'], 0) + 1
    # counted work: the vote tests every (selected detection, star inside the frame's box grown by P) pair; a fit reads
    # five fp64 values per matched row and pass (normal equations, then residuals) and one byte of keep
    nsel = np.array([min(d[0].size, 1024) for d in dets])
    ninside = np.array([(owner == k).sum() for k in field])
    doc = dict(case=case, **cfg, rows=int(offsets[-1]), catalogue=int(ref[0].size), gpu_ms=times[1:], gpu_first_call_ms=times[0],
               status=status, rounds=[int(np.min([i['rounds'] for i in infos])), int(np.max([i['rounds'] for i in infos]))],
               vote_pairs=int((nsel * ninside).sum()),
               fit_bytes_per_pass=int(sum(int(i['nmatch']) for i in infos) * (5 * 8 + 1)))
    t_ref, agree = [], True
    for f in range(cfg['sample']):                          # the restatement sees only the stars of the frame's field
        k = owner == field[f]
        t0 = time.perf_counter()
        r = am.solve_frame(headers[f], *dets[f], ref[0][k], ref[1][k], ref[2][k])
        t_ref.append(1e3 * (time.perf_counter() - t0))
        agree = agree and am.STATUS[r['status']] == infos[f]['status'] and r['nused'] == infos[f]['nused']
    doc.update(restatement_ms_per_frame=t_ref, restatement_frames=cfg['sample'], restatement_agrees=bool(agree),
               restatement_note="numpy, one frame at a time, given only the stars of the frame's field")
    with open(out, 'w') as fh:
        json.dump(doc, fh)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'astrom_probe.json'))
    ap.add_argument('--cases', default='stack,night')
    ap.add_argument('--limit', type=int, default=300, help='seconds per child process')
    ap.add_argument('--child')
    ap.add_argument('--child-out')
    args = ap.parse_args(argv)
    if args.child:
        child(args.child, args.child_out)
        return 0
    doc = dict(tool='tools/astrom_probe.py', cases=[])
    for case in args.cases.split(','):
        tmp = args.out + f'.{case}.part'
        cmd = [sys.executable, os.path.abspath(__file__), '--child', case, '--child-out', tmp]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc == 0 and os.path.exists(tmp):
            with open(tmp) as fh:
                doc['cases'].append(json.load(fh))
            os.remove(tmp)
        else:
            doc['cases'].append(dict(case=case, measured=False, returncode=rc))
            if rc in (124, 134, 137, 139, -6, -9, -11):     # a child that hung or died on the GPU: start nothing more
                break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(doc, fh, indent=1)
        fh.write('\n')
    print(json.dumps(doc, indent=1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
