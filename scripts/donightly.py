#!/usr/bin/env python
"""Nightly subtractions + forced photometry: the job of the reference's
``scripts/donightly.py`` (per image: ``dosub.do_one``) followed by ``scripts/dophot.py``
(``raw_aperture_photometry`` at known sky positions), database-free, with the kernel fits of B
subtractions as one batch of launches on each of J lanes (``nightly.SubtractionPool(J, batch=B)``;
``--fit-batch 0``: J separate subtractions in flight).

usage: donightly.py images.txt ref.fits [positions.txt] [--jobs J] [--fit-batch B] [--batch FRAMES] [--nreg-side N]
                    [--detect [--stamps] [--deblend] [--clean [--clean-param X]] [--rb-model BASE [--rb-cut X]] [--associate [--stars F]]]
                    [--maglim] [--psf] [--fakes [N] [--fake-mags A,B] [--fake-seed S]]

* ``images.txt``: science image paths (``*sciimg.fits``; the mask is ``*mskimg.fits``; a
  ``.weight.fits`` sibling is required: 1 / rms^2, 0 on bad pixels).  The list is sharded over
  ranks as ``zuds.get_my_share_of_work`` does (RANK / WORLD_SIZE, one rank per GPU).
* ``ref.fits`` with ``ref.mask.fits`` and ``ref.weight.fits`` next to it.
* ``positions.txt``: ``ra dec`` per line (degrees); forced r = 3 px apertures are measured on
  every difference image and written to ``<sub>.phot.txt``
  (columns of the reference's photometry table: ra dec flux fluxerr flags zp obsjd).

Products per image, with the reference's names: ``sub.<sci>_<ref>.fits``, ``.rms.fits``,
``.mask.fits`` next to the science image.  An image whose subtraction exists is skipped
(the reference's checkpoint by name, ``scripts/dosub.py:85-94``).

``--detect``: every subtraction also gets its filtered detection catalog ``sub.*.cat`` (FITS_LDAC, the file of
``dosub.py --detect``: what ``dosub.do_one`` hands back to the reference's night), made on the planes in HBM
(``DeviceSubtraction.candidates``).  ``--stamps`` (needs ``--detect``): and ``sub.*.stamps.fits``, the thumbnails of
its ``GOODCUT == 1`` rows in the layout of ``dosub.py --stamps``; more than 50 such rows: no stamps file (the
reference's TooManyDetectionsError).  ``--deblend`` (needs ``--detect``): the extraction deblends (``DEBLEND_NTHRESH`` 32,
``DEBLEND_MINCONT`` 0.005; DESIGN.md "Deblending"): the tables carry ``PARENT_NUMBER`` and the headers say ``ZMDEBLND = T``.
``--clean`` (needs ``--detect``): the extraction ends with the CLEAN pass (``CLEAN_PARAM`` 1.0, or ``--clean-param X``;
DESIGN.md "CLEAN"): the tables carry ``NMERGED`` and the headers say ``ZMCLEAN = T`` and ``ZMCLNPAR``.
``--maglim``: every ``sub.*.fits`` gets a ``MAGLIM`` card, 5 sigma in an r = 3 px aperture, measured by the pool on the noise
plane and mask in HBM (``SubtractionJob(maglim=True)`` -> ``DeviceSubtraction.maglim``) with ``MAGZP + APCOR4`` of the science
header; a frame without those cards gets a warning and no card.
``--psf``: the PSF model of every science frame is built from its own stars (``psf.build_psf_planes``; DESIGN.md, "PSF
photometry"), written as ``<sci>.psf.fits`` and copied as ``sub.*.psf.fits``; its cards go into the subtraction's header.
``--fakes [N]`` (needs ``--detect`` and a PSF model: ``--psf``, or an existing ``<sci>.psf.fits``): the detection efficiency
of every subtraction is measured with N (200) fake sources (``SubtractionJob(fakes=...)`` -> ``fakes.recover_dev``; DESIGN.md,
"Fake sources"): uniform in ``MAGLIM - 2.5 .. MAGLIM + 1`` of the science header (or ``--fake-mags A,B``), seed 0
(``--fake-seed S``).  ``sub.*.fakes.csv`` is written and ``sub.*.fits`` gets ``FAKEN``, ``FAKESEED``, ``FAKEM50``, ``FAKEM80``.
Such jobs run on per-job workers (``--fit-batch`` is ignored).  The other products are the same bytes.
``--associate`` (needs ``--detect``): once the pool has drained, the night's
in-memory tables go through ``zuds.associate`` (the job of ``nersc/makesources.py``; ``scripts/makesources.py`` does the
same from the ``sub.*.cat`` files) and ``<images>.sources.txt`` / ``<images>.sources.det.txt`` are written next to the
image list; ``--stars F``: ``ra dec`` per line, the star veto."""
import argparse
import importlib
import os
import sys
import time
import traceback

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zuds_amd as zuds

zuds.init_db()


def load_reference(io, refname):
    """The reference planes in HBM: image, rms (1 / sqrt(w), BIG_RMS where bad: zuds/image.py:173-208)
    and mask."""
    import torch
    img, hdr = io.load(refname, 'f32')
    wgt, _ = io.load(refname.replace('.fits', '.weight.fits'), 'f32')
    mask, _ = io.load(refname.replace('.fits', '.mask.fits'), 'i32')
    eng = io.engine
    rms = torch.empty_like(img)
    bad = torch.empty(mask.shape, dtype=torch.uint8, device=mask.device)
    with torch.cuda.stream(io.stream):
        zuds._lib.check(eng.L.zm_mask_bad_dev(eng.ctx, mask.data_ptr(), None, zuds.BAD_SUM, mask.numel(),
                                              None, bad.data_ptr()))
        zuds._lib.check(eng.L.zm_rms_from_weight_dev(eng.ctx, wgt.data_ptr(), bad.data_ptr(), wgt.numel(),
                                                     float(zuds.BIG_RMS), rms.data_ptr()))
    io.stream.synchronize()
    return dict(img=img, rms=rms, mask=mask, wcs=zuds.WCS.from_header(hdr),
                flxscale=float(hdr.get('FLXSCALE', 1.0)), header=hdr, path=refname)


def science_files(fn):
    """The three files of a science frame, as the ring / the device loader take them."""
    return [(fn, 'f32'), (fn.replace('sciimg', 'mskimg'), 'i32'), (fn.replace('.fits', '.weight.fits'), 'f32')]


def finish_science(io, fn, img, hdr, mask, wgt):
    """Behind the loads, on ``io.stream`` (not waited for): rms = 1 / sqrt(w), BIG_RMS where the mask is bad or the
    pixel saturated (zuds/image.py:173-208)."""
    import torch
    if 'SEEING' not in hdr:
        raise RuntimeError(f'{fn}: no SEEING card (run estimate_seeing on the frame first)')
    eng = io.engine
    eng.set_stream(io.stream.cuda_stream)
    with torch.cuda.stream(io.stream):
        rms = torch.empty_like(img)
        bad = torch.empty(mask.shape, dtype=torch.uint8, device=mask.device)
        zuds._lib.check(eng.L.zm_mask_bad_dev(eng.ctx, mask.data_ptr(), None, zuds.BAD_SUM, mask.numel(),
                                              None, bad.data_ptr()))
        zuds._lib.check(eng.L.zm_rms_from_weight_dev(eng.ctx, wgt.data_ptr(), bad.data_ptr(), wgt.numel(),
                                                     float(zuds.BIG_RMS), rms.data_ptr()))
        if 'SATURATE' in hdr:         # zuds/image.py:203-204
            rms = torch.where(img >= 0.9 * float(hdr['SATURATE']), torch.full_like(rms, float(zuds.BIG_RMS)), rms)
    return dict(img=img, rms=rms, mask=mask, wgt=wgt, wcs=zuds.WCS.from_header(hdr),
                seeing=float(hdr['SEEING']), flxscale=float(hdr.get('FLXSCALE', 1.0)), header=hdr, path=fn)


def load_science(io, fn):
    """One frame, serially (the ring of ``run_night`` loads a batch ahead instead)."""
    (img, hdr), (mask, _), (wgt, _) = (io.load(p, k) for p, k in science_files(fn))
    sci = finish_science(io, fn, img, hdr, mask, wgt)
    io.stream.synchronize()
    return sci


def science_psf(io, fn, sci, build):
    """The PSF model of a science frame: built from its own stars on the planes the ring decoded (``--psf``: the planes go
    to the host once, ``psf.build_psf_planes``) and written as ``<sci>.psf.fits``, or read from that file."""
    path = fn.replace('.fits', '.psf.fits')
    if not build:
        return zuds.PSFModel.from_file(path)
    io.stream.synchronize()
    sat = sci['header'].get('SATURATE')
    res = zuds.psf.build_psf_planes(sci['img'].cpu().numpy(), mask=sci['mask'].cpu().numpy(), rms=sci['rms'].cpu().numpy(),
                                    saturate=float(sat) if sat else None, engine=io.engine)
    res['psf'].save(path)
    return res['psf']


def _load_dosub():
    """scripts/dosub.py as a module: it owns the layout of the stamps file and the guard MAX_DETS."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('dosub', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dosub.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dosub = _load_dosub()
MAX_DETS = dosub.MAX_DETS         # more detections than this on one subtraction and it gets no stamps


def write_detections(out, hdr, ref, res):
    """``sub.*.cat`` and ``sub.*.stamps.fits`` of one result (``SubtractionJob(detect=True, stamps=...)``)."""
    name = os.path.basename(out)
    if res.get('cat') is None:
        print(f'{name}: no detections: {res.get("detect_error")}', flush=True)
        return
    cat = zuds.PipelineFITSCatalog()
    cat.basename = name.replace('.fits', '.cat')
    cat.map_to_local_file(out.replace('.fits', '.cat'))
    cat.data, cat.header, cat.header_comments = res['cat'], dict(hdr), {}
    cat.deblend = res.get('deblend')
    cat.clean = res.get('clean')
    cat.save()
    if res.get('too_many'):
        print(f'Error: {int((res["cat"]["GOODCUT"] == 1).sum())} detections (>{MAX_DETS}) '
              f'on "{name}", something wrong with the image probably', flush=True)
    elif 'stamps_error' in res:
        print(f'{name}: no stamps: {res["stamps_error"]}', flush=True)
    elif 'stamps' in res:
        st = res['stamps']
        thumbs = importlib.import_module('zuds-pipeline_amd.thumbnails')
        gnx, gny = (int(v) for v in ref['wcs'].naxis)
        size = st['blocks'].shape[-1]
        trimmed = []
        for x0, y0 in zip(st['x0'], st['y0']):
            (sy, sx), _ = thumbs.trim_slices(int(x0), int(y0), size, gnx, gny)
            trimmed.append((sx.stop - sx.start, sy.stop - sy.start))
        dosub.write_stamp_blocks(out.replace('.fits', '.stamps.fits'), st['blocks'], st['ra'], st['dec'], st['x0'],
                                    st['y0'], trimmed)


def write_products(io, sci, ref, res):
    """``io``: anything with ``save(path, tensor, header)`` - the ring (files written behind the caller's back,
    ``flush`` waits for them) or a ``FITSDeviceIO`` (each file written before the call returns)."""
    out = zuds.sub_name(sci['path'], ref['path'])
    hdr = dict(sci['header'])
    hdr.update(zuds.hotpants.info_cards(res['info']))    # KSUM00, NSTAMPS, ZMSTATUS, ZMUNSOLV, ZMRETRY
    ml = res.get('maglim')
    if ml is not None:
        # --maglim: measured by the pool on the planes in HBM (DeviceSubtraction.maglim) with the science header's zero point
        if np.isfinite(ml['maglim']):
            hdr['MAGLIM'] = float(ml['maglim'])
        else:
            print(f'{os.path.basename(out)}: no usable aperture on the noise plane, MAGLIM is not written', flush=True)
    model = sci.get('psf_built')
    if model is not None:
        # --psf: the science frame's model beside the subtraction, its cards in the header (as dosub.py --psf)
        hdr.update(model.cards)
        model.save(out.replace('.fits', '.psf.fits'))
    if res.get('fakes_error'):
        print(f'{os.path.basename(out)}: no efficiency from fakes: {res["fakes_error"]}', flush=True)
    if res.get('fakes') is not None:
        # --fakes: the matched table, and where the efficiency curve went
        zuds.write_fakes_csv(out.replace('.fits', '.fakes.csv'), res['fakes'])
        # (the cards go on the subtraction alone: its rms map and catalog keep the header of a run without --fakes)
        fhdr = dict(hdr)
        dosub.write_fake_cards(fhdr, None, sci['fake_settings'], res['efficiency'])
        e = res['efficiency']
        print(f'{os.path.basename(out)}: {int(e["nrec"].sum())} of {e["nused"]} fakes recovered, m50 {e["m50"]:.3f}', flush=True)
    io.save(out, res['diff'], fhdr if res.get('fakes') is not None else hdr)
    io.save(out.replace('.fits', '.rms.fits'), res['noise'], hdr)
    mh = dict(sci['header'])
    mh['BIT17'] = 17
    io.save(out.replace('.fits', '.mask.fits'), res['mask'], mh)
    if 'phot' in res:
        p = res['phot']
        zp = float(hdr.get('MAGZP', 0.0)) + float(hdr.get(zuds.APER_KEY, 0.0))
        jd = float(hdr.get('OBSJD', 0.0))
        ra, dec = sci['radec']
        # (np.savetxt's bytes - '# ' + header, one '%'-formatted row per line - without its per-row overhead: 1.6 -> 0.3 ms
        # per table, which at 2 ms per subtraction is host time that matters)
        fmt = '%.8f %.8f %.6e %.6e %d %.5f %.6f\n'
        rows = zip(ra.tolist(), dec.tolist(), np.asarray(p['flux'], dtype=np.float64).tolist(),
                   np.asarray(p['fluxerr'], dtype=np.float64).tolist(), np.asarray(p['flags']).tolist(),
                   [zp] * ra.size, [jd] * ra.size)
        with open(out.replace('.fits', '.phot.txt'), 'w') as fh:
            fh.write('# ra dec flux fluxerr flags zp obsjd\n' + ''.join([fmt % r for r in rows]))
    if 'cat' in res:
        write_detections(out, hdr, ref, res)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('infile')
    ap.add_argument('refname')
    ap.add_argument('positions', nargs='?')
    ap.add_argument('--jobs', type=int, default=3,
                    help='lanes (host thread, context, stream) working on the GPU at the same time; with --fit-batch 0: '
                         'subtractions in flight')
    ap.add_argument('--nreg-side', type=int, default=3)
    ap.add_argument('--batch', type=int, default=36, help='science frames resident at a time')
    ap.add_argument('--fit-batch', type=int, default=12,
                    help='kernel fits per launch chain (SubtractionPool(jobs, batch=N): --jobs lanes whose N fits run '
                         'as one batch, zm_subtract_batch_dev; measured on 32 subtractions of 3072^2: three lanes of '
                         '11 = 2.0 - 2.1 ms each whether the frames share one seeing or fall into three seeing '
                         'groups, two lanes of 16 1.95 / 2.8, 8 - 16 separate chains 3.0); 0: one chain per job')
    ap.add_argument('--detect', action='store_true', help='write the filtered detection catalog sub.*.cat of every subtraction')
    ap.add_argument('--stamps', action='store_true', help='with --detect: write sub.*.stamps.fits, the thumbnails of the detections')
    ap.add_argument('--deblend', action='store_true', help='with --detect: multi-threshold deblending (DEBLEND_NTHRESH 32, '
                                                           'DEBLEND_MINCONT 0.005); the catalogs say ZMDEBLND = T')
    ap.add_argument('--clean', action='store_true', help='with --detect: the CLEAN pass (CLEAN_PARAM 1.0); the catalogs say '
                                                         'ZMCLEAN = T')
    ap.add_argument('--clean-param', type=float, help='with --clean: CLEAN_PARAM, in [0.1, 10]')
    ap.add_argument('--rb-model', help='with --detect: BASE of BASE.architecture.json + BASE.weights.npz, the real / bogus '
                                       'network the candidate filter ends with (realbogus.load_model)')
    ap.add_argument('--rb-cut', type=float, help='with --rb-model: the score below which a candidate is cut; default '
                                                 'RB_CUT of the frame\'s FID / FILTERID card (a frame without one is an error)')
    ap.add_argument('--associate', action='store_true', help='with --detect: cluster the night\'s detections into sources '
                                                             'and write <images>.sources.txt / .sources.det.txt')
    ap.add_argument('--stars', help='with --associate: star catalogue (ra dec per line) for the 1.5 arcsec veto')
    ap.add_argument('--maglim', action='store_true', help='write MAGLIM into sub.*.fits: 5 sigma in an r = 3 px aperture, from the '
                                                          'subtraction\'s own noise plane and the MAGZP / APCOR4 of the science '
                                                          'header (a frame without them: a warning, no card)')
    ap.add_argument('--psf', action='store_true', help='build the PSF model of every science frame from its own stars: '
                                                       '<sci>.psf.fits, sub.*.psf.fits and the PSF* cards of sub.*.fits')
    ap.add_argument('--fakes', nargs='?', type=int, const=200, default=None, metavar='N',
                    help='with --detect and a PSF model (--psf, or <sci>.psf.fits): the detection efficiency from N (200) fake '
                         'sources; writes sub.*.fakes.csv and FAKEN / FAKESEED / FAKEM50 / FAKEM80')
    ap.add_argument('--fake-mags', metavar='A,B', help='with --fakes: the magnitude range (default MAGLIM - 2.5 .. MAGLIM + 1)')
    ap.add_argument('--fake-seed', metavar='S', help='with --fakes: the seed of the draw (default 0)')
    args = ap.parse_args(argv)
    if (args.fakes is not None or args.fake_mags is not None or args.fake_seed is not None) and not args.detect:
        print('--fakes needs --detect', file=sys.stderr)
        return 2
    fakes, err = dosub.check_fake_switches(args.fakes, args.fake_mags, args.fake_seed)      # (one validator for both drivers)
    if err:
        print(err, file=sys.stderr)
        return 2
    if (args.associate or args.stars) and not (args.detect and (args.associate or not args.stars)):
        print('--associate needs --detect (and --stars needs --associate)', file=sys.stderr)
        return 2
    if args.stamps and not args.detect:
        print('--stamps needs --detect', file=sys.stderr)
        return 2
    if args.deblend and not args.detect:
        print('--deblend needs --detect', file=sys.stderr)
        return 2
    if (args.clean or args.clean_param is not None) and not (args.detect and args.clean):
        print('--clean needs --detect (and --clean-param needs --clean)', file=sys.stderr)
        return 2
    clean = args.clean
    if args.clean_param is not None:
        try:
            clean = zuds.clean_settings(dict(param=args.clean_param))
        except ValueError as exc:
            print(f'--clean-param: {exc}', file=sys.stderr)
            return 2
    if (args.rb_model or args.rb_cut is not None) and not args.detect:
        print('--rb-model needs --detect', file=sys.stderr)
        return 2
    if args.rb_cut is not None and not args.rb_model:
        print('--rb-cut needs --rb-model', file=sys.stderr)
        return 2

    nightly = importlib.import_module('zuds-pipeline_amd.nightly')
    device = importlib.import_module('zuds-pipeline_amd.device')
    imgs = [str(f) for f in zuds.get_my_share_of_work(args.infile)]
    if fakes and not args.psf:
        missing = [fn for fn in imgs if not os.path.exists(fn.replace('.fits', '.psf.fits'))]
        if missing:
            print(f'--fakes needs a PSF model: --psf, or {os.path.basename(missing[0]).replace(".fits", ".psf.fits")} beside '
                  f'the frame ({len(missing)} frame(s) without one)', file=sys.stderr)
            return 2
    local = int(os.environ.get('LOCAL_RANK', '0'))
    import torch
    local %= max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    radec = None
    if args.positions:
        t = np.atleast_2d(np.loadtxt(args.positions))
        radec = (t[:, 0].copy(), t[:, 1].copy())

    io = device.FITSDeviceIO(local, engine=zuds.Engine(local))
    ref = load_reference(io, args.refname)
    # (a job with fakes runs on a per-job worker: SubtractionJob(fakes=...))
    pool = nightly.SubtractionPool(args.jobs, device=local, batch=1 if fakes else args.fit_batch)
    ring = importlib.import_module('zuds-pipeline_amd.fitsring').FITSRing(local)
    rb_model = zuds.load_model(args.rb_model) if args.rb_model else None
    tables = [] if args.associate else None
    try:
        done = run_night(imgs, ref, pool, io, ring, radec, batch=args.batch, nreg_side=args.nreg_side,
                         detect=args.detect, stamps=args.stamps, rb_model=rb_model, rb_cut=args.rb_cut, tables=tables,
                         deblend=args.deblend, clean=clean, maglim=args.maglim, psf=args.psf, fakes=fakes)
    finally:
        pool.close()
        ring.close()
    if args.associate:
        make_sources(tables, os.path.splitext(args.infile)[0] + '.sources', args.stars, engine=io.engine)
    return done


def make_sources(tables, prefix, stars=None, engine=None):
    """``--associate``: the night's tables (``(difference image, out['cat'])`` in the order the images were given) into
    sources, and the two tables of ``scripts/makesources.py``."""
    dets = []
    for out, cat in tables:
        dets += zuds.detections_from_cat(cat, image=os.path.basename(out).replace('.fits', '.cat'))
    star_pos = None
    if stars:
        t = np.atleast_2d(np.loadtxt(stars))
        star_pos = (t[:, 0].copy(), t[:, 1].copy()) if t.size else None
    sources = zuds.associate(dets, stars=star_pos, engine=engine)
    zuds.write_source_tables(sources, dets, prefix + '.txt', prefix + '.det.txt')
    print(f'{len(dets)} detections of {len(tables)} subtractions: {len(sources)} sources', flush=True)
    return sources


def run_night(imgs, ref, pool, io, ring, radec=None, batch=36, nreg_side=3, detect=False, stamps=False, rb_model=None,
              rb_cut=None, tables=None, deblend=False, clean=False, maglim=False, psf=False, fakes=None):
    """The images of this rank against one reference.  The files of batch b + 1 are read, sent and decoded by the
    ring (fitsring.FITSRing: reader threads, copy stream) while the pool subtracts batch b; the products of batch b
    are encoded on the device, copied back on a third stream and written by the ring's writer threads while
    batch b + 1 runs.  Returns the paths of the difference images, in order.  ``tables``: a list that receives
    ``(difference image, out['cat'])`` of every subtraction that has a catalog (``--associate``)."""
    nightly = importlib.import_module('zuds-pipeline_amd.nightly')
    refname = ref['path']
    chunks = [imgs[b0:b0 + batch] for b0 in range(0, len(imgs), batch)]

    def ask(b):
        todo = []
        for fn in chunks[b]:
            if os.path.exists(zuds.sub_name(fn, refname)):
                print(f'{os.path.basename(fn)}: subtraction exists, skipping', flush=True)
            else:
                todo.append(fn)
        wanted = [w for fn in todo for w in science_files(fn)]
        return todo, (ring.prefetch(wanted, [k == 'f32' and i % 3 == 0 for i, (_, k) in enumerate(wanted)],
                                    return_exceptions=True) if wanted else None)
    from concurrent.futures import ThreadPoolExecutor

    def finish(scis, results):
        # headers, photometry tables and the hand-over of the planes to the ring: host work of ~3 ms per image, done
        # on a thread of its own while the pool is at the next batch
        out = []
        for sci, res in zip(scis, results):
            if 'error' in res:
                # the job raised: no products, the night goes on
                print(f'{os.path.basename(sci["path"])}: subtraction failed: {res["error"]}', flush=True)
                continue
            if res['info']['status'] != 0:
                # some regions of the fit have no solution: their pixels carry the fill value and
                # bit 17; the products are written with ZMSTATUS / ZMUNSOLV in their headers
                print(f'{os.path.basename(sci["path"])}: {res["info"]["nunsolved"]} region(s) of the '
                      f'kernel fit unsolved (status {res["info"]["status"]}, '
                      f'{res["info"]["nstamps_used"]} stamps)', flush=True)
            out.append(write_products(ring, sci, ref, res))
            if tables is not None and res.get('cat') is not None:
                tables.append((out[-1], res['cat']))
        return out
    def prepare(todo, ticket):
        # the decoded planes of a batch -> its jobs (rms maps enqueued on io.stream and waited for): host work of
        # ~0.8 ms per frame, done for batch b + 1 on a thread of its own while the pool is at batch b
        t0 = time.time()
        loaded = ticket.result(io.stream) if ticket is not None else []
        t1 = time.time()
        scis, jobs = [], []
        for k, fn in enumerate(todo):
            trio = loaded[3 * k:3 * k + 3]
            try:
                for item in trio:
                    if isinstance(item, BaseException):
                        raise item
                (img, hdr), (mask, _), (wgt, _) = trio
                sci = finish_science(io, fn, img, hdr, mask, wgt)
                rbkw = {}
                if rb_model is not None:
                    # the filter id as image.py reads it; a frame without the card and no --rb-cut fails here (ValueError)
                    rbkw = dict(rb_model=rb_model, rb_cut=rb_cut, fid=hdr.get('FID', hdr.get('FILTERID')))
                if psf or fakes:
                    sci_model = science_psf(io, fn, sci, build=psf)
                    if psf:
                        sci['psf_built'] = sci_model
                if fakes:
                    if 'MAGZP' not in hdr or 'PSFCOR' not in sci_model.cards:
                        raise RuntimeError(f'{fn}: no MAGZP / PSFCOR: the fakes would have no zero point')
                    spec = dict(psf=sci_model, zp=float(hdr['MAGZP']) + float(sci_model.cards['PSFCOR']), N=fakes['n'],
                                SEED=fakes['seed'])
                    if fakes.get('mags'):
                        spec.update(MAG_MIN=fakes['mags'][0], MAG_MAX=fakes['mags'][1])
                    rbkw['fakes'] = spec
                job = nightly.SubtractionJob(sci, ref, radec=radec, nreg_side=nreg_side, tag=fn, detect=detect,
                                             stamps=stamps, max_detections=MAX_DETS, deblend=deblend, clean=clean, maglim=maglim,
                                             **rbkw)
                sci['fake_settings'] = job.fake_settings
            except Exception:
                # (the reference's drivers: try / except per image, scripts/dosub.py:205-213)
                traceback.print_exception(*sys.exc_info())
                continue
            sci['radec'] = radec
            scis.append(sci)
            jobs.append(job)
        io.stream.synchronize()                  # (the rms maps; the pool's lanes read them on their own streams)
        return scis, jobs, (1e3 * (t1 - t0), 1e3 * (time.time() - t1))
    finisher = ThreadPoolExecutor(1, thread_name_prefix='zmnight-fin')
    prep = ThreadPoolExecutor(1, thread_name_prefix='zmnight-prep')
    pending = []
    try:
        # two batches ahead in files (the ring reads b + 2 while b + 1 is prepared and b subtracted), one in jobs
        asked = [ask(b) for b in range(min(2, len(chunks)))]
        ready = prep.submit(prepare, *asked[0]) if chunks else None
        for b in range(len(chunks)):
            t0 = time.time()
            scis, jobs, (ms_files, ms_prep) = ready.result()
            if b + 2 < len(chunks):
                asked.append(ask(b + 2))
            ready = prep.submit(prepare, *asked[b + 1]) if b + 1 < len(chunks) else None
            t3 = time.time()
            results = pool.map(jobs, sync=False)
            pending.append(finisher.submit(finish, scis, results))
            if jobs:
                print(f'took {time.time() - t0:.2f} sec to make {len(jobs)} subtractions', flush=True)
            if os.environ.get('ZM_NIGHT_TRACE'):
                print(f'  batch {b}: waited {1e3 * (t3 - t0):.1f} ms for its jobs (files {ms_files:.1f}, rms maps {ms_prep:.1f} on the '
                      f'preparing thread), pool {1e3 * (time.time() - t3):.1f}', flush=True)
        t0 = time.time()
        done = [out for f in pending for out in f.result()]
        t1 = time.time()
    finally:
        prep.shutdown(wait=True)
        finisher.shutdown(wait=True)
    ring.flush()                                 # every product is on disk when this returns
    if os.environ.get('ZM_NIGHT_TRACE'):
        print(f'  finisher {1e3 * (t1 - t0):.1f} ms behind the last batch, files on disk {1e3 * (time.time() - t1):.1f} ms '
              f'later', flush=True)
    return done


if __name__ == '__main__':
    main()
