#!/usr/bin/env python
"""Forced photometry of known sources on a list of subtractions: the job of the reference's ``scripts/dophot.py``,
database-free.

usage: dophot.py subs.txt out.csv --sources sources.txt [--done prior.csv] [--batch N] [--psf]

* ``subs.txt``: one subtraction per line, ``path [image id]`` (the id defaults to the file's name).  ``X.rms.fits`` and
  ``X.mask.fits`` are looked for beside ``X.fits``; a triple that is incomplete is skipped with the reference's message.
* ``--sources sources.txt``: the sources table ``makesources.py`` / ``donightly.py --associate`` wrote (id, ra, dec).
* ``--done prior.csv``: an earlier output of this script: (source, image) pairs it holds are left out - the reference's
  outer join against the ``forcedphotometry`` table.
* ``--batch N``: triples brought into HBM, joined and photometered per call (default 16).
* ``--psf``: PSF fits in place of the aperture sums ("PSF photometry"): the model ``X.psf.fits`` that
  ``dosub.py --psf`` wrote beside ``X.fits`` is fitted at every source (``method='psf'``: no sky term on a difference
  image), ``flags`` are those of the fit and ``zp = MAGZP + PSFCOR``.  A subtraction without a model is skipped with a
  warning.  The columns stay the reference's; write a PSF run to a file of its own.

For every subtraction the reference asks the database which sources lie inside ``wcs.calc_footprint()`` and are not yet
photometered, then runs ``raw_aperture_photometry`` there.  Here ``N`` triples at a time are read straight into HBM
(``FITSDeviceIO.load_many``), joined against the whole source table and photometered in one launch
(``zuds.forced_photometry_batch``: ``csrc/lightcurve.hip``).  ``out.csv`` has the reference's columns, in its order:
``source_id,image_id,flux,fluxerr,flags,ra,dec,zp,filtercode,obsjd`` with ``zp = MAGZP + APCOR4``, ``obsjd`` and
``filtercode`` from each header; rows follow ``subs.txt``, sources in table order within an image."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zuds_amd as zuds

zuds.init_db()


def read_subs(path):
    """[(path, image id)] of the lines of ``subs.txt`` whose three files exist."""
    out = []
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t or t[0].startswith('#'):
                continue
            fn = t[0]
            imgid = t[1] if len(t) > 1 else os.path.basename(fn)
            maskname = fn.replace('.fits', '.mask.fits')
            rmsname = fn.replace('.fits', '.rms.fits')
            if not (os.path.exists(fn) and os.path.exists(maskname) and os.path.exists(rmsname)):
                print(f'{fn}, {maskname}, and {rmsname} do not all exist, continuing...', flush=True)
                continue
            out.append((fn, int(imgid) if imgid.lstrip('-').isdigit() else imgid))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('infile', help='file listing the subtractions to do photometry on')
    ap.add_argument('outfile', help='the photometry, as CSV')
    ap.add_argument('--sources', required=True, help='sources table (id ra dec ...)')
    ap.add_argument('--done', help='an earlier output: pairs it holds are left out')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--psf', action='store_true', help='PSF fits with the model beside each subtraction')
    args = ap.parse_args(argv)
    start = time.time()
    subs = read_subs(args.infile)
    if args.psf:
        for fn, _ in subs:
            if not os.path.exists(fn.replace('.fits', '.psf.fits')):
                print(f'phot: {fn} has no {os.path.basename(fn).replace(".fits", ".psf.fits")} beside it, skipped '
                      f'(dosub.py --psf writes it)', flush=True)
        subs = [(fn, imgid) for fn, imgid in subs if os.path.exists(fn.replace('.fits', '.psf.fits'))]
    sources = zuds.read_sources_table(args.sources)
    ids = [s.id for s in sources]
    ra = np.array([s.ra for s in sources], dtype=np.float64)
    dec = np.array([s.dec for s in sources], dtype=np.float64)
    row_of = {str(sid): k for k, sid in enumerate(ids)}
    prior = {}
    if args.done:
        for r in zuds.read_phot_csv(args.done):
            if str(r['source_id']) in row_of:
                prior.setdefault(str(r['image_id']), []).append(row_of[str(r['source_id'])])
    io = importlib.import_module('zuds-pipeline_amd.device').FITSDeviceIO() if subs else None
    zuds.write_phot_csv(args.outfile, [])
    nrows = 0
    for b0 in range(0, len(subs), max(args.batch, 1)):
        batch = subs[b0:b0 + max(args.batch, 1)]
        wanted = []
        for fn, _ in batch:
            wanted += [(fn, 'f32'), (fn.replace('.fits', '.rms.fits'), 'f32'), (fn.replace('.fits', '.mask.fits'), 'i32')]
        planes = io.load_many(wanted)
        images, headers = [], []
        for k in range(len(batch)):
            (img, hdr), (rms, _), (mask, _) = planes[3 * k:3 * k + 3]
            images.append(dict(img=img, rms=rms, mask=mask, wcs=zuds.WCS.from_header(hdr)))
            if args.psf:
                images[-1]['psf'] = zuds.PSFModel.from_file(batch[k][0].replace('.fits', '.psf.fits'))
                hdr = dict(hdr)
                hdr.setdefault('PSFCOR', images[-1]['psf'].cards.get('PSFCOR'))
            headers.append(hdr)
        done = [(k, s) for k, (_, imgid) in enumerate(batch) for s in prior.get(str(imgid), ())]
        tstart = time.time()
        method = dict(method='psf') if args.psf else {}
        table = zuds.forced_photometry_batch(images, ra, dec, done=done or None, engine=io.engine, **method)
        rows = zuds.photometry_rows(table, headers, ra, dec, source_ids=ids, image_ids=[imgid for _, imgid in batch], **method)
        zuds.write_phot_csv(args.outfile, rows, append=True)
        nrows += len(rows)
        for k, (fn, _) in enumerate(batch):
            n = int(table['offsets'][k + 1] - table['offsets'][k])
            if n == 0:
                print(f'phot: no photometry needed on {fn}, all done', flush=True)
        print(f'phot: {len(rows)} rows on {len(batch)} subtractions in {time.time() - tstart:.2f} sec', flush=True)
    print(f'{nrows} rows of {len(subs)} subtractions and {len(sources)} sources in {time.time() - start:.2f} sec', flush=True)
    return args.outfile


if __name__ == '__main__':
    main()
