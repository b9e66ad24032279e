#!/usr/bin/env python
"""Build science coadds for a list of jobs on the GPU engine.

    dostack.py jobs.csv            (one process)
    torchrun --nproc-per-node N dostack.py jobs.csv     (jobs dealt over N ranks)

Plays the part of the reference's ``scripts/dostack.py`` with its database
queries replaced by a job file: every row of ``jobs.csv`` has ``target`` (science
image paths joined by ';' -- each with its ``*mskimg.fits`` beside it) and the
bin edges ``left`` / ``right`` that go into the coadd's file name.  A job whose
output already exists is skipped, which is how an interrupted run resumes.

    dostack.py jobs.csv --solve-astrometry --astref stars.cat [--distort-degrees N]

refits the astrometry of the inputs and of the coadd against the FITS_LDAC star catalogue ``stars.cat``
(``from_images(solve_astrometry=True)``; the reference's SCAMP step, ``zuds/coadd.py:120-123,219-223``).

    dostack.py jobs.csv --photcal [--photref stars.cat]

measures ``APCORk`` and ``MAGLIM`` on every coadd - with ``--photref``, a FITS_LDAC star catalogue with a ``MAG`` column,
``MAGZP`` as well - and writes the cards into its header (``from_images(calibrate_photometry=True)``, photcal.py).
"""
import argparse
import os
import sys
import time

import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zuds_amd as zuds  # noqa: E402


def load_inputs(target):
    """ScienceImages (mask attached) of one job."""
    images = []
    for path in (p.strip() for p in str(target).split(';')):
        sci = zuds.ScienceImage.from_file(path)
        sci.mask_image = zuds.MaskImage.from_file(path.replace('sciimg', 'mskimg'))
        images.append(sci)
    zuds.ensure_images_have_the_same_properties(images, zuds.GROUP_PROPERTIES)
    return images


def coadd_name(first, left, right):
    """<field>_<ccd>_<quadrant>_<filter>_<left>_<right>.coadd.fits next to the inputs."""
    stem = '_'.join([f'{int(first.field):06d}', f'c{int(first.ccdid):02d}',
                     f'q{int(first.qid)}', zuds.fid_map[int(first.fid)],
                     str(left), str(right)])
    return os.path.join(os.path.dirname(first.local_path), stem + '.coadd.fits')


def run_job(job, tmpdir, scamp_kws=None, photcal_kws=None):
    t0 = time.time()
    images = load_inputs(job['target'])
    outname = coadd_name(images[0], job['left'], job['right'])
    if os.path.exists(outname):
        return None
    t1 = time.time()
    print(f'load: {t1 - t0:.2f} sec to load input images for {outname}', flush=True)
    try:
        stack = zuds.ScienceCoadd.from_images(images, outfile_name=outname,
                                              data_product=False, tmpdir=tmpdir,
                                              nthreads=zuds.get_nthreads(),
                                              solve_astrometry=scamp_kws is not None, scamp_kws=scamp_kws,
                                              calibrate_photometry=photcal_kws is not None, photcal_kws=photcal_kws)
    except Exception as exc:        # one bad job must not end the night's run
        print(exc, [im.basename for im in images], flush=True)
        return None
    stack.binleft, stack.binright = job['left'], job['right']
    t2 = time.time()
    print(f'stack: {t2 - t1:.2f} sec to make {stack.basename}', flush=True)
    for frame in (*images, stack):
        frame.unmap()
    t3 = time.time()
    print(f'clean: took {t3 - t2:.2f} sec to clean up after {stack.basename}', flush=True)
    print(f'took {t3 - t0:.2f} sec to make "{stack.basename}"', flush=True)
    return stack.basename


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('jobs')
    ap.add_argument('--tmpdir', default='/tmp')
    ap.add_argument('--solve-astrometry', action='store_true', help='refit the astrometry of the inputs and of the coadd')
    ap.add_argument('--astref', help='FITS_LDAC star catalogue (ASTREF_CATALOG FILE, ASTREFCAT_NAME)')
    ap.add_argument('--distort-degrees', type=int, default=3, help='degree of the distortion polynomial (1, 2 or 3)')
    ap.add_argument('--photcal', action='store_true', help='measure APCORk and MAGLIM (with --photref: MAGZP) on the coadd')
    ap.add_argument('--photref', help='FITS_LDAC star catalogue with a MAG column (PHOTREF_NAME)')
    args = ap.parse_args(argv)
    if args.photref and not args.photcal:
        ap.error('--photref is only read with --photcal')
    photcal_kws = None
    if args.photcal:
        photcal_kws = {'PHOTREF_NAME': args.photref} if args.photref else {}
    scamp_kws = None
    if args.solve_astrometry:
        if not args.astref:
            ap.error('--solve-astrometry needs --astref FILE')
        scamp_kws = {'ASTREF_CATALOG': 'FILE', 'ASTREFCAT_NAME': args.astref, 'DISTORT_DEGREES': args.distort_degrees}
    zuds.init_db()
    share = zuds.get_my_share_of_work(args.jobs, reader=pd.read_csv)
    table = share if isinstance(share, pd.DataFrame) else pd.DataFrame(list(share))
    for _, row in table.iterrows():
        run_job(row, args.tmpdir, scamp_kws, photcal_kws)
    return 0


if __name__ == '__main__':
    sys.exit(main())
