#!/usr/bin/env python
"""Detections into sources: the job of the reference's ``nersc/makesources.py`` (``associate()``), database-free.

usage: makesources.py sub.A.cat sub.B.cat ... [--sources prev.txt] [--stars stars.txt] [--rb-min X] [--out PREFIX]

* ``sub.*.cat``: the filtered detection catalogs ``dosub.py --detect`` / ``donightly.py --detect`` wrote (FITS_LDAC); the
  ``GOODCUT == 1`` rows of all of them are the night's detections.
* ``--sources prev.txt``: a sources table of an earlier run: a detection within 2 arcsec of one of its sources joins
  that source (the nearest), which moves to the position of the best-S/N detection that joined it.
* ``--stars stars.txt``: ``ra dec`` per line (degrees); a new source less than 1.5 arcsec from a star is rejected
  (score -1).
* ``--rb-min X``: only detections with ``rb > X`` seed new sources (default ``ASSOC_RB_MIN`` = 0.4; catalogs without an
  ``rb`` column: every detection).

Writes ``PREFIX.txt`` (``id ra dec ndet score best_image rejected`` per source, known sources first) and
``PREFIX.det.txt`` (``image row ra dec source`` per detection); ``PREFIX`` defaults to ``sources``.  The join and the
clustering run on the GPU (``zuds.associate``: ``csrc/associate.hip``)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zuds_amd as zuds

zuds.init_db()


def load_stars(path):
    t = np.atleast_2d(np.loadtxt(path))
    if t.size == 0:
        return np.zeros(0), np.zeros(0)
    return t[:, 0].copy(), t[:, 1].copy()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('catalogs', nargs='+')
    ap.add_argument('--sources', help='sources table of an earlier run')
    ap.add_argument('--stars', help='star catalogue: ra dec per line')
    ap.add_argument('--rb-min', type=float, default=zuds.ASSOC_RB_MIN)
    ap.add_argument('--out', default='sources', help='prefix of the two tables')
    args = ap.parse_args(argv)
    dets = []
    for path in args.catalogs:
        cat = zuds.PipelineFITSCatalog.from_file(path)
        dets += zuds.detections_from_cat(cat.data, image=os.path.basename(path))
    known = zuds.read_sources_table(args.sources) if args.sources else None
    stars = load_stars(args.stars) if args.stars else None
    sources = zuds.associate(dets, sources=known, stars=stars, rb_min=args.rb_min)
    zuds.write_source_tables(sources, dets, args.out + '.txt', args.out + '.det.txt')
    nnew = len(sources) - (len(known) if known else 0)
    print(f'{len(dets)} detections of {len(args.catalogs)} catalogs: {nnew} new sources, '
          f'{sum(1 for d in dets if d.source is not None)} detections associated, '
          f'{sum(1 for s in sources if s.rejected)} sources rejected', flush=True)
    return args.out + '.txt', args.out + '.det.txt'


if __name__ == '__main__':
    main()
