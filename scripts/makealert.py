#!/usr/bin/env python
"""Alert packets of a night's detections: the job of the reference's ``scripts/makealert.py`` (``Alert.from_detection``),
without database, network or Kafka.

usage: makealert.py sub.A.cat sub.B.cat ... --sources sources.txt --detsource sources.det.txt --phot phot.csv
                    --refimages ref.txt [--catalogs DIR] [--stamps] [--rb-version NAME] [--strict] [--out alerts.jsonl]

* ``sub.*.cat``: the filtered detection catalogs ``dosub.py --detect`` / ``donightly.py --detect`` wrote; the header they
  carry is that of the science image.  Every ``GOODCUT == 1`` row that has a source gets an alert.
* ``--sources``, ``--detsource``: the two tables of ``makesources.py`` (sources; ``image row ra dec source``).
* ``--phot``: the photometry ``dophot.py`` wrote: the light curves.
* ``--refimages``: the list of frames the reference image was made of (``makeref.py``'s input): their dates.
* ``--catalogs DIR``: one ``NAME.npz`` per table to cross-match (``ps1``, ``legacysurvey``, ``ztfalerts``, ``milliquas``,
  ``tns``; ``ra``, ``dec`` and the table's columns); tables that are not there contribute nothing.
* ``--stamps``: take the cutouts from the ``sub.*.stamps.fits`` beside each catalog (base64 in the output).
* ``--strict``: check every packet against the reference's field lists; one that does not fit is an error.

Writes one JSON object per line.  The cone searches run on the GPU, once per table for the whole night
(``zuds.make_alerts``: ``csrc/skyindex.hip``); everything else here reads and writes."""
import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zuds_amd as zuds

zuds.init_db()


def read_detsource(path):
    """{(image, row): source id} of the rows of ``sources.det.txt`` that have a source."""
    out = {}
    with open(path) as f:
        for line in f:
            t = line.split()
            if t and not t[0].startswith('#') and t[4] != '-':
                out[(t[0], int(t[1]))] = t[4]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('catalogs_in', nargs='+', metavar='sub.cat')
    ap.add_argument('--sources', required=True)
    ap.add_argument('--detsource', required=True)
    ap.add_argument('--phot', required=True)
    ap.add_argument('--refimages', required=True, help='list of the frames the reference image was made of')
    ap.add_argument('--catalogs', help='directory with one NAME.npz per table')
    ap.add_argument('--stamps', action='store_true')
    ap.add_argument('--rb-version', default=None, help='name of the real / bogus model the catalogs were scored with')
    ap.add_argument('--strict', action='store_true')
    ap.add_argument('--out', default='alerts.jsonl')
    args = ap.parse_args(argv)

    sources = {str(s.id): s for s in zuds.read_sources_table(args.sources)}
    zuds.light_curves(zuds.read_phot_csv(args.phot), list(sources.values()))
    source_of = read_detsource(args.detsource)
    with open(args.refimages) as f:
        frames = [zuds.HeaderImage(zuds.fits.read_header(p)[0], basename=os.path.basename(p)) for p in f.read().split()]
    reference = zuds.HeaderImage({}, basename='reference', input_images=frames)

    dets = []
    for pid, path in enumerate(args.catalogs_in):
        cat = zuds.PipelineFITSCatalog.from_file(path)
        cat.rb_version = args.rb_version
        name = os.path.basename(path)
        science = zuds.HeaderImage(cat.header, basename=name.replace('.cat', '.fits'))
        cat.image = zuds.HeaderImage(cat.header, basename=name.replace('.cat', '.fits'), id=pid, target_image=science,
                                     reference_image=reference)
        rows = np.flatnonzero(cat.data['GOODCUT'] == 1).tolist()
        every = zuds.Detection.from_catalog(cat, filter=False)
        stamps = zuds.fits.read_image_table(path.replace('.cat', '.stamps.fits')) if args.stamps else None
        for k, row in enumerate(rows):
            d = every[row]
            sid = source_of.get((name, row))
            if sid is None:
                continue
            d.row, d.id, d.source = row, pid * 1000000 + row, sources[sid]
            d.source.detections.append(d)
            if stamps is not None:
                t = stamps[2][k]
                d.thumbnails = zuds.thumbnails_of_blocks(stamps[0][k], t['x0'], t['y0'], t['nx_trim'], t['ny_trim'], detection=d)
            dets.append(d)

    cats = [zuds.ExternalCatalog.from_npz(p) for p in sorted(glob.glob(os.path.join(args.catalogs, '*.npz')))] if args.catalogs else []
    alerts = zuds.make_alerts(dets, cats, strict=args.strict)
    with open(args.out, 'w') as f:
        for a in alerts:
            f.write(a.to_json() + '\n')
    print(f'{len(alerts)} alerts of {len(args.catalogs_in)} catalogs against {len(cats)} tables: {args.out}', flush=True)
    return args.out


if __name__ == '__main__':
    main()
