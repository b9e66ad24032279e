"""``scripts/makealert.py`` as a child process on a tiny synthetic night on disk: three filtered catalogs with their stamps
files, the two tables of ``makesources.py``, a photometry CSV, the frames of the reference image and a directory of
external tables.  One line per detection that has a source, and every line validates."""
import base64
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alert_scenes as sc
import assoc_ref as ar
from util import pkg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = [('X_WORLD', 'f8'), ('Y_WORLD', 'f8'), ('FLUX_APER', 'f4'), ('FLUXERR_APER', 'f4'), ('ELONGATION', 'f4'), ('FLAGS', 'i2'),
           ('IMAFLAGS_ISO', 'i4'), ('A_IMAGE', 'f4'), ('B_IMAGE', 'f4'), ('FWHM_IMAGE', 'f4'), ('X_IMAGE', 'f4'), ('Y_IMAGE', 'f4'),
           ('GOODCUT', 'i2'), ('rb', 'f4')]


def test_makealert_writes_one_valid_packet_per_associated_detection(tmp_path, engine):
    z = pkg()
    d = str(tmp_path)
    dets, known, stars = ar.toy_night(z.Detection, z.Source)
    # the night on disk: one catalog per image, its toy detections as GOODCUT rows behind one row that failed the cuts
    cats, per_image = [], {}
    for det in dets:
        per_image.setdefault(det.image, []).append(det)
    rng = np.random.default_rng(12)
    for k, (image, rows) in enumerate(sorted(per_image.items())):
        tab = np.zeros(len(rows) + 1, dtype=COLUMNS)
        tab[0] = (rows[0].ra + 0.1, rows[0].dec, 10.0, 1.0, 1.0, 0, 0, 1.0, 1.0, 2.0, 5.0, 5.0, 0, 0.9)
        for j, det in enumerate(rows):
            tab[j + 1] = (det.ra, det.dec, det.flux, det.fluxerr, 1.25, 0, 0, 1.5, 1.25, 2.5 + j, 40.0 + j, 50.0 + j, 1, det.rb)
        header = dict(FIELD=651, CCDID=3, QID=2, FID=2, OBSMJD=58100.0 + k, NID=100 + k, MAGLIM=20.5, EXPTIME=30.0, PROGRMPI='Kulkarni',
                      PROGRMID=2)
        path = os.path.join(d, f'sub.{image}.cat')
        z.fits.write_ldac(path, tab, header, {})
        n, size = len(rows), 9
        blocks = rng.normal(size=(n, 3, size, size)).astype(np.float32)
        st = np.zeros(n, dtype=[('ra', 'f8'), ('dec', 'f8'), ('x0', 'i4'), ('y0', 'i4'), ('nx_trim', 'i4'), ('ny_trim', 'i4')])
        for j, det in enumerate(rows):
            st[j] = (det.ra, det.dec, -2 if j == 0 else 30 + j, 40, 7 if j == 0 else 9, 9)          # the first stamp is trimmed
        z.fits.write_image_table(path.replace('.cat', '.stamps.fits'), blocks, st, {'STAMPSZ': size, 'NDET': n})
        cats.append(path)
    # the tables of makesources.py, made the way it makes them
    from_cats = []
    for path in cats:
        from_cats += z.detections_from_cat(z.PipelineFITSCatalog.from_file(path).data, image=os.path.basename(path))
    sources = z.associate(from_cats, stars=stars, engine=engine)
    stab, dtab = os.path.join(d, 'sources.txt'), os.path.join(d, 'sources.det.txt')
    z.write_source_tables(sources, from_cats, stab, dtab)
    nwith = sum(1 for x in from_cats if x.source is not None)
    assert len(sources) == 4 and nwith == 9 and len(from_cats) == 12              # (no known source here: S0's two detections cluster)
    # photometry: three points per source, one of them after the night
    rows = [{'source_id': s.id, 'image_id': 700 + j, 'flux': 100.0 + j, 'fluxerr': 5.0, 'flags': 0, 'ra': s.ra, 'dec': s.dec, 'zp': 26.0,
             'filtercode': 'zr', 'obsjd': m + sc.MJD_TO_JD} for s in sources for j, m in enumerate((58090.0, 58100.0, 58200.0))]
    phot = os.path.join(d, 'phot.csv')
    z.write_phot_csv(phot, rows)
    # the frames of the reference image
    reflist = os.path.join(d, 'ref.txt')
    with open(reflist, 'w') as f:
        for j, m in enumerate((58010.5, 58000.25, 58005.0)):
            p = os.path.join(d, f'refframe{j}.fits')
            z.fits.write(p, np.zeros((4, 4), np.float32), {'OBSMJD': m})
            f.write(p + '\n')
    # the external tables
    ra, dec = np.array([x.ra for x in from_cats if x.source is not None]), np.array([x.dec for x in from_cats if x.source is not None])
    tabs = sc.tables(ra, dec)
    os.mkdir(os.path.join(d, 'xcats'))
    for name, t in tabs.items():
        np.savez(os.path.join(d, 'xcats', name + '.npz'), **t)

    out = os.path.join(d, 'alerts.jsonl')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'makealert.py')] + cats +
                       ['--sources', stab, '--detsource', dtab, '--phot', phot, '--refimages', reflist, '--catalogs', os.path.join(d, 'xcats'),
                        '--stamps', '--rb-version', 'braai_d6_m9', '--strict', '--out', out], cwd=d, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f'{nwith} alerts of 3 catalogs against 5 tables' in r.stdout
    lines = open(out).read().splitlines()
    assert len(lines) == nwith
    packets = [json.loads(line) for line in lines]
    for p in packets:
        assert z.validate(p, p['candidate']['alert_type']) == []
    want = sc.expected_xmatch(tabs, ra, dec)
    keys = set().union(*want)
    sc.assert_xmatch_equal([{k: v for k, v in p['candidate'].items() if k in keys} for p in packets], want)
    p = packets[0]
    c = p['candidate']
    assert (p['objectId'], p['candid'], c['pid'], c['pdiffimfilename']) == (from_cats[0].source.id, 1, 0, 'sub.img0.fits')
    assert (c['alert_type'], c['jd'], c['nid'], c['diffmaglim'], c['exptime'], c['drbversion']) == \
        ('single', 58100.0 + sc.MJD_TO_JD, 100, 20.5, 30.0, 'braai_d6_m9')
    assert (c['jdstartref'], c['jdendref'], c['nframesref'], c['rcid'], c['programpi']) == (58000.25, 58010.5, 3, 9, 'Kulkarni')
    assert [x['flux'] for x in p['light_curve']] == [100.0, 101.0]                          # the point after the night is cut
    # the first detection's stamp was trimmed to 7 x 9 at the grid's edge
    data = z.fits.from_bytes(gzip.decompress(base64.b64decode(p['cutoutDifference'])))[0]
    assert data.shape == (9, 7)
    # ... and without --strict, --stamps and --catalogs the driver still writes every packet
    out2 = os.path.join(d, 'bare.jsonl')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'makealert.py')] + cats +
                       ['--sources', stab, '--detsource', dtab, '--phot', phot, '--refimages', reflist, '--out', out2], cwd=d,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    bare = [json.loads(line) for line in open(out2)]
    assert len(bare) == nwith and bare[0]['cutoutScience'] is None and bare[0]['candidate']['ztfname'] == ''
