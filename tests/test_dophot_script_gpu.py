"""``scripts/dophot.py`` as a child process: three synthetic triples and a sources table on disk, the CSV it writes
against the headers (plumbing) and against ``forced_photometry_batch`` on the same files (values, bit for bit), and a
second run with ``--done``."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lightcurve_ref as lr
from util import pkg, synth, to_oracle_wcs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_dophot(args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'dophot.py')] + args, cwd=cwd, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_dophot_rows_order_columns_and_values(tmp_path, engine):
    z, s = pkg(), synth()
    d = str(tmp_path)
    ws = [s.ztf_wcs(128, 96, dx=dx, dy=dy, rot_deg=rot, tpv=True) for dx, dy, rot in ((0, 0, 0), (14.5, -8.25, 9.0), (-20.0, 11.0, -17.0))]
    ows = [to_oracle_wcs(w) for w in ws]
    paths, ids, filt = [], [701, 'epoch_b', 703], ['ZTF g', 'ZTF r', 'ZTF i']
    for k, w in enumerate(ws):
        img, rms, mask = lr.make_planes(128, 96, seed=50 + k)
        hdr = dict(w.to_header(), MAGZP=26.125 + 0.25 * k, APCOR4=-0.0625 * (k + 1), OBSJD=2458850.5 + 1.25 * k, FILTER=filt[k])
        p = os.path.join(d, f'sub{k}.fits')
        z.fits.write(p, img, hdr)
        z.fits.write(p.replace('.fits', '.rms.fits'), rms, hdr)
        z.fits.write(p.replace('.fits', '.mask.fits'), mask, hdr)
        paths.append(p)
    lonely = os.path.join(d, 'lonely.fits')                   # no rms, no mask beside it: skipped with the reference's message
    z.fits.write(lonely, np.zeros((96, 128), np.float32), dict(ws[0].to_header(), MAGZP=26.0, APCOR4=0.0))
    rng = np.random.default_rng(77)
    ra, dec = ows[0].pix2sky(rng.uniform(-30.0, 160.0, 90), rng.uniform(-25.0, 120.0, 90))
    lr.assert_clear(ows, ra, dec)
    sources = [z.Source(id=f'src{k:07d}', ra=float(a), dec=float(b)) for k, (a, b) in enumerate(zip(ra, dec))]
    stab = os.path.join(d, 'sources.txt')
    z.write_source_tables(sources, [], stab, os.path.join(d, 'sources.det.txt'))
    tra = np.array([t.ra for t in z.read_sources_table(stab)])           # what the script sees: the table's digits
    tdec = np.array([t.dec for t in z.read_sources_table(stab)])
    lr.assert_clear(ows, tra, tdec)
    subs = os.path.join(d, 'subs.txt')
    with open(subs, 'w') as f:
        f.write(f'{paths[0]} {ids[0]}\n{lonely} 999\n{paths[1]} {ids[1]}\n{paths[2]} {ids[2]}\n')
    out = os.path.join(d, 'out.csv')
    log = run_dophot([subs, out, '--sources', stab, '--batch', '2'], d)
    assert f'{lonely}, {lonely.replace(".fits", ".mask.fits")}, and {lonely.replace(".fits", ".rms.fits")} do not all exist, continuing...' in log
    rows = z.read_phot_csv(out)
    assert open(out).readline().strip() == 'source_id,image_id,flux,fluxerr,flags,ra,dec,zp,filtercode,obsjd'
    # the row set and its order: images as listed, sources in table order within an image - the restatement's join
    off, idx = lr.membership(ows, tra, tdec)
    assert (np.diff(off) > 5).all()
    assert [(r['image_id'], r['source_id']) for r in rows] == \
        [(ids[k], f'src{j:07d}') for k in range(3) for j in idx[off[k]:off[k + 1]].tolist()]
    hdrs = [z.fits.read_header(p)[0] for p in paths]
    for r in rows:
        k, j = ids.index(r['image_id']), int(r['source_id'][3:])
        assert r['zp'] == hdrs[k]['MAGZP'] + hdrs[k]['APCOR4'] and r['obsjd'] == hdrs[k]['OBSJD'] == 2458850.5 + 1.25 * k
        assert r['filtercode'] == 'z' + filt[k][-1] and r['ra'] == tra[j] and r['dec'] == tdec[j]
    # values: the library on the same files, bit for bit (numbers are judged in test_lightcurve_gpu.py)
    images = []
    for p in paths:
        img, hdr, _ = z.fits.read(p)
        images.append(dict(img=img, rms=z.fits.read(p.replace('.fits', '.rms.fits'))[0],
                           mask=z.fits.read(p.replace('.fits', '.mask.fits'))[0], wcs=z.WCS.from_header(hdr)))
    t = z.forced_photometry_batch(images, tra, tdec, engine=engine)
    assert np.array_equal(t['offsets'], off)
    assert np.array([r['flux'] for r in rows]).tobytes() == t['flux'].tobytes()
    assert np.array([r['fluxerr'] for r in rows]).tobytes() == t['fluxerr'].tobytes()
    assert [r['flags'] for r in rows] == t['flags'].tolist() and any(r['flags'] for r in rows)
    # --done with the first half of the rows: exactly the complement, same bytes
    half = len(rows) // 2
    prior = os.path.join(d, 'prior.csv')
    z.write_phot_csv(prior, rows[:half])
    out2 = os.path.join(d, 'out2.csv')
    run_dophot([subs, out2, '--sources', stab, '--done', prior], d)
    assert open(out2).read().splitlines()[1:] == open(out).read().splitlines()[1 + half:]
    assert 0 < half < len(rows)
