"""``scripts/dosub.py --detect --psf`` (through ``main``) followed by ``scripts/dophot.py --psf`` on a synthetic night: the two model files and the
cards, a PSF light-curve CSV whose fluxes are the restatement's (tests/psf_ref.py) and whose ``zp`` is ``MAGZP + PSFCOR``;
and the subtraction's own products stay what a run without ``--psf`` writes."""
import os

import numpy as np
import pytest

import psf_ref as pr
from test_scripts_gpu import _scene, load_script
from util import pkg, synth

pytestmark = pytest.mark.gpu
SUFFIXES = ('.fits', '.rms.fits', '.mask.fits')
CARDS = ('PSFCOR', 'PSFCORUN', 'PSFNSTAR', 'PSFHALF', 'PSFFITR', 'PSFFWHM', 'ZMPSF')


def test_dosub_psf_then_dophot_psf(tmp_path, engine, capsys):
    z, s = pkg(), synth()
    d = str(tmp_path)
    refims, _ = _scene(z, s, d, 640, 600, 3, 5300, '201912', fwhm=2.0)
    refname = os.path.join(d, 'ref.000651_c03_q1_zg.fits')
    z.ReferenceImage.from_images(refims, refname, sci_swarp_kws={'COMBINE_TYPE': 'WEIGHTED'})
    _, (spath,) = _scene(z, s, d, 640, 600, 1, 5400, '202003', fwhm=2.4, extra=lambda i: {'APCOR4': -0.125, 'FILTER': 'ZTF g'})
    dosub = load_script('dosub')
    out = z.sub_name(spath, refname)
    imgs = os.path.join(d, 'images.txt')
    with open(imgs, 'w') as f:
        f.write(spath + '\n')
    assert dosub.main([imgs, refname, '--psfref', os.path.join(d, 'stars.cat')]) == 2
    assert '--psfref needs --psf' in capsys.readouterr().err and not os.path.exists(out)

    def products():
        got = {sfx: open(out.replace('.fits', sfx), 'rb').read() for sfx in SUFFIXES}
        assert os.path.exists(out.replace('.fits', '.cat'))
        for name in os.listdir(d):
            if name.startswith('sub.'):
                os.remove(os.path.join(d, name))
        return got
    # without --psf: the products, and no model file
    assert dosub.main([imgs, refname, '--detect']) == 0
    assert not os.path.exists(out.replace('.fits', '.psf.fits')) and not os.path.exists(spath.replace('.fits', '.psf.fits'))
    plain_hdr = z.fits.read_header(out)[0]
    plain = products()
    # --detect --psf --psfref: a catalogue of the stars the image's own route finds; the model files and the cards
    sci = z.ScienceImage.from_file(spath)
    sci.mask_image = z.MaskImage.from_file(spath.replace('sciimg', 'mskimg'))
    own = sci.build_psf()
    cra, cdec = sci.wcs.all_pix2world(own['x'], own['y'], 0)
    cat = os.path.join(d, 'stars.cat')
    z.scamp.write_astrefcat(cat, cra, cdec, mag=np.full(len(cra), 18.0))
    assert dosub.main([imgs, refname, '--detect', '--psf', '--psfref', cat]) == 0
    by_cat = z.PSFModel.from_file(out.replace('.fits', '.psf.fits'))
    assert 10 <= by_cat.cards['PSFNSTAR'] <= len(cra) and np.abs(by_cat.data - own['psf'].data).max() < 1e-3
    assert products()['.rms.fits'] == plain['.rms.fits']
    os.remove(spath.replace('.fits', '.psf.fits'))
    # --detect --psf: the same planes, the header plus the cards, the two model files
    assert dosub.main([imgs, refname, '--detect', '--psf']) == 0
    for sfx in SUFFIXES[1:]:
        assert open(out.replace('.fits', sfx), 'rb').read() == plain[sfx], sfx
    data, hdr, _ = z.fits.read(out)
    assert data.tobytes() == z.fits.from_bytes(plain['.fits'])[0].tobytes()
    assert {k: v for k, v in hdr.items() if k not in CARDS} == plain_hdr and all(k in hdr for k in CARDS)
    a, b = (open(p.replace('.fits', '.psf.fits'), 'rb').read() for p in (spath, out))
    assert a == b
    model = z.PSFModel.from_file(out.replace('.fits', '.psf.fits'))
    assert model.half == 12 and abs(model.data.sum() - 1.0) < 1e-14 and model.cards == {k: hdr[k] for k in CARDS}
    assert model.cards['PSFNSTAR'] >= 10 and abs(model.cards['PSFCOR']) < 0.1 and 2.0 < model.cards['PSFFWHM'] < 2.9
    assert model.data.tobytes() == own['psf'].data.tobytes()
    print(f'dosub --detect --psf: {model.cards}')
    # dophot --psf on that subtraction, and on one without a model (skipped with a warning)
    w = z.WCS.from_header(hdr)
    rng = np.random.default_rng(8)
    ra, dec = w.all_pix2world(rng.uniform(-40.0, 680.0, 120), rng.uniform(-40.0, 640.0, 120), 0)
    sources = [z.Source(id=f'src{k:05d}', ra=float(p), dec=float(q)) for k, (p, q) in enumerate(zip(ra, dec))]
    stab = os.path.join(d, 'sources.txt')
    z.write_source_tables(sources, [], stab, os.path.join(d, 'sources.det.txt'))
    bare = os.path.join(d, 'bare.fits')
    for sfx in SUFFIXES:
        with open(bare.replace('.fits', sfx), 'wb') as f:
            f.write(plain[sfx])
    with open(os.path.join(d, 'subs.txt'), 'w') as f:
        f.write(f'{out} 41\n{bare} 42\n')
    csv = os.path.join(d, 'psf.csv')
    load_script('dophot').main([os.path.join(d, 'subs.txt'), csv, '--sources', stab, '--psf'])
    assert 'has no bare.psf.fits beside it, skipped' in capsys.readouterr().out
    rows = z.read_phot_csv(csv)
    assert len(rows) > 60 and {r['image_id'] for r in rows} == {41}
    tab = z.read_sources_table(stab)
    tra, tdec = np.array([t.ra for t in tab]), np.array([t.dec for t in tab])
    rms, mask = (z.fits.read(out.replace('.fits', sfx))[0] for sfx in SUFFIXES[1:])
    # the library on the same files: the script's rows bit for bit, and at its own positions the restatement's fits
    t = z.forced_photometry_batch([dict(img=data, rms=rms, mask=mask, wcs=w, psf=model)], tra, tdec, engine=engine, method='psf')
    assert [int(r['source_id'][3:]) for r in rows] == t['source'].tolist()
    flux, err = np.array([r['flux'] for r in rows]), np.array([r['fluxerr'] for r in rows])
    assert flux.tobytes() == t['flux'].tobytes() and err.tobytes() == t['fluxerr'].tobytes()
    assert [r['flags'] for r in rows] == t['flags'].tolist()
    ref = pr.fit(data, t['x'], t['y'], model.data, 6.0, 0, rms=rms, mask=mask, bad_bits=z.BAD_SUM)
    assert ref['margin'].min() >= 1e-9 and np.array_equal(t['flags'], ref['flags']) and np.array_equal(t['npix'], ref['npix'])
    fin = np.isfinite(ref['flux'])
    assert np.array_equal(np.isfinite(flux), fin) and fin.sum() > 50
    tol = pr.FLUX_ATOL + pr.FLUX_RTOL * np.abs(ref['flux'])
    print(f'dophot --psf: {len(rows)} rows, largest flux difference {np.abs(flux - ref["flux"])[fin].max():.3e}, '
          f'{np.max(np.abs(flux - ref["flux"])[fin] / tol[fin]):.3e} of its tolerance')
    assert (np.abs(flux - ref['flux'])[fin] <= tol[fin]).all()
    assert (np.abs(err - ref['err'])[fin] <= pr.ERR_RTOL * ref['err'][fin]).all()
    assert all(r['zp'] == hdr['MAGZP'] + hdr['PSFCOR'] and r['filtercode'] == 'zg' for r in rows)
    # the object layer on the same subtraction: the model comes from the sibling file, the points are psf_photometry's
    sub = z.SingleEpochSubtraction.from_file(out)
    sub.mask_image = z.MaskImage.from_file(out.replace('.fits', '.mask.fits'))
    some = sources[:40]
    pts = sub.force_photometry(some, assume_background_subtracted=True, method='psf')
    assert sub.psf_model.data.tobytes() == model.data.tobytes() and sub.psf_model.n_used is None
    hx, hy = sub.wcs.all_world2pix([p.ra for p in some], [p.dec for p in some], 0)
    direct = z.psf.psf_photometry(sub, hx, hy, model, fit_sky=0, engine=engine)
    assert np.array([p.flux for p in pts]).tobytes() == direct['flux'].tobytes()
    assert [p.flags for p in pts] == direct['flags'].tolist() and all(p.zp == hdr['MAGZP'] + hdr['PSFCOR'] for p in pts)
    inside = [p for p in pts if not p.flags & z.psf.PSF_FLAGS['SINGULAR']]
    assert len(inside) > 10 and all(p.filtercode == 'zg' and p.source is q for p, q in zip(pts, some))
    one = some[0].force_photometry([sub], method='psf') if some[0].images([sub]) else []
    assert all(p.flux == pts[0].flux for p in one)
    with pytest.raises(ValueError, match='neither'):
        sub.force_photometry(some, method='optimal')
