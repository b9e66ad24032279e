"""``scripts/donightly.py --maglim`` on a small synthetic night: every ``sub.*.fits`` of the pool carries a ``MAGLIM`` card
measured on the planes in HBM (``DeviceSubtraction.maglim``) with the zero point of the science header; a frame without
``MAGZP`` / ``APCOR4`` gets a warning and no card.  The card is held to the restatement (tests/photcal_ref.py) on the
noise plane and the mask the night wrote."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

import photcal_ref as pr
import photcal_scenes as ps
from util import pkg, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_donightly_maglim_writes_the_card_into_the_pool_s_subtractions(tmp_path, engine):
    z, s = pkg(), synth()
    d = str(tmp_path)
    nx = ny = 512
    base = s.ztf_wcs(nx, ny, tpv=True)
    rng = np.random.default_rng(79)
    xs, ys = rng.uniform(-20, nx + 20, 60), rng.uniform(-20, ny + 20, 60)
    fl = np.exp(rng.uniform(np.log(3e3), np.log(8e4), 60))
    ra, dec = base.all_pix2world(xs, ys, 0)

    def write(name, f, seeing, drop=()):
        path = os.path.join(d, name)
        f['header']['SEEING'] = seeing
        f['header']['OBSJD'] = 2458000.5 + f['header']['OBSMJD'] - 58000.0
        for k in drop:
            f['header'].pop(k)
        z.fits.write(path, f['img'], f['header'])
        z.fits.write(path.replace('sciimg', 'mskimg'), f['mask'].astype(np.int16), f['header'])
        z.fits.write(path.replace('.fits', '.weight.fits'), f['wgt'], f['header'])
        im = z.ScienceImage.from_file(path)
        im.mask_image = z.MaskImage.from_file(path.replace('sciimg', 'mskimg'))
        return im

    refims = []
    for i in range(3):
        w = s.ztf_wcs(nx, ny, dx=rng.uniform(-3, 3), dy=rng.uniform(-3, 3), rot_deg=rng.uniform(-0.03, 0.03))
        f = s.make_frame(nx, ny, 720 + i, w, star_sky=(ra, dec, fl), fwhm=2.0, noise=3.0, bad_block=(100 + 100 * i, 300, 4))
        refims.append(write(f'ztf_2020010{i}_000651_zg_c03_o_q1_sciimg.fits', f, 2.0))
    refname = os.path.join(d, 'ref.000651_c03_q1_zg.fits')
    z.ReferenceImage.from_images(refims, refname, sci_swarp_kws={'COMBINE_TYPE': 'WEIGHTED'})
    names, zps = [], []
    for i in range(2):
        w = s.ztf_wcs(nx, ny, dx=rng.uniform(-5, 5), dy=rng.uniform(-5, 5), rot_deg=rng.uniform(-0.05, 0.05))
        f = s.make_frame(nx, ny, 820 + i, w, star_sky=(ra, dec, fl), fwhm=2.6, sky=170.0 + 15 * i, magzp=26.0 + 0.2 * i,
                         bad_block=(150 + 150 * i, 200, 4))
        zps.append(f['header']['MAGZP'] + f['header']['APCOR4'])
        nm_ = f'ztf_2020020{i}_000651_zg_c03_o_q1_sciimg.fits'
        write(nm_, f, 2.6, drop=('APCOR4',) if i == 1 else ())           # the second frame has no zero point
        names.append(os.path.join(d, nm_))
    with open(os.path.join(d, 'images.txt'), 'w') as fh:
        fh.write('\n'.join(names) + '\n')

    script = load_script('donightly')
    with pytest.warns(UserWarning, match='has no MAGZP / APCOR4 card: MAGLIM is not measured'):
        done = script.main([os.path.join(d, 'images.txt'), refname, '--jobs', '2', '--fit-batch', '0', '--nreg-side', '1',
                            '--maglim'])
    assert len(done) == 2
    with_zp, without = done                              # (the paths of the difference images, in order)
    assert 'MAGLIM' not in z.fits.read(without)[1]
    hdr = z.fits.read(with_zp)[1]
    rms = z.fits.read(with_zp.replace('.fits', '.rms.fits'))[0]
    mask = z.fits.read(with_zp.replace('.fits', '.mask.fits'))[0]
    med, nused, npts, _, _ = pr.maglim_sigma(rms, mask, ps.BAD_BITS, 3.0, 32)
    want = zps[0] - 2.5 * np.log10(5.0 * med)
    print(f'MAGLIM of {os.path.basename(with_zp)}: {hdr["MAGLIM"]!r}, restatement {want!r} ({nused} of {npts} apertures)')
    assert nused > 0 and abs(hdr['MAGLIM'] - want) <= pr.CARD_TOL + 1e-9               # (a card keeps 15 digits of a float)
