"""``scripts/dosub.py --detect --fakes`` and ``scripts/donightly.py --detect --fakes`` (through ``main``) on one synthetic
frame with a ``<sci>.psf.fits`` beside it: the table ``sub.*.fakes.csv``, the ``FAKE*`` cards, products that are otherwise
the bytes of a run without ``--fakes``, and nothing left behind by the fake run."""
import glob
import os
import tempfile

import numpy as np
import pytest

from test_scripts_gpu import load_script
from util import pkg, synth

pytestmark = pytest.mark.gpu
SUFFIXES = ('.fits', '.rms.fits', '.mask.fits', '.cat')
CARDS = ('FAKEN', 'FAKESEED', 'FAKEM50', 'FAKEM80')
SWITCHES = ['--fakes', '40', '--fake-mags', '16,20.5', '--fake-seed', '4']


def night(z, s, d, nx=640, ny=600):
    """Three reference frames and one science frame of one star field, with weight maps (donightly.py wants them)."""
    base = s.ztf_wcs(nx, ny, tpv=True)
    rng = np.random.default_rng(6100)
    nst = int(nx * ny / 2500)
    xs, ys = rng.uniform(-20, nx + 20, nst), rng.uniform(-20, ny + 20, nst)
    fl = np.exp(rng.uniform(np.log(3e3), np.log(8e4), nst))
    ra, dec = base.all_pix2world(xs, ys, 0)

    def write(name, f, seeing):
        path = os.path.join(d, name)
        f['header']['SEEING'] = seeing
        f['header']['OBSJD'] = 2458000.5 + f['header']['OBSMJD'] - 58000.0
        z.fits.write(path, f['img'], f['header'])
        z.fits.write(path.replace('sciimg', 'mskimg'), f['mask'].astype(np.int16), f['header'])
        z.fits.write(path.replace('.fits', '.weight.fits'), f['wgt'], f['header'])
        im = z.ScienceImage.from_file(path)
        im.mask_image = z.MaskImage.from_file(path.replace('sciimg', 'mskimg'))
        return im

    refims = []
    for i in range(3):
        w = s.ztf_wcs(nx, ny, dx=rng.uniform(-3, 3), dy=rng.uniform(-3, 3), rot_deg=rng.uniform(-0.03, 0.03))
        f = s.make_frame(nx, ny, 6110 + i, w, star_sky=(ra, dec, fl), fwhm=2.0, noise=3.0, bad_block=(100 + 150 * i, 300, 4))
        refims.append(write(f'ztf_2020010{i}_000651_zg_c03_o_q1_sciimg.fits', f, 2.0))
    refname = os.path.join(d, 'ref.000651_c03_q1_zg.fits')
    z.ReferenceImage.from_images(refims, refname, sci_swarp_kws={'COMBINE_TYPE': 'WEIGHTED'})
    w = s.ztf_wcs(nx, ny, dx=2.3, dy=-3.1, rot_deg=0.02)
    f = s.make_frame(nx, ny, 6120, w, star_sky=(ra, dec, fl), fwhm=2.4, sky=170.0, bad_block=(150, 400, 4))
    sci = write('ztf_20200200_000651_zg_c03_o_q1_sciimg.fits', f, 2.4)
    return sci, refname


def test_dosub_and_donightly_fakes(tmp_path, engine, capsys):
    z, s = pkg(), synth()
    d = str(tmp_path)
    sci, refname = night(z, s, d)
    spath = sci.local_path
    model = sci.build_psf()['psf']
    model.save(spath.replace('.fits', '.psf.fits'))
    out = z.sub_name(spath, refname)
    imgs = os.path.join(d, 'images.txt')
    with open(imgs, 'w') as fh:
        fh.write(spath + '\n')
    zp = sci.header['MAGZP'] + model.cards['PSFCOR']

    def products():
        got = {sfx: open(out.replace('.fits', sfx), 'rb').read() for sfx in SUFFIXES}
        for name in os.listdir(d):
            if name.startswith('sub.'):
                os.remove(os.path.join(d, name))
        return got

    def check_table(path, hdr, who):
        t = z.read_fakes_csv(path)
        assert len(t) == 40 and hdr['FAKEN'] == 40 and hdr['FAKESEED'] == 4
        assert (t['mag'] >= 16.0).all() and (t['mag'] < 20.5).all() and (t['inj_flags'] == 0).all()
        assert np.array_equal(t['flux'], 10.0 ** (-0.4 * (t['mag'] - zp)))
        np.testing.assert_allclose(t['flux_in'], t['flux'], rtol=1e-6)
        assert (t['recovered'] <= t['detected']).all() and np.isfinite(t['sep_px'][t['detected']]).all()
        e = z.efficiency(t)
        for key, name in (('FAKEM50', 'm50'), ('FAKEM80', 'm80')):
            assert (key in hdr) == bool(np.isfinite(e[name])) and (key not in hdr or hdr[key] == e[name])
        print(f'{who}: {int(t["recovered"].sum())} of 40 fakes recovered, efficiency per bin {np.round(e["eff"], 2).tolist()} from mag '
              f'{e["edges"][0]:g} in steps of 0.25, m50 {e["m50"]:.3f}, m80 {e["m80"]:.3f}')
        return t

    dosub, donightly = load_script('dosub'), load_script('donightly')
    # dosub.py: without and with --fakes
    assert dosub.main([imgs, refname, '--detect']) == 0
    plain_hdr = z.fits.read_header(out)[0]
    written = sorted(os.listdir(d))
    plain = products()
    held = set(glob.glob(os.path.join(tempfile.gettempdir(), 'zmfakes*')))
    assert dosub.main([imgs, refname, '--detect'] + SWITCHES) == 0
    # the files of the run without --fakes and the table: the fake run left nothing beside them
    assert sorted(os.listdir(d)) == sorted(written + [os.path.basename(out).replace('.fits', '.fakes.csv')])
    assert set(glob.glob(os.path.join(tempfile.gettempdir(), 'zmfakes*'))) == held         # the fake run's directory is gone
    data, hdr, _ = z.fits.read(out)
    assert {k: v for k, v in hdr.items() if k not in CARDS} == plain_hdr
    t_sub = check_table(out.replace('.fits', '.fakes.csv'), hdr, 'dosub.py')
    got = products()
    assert data.tobytes() == z.fits.from_bytes(plain['.fits'])[0].tobytes()
    for sfx in SUFFIXES[1:]:
        assert got[sfx] == plain[sfx], sfx
    # donightly.py: the same, on the pool
    argv = [imgs, refname, '--jobs', '1', '--detect']
    assert len(donightly.main(argv)) == 1
    plain_hdr = z.fits.read_header(out)[0]
    plain = products()
    assert len(donightly.main(argv + SWITCHES)) == 1
    data, hdr, _ = z.fits.read(out)
    assert {k: v for k, v in hdr.items() if k not in CARDS} == plain_hdr
    t_night = check_table(out.replace('.fits', '.fakes.csv'), hdr, 'donightly.py')
    got = products()
    assert data.tobytes() == z.fits.from_bytes(plain['.fits'])[0].tobytes()
    for sfx in SUFFIXES[1:]:
        assert got[sfx] == plain[sfx], sfx
    # both drivers drew from one seed, each away from its own detections
    assert np.array_equal(t_sub['mag'], t_night['mag'])
    # donightly.py --psf builds the model itself: beside the frame and beside the subtraction, its cards in the header
    os.remove(spath.replace('.fits', '.psf.fits'))
    assert donightly.main(argv + SWITCHES) == 2 and '--fakes needs a PSF model' in capsys.readouterr().err
    assert len(donightly.main(argv + ['--psf'] + SWITCHES)) == 1
    a, b = (open(p.replace('.fits', '.psf.fits'), 'rb').read() for p in (spath, out))
    built = z.PSFModel.from_file(out.replace('.fits', '.psf.fits'))
    hdr = z.fits.read_header(out)[0]
    assert a == b and built.half == 12 and abs(built.data.sum() - 1.0) < 1e-14 and built.cards['PSFNSTAR'] >= 10
    assert built.cards == {k: hdr[k] for k in built.cards} and hdr['FAKEN'] == 40
    assert len(z.read_fakes_csv(out.replace('.fits', '.fakes.csv'))) == 40
