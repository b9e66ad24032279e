"""``scripts/donightly.py --detect --stamps`` on a small synthetic night (built as tests/test_scripts_gpu.py builds
one): every subtraction gets its FITS_LDAC catalog and its stamps file, written by the finisher thread."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

from util import pkg, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stamps_without_detect_is_refused(tmp_path):
    script = load_script('donightly')
    assert script.main([str(tmp_path / 'images.txt'), str(tmp_path / 'ref.fits'), '--stamps']) == 2


def test_donightly_detect_writes_catalogs_and_stamps(tmp_path, engine, capsys):
    import torch
    z, s = pkg(), synth()
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    devmod = importlib.import_module('zuds-pipeline_amd.device')
    d = str(tmp_path)
    nx = ny = 1024
    base = s.ztf_wcs(nx, ny, tpv=True)
    rng = np.random.default_rng(78)
    xs, ys = rng.uniform(-20, nx + 20, 80), rng.uniform(-20, ny + 20, 80)
    fl = np.exp(rng.uniform(np.log(3e3), np.log(8e4), 80))
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
        f = s.make_frame(nx, ny, 710 + i, w, star_sky=(ra, dec, fl), fwhm=2.0, noise=3.0, bad_block=(100 + 200 * i, 300, 4))
        refims.append(write(f'ztf_2020010{i}_000651_zg_c03_o_q1_sciimg.fits', f, 2.0))
    refname = os.path.join(d, 'ref.000651_c03_q1_zg.fits')
    z.ReferenceImage.from_images(refims, refname, sci_swarp_kws={'COMBINE_TYPE': 'WEIGHTED'})
    names = []
    for i in range(2):
        w = s.ztf_wcs(nx, ny, dx=rng.uniform(-5, 5), dy=rng.uniform(-5, 5), rot_deg=rng.uniform(-0.05, 0.05))
        tx, ty = rng.uniform(150, nx - 150, 5), rng.uniform(150, ny - 150, 5)
        tra, tdec = w.all_pix2world(tx, ty, 0)
        f = s.make_frame(nx, ny, 810 + i, w, star_sky=(np.concatenate([ra, tra]), np.concatenate([dec, tdec]),
                                                      np.concatenate([fl, np.full(5, 8e3)])),
                         fwhm=2.6, sky=170.0 + 15 * i, bad_block=(150 + 250 * i, 600, 4))
        nm_ = f'ztf_2020020{i}_000651_zg_c03_o_q1_sciimg.fits'
        write(nm_, f, 2.6)
        names.append(os.path.join(d, nm_))
    with open(os.path.join(d, 'images.txt'), 'w') as fh:
        fh.write('\n'.join(names) + '\n')

    script = load_script('donightly')
    argv = [os.path.join(d, 'images.txt'), refname, '--jobs', '2', '--fit-batch', '0', '--nreg-side', '1', '--detect',
            '--stamps']
    done = script.main(argv)
    assert len(done) == 2
    # the pool's rows for the same frames, asked for directly
    io = devmod.FITSDeviceIO(0, engine=z.Engine(0))
    ref = script.load_reference(io, refname)
    pool = nm.SubtractionPool(1)
    nstamped = 0
    for fn, out in zip(names, done):
        sci = script.load_science(io, fn)
        res, = pool.map([nm.SubtractionJob(sci, ref, nreg_side=1, tag=fn, detect=True, stamps=True)])
        cat = z.PipelineFITSCatalog.from_file(out.replace('.fits', '.cat'))
        assert cat.data.dtype.names == res['cat'].dtype.names and len(cat.data) == len(res['cat']) > 0
        for name in cat.data.dtype.names:
            assert np.array_equal(cat.data[name], res['cat'][name], equal_nan=True), name
        assert cat.table_header['ZMDEBLND'] is False and cat.table_header['ZMCLEAN'] is False
        assert float(cat.header['SEEING']) == 2.6 and 'NSTAMPS' in cat.header          # the science header + the fit's cards
        dets = z.Detection.from_catalog(cat, filter=True)
        good = cat.data[cat.data['GOODCUT'] == 1]
        assert len(dets) == len(good) > 0
        assert [dt.x_image for dt in dets] == [float(v) for v in good['X_IMAGE']]
        # the stamps file: the layout of dosub.write_stamps
        sp = out.replace('.fits', '.stamps.fits')
        if res.get('too_many'):                              # more than 50 detections: the catalog, no stamps
            assert len(good) > 50 and not os.path.exists(sp)
            continue
        nstamped += 1
        blocks, hdr, tab, th = z.fits.read_image_table(sp)
        assert blocks.shape == (len(good), 3, 63, 63) and blocks.dtype == np.float32
        assert hdr['STAMPSZ'] == 63 and hdr['NDET'] == len(good) and th['EXTNAME'] == 'STAMPS'
        assert tab.dtype.names == ('ra', 'dec', 'x0', 'y0', 'nx_trim', 'ny_trim')
        assert np.array_equal(tab['ra'], good['X_WORLD']) and np.array_equal(tab['dec'], good['Y_WORLD'])
        assert np.array_equal(tab['x0'], res['stamps']['x0']) and np.array_equal(tab['y0'], res['stamps']['y0'])
        assert (tab['nx_trim'] <= 63).all() and (tab['ny_trim'] <= 63).all() and (tab['nx_trim'] > 0).all()
        assert np.array_equal(blocks, res['stamps']['blocks'])
    pool.close()
    io.close()
    assert nstamped >= 1
    # a second run skips every image
    capsys.readouterr()
    assert script.main(argv) == []
    assert capsys.readouterr().out.count('subtraction exists, skipping') == 2
