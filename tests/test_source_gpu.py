"""``source.associate`` on the GPU: the toy night of tests/test_source_host.py through the real library, and the two
drivers - ``donightly.py --detect --associate`` and ``makesources.py`` - on a small synthetic night (built as
tests/test_nightly_detect_script_gpu.py builds one, with the same transients in both science frames), their two tables
against tests/assoc_ref.py."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

import assoc_ref as ar
from util import pkg, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_associate_on_the_toy_night(engine):
    z = pkg()
    dets, known, stars = ar.toy_night(z.Detection, z.Source)
    names = []
    out = z.associate(dets, sources=known, stars=stars, name=lambda k: names.append(k) or f'n{k}', engine=engine)
    ar.check_toy_night(dets, out, names)


def test_flags_are_checked(tmp_path):
    script = load_script('donightly')
    assert script.main([str(tmp_path / 'images.txt'), str(tmp_path / 'ref.fits'), '--associate']) == 2
    assert script.main([str(tmp_path / 'images.txt'), str(tmp_path / 'ref.fits'), '--detect', '--stars', 'x.txt']) == 2


@pytest.fixture(scope='module')
def night(tmp_path_factory, engine):
    """Two science frames with the same eight transients, subtracted and associated by donightly.py."""
    z, s = pkg(), synth()
    d = str(tmp_path_factory.mktemp('assoc_night'))
    nx = ny = 1024
    base = s.ztf_wcs(nx, ny, tpv=True)
    rng = np.random.default_rng(178)
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
        f = s.make_frame(nx, ny, 1710 + i, w, star_sky=(ra, dec, fl), fwhm=2.0, noise=3.0, bad_block=(100 + 200 * i, 300, 4))
        refims.append(write(f'ztf_2020010{i}_000651_zg_c03_o_q1_sciimg.fits', f, 2.0))
    refname = os.path.join(d, 'ref.000651_c03_q1_zg.fits')
    z.ReferenceImage.from_images(refims, refname, sci_swarp_kws={'COMBINE_TYPE': 'WEIGHTED'})
    tx, ty = rng.uniform(200, nx - 200, 8), rng.uniform(200, ny - 200, 8)
    tra, tdec = base.all_pix2world(tx, ty, 0)
    names = []
    for i in range(2):
        w = s.ztf_wcs(nx, ny, dx=rng.uniform(-5, 5), dy=rng.uniform(-5, 5), rot_deg=rng.uniform(-0.05, 0.05))
        f = s.make_frame(nx, ny, 1810 + i, w, star_sky=(np.concatenate([ra, tra]), np.concatenate([dec, tdec]),
                                                       np.concatenate([fl, np.full(8, 8e3 * (1 + i))])),
                         fwhm=2.6, sky=170.0 + 15 * i, bad_block=(150 + 250 * i, 600, 4))
        nm_ = f'ztf_2020020{i}_000651_zg_c03_o_q1_sciimg.fits'
        write(nm_, f, 2.6)
        names.append(os.path.join(d, nm_))
    images = os.path.join(d, 'images.txt')
    with open(images, 'w') as fh:
        fh.write('\n'.join(names) + '\n')
    # a star on top of the first transient, one 30 arcsec from everything
    stars = os.path.join(d, 'stars.txt')
    np.savetxt(stars, np.array([[tra[0], tdec[0]], [tra[0], tdec[0] + 30.0 / 3600]]), fmt='%.10f')
    done = load_script('donightly').main([images, refname, '--jobs', '2', '--fit-batch', '0', '--nreg-side', '1', '--detect',
                                          '--associate', '--stars', stars])
    assert len(done) == 2
    return dict(dir=d, done=done, images=images, stars=stars, transients=(tra, tdec))


def expected(night):
    """The detections of the catalogs on disk and what the restatement makes of them."""
    z = pkg()
    rows = []
    for out in night['done']:
        cat = z.PipelineFITSCatalog.from_file(out.replace('.fits', '.cat'))
        t = cat.data
        for k in np.flatnonzero(t['GOODCUT'] == 1):
            rows.append((os.path.basename(out).replace('.fits', '.cat'), int(k), float(t['X_WORLD'][k]), float(t['Y_WORLD'][k]),
                         float(t['FLUX_APER'][k]) / float(t['FLUXERR_APER'][k])))
    ra, dec, snr = (np.array([r[i] for r in rows]) for i in (2, 3, 4))
    return rows, ra, dec, ar.cluster_ref(ra, dec, snr, None, 2.0)


def check_tables(night, sources_path, det_path):
    rows, ra, dec, want = expected(night)
    assert want['nsrc'] >= 4                                      # most of the eight transients are found in both frames
    src_lines = [l.split() for l in open(sources_path).read().splitlines()[1:]]
    det_lines = [l.split() for l in open(det_path).read().splitlines()[1:]]
    assert len(src_lines) == want['nsrc'] and len(det_lines) == len(rows)
    ids = [f[0] for f in src_lines]
    assert ids == [f'src{k:07d}' for k in range(want['nsrc'])]
    for k, (f, row) in enumerate(zip(det_lines, rows)):
        assert (f[0], int(f[1])) == row[:2] and abs(float(f[2]) - row[2]) < 1e-8 and abs(float(f[3]) - row[3]) < 1e-8
        assert f[4] == (ids[want['label'][k]] if want['label'][k] >= 0 else '-')
    sidx, ssep = ar.crossmatch_ref(ra[want['best']], dec[want['best']], *np.loadtxt(night['stars']).T, 1.5, check=False)
    nrej = 0
    for s, f in enumerate(src_lines):
        b = want['best'][s]
        assert abs(float(f[1]) - ra[b]) < 1e-8 and abs(float(f[2]) - dec[b]) < 1e-8 and int(f[3]) == want['count'][s]
        assert f[5] == rows[b][0]
        rejected = sidx[s] >= 0 and ssep[s] < 1.5
        nrej += rejected
        assert int(f[6]) == int(rejected) and float(f[4]) == (-1.0 if rejected else 0.0)
    return nrej


def test_donightly_associate_writes_the_two_tables(night):
    prefix = os.path.splitext(night['images'])[0] + '.sources'
    nrej = check_tables(night, prefix + '.txt', prefix + '.det.txt')
    assert nrej == 1                                              # the star on the first transient


def test_makesources_from_the_catalogs_on_disk(night, capsys):
    script = load_script('makesources')
    cats = [out.replace('.fits', '.cat') for out in night['done']]
    prefix = os.path.join(night['dir'], 'ms')
    sp, dp = script.main(cats + ['--stars', night['stars'], '--out', prefix])
    check_tables(night, sp, dp)
    night_prefix = os.path.splitext(night['images'])[0] + '.sources'
    assert open(sp).read() == open(night_prefix + '.txt').read() and open(dp).read() == open(night_prefix + '.det.txt').read()
    # a second run against the first one's sources: every clustered detection joins its source, nothing new is made
    sp2, dp2 = script.main(cats + ['--sources', sp, '--out', prefix + '2'])
    a = [l.split() for l in open(dp).read().splitlines()[1:]]
    b = [l.split() for l in open(dp2).read().splitlines()[1:]]
    assert [r[4] for r in a] == [r[4] for r in b]
    assert len(open(sp2).read().splitlines()) == len(open(sp).read().splitlines())
