"""zm_extract_deblend (csrc/deblend.hip) against the numpy restatement (tests/deblend_ref.py) on the GPU.

The filtered plane, the segmentation map, every integer column and PARENT_NUMBER are compared bit for bit.  The float
columns are held to the bounds of tests/test_extract_gpu.py, figures printed before anything is asserted: 10 x the
difference between the restatement's forward and reversed summation order, plus ``extract_ref.LIBM_ULPS`` spacings for
THETA_IMAGE and FWHM_IMAGE; FLUX_APER and FLUXERR_APER to the aperture kernel's existing pin (rtol 1e-10, atol 1e-9).
Every row is compared in every column: the NaN / +inf / -inf pattern of a float column must equal the restatement's, and
outside the poisoned scenes every float must be finite.  Where the restatement's filtered plane holds a NaN (``filter=False``
over a NaN pixel) NaN-ness is compared instead of the bytes.  Every test calls ``deblend=``.

The scenes added for the tree kernel's indexing (tests/deblend_scenes.py; tests/test_deblend_ref.py proves on the
restatement that each reaches what it names): every accepted ``nthresh`` (2 .. 64; one scene changes its outcome between 2
and 32, one between 32 and 64, one object occupies 51 of the 64 levels); bounding boxes of 1, 2 and 3 pixels' width and
blocks on either side of the LDS limit, the thin ones hanging together through one diagonal step; blends on the right
and bottom edge, in the four corners, frames that are one object (37 x 29, 31 x 29, 1 x 40, 40 x 1); bad pixels on a
saddle, on the peak, along a diagonal line, as holes in a wing, along the frame's edge; a flag plane; and NaN, +inf, -inf
in ``img`` and NaN, 0, -1 in ``sigma`` at the saddle and in the hole, measured with an aperture that reaches them.

Outcomes of the scenes (restatement and GPU alike): pairs 3 and 4 px apart stay one object, 5, 6 and 8 px apart give
two; the companion of 0.4 % of the flux stays merged, the one of 1.2 % splits; three nested peaks give three objects; the
mesas split 112 / 112; the noisy field goes from 15 objects to 20 (three parents split, one of them in four); the lone
star stays whole; the two 512 x 512 single-object frames split in two.
"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import deblend_scenes as ds
import extract_ref as xr

pytestmark = pytest.mark.gpu

APER_COLUMNS = ('FLUX_APER', 'FLUXERR_APER')
INT_COLUMNS = xr.INT_COLUMNS + ['PARENT_NUMBER']


def run(engine, name, **more):
    img, sigma, kw = ds.scene(name)
    ex, db = ds.split_kw(kw)
    return engine.extract(img, sigma, full=True, deblend=db or True, **ex, **more)


def compare(engine, name, finite=True):
    """``finite``: every float of both tables must be finite (every scene but the poisoned ones).  Otherwise the NaN / inf
    pattern of every float column must equal the restatement's; no row and no column is left out either way."""
    got, ref, rev = run(engine, name), ds.reference(name), ds.reference(name, reverse=True)
    assert got['status'] == 0
    ds.assert_same_plane(got['filtered'], ref['filtered'])
    assert np.array_equal(got['segm'], ref['segm']), 'segmentation map'
    t, r = got['table'], ref['table']
    assert got['nfound'] == len(r) == len(t)
    for c in INT_COLUMNS:
        assert np.array_equal(t[c], r[c]), c
    worst, bounds, fails = ds.float_columns(t, r, rev['table'], APER_COLUMNS, finite)
    print(f'deblend {name}: {len(ref["first"]["table"])} -> {len(r)} objects; column measured (order bound; libm allowance '
          f'in spacings): ' + ', '.join(f'{c} {worst[c]:.3g} ({bounds[c]:.3g}; {xr.LIBM_ULPS.get(c, 0)})'
                                        for c in xr.FLOAT_COLUMNS))
    assert not fails, fails
    return got, ref


@pytest.mark.parametrize('sep,n', [(3, 1), (4, 1), (5, 2), (6, 2), (8, 2)])
def test_pair(engine, sep, n):
    got, ref = compare(engine, f'pair{sep}')
    t = got['table']
    assert len(t) == n and (t['PARENT_NUMBER'] == 1).all()
    assert ((t['FLAGS'] & 2) != 0).all() == (n == 2) and not (t['FLAGS'] & 1).any()
    if n == 2:                                            # one row per star, each within a pixel of its centre
        assert np.abs(t['X_IMAGE'] - 1.0 - [20, 20 + sep]).max() < 1.0 and np.abs(t['Y_IMAGE'] - 25.0).max() < 0.5


def assert_equals_default_call(engine, name, got):
    img, sigma, kw = ds.scene(name)
    ex, _ = ds.split_kw(kw)
    plain = engine.extract(img, sigma, full=True, **ex)
    assert 'PARENT_NUMBER' not in plain['table'].dtype.names
    assert got['segm'].tobytes() == plain['segm'].tobytes() and got['nfound'] == plain['nfound']
    for c in plain['table'].dtype.names:
        assert got['table'][c].tobytes() == plain['table'][c].tobytes(), c
    assert np.array_equal(got['table']['PARENT_NUMBER'], plain['table']['NUMBER'])


def test_contrast_on_both_sides_of_mincont(engine):
    got, _ = compare(engine, 'contrast20')
    assert len(got['table']) == 1
    assert_equals_default_call(engine, 'contrast20', got)
    got, _ = compare(engine, 'contrast60')
    assert len(got['table']) == 2 and ((got['table']['FLAGS'] & 2) != 0).all()
    # mincont is what decides: the faint companion splits off at a lower one, the brighter one merges at a higher one
    img, sigma, _ = ds.scene('contrast20')
    assert len(engine.extract(img, sigma, deblend=dict(mincont=0.001))[0]) == 2
    img, sigma, _ = ds.scene('contrast60')
    assert len(engine.extract(img, sigma, deblend=dict(mincont=0.05))[0]) == 1


def test_nested_peaks_keep_their_earlier_split(engine):
    got, _ = compare(engine, 'nested')
    t = got['table']
    assert len(t) == 3 and ((t['FLAGS'] & 2) != 0).all() and (t['PARENT_NUMBER'] == 1).all()
    assert np.abs(np.sort(t['X_IMAGE']) - 1.0 - [20, 25, 34]).max() < 1.0


def test_plateaus_and_every_tie_rule(engine):
    got, _ = compare(engine, 'plateaus')
    assert got['table']['ISOAREA_IMAGE'].tolist() == [112, 112]


def test_sigma_step_across_a_blend(engine):
    got, ref = compare(engine, 'sigma_step')
    assert len(got['table']) == 2
    assert np.array_equal(got['segm'] > 0, ref['first']['segm'] > 0)          # level 0 is the whole object


def test_noisy_field_and_lone_star(engine):
    got, ref = compare(engine, 'noisy_field')
    t = got['table']
    parts = np.bincount(t['PARENT_NUMBER'])
    assert (len(ref['first']['table']), len(t), parts.max()) == (15, 20, 4)
    assert np.array_equal((t['FLAGS'] & 2) != 0, parts[t['PARENT_NUMBER']] > 1)
    got, _ = compare(engine, 'lone_star')
    assert len(got['table']) == 1
    assert_equals_default_call(engine, 'lone_star', got)


@pytest.mark.parametrize('name', ['all_above', 'spiral_with_knots'])
def test_single_objects_of_a_whole_frame(engine, name):
    got, _ = compare(engine, name)
    t = got['table']
    assert len(t) == 2 and t['ISOAREA_IMAGE'].sum() == (got['segm'] > 0).sum() and ((t['FLAGS'] & 2) != 0).all()


@pytest.mark.parametrize('width', [32, 33])
def test_boxes_on_either_side_of_the_lds_limit(engine, width):
    """The tree kernel keeps an object's planes in LDS up to 1024 box pixels (32 x 32) and in global memory beyond."""
    got, ref = compare(engine, f'box{32 * width}')
    t = got['table']
    assert len(t) == 2 and (t['XMAX_IMAGE'].max() - t['XMIN_IMAGE'].min() + 1, t['YMAX_IMAGE'].max() - t['YMIN_IMAGE'].min() + 1) \
        == (width, 32) and t['ISOAREA_IMAGE'].sum() == 32 * width


@pytest.mark.parametrize('nthresh', ds.NTHRESH)
@pytest.mark.parametrize('base', list(ds.NTHRESH_OBJECTS))
def test_every_nthresh(engine, base, nthresh):
    """nlev = nthresh sets the length of u[] / hist[] (full at 64), the number of square roots and every per-level loop."""
    got, ref = compare(engine, f'{base}@{nthresh}')
    assert len(got['table']) == ds.NTHRESH_OBJECTS[base][nthresh]
    assert len(run(engine, base)['table']) == ds.NTHRESH_OBJECTS[base][32]     # the engine is not left at another nthresh


@pytest.mark.parametrize('name', list(ds.BOX_SCENES))
def test_box_shapes_around_the_lds_limit(engine, name):
    """1, 2 and 3 pixels wide and blocks, in both forms of the tree kernel; the thin ones hold a diagonal-only connection."""
    got, ref = compare(engine, name)
    t = got['table']
    bw, bh, npix, _, n = ds.EXPECT[name]
    assert len(t) == n == 2 and t['ISOAREA_IMAGE'].sum() == npix and ((t['FLAGS'] & 2) != 0).all()
    assert (t['XMAX_IMAGE'].max() - t['XMIN_IMAGE'].min() + 1, t['YMAX_IMAGE'].max() - t['YMIN_IMAGE'].min() + 1) == (bw, bh)


@pytest.mark.parametrize('name', list(ds.SINGLE_LINES))
def test_single_peak_lines_equal_the_default_call(engine, name):
    """One thin line on either side of DB_CELLS that does not split: table and map are the default call's bit for bit."""
    got, ref = compare(engine, name)
    assert len(got['table']) == 1 and ref['nsplit'] == 0 and got['table']['ISOAREA_IMAGE'][0] == ds.EXPECT[name][2]
    assert_equals_default_call(engine, name, got)


@pytest.mark.parametrize('name', list(ds.EDGE_SCENES))
def test_frame_edges(engine, name):
    """Right and bottom edge, the four corners, frames that are one object (global and LDS form), one column, one row."""
    got, ref = compare(engine, name)
    t = got['table']
    assert len(t) == ds.EXPECT[name][4] and ((t['FLAGS'] & 2) != 0).all() and ((t['FLAGS'] & 8) != 0).any()
    ny, nx = got['segm'].shape
    if name.startswith('frame'):
        assert (got['segm'] > 0).all() and t['ISOAREA_IMAGE'].sum() == nx * ny and ((t['FLAGS'] & 8) != 0).all()


@pytest.mark.parametrize('name', list(ds.BAD_SCENES))
def test_bad_pixels_and_flags(engine, name):
    """``bad`` and ``flag`` planes as DeviceSubtraction.extract always passes them; the bad pixels hold finite values, so
    every float of the table must be finite."""
    got, ref = compare(engine, name, finite=True)
    t, kw = got['table'], ds.scene(name)[2]
    assert len(t) == ds.EXPECT[name][4] and not (got['segm'][kw['bad'] != 0] != 0).any()
    plain = engine.extract(*ds.scene(name)[:2], full=True, deblend=True, filter=kw['filter'])      # the plane matters
    assert not np.array_equal(plain['segm'], got['segm'])
    if 'flags' in name:
        assert t['IMAFLAGS_ISO'].tolist() == [0, 0x40000010] and t['FLAGS_WEIGHT'].tolist() == [1, 0]


@pytest.mark.parametrize('name', list(ds.POISON_SCENES))
def test_poisoned_pixels(engine, name):
    """NaN, +inf, -inf in img; NaN, 0, -1 in sigma, at the saddle and as a 3 x 3 hole: they are bad pixels to the map, and
    the aperture of radius 7 sums over whatever they hold - the NaN / inf pattern must be the restatement's."""
    got, ref = compare(engine, name, finite=False)
    t = got['table']
    assert len(t) == ds.EXPECT[name][4] == 2 and (t['FLAGS'] & 16).any()
    column = 'FLUX_APER' if name.startswith('img') else 'FLUXERR_APER'
    assert name.startswith(('sig0', 'signeg')) or not np.isfinite(t[column]).all()


def test_limits(engine):
    got, _ = compare(engine, 'edge')
    assert len(got['table']) == 2 and ((got['table']['FLAGS'] & 8) != 0).all()
    got, _ = compare(engine, 'just_too_small')
    assert got['table']['ISOAREA_IMAGE'].tolist() == [9, 6, 5] and got['table']['FLAGS'].tolist() == [0, 2, 2]
    one = np.full((1, 1), 10.0, np.float32)
    for minarea, n in ((1, 1), (5, 0)):
        r = engine.extract(one, np.ones_like(one), full=True, deblend=True, detect_minarea=minarea)
        assert len(r['table']) == n == r['nfound'] and int(r['segm'][0, 0]) == n and r['status'] == 0
        assert 'PARENT_NUMBER' in r['table'].dtype.names
    empty = np.zeros((40, 56), np.float32)
    r = engine.extract(empty, np.ones_like(empty), full=True, deblend=True)
    assert len(r['table']) == 0 and r['nfound'] == 0 and not r['segm'].any()


def test_fewer_rows_than_objects(engine):
    full = run(engine, 'noisy_field')
    part = run(engine, 'noisy_field', max_objects=7)
    assert len(part['table']) == 7 and part['nfound'] == len(full['table']) == 20 and part['status'] == 0
    assert part['table'].tobytes() == full['table'][:7].tobytes()
    assert np.array_equal(part['segm'], full['segm'])
    none = run(engine, 'noisy_field', max_objects=0)
    assert len(none['table']) == 0 and none['nfound'] == 20 and np.array_equal(none['segm'], full['segm'])


def test_entry_points_and_runs_give_the_same_bytes(engine):
    hipmem = importlib.import_module('zuds-pipeline_amd.hipmem')
    img, sigma, _ = ds.scene('noisy_field')
    a, b = run(engine, 'noisy_field'), run(engine, 'noisy_field')
    assert a['table'].tobytes() == b['table'].tobytes() and a['segm'].tobytes() == b['segm'].tobytes()
    bufs = []
    for arr in (img, sigma):
        d = hipmem.DeviceBuffer(arr.nbytes)
        d.upload(np.ascontiguousarray(arr))
        bufs.append(d)
    dseg = hipmem.DeviceBuffer(a['segm'].nbytes)
    dtab, nfound = engine.extract_dev(bufs[0].ptr, bufs[1].ptr, None, None, 128, 128, segm=dseg.ptr, deblend=True)
    assert nfound == 20 and dtab.dtype == a['table'].dtype and dtab.tobytes() == a['table'].tobytes()
    assert np.array_equal(dseg.download(np.int32, a['segm'].shape), a['segm'])
    # ... and with a bad and a flag plane on the device, as DeviceSubtraction.extract calls it
    for name in ('bad_flags.f1', 'bad_diag.f0'):
        img, sigma, kw = ds.scene(name)
        flag = kw.get('flag', np.arange(48 * 48, dtype=np.int32).reshape(48, 48) % 7)
        a, b = (engine.extract(img, sigma, kw['bad'], flag, full=True, deblend=True, filter=kw['filter']) for _ in range(2))
        assert a['table'].tobytes() == b['table'].tobytes() and a['segm'].tobytes() == b['segm'].tobytes()
        assert a['table']['IMAFLAGS_ISO'].any() and a['table']['FLAGS_WEIGHT'].any()
        bufs = []
        for arr, dt in ((img, np.float32), (sigma, np.float32), (kw['bad'], np.uint8), (flag, np.int32)):
            arr = np.ascontiguousarray(arr, dt)
            d = hipmem.DeviceBuffer(arr.nbytes)
            d.upload(arr)
            bufs.append(d)
        dseg = hipmem.DeviceBuffer(a['segm'].nbytes)
        dtab, nfound = engine.extract_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 48, 48, segm=dseg.ptr, deblend=True,
                                          filter=kw['filter'])
        assert nfound == len(a['table']) and dtab.tobytes() == a['table'].tobytes()
        assert np.array_equal(dseg.download(np.int32, a['segm'].shape), a['segm'])


def test_wide_table_measures_the_sub_objects(engine):
    img, sigma, _ = ds.scene('pair8')
    iso = engine.extract(img, sigma, full=True, deblend=True)
    wide = engine.extract(img, sigma, full=True, deblend=True, columns='param')
    t = wide['table']
    assert len(t) == 2 and np.array_equal(wide['segm'], iso['segm'])
    for c in iso['table'].dtype.names:
        assert t[c].tobytes() == iso['table'][c].tobytes(), c
    assert np.isfinite(t['FLUX_AUTO']).all() and (t['FLUX_AUTO'] > 0).all()
    assert np.abs(t['XWIN_IMAGE'] - 1.0 - [20, 28]).max() < 0.5 and np.abs(t['YWIN_IMAGE'] - 25.0).max() < 0.5
    # the second pass read the deblended map: its rows are those of the same pass on that map and those rows
    merged = engine.extract(img, sigma, columns='param')[0]
    assert len(merged) == 1 and abs(merged['XWIN_IMAGE'][0] - 1.0 - 20) < 1.0


def test_bad_settings_are_refused(engine, zuds):
    img, sigma, _ = ds.scene('pair5')
    for bad in (dict(nthresh=24), dict(nthresh=128), dict(mincont=1.5), dict(levels=3)):
        with pytest.raises(ValueError):
            engine.extract(img, sigma, deblend=bad)
    # ... and by the library itself
    L, lib = zuds._lib.lib(), zuds._lib
    p, d = lib.zm_extract_params(), lib.zm_deblend_params()
    L.zm_extract_params_default(C.byref(p))
    L.zm_deblend_params_default(C.byref(d))
    assert (d.nthresh, d.mincont) == (32, 0.005)
    n = C.c_int()
    src = np.ascontiguousarray(img)
    for nthresh, mincont in ((24, 0.005), (32, 1.5), (32, float('nan'))):
        d.nthresh, d.mincont = nthresh, mincont
        rc = L.zm_extract_deblend(engine.ctx, src.ctypes.data, sigma.ctypes.data, None, None, 48, 48, None, C.byref(p), 0, None,
                                  None, None, C.byref(n), C.byref(n), None, C.byref(d), None)
        assert rc != 0 and b'zm_extract_deblend: bad parameters' in L.zm_last_error()
    rc = L.zm_extract_deblend(engine.ctx, src.ctypes.data, sigma.ctypes.data, None, None, 48, 48, None, C.byref(p), 0, None, None,
                              None, C.byref(n), C.byref(n), None, None, None)
    assert rc != 0 and b'zm_extract_deblend' in L.zm_last_error()


# ---- through the layers ---------------------------------------------------------------------------------------------
PAIR_SEP = 5.0


@pytest.fixture(scope='module')
def blended_subtraction(tmp_path_factory):
    """BASELINE config 0 as tests/test_catalog_gpu.py sets it up (4 frames 512 x 512, shared TAN WCS, the last one is the
    science frame), with one pair of point sources PAIR_SEP px apart injected into the science frame."""
    from test_catalog_gpu import choose_injections, write_frame
    from util import pkg, synth
    z, s = pkg(), synth()
    d = str(tmp_path_factory.mktemp('deblend'))
    base = s.tan_wcs(512, 512)
    rng = np.random.default_rng(4321)
    xs, ys = rng.uniform(10, 500, 40), rng.uniform(10, 500, 40)
    fl = np.exp(rng.uniform(np.log(1e3), np.log(1e5), 40))
    ra, dec = base.all_pix2world(xs, ys, 0)
    frames = []
    for i, (dx, dy) in enumerate([(0, 0), (3.3, -2.2), (-1.6, 4.1), (2.4, 1.3)]):
        w = s.tan_wcs(512, 512, dx=dx, dy=dy)
        f = s.make_frame(512, 512, 4321 + i, w, star_sky=(ra, dec, fl), fwhm=2.0, bad_block=(50 + 60 * i, 80 + 40 * i, 5))
        f['header']['SEEING'] = 2.0
        frames.append(f)
    f3 = frames[3]
    sx, sy = f3['wcs'].all_world2pix(ra, dec, 0)
    (px,), (py,) = choose_injections(np.random.default_rng(99), 1, 512, 512, (sx, sy), f3['mask'] != 0, border=60, apart=25.0)
    px, py = float(np.round(px)), float(np.round(py))
    img = f3['img'].astype(np.float64)
    s.add_stars(img, np.array([px, px + PAIR_SEP]), np.array([py, py]), np.array([6000.0, 4500.0]), 2.0)
    f3['img'] = img.astype(np.float32)
    ims = [write_frame(z, d, f'ztf_2020053{i}_000651_zg_c03_o_q1_sciimg.fits', f) for i, f in enumerate(frames)]
    refname = os.path.join(d, 'ref.000651_c03_q1_zg.fits')
    ref = z.ReferenceImage.from_images(ims[:3], refname)
    return dict(z=z, d=d, frames=frames, ims=ims, ref=ref, refname=refname, pair=(px, py))


def rows_near(tab, x, y, radius=1.5):
    return np.flatnonzero(np.hypot(tab['X_IMAGE'] - 1.0 - x, tab['Y_IMAGE'] - 1.0 - y) < radius)


def test_candidates_return_both_members_of_an_injected_pair(blended_subtraction, engine):
    import torch
    sc = blended_subtraction
    ref, sci, f = sc['ref'], sc['ims'][3], sc['frames'][3]
    px, py = sc['pair']
    dmod = importlib.import_module('zuds-pipeline_amd.device')
    chain = dmod.DeviceSubtraction(sci.wcs, ref.wcs, device=0, engine=engine)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to('cuda:0')
    args = (t(f['img'], np.float32), t(sci.rms_image.data, np.float32), t(f['mask'], np.int32),
            t(sci.weight_image.data, np.float32), t(ref.data, np.float32), t(ref.rms_image.data, np.float32),
            t(ref.mask_image.data, np.int32))
    torch.cuda.synchronize()
    chain.run(*args, seeing=2.0, nreg_side=1, hotpants_kws={'ko': 0, 'bgo': 0},
              ref_flxscale=float(ref.header.get('FLXSCALE', 1.0)))
    plain, nplain = chain.candidates(2.0)
    both, nboth = chain.candidates(2.0, deblend=True)
    chain.stream.synchronize()
    engine.set_stream(0)
    assert 'PARENT_NUMBER' in both.dtype.names and 'PARENT_NUMBER' not in plain.dtype.names and nboth > nplain
    # one row between the two without deblending; with it a row on either member, both flagged as deblended
    assert len(rows_near(plain, px, py)) + len(rows_near(plain, px + PAIR_SEP, py)) == 0
    assert len(rows_near(plain, px + 0.5 * PAIR_SEP, py, radius=2.5)) == 1
    a, b = rows_near(both, px, py), rows_near(both, px + PAIR_SEP, py)
    assert len(a) == 1 and len(b) == 1 and a[0] != b[0]
    assert (both['FLAGS'][[a[0], b[0]]] & 2).all() and both['PARENT_NUMBER'][a[0]] == both['PARENT_NUMBER'][b[0]]
    assert 'GOODCUT' in both.dtype.names


def test_dosub_detect_deblend_writes_the_cards(blended_subtraction, engine, monkeypatch, capsys):
    from test_catalog_gpu import load_script
    sc = blended_subtraction
    z, d = sc['z'], sc['d']
    script = load_script('dosub')
    monkeypatch.setattr(script, 'MAX_DETS', 10 ** 6)
    jobs = os.path.join(d, 'images.txt')
    with open(jobs, 'w') as f:
        f.write(sc['ims'][3].local_path + '\n')
    assert script.main([jobs, sc['refname'], '--deblend']) == 2            # needs --detect
    capsys.readouterr()
    assert script.main([jobs, sc['refname'], '--detect', '--deblend']) == 0
    out = capsys.readouterr().out
    assert 'cat: ' in out and 'Traceback' not in out
    cat = z.PipelineFITSCatalog.from_file(z.sub_name(sc['ims'][3].local_path, sc['refname']).replace('.fits', '.cat'))
    th = cat.table_header
    assert th['ZMDEBLND'] is True and th['ZMDBNTHR'] == 32 and abs(th['ZMDBMINC'] - 0.005) < 1e-12 and th['ZMCLEAN'] is False
    assert 'PARENT_NUMBER' in cat.data.dtype.names and 'GOODCUT' in cat.data.dtype.names
    px, py = sc['pair']
    assert len(rows_near(cat.data, px, py)) == 1 and len(rows_near(cat.data, px + PAIR_SEP, py)) == 1
