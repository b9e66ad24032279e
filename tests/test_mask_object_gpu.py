"""The masked second pass through the layers: run_sextractor -> catalog file -> Engine.extract, DeviceSubtraction.extract
on resident planes, and scripts/dosub.py --detect --param-columns --mask-type correct."""
import importlib
import os

import numpy as np
import pytest

import mask_scenes as ms
from test_deblend_gpu import blended_subtraction                             # noqa: F401  (the fixture: one small subtraction)
from util import pkg, synth

pytestmark = pytest.mark.gpu

MASK_NAMES = ['NREPL_AUTO', 'NLOST_AUTO', 'NREPL_APER', 'NLOST_APER', 'NREPL_WIN', 'NLOST_WIN']


def test_run_sextractor_writes_a_masked_catalog_that_equals_the_engines_rows(tmp_path, engine):
    from test_catalog_gpu import write_frame
    z, s = pkg(), synth()
    sx = importlib.import_module('zuds-pipeline_amd.sextractor')
    stars, _ = ms.deblended_planes()
    f = s.make_frame(96, 80, 11, s.tan_wcs(96, 80), nstars=0, sky=150.0, noise=1.0)
    f['img'] = (f['img'].astype(np.float64) + stars).astype(np.float32)
    im = write_frame(z, str(tmp_path), 'ztf_20200531_000651_zg_c03_o_q1_sciimg.fits', f)
    cat, sub = sx.run_sextractor(im, checkimage_type=['bkgsub'], catalog=True, columns='param', mask='correct', deblend=True)
    assert cat.mask == 'correct' and cat.deblend == dict(nthresh=32, mincont=0.005)
    back = z.PipelineFITSCatalog.from_file(cat.local_path)
    assert back.table_header['ZMMASKTY'] == 'CORRECT' and back.mask == 'correct' and back.table_header['ZMDEBLND'] is True
    names = back.data.dtype.names
    assert set(MASK_NAMES) <= set(names) and 'PARENT_NUMBER' in names and 'FLUX_AUTO' in names
    for c in cat.data.dtype.names:
        assert np.array_equal(np.asarray(back.data[c]), cat.data[c], equal_nan=True), c
    # its rows are Engine.extract's on the same planes
    tab, segm = engine.extract(sub.data, im.rms_image.data, bad=im.weight_image.data == 0, flag=im.mask_image.data,
                               wcs=im.wcs, columns='param', mask='correct', deblend=True,
                               satur_level=float(im.header['SATURATE']))
    assert tab.dtype == cat.data.dtype and tab.tobytes() == cat.data.tobytes()
    # a real deblended pair went through: both members replaced pixels of the other, and the table says so
    pair = np.flatnonzero((tab['FLAGS'] & 2) != 0)
    assert len(pair) >= 2 and (tab['NREPL_AUTO'][pair] > 0).all() and len(tab) >= 10
    plain, _ = engine.extract(sub.data, im.rms_image.data, bad=im.weight_image.data == 0, flag=im.mask_image.data,
                              wcs=im.wcs, columns='param', deblend=True, satur_level=float(im.header['SATURATE']))
    assert len(plain) == len(tab) and (tab['FLUX_AUTO'][pair] < plain['FLUX_AUTO'][pair]).all()
    quiet = np.flatnonzero((tab['NREPL_AUTO'] + tab['NLOST_AUTO'] + tab['NREPL_WIN'] + tab['NLOST_WIN'] +
                            tab['NREPL_APER'] + tab['NLOST_APER']) == 0)
    assert len(quiet) >= 4 and np.array_equal(tab['XWIN_IMAGE'][quiet], plain['XWIN_IMAGE'][quiet])
    # MASK_TYPE in sextractor_kws overrides the keyword; NONE is the plain second pass; alone it stays refused
    none = sx.run_sextractor(im, catalog=True, columns='param', mask='correct', deblend=True,
                             sextractor_kws={'MASK_TYPE': 'NONE'})[0]
    assert none.mask is None and none.data.dtype == plain.dtype and none.data.tobytes() == plain.tobytes()
    assert z.PipelineFITSCatalog.from_file(none.local_path).table_header['ZMMASKTY'] == 'NONE'
    blank = sx.run_sextractor(im, catalog=True, columns='param', mask='correct', sextractor_kws={'MASK_TYPE': 'BLANK'})[0]
    assert blank.mask == 'blank' and not blank.data['NREPL_AUTO'].any()
    with pytest.raises(ValueError, match='MASK_TYPE'):
        sx.run_sextractor(im, catalog=True, columns='param', sextractor_kws={'MASK_TYPE': 'CORRECT'})
    with pytest.raises(ValueError, match="needs columns='param'"):
        sx.run_sextractor(im, catalog=True, mask='correct')
    with pytest.raises(ValueError, match="needs columns='param'"):
        engine.extract(sub.data, im.rms_image.data, mask='blank')


def test_device_planes_give_the_host_routes_table(blended_subtraction, engine):
    import torch
    sc = blended_subtraction
    z, ref, sci, f = sc['z'], sc['ref'], sc['ims'][3], sc['frames'][3]
    dmod = importlib.import_module('zuds-pipeline_amd.device')
    chain = dmod.DeviceSubtraction(sci.wcs, ref.wcs, device=0, engine=engine)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to('cuda:0')      # noqa: E731
    args = (t(f['img'], np.float32), t(sci.rms_image.data, np.float32), t(f['mask'], np.int32),
            t(sci.weight_image.data, np.float32), t(ref.data, np.float32), t(ref.rms_image.data, np.float32),
            t(ref.mask_image.data, np.int32))
    torch.cuda.synchronize()
    diff, noise, submask = chain.run(*args, seeing=2.0, nreg_side=1, hotpants_kws={'ko': 0, 'bgo': 0},
                                     ref_flxscale=float(ref.header.get('FLXSCALE', 1.0)))
    tab, nfound, segm = chain.extract(columns='param', mask='correct', deblend=True)
    ptab, _, _ = chain.extract(columns='param', deblend=True)
    cand, ncand = chain.candidates(2.0, columns='param', mask='correct', deblend=True)
    chain.stream.synchronize()
    engine.set_stream(0)
    m = submask.cpu().numpy()
    htab, hsegm = engine.extract(diff.cpu().numpy(), noise.cpu().numpy(), bad=(m & z.BAD_SUM) != 0, flag=m, wcs=sci.wcs,
                                 columns='param', mask='correct', deblend=True)
    assert nfound == len(htab) > 0 and tab.dtype == htab.dtype and tab.tobytes() == htab.tobytes()
    assert np.array_equal(segm.cpu().numpy(), hsegm)
    assert set(MASK_NAMES) <= set(tab.dtype.names) and not set(MASK_NAMES) & set(ptab.dtype.names)
    assert len(ptab) == len(tab) and (tab['NREPL_AUTO'] + tab['NLOST_AUTO']).any()
    assert ncand == nfound and set(MASK_NAMES) <= set(cand.dtype.names) and 'GOODCUT' in cand.dtype.names
    with pytest.raises(ValueError, match="needs columns='param'"):
        chain.extract(mask='correct')


def test_dosub_detect_param_columns_mask_type_writes_the_card(blended_subtraction, engine, monkeypatch, capsys):
    from test_catalog_gpu import load_script
    sc = blended_subtraction
    z, d = sc['z'], sc['d']
    script = load_script('dosub')
    monkeypatch.setattr(script, 'MAX_DETS', 10 ** 6)
    jobs = os.path.join(d, 'images.txt')
    with open(jobs, 'w') as f:
        f.write(sc['ims'][3].local_path + '\n')
    assert script.main([jobs, sc['refname'], '--detect', '--mask-type', 'correct']) == 2      # needs --param-columns
    capsys.readouterr()
    assert script.main([jobs, sc['refname'], '--detect', '--param-columns', '--mask-type', 'correct', '--deblend']) == 0
    out = capsys.readouterr().out
    assert 'cat: ' in out and 'Traceback' not in out
    cat = z.PipelineFITSCatalog.from_file(z.sub_name(sc['ims'][3].local_path, sc['refname']).replace('.fits', '.cat'))
    th = cat.table_header
    assert th['ZMMASKTY'] == 'CORRECT' and cat.mask == 'correct' and th['ZMDEBLND'] is True
    assert set(MASK_NAMES) <= set(cat.data.dtype.names) and 'GOODCUT' in cat.data.dtype.names
    assert 'PARENT_NUMBER' in cat.data.dtype.names and len(cat.data) > 0
