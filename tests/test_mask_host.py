"""The MASK_TYPE option in the host layers (no GPU): the ``mask`` / ``MASK_TYPE`` keyword rules with every refusal, the
table and the header made from synthetic zm_object_ext / zm_object_mask arrays, a FITS_LDAC round trip of the new columns
and of ZMMASKTY, the layout of the new structs against include/zudsmi.h as gcc sees it, and what SubtractionJob and the
driver refuse before any GPU work."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = dict(detect_thresh=1.5, detect_minarea=5, filter=True, satur_level=50000.0, aper_radius=3.0)


def ex():
    return importlib.import_module('zuds-pipeline_amd.extract')


def test_mask_setting_and_the_library_defaults():
    z, e = pkg(), ex()
    for off in (None, False, 'none', 'NONE', ' None '):
        assert e.mask_setting(off) is None and e.mask_params(off) is None
    for on, want in (('blank', 'blank'), ('BLANK', 'blank'), ('correct', 'correct'), (' Correct ', 'correct')):
        assert e.mask_setting(on) == want
    for bad in ('replace', '', True, 1, 2, dict(type='correct'), ['correct']):
        with pytest.raises(ValueError):
            e.mask_setting(bad)
        with pytest.raises(ValueError):
            e.mask_params(bad)
    p = z._lib.zm_mask_params()
    z._lib.lib().zm_mask_params_default(C.byref(p))
    assert (p.type, p.pad_, p.aper_radius) == (z._lib.MASK_CORRECT, 0, 3.0)
    assert (z._lib.MASK_BLANK, z._lib.MASK_CORRECT, z._lib.AUTO_CROWDED) == (1, 2, 8)
    q = e.mask_params('blank', 4.5)
    assert (q.type, q.aper_radius) == (z._lib.MASK_BLANK, 4.5) and e.mask_params('correct').aper_radius == 3.0
    assert z.mask_setting is e.mask_setting and z.mask_params is e.mask_params and z.MASK_COLUMNS is e.MASK_COLUMNS


def test_mask_needs_the_wide_table():
    e = ex()
    assert e._split_params('isophotal', {}, None) == ({}, None, None)
    assert e._split_params('isophotal', {}, 'none')[2] is None
    for typ in ('blank', 'correct', 'CORRECT'):
        with pytest.raises(ValueError, match="needs columns='param'"):
            e._split_params('isophotal', {}, typ)
    with pytest.raises(ValueError):
        e._split_params('param', {}, 'mirror')
    params, mp, mk = e._split_params('param', dict(aper_radius=4.0, kron_fact=2.0, detect_thresh=2.0), 'correct')
    assert params == dict(aper_radius=4.0, detect_thresh=2.0) and mp.kron_fact == 2.0
    assert (mk.type, mk.aper_radius) == (2, 4.0)                      # the first pass's radius
    params, mp, mk = e._split_params('param', {}, None)
    assert mp is not None and mk is None                             # the plain second pass is what it was


def test_extraction_settings_with_and_without_the_opt_in():
    sx = importlib.import_module('zuds-pipeline_amd.sextractor')
    assert sx.extraction_settings(None, None) == DEFAULT == sx.extraction_settings(None, None, mask=None)
    assert sx.extraction_settings(None, None, mask='none') == DEFAULT           # not asked for: no 'mask' key
    # without mask=, MASK_TYPE keeps raising, whatever it says and whatever else is on
    for v in ('NONE', 'BLANK', 'CORRECT'):
        for more in ({}, dict(mask=None), dict(mask='none'), dict(deblend=True), dict(clean=True)):
            with pytest.raises(ValueError, match='MASK_TYPE'):
                sx.extraction_settings({'MASK_TYPE': v}, None, **more)
    assert sx.extraction_settings(None, None, mask='correct') == dict(DEFAULT, mask='correct')
    assert sx.extraction_settings({}, None, mask='BLANK') == dict(DEFAULT, mask='blank')
    # MASK_TYPE overrides the keyword; NONE means the plain second pass
    assert sx.extraction_settings({'MASK_TYPE': 'BLANK'}, None, mask='correct')['mask'] == 'blank'
    assert sx.extraction_settings({'mask_type': 'correct'}, None, mask='blank')['mask'] == 'correct'
    assert sx.extraction_settings({'MASK_TYPE': 'NONE', 'DETECT_MINAREA': 7}, None, mask='correct') == \
        dict(DEFAULT, detect_minarea=7, mask=None)
    for v in ('REPLACE', '', 1, None):
        with pytest.raises(ValueError, match='MASK_TYPE'):
            sx.extraction_settings({'MASK_TYPE': v}, None, mask='correct')
    with pytest.raises(ValueError):
        sx.extraction_settings({}, None, mask='mirror')
    with pytest.raises(ValueError):
        sx.extraction_settings({'FILTER_NAME': 'gauss.conv'}, None, mask='correct')
    both = sx.extraction_settings({'DEBLEND_NTHRESH': 16, 'CLEAN_PARAM': 1.5, 'MASK_TYPE': 'CORRECT'}, None, deblend=True,
                                  clean=True, mask='blank')
    assert both == dict(DEFAULT, deblend=dict(nthresh=16, mincont=0.005), clean=dict(param=1.5), mask='correct')


class _Image:
    header, header_comments, ismapped, basename = {}, {}, False, 'x.fits'


def test_the_object_layer_refuses_a_mask_without_the_wide_table():
    sx = importlib.import_module('zuds-pipeline_amd.sextractor')
    call = dict(catalog_type='FITS_LDAC', weight=np.ones((4, 4)))
    for cols in ('isophotal',):
        for typ in ('blank', 'correct'):
            with pytest.raises(ValueError, match="needs columns='param'"):
                sx._extract(_Image(), call, np.zeros((4, 4), np.float32), None, columns=cols, mask=typ)
    with pytest.raises(ValueError, match='MASK_TYPE'):                  # and MASK_TYPE alone stays refused
        sx._extract(_Image(), call, np.zeros((4, 4), np.float32), {'MASK_TYPE': 'CORRECT'}, columns='param')
    with pytest.raises(ValueError):
        sx._extract(_Image(), call, np.zeros((4, 4), np.float32), None, columns='param', mask='mirror')


def synthetic(n=4):
    z = pkg()
    rows = (z._lib.zm_object * n)()
    ext = (z._lib.zm_object_ext * n)()
    msk = (z._lib.zm_object_mask * n)()
    for k in range(n):
        rows[k].number = ext[k].number = msk[k].number = k + 1
        rows[k].x_image, rows[k].y_image = 10.5 + k, 20.25 + k
        rows[k].flux_aper, rows[k].fluxerr_aper = 1000.0 + k, 10.0 + k
        rows[k].flags = (0, 2, 16, 3)[k % 4]
        ext[k].flux_auto, ext[k].kron_radius, ext[k].flags_auto = 1200.0 + k, 3.5, 8 if k % 2 else 0
        ext[k].xwin_image = 10.75 + k
        msk[k].nrepl_auto, msk[k].nlost_auto, msk[k].nap = 3 * k, k, 45
        msk[k].nrepl_aper, msk[k].nlost_aper, msk[k].nrepl_win, msk[k].nlost_win = k, 2 * k, 5 * k, 7 * k
        msk[k].crowded = k % 2
        msk[k].flux_aper, msk[k].fluxerr_aper = 900.0 + k, 9.0 + k
    return rows, ext, msk


def test_the_table_from_synthetic_rows():
    e = ex()
    rows, ext, msk = synthetic()
    wide, _ = e.ext_to_table(rows, ext, 4)
    tab, rext, rmsk = e.masked_table(rows, ext, msk, 4)
    assert tab.dtype.names == e.PARAM_DTYPE.names + tuple(c for c, _, _ in e.MASK_COLUMNS)
    assert [c for c, _, _ in e.MASK_COLUMNS] == ['NREPL_AUTO', 'NLOST_AUTO', 'NREPL_APER', 'NLOST_APER', 'NREPL_WIN', 'NLOST_WIN']
    assert tab['FLUX_APER'].tolist() == [900.0, 901.0, 902.0, 903.0] and tab['FLUXERR_APER'].tolist() == [9.0, 10.0, 11.0, 12.0]
    assert wide['FLUX_APER'].tolist() == [1000.0, 1001.0, 1002.0, 1003.0]            # the plain table is what it was
    assert wide['FLAGS'].tolist() == [0, 2, 16, 3] and tab['FLAGS'].tolist() == [0, 3, 16, 3]   # bit 1 where crowded
    assert tab['FLAGS_AUTO'].tolist() == [0, 8, 0, 8] and tab['NREPL_AUTO'].tolist() == [0, 3, 6, 9]
    assert tab['NLOST_AUTO'].tolist() == [0, 1, 2, 3] and tab['NREPL_APER'].tolist() == [0, 1, 2, 3]
    assert tab['NLOST_APER'].tolist() == [0, 2, 4, 6] and tab['NREPL_WIN'].tolist() == [0, 5, 10, 15]
    assert tab['NLOST_WIN'].tolist() == [0, 7, 14, 21]
    for c in e.PARAM_DTYPE.names:
        if c not in ('FLUX_APER', 'FLUXERR_APER', 'FLAGS'):
            assert np.array_equal(tab[c], wide[c], equal_nan=True), c
    assert rmsk['nap'].tolist() == [45] * 4 and rext['flux_auto'].tolist() == [1200.0, 1201.0, 1202.0, 1203.0]
    empty, _, m0 = e.masked_table(rows, ext, msk, 0)
    assert len(empty) == 0 and len(m0) == 0 and empty.dtype == tab.dtype
    # the other opt-in columns go behind the mask's
    both = e.with_column(e.with_parent(tab, np.arange(4, dtype=np.int32)), 'NMERGED', np.ones(4, np.int32))
    assert both.dtype.names[-3:] == ('NLOST_WIN', 'PARENT_NUMBER', 'NMERGED')


def test_header_cards_and_a_fits_ldac_round_trip(tmp_path):
    z, e = pkg(), ex()
    cmod = importlib.import_module('zuds-pipeline_amd.catalog')
    none = [('ZMMASKTY', 'NONE', 'MASK_TYPE of the Kron and windowed sums')]
    assert cmod.wide_cards() == cmod.wide_cards(None) == none == cmod.WIDE_CARDS
    assert [c[:2] for c in cmod.wide_cards('blank')] == [('ZMMASKTY', 'BLANK')]
    assert [c[:2] for c in cmod.wide_cards('correct')] == [('ZMMASKTY', 'CORRECT')]
    rows, ext, msk = synthetic()
    tab, _, _ = e.masked_table(rows, ext, msk, 4)
    plain, _ = e.ext_to_table(rows, ext, 4)
    for typ, data in ((None, plain), ('blank', tab), ('correct', tab)):
        cat = z.PipelineFITSCatalog()
        cat.basename = 'x.cat'
        cat.data, cat.header, cat.header_comments, cat.mask = data, {'SEEING': 2.0}, {}, typ
        cat.map_to_local_file(str(tmp_path / f'{typ}.cat'))
        cat.save()
        back = z.PipelineFITSCatalog.from_file(cat.local_path)
        assert back.table_header['ZMMASKTY'] == (typ or 'none').upper() and back.mask == typ
        assert back.data.dtype.names == data.dtype.names
        for c in data.dtype.names:
            assert np.array_equal(np.asarray(back.data[c]), data[c], equal_nan=True), c
        if typ:
            assert back.data['NLOST_WIN'].tolist() == [0, 7, 14, 21] and back.data['FLAGS'].tolist() == [0, 3, 16, 3]
            back.kill_flagged()                                          # a rewrite keeps the card and the columns
            again = z.PipelineFITSCatalog.from_file(cat.local_path)
            assert again.table_header['ZMMASKTY'] == typ.upper() and again.mask == typ and 'NREPL_APER' in again.data.dtype.names
    # an isophotal catalog has no such card, with or without the attribute
    iso = z.PipelineFITSCatalog()
    iso.basename = 'i.cat'
    iso.data, iso.header, iso.header_comments = np.zeros(2, dtype=e.TABLE_DTYPE).view(np.recarray), {}, {}
    iso.map_to_local_file(str(tmp_path / 'i.cat'))
    iso.save()
    back = z.PipelineFITSCatalog.from_file(iso.local_path)
    assert 'ZMMASKTY' not in back.table_header and back.mask is None


def test_mask_struct_layout_matches_the_header(tmp_path):
    z = pkg()
    structs = {'zm_mask_params': z._lib.zm_mask_params, 'zm_object_mask': z._lib.zm_object_mask,
               'zm_object_ext': z._lib.zm_object_ext, 'zm_measure_params': z._lib.zm_measure_params}
    head = ['#include <stdio.h>', '#include <stddef.h>', '#include "zudsmi.h"', 'int main(void) {']
    sizes = []
    for name, cls in structs.items():
        sizes.append(f'  printf("{name} . %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            sizes.append(f'  printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    for bit in ('ZM_MASK_BLANK', 'ZM_MASK_CORRECT', 'ZM_AUTO_CROWDED', 'ZM_AUTO_SKIPPED'):
        sizes.append(f'  printf("{bit} . %d\\n", {bit});')
    decls = ['  int (*a)(zm_ctx*, const float*, const float*, const uint8_t*, const int32_t*, int, int, const zm_wcs*,',
             '           const zm_measure_params*, int, const zm_object*, zm_object_ext*, const zm_mask_params*,',
             '           zm_object_mask*) = zm_extract_measure_masked_dev;',
             '  a = zm_extract_measure_masked;',
             '  void (*b)(zm_mask_params*) = zm_mask_params_default;',
             '  (void)a; (void)b;']
    tail = ['  return 0;', '}']
    src = tmp_path / 'decls.c'
    src.write_text('\n'.join(head + decls + tail) + '\n')
    subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o',
                           str(tmp_path / 'decls.o')])
    src = tmp_path / 'sizes.c'
    src.write_text('\n'.join(head + sizes + tail) + '\n')
    exe = tmp_path / 'sizes'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    bits = {'ZM_MASK_BLANK': 1, 'ZM_MASK_CORRECT': 2, 'ZM_AUTO_CROWDED': 8, 'ZM_AUTO_SKIPPED': 1}
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        name, field, value = line.split()
        if name in bits:
            assert int(value) == bits.pop(name)
            continue
        cls = structs[name]
        want = C.sizeof(cls) if field == '.' else getattr(cls, field).offset
        assert int(value) == want, (name, field, int(value), want)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in structs.values()) and not bits
    assert C.sizeof(z._lib.zm_mask_params) == 16 and C.sizeof(z._lib.zm_object_mask) == 56


def test_subtraction_job_refuses_before_any_gpu_work():
    nightly = importlib.import_module('zuds-pipeline_amd.nightly')
    with pytest.raises(ValueError, match='mask needs detect'):
        nightly.SubtractionJob({}, {}, mask='correct')
    with pytest.raises(ValueError, match='columns needs detect'):
        nightly.SubtractionJob({}, {}, columns='param')
    with pytest.raises(ValueError, match="needs columns='param'"):
        nightly.SubtractionJob({}, {}, detect=True, mask='correct')
    with pytest.raises(ValueError):
        nightly.SubtractionJob({}, {}, detect=True, columns='param', mask='mirror')
    with pytest.raises(ValueError):
        nightly.SubtractionJob({}, {}, detect=True, columns='wide')
    job = nightly.SubtractionJob({}, {}, detect=True, columns='param', mask='BLANK', deblend=True)
    assert (job.columns, job.mask) == ('param', 'blank') and job.deblend == dict(nthresh=32, mincont=0.005)
    job = nightly.SubtractionJob({}, {}, detect=True)
    assert (job.columns, job.mask) == ('isophotal', None)


def test_the_driver_refuses_a_mask_type_without_the_wide_table(capsys):
    from test_catalog_gpu import load_script
    script = load_script('dosub')
    assert script.main(['images.txt', 'ref.fits', '--detect', '--mask-type', 'correct']) == 2
    assert '--mask-type needs --param-columns' in capsys.readouterr().err
    assert script.main(['images.txt', 'ref.fits', '--mask-type', 'blank']) == 2
    assert '--mask-type needs --param-columns' in capsys.readouterr().err
    assert script.main(['images.txt', 'ref.fits', '--detect', '--param-columns', '--mask-type', 'mirror']) == 2
    assert 'neither blank nor correct' in capsys.readouterr().err
    assert script.main(['images.txt', 'ref.fits', '--detect', '--param-columns', '--mask-type']) == 2
    assert '--mask-type needs a value' in capsys.readouterr().err
