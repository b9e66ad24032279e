"""The CLEAN option in the host layers (no GPU): settings and refusals, the catalog's header cards on, off and after a
rewrite, the layout of zm_clean_params and ZM_EXTRACT_CLEAN against include/zudsmi.h as gcc sees it, and what
SubtractionJob refuses before any GPU work."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = dict(detect_thresh=1.5, detect_minarea=5, filter=True, satur_level=50000.0, aper_radius=3.0)


def test_clean_settings_and_the_library_defaults():
    z = pkg()
    ex = importlib.import_module('zuds-pipeline_amd.extract')
    assert ex.clean_settings(False) is None and ex.clean_settings(None) is None and ex.clean_params(False) is None
    assert ex.clean_settings(True) == dict(param=1.0) == ex.CLEAN_DEFAULTS
    for ok in (0.1, 0.5, 1, 2.0, 10.0):
        assert ex.clean_settings(dict(param=ok)) == dict(param=float(ok))
    for bad in (dict(param=0.09), dict(param=10.5), dict(param=0), dict(param=-1.0), dict(param=float('nan')),
                dict(param=float('inf')), dict(param='x'), dict(param=None), dict(beta=1.0)):
        with pytest.raises(ValueError):
            ex.clean_settings(bad)
        with pytest.raises(ValueError):
            ex.clean_params(bad)
    p = z._lib.zm_clean_params()
    z._lib.lib().zm_clean_params_default(C.byref(p))
    assert dict(param=p.param) == ex.CLEAN_DEFAULTS
    assert ex.clean_params(dict(param=2.5)).param == 2.5
    assert z._lib.EXTRACT_CLEAN == 4
    assert z.clean_settings is ex.clean_settings and z.clean_params is ex.clean_params


def test_extraction_settings_with_and_without_the_opt_in():
    sx = importlib.import_module('zuds-pipeline_amd.sextractor')
    assert sx.extraction_settings(None, None, clean=False) == DEFAULT        # unchanged, and no 'clean' key
    for kws in ({'CLEAN': 'Y'}, {'CLEAN_PARAM': 1.0}, {'clean': 'N'}):
        for more in ({}, dict(clean=False), dict(deblend=True)):
            with pytest.raises(ValueError):
                sx.extraction_settings(kws, None, **more)
    assert sx.extraction_settings(None, None, clean=True) == dict(DEFAULT, clean=dict(param=1.0))
    assert sx.extraction_settings({'CLEAN': 'Y', 'CLEAN_PARAM': 2.0, 'DETECT_MINAREA': 9}, None, clean=True) == \
        dict(DEFAULT, detect_minarea=9, clean=dict(param=2.0))
    assert sx.extraction_settings({'CLEAN_PARAM': '0.5'}, None, clean=dict(param=3.0))['clean'] == dict(param=0.5)
    both = sx.extraction_settings({'DEBLEND_NTHRESH': 16, 'CLEAN_PARAM': 1.5}, None, deblend=True, clean=True)
    assert both == dict(DEFAULT, deblend=dict(nthresh=16, mincont=0.005), clean=dict(param=1.5))
    for kws, cl in (({'CLEAN': 'N'}, True), ({'CLEAN_PARAM': 11.0}, True), ({'CLEAN_PARAM': 'much'}, True),
                    ({}, dict(param=0.01)), ({}, dict(exponent=1.0)), ({'MASK_TYPE': 'CORRECT'}, True),
                    ({'DEBLEND_NTHRESH': 32}, True), ({'CLEAN_TYPE': 1}, True)):
        with pytest.raises(ValueError):
            sx.extraction_settings(kws, None, clean=cl)


def test_header_cards_on_off_and_after_a_rewrite(tmp_path):
    z = pkg()
    cmod = importlib.import_module('zuds-pipeline_amd.catalog')
    ex = importlib.import_module('zuds-pipeline_amd.extract')
    off = [('ZMDEBLND', False, 'multi-threshold deblending (not in this version)'),
           ('ZMCLEAN', False, 'CLEAN pass (not in this version)')]
    assert cmod.header_cards() == off == cmod.header_cards(None, None) == cmod.header_cards(clean=None)
    db = dict(nthresh=16, mincont=0.01)
    assert cmod.header_cards(db) == cmod.header_cards(db, None)
    assert [c[:2] for c in cmod.header_cards(db)] == [('ZMDEBLND', True), ('ZMDBNTHR', 16), ('ZMDBMINC', 0.01), ('ZMCLEAN', False)]
    assert [c[:2] for c in cmod.header_cards(None, dict(param=2.0))] == [('ZMDEBLND', False), ('ZMCLEAN', True), ('ZMCLNPAR', 2.0)]
    assert [c[:2] for c in cmod.header_cards(db, dict(param=1.0))] == \
        [('ZMDEBLND', True), ('ZMDBNTHR', 16), ('ZMDBMINC', 0.01), ('ZMCLEAN', True), ('ZMCLNPAR', 1.0)]
    tab = ex.with_column(np.zeros(3, dtype=ex.TABLE_DTYPE).view(np.recarray), 'NMERGED', np.array([1, 4, 1], np.int32))
    assert tab.dtype.names == ex.TABLE_DTYPE.names + ('NMERGED',) and tab['NMERGED'].tolist() == [1, 4, 1]
    for cl in (None, dict(param=2.0)):
        cat = z.PipelineFITSCatalog()
        cat.basename = 'x.cat'
        cat.data, cat.header, cat.header_comments, cat.clean = tab, {'SEEING': 2.0}, {}, cl
        cat.map_to_local_file(str(tmp_path / ('on.cat' if cl else 'off.cat')))
        cat.save()
        back = z.PipelineFITSCatalog.from_file(cat.local_path)
        th = back.table_header
        assert th['ZMDEBLND'] is False and back.data['NMERGED'].tolist() == [1, 4, 1] and back.deblend is None
        if cl is None:
            assert th['ZMCLEAN'] is False and 'ZMCLNPAR' not in th and back.clean is None
        else:
            assert th['ZMCLEAN'] is True and th['ZMCLNPAR'] == 2.0 and back.clean == cl
            back.kill_flagged()                                              # a rewrite keeps the cards
            again = z.PipelineFITSCatalog.from_file(cat.local_path)
            assert again.table_header['ZMCLEAN'] is True and again.table_header['ZMCLNPAR'] == 2.0 and again.clean == cl


def test_clean_struct_layout_matches_the_header(tmp_path):
    z = pkg()
    structs = {'zm_clean_params': z._lib.zm_clean_params, 'zm_deblend_params': z._lib.zm_deblend_params,
               'zm_extract_params': z._lib.zm_extract_params, 'zm_object': z._lib.zm_object}
    head = ['#include <stdio.h>', '#include <stddef.h>', '#include "zudsmi.h"', 'int main(void) {']
    sizes = []
    for name, cls in structs.items():
        sizes.append(f'  printf("{name} . %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            sizes.append(f'  printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    for bit in ('ZM_EXTRACT_CHAIN', 'ZM_EXTRACT_DEBLEND', 'ZM_EXTRACT_CLEAN'):
        sizes.append(f'  printf("{bit} . %d\\n", {bit});')
    # the entry points are declared with the arguments the ctypes mirrors pass (compiled, not linked)
    decls = ['  int (*a)(zm_ctx*, const float*, const float*, const uint8_t*, const int32_t*, int, int, const zm_wcs*,',
             '           const zm_extract_params*, int, zm_object*, int32_t*, float*, int*, int*, int*, const zm_deblend_params*,',
             '           const zm_clean_params*, int32_t*, int32_t*) = zm_extract_clean_dev;',
             '  a = zm_extract_clean;',
             '  int (*b)(zm_ctx*, int, const zm_object*, const double*, const float*, const float*, int, const zm_clean_params*,',
             '           int32_t*, int32_t*) = zm_clean_decide;',
             '  void (*c)(zm_clean_params*) = zm_clean_params_default;',
             '  (void)a; (void)b; (void)c;']
    tail = ['  return 0;', '}']
    src = tmp_path / 'decls.c'
    src.write_text('\n'.join(head + decls + tail) + '\n')
    subprocess.check_call(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-c', str(src), '-o',
                           str(tmp_path / 'decls.o')])
    src = tmp_path / 'sizes.c'
    src.write_text('\n'.join(head + sizes + tail) + '\n')
    exe = tmp_path / 'sizes'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    bits = {'ZM_EXTRACT_CHAIN': z._lib.EXTRACT_CHAIN, 'ZM_EXTRACT_DEBLEND': z._lib.EXTRACT_DEBLEND,
            'ZM_EXTRACT_CLEAN': z._lib.EXTRACT_CLEAN}
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
    assert C.sizeof(z._lib.zm_clean_params) == 8 and C.sizeof(z._lib.zm_extract_params) == 24
    assert z._lib.EXTRACT_CLEAN == 4


def test_subtraction_job_refuses_before_any_gpu_work():
    nightly = importlib.import_module('zuds-pipeline_amd.nightly')
    with pytest.raises(ValueError, match='clean needs detect'):
        nightly.SubtractionJob({}, {}, clean=True)
    with pytest.raises(ValueError, match='clean needs detect'):
        nightly.SubtractionJob({}, {}, clean=dict(param=2.0), deblend=False)
    with pytest.raises(ValueError):
        nightly.SubtractionJob({}, {}, detect=True, clean=dict(param=0.01))
    with pytest.raises(ValueError):
        nightly.SubtractionJob({}, {}, detect=True, clean=dict(exponent=1.0))
    job = nightly.SubtractionJob({}, {}, detect=True, clean=True)
    assert job.clean == dict(param=1.0) and job.deblend is None
    job = nightly.SubtractionJob({}, {}, detect=True, clean=dict(param=2), deblend=True)
    assert job.clean == dict(param=2.0) and job.deblend == dict(nthresh=32, mincont=0.005)
    assert nightly.SubtractionJob({}, {}, detect=True).clean is None


def test_scripts_refuse_clean_without_detect(capsys):
    from test_catalog_gpu import load_script
    for name in ('dosub', 'donightly'):
        script = load_script(name)
        assert script.main(['images.txt', 'ref.fits', '--clean']) == 2
        assert '--clean needs --detect' in capsys.readouterr().err
    script = load_script('dosub')
    assert script.main(['images.txt', 'ref.fits', '--detect', '--clean-param', '2']) == 2
    assert '--clean-param needs --clean' in capsys.readouterr().err
    assert script.main(['images.txt', 'ref.fits', '--detect', '--clean', '--clean-param', '20']) == 2
    assert '--clean-param' in capsys.readouterr().err
