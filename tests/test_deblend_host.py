"""The deblending option in the host layers (no GPU): settings and refusals, the catalog's header cards, the layout of
zm_deblend_params against include/zudsmi.h as gcc sees it."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = dict(detect_thresh=1.5, detect_minarea=5, filter=True, satur_level=50000.0, aper_radius=3.0)


def test_extraction_settings_with_and_without_the_opt_in():
    sx = importlib.import_module('zuds-pipeline_amd.sextractor')
    assert sx.extraction_settings(None, None) == DEFAULT                     # unchanged, and no 'deblend' key
    assert sx.extraction_settings(None, None, deblend=False) == DEFAULT
    for kws in ({'DEBLEND_NTHRESH': 32}, {'DEBLEND_MINCONT': 0.005}, {'deblend_nthresh': 16}):
        with pytest.raises(ValueError):
            sx.extraction_settings(kws, None)
        with pytest.raises(ValueError):
            sx.extraction_settings(kws, None, deblend=False)
    assert sx.extraction_settings(None, None, deblend=True) == dict(DEFAULT, deblend=dict(nthresh=32, mincont=0.005))
    d = sx.extraction_settings({'DEBLEND_NTHRESH': 16, 'DEBLEND_MINCONT': 0.01, 'DETECT_MINAREA': 9}, None, deblend=True)
    assert d == dict(DEFAULT, detect_minarea=9, deblend=dict(nthresh=16, mincont=0.01))
    d = sx.extraction_settings({'DEBLEND_MINCONT': 0.02}, None, deblend=dict(nthresh=64, mincont=0.5))
    assert d['deblend'] == dict(nthresh=64, mincont=0.02)                    # the keys override the dict
    for kws, db in (({'DEBLEND_NTHRESH': 24}, True), ({'DEBLEND_MINCONT': 1.5}, True), ({}, dict(nthresh=24)),
                    ({}, dict(nthresh=128)), ({}, dict(nthresh=1)), ({}, dict(mincont=1.5)), ({}, dict(mincont=-0.1)),
                    ({}, dict(nlevels=32)), ({'CLEAN': 'Y'}, True), ({'CLEAN_PARAM': 1.0}, True),
                    ({'MASK_TYPE': 'CORRECT'}, True)):
        with pytest.raises(ValueError):
            sx.extraction_settings(kws, None, deblend=db)


def test_deblend_settings_and_the_library_defaults():
    z = pkg()
    ex = importlib.import_module('zuds-pipeline_amd.extract')
    assert ex.deblend_settings(False) is None and ex.deblend_settings(None) is None and ex.deblend_params(False) is None
    assert ex.deblend_settings(True) == dict(nthresh=32, mincont=0.005)
    for n in (2, 4, 8, 16, 32, 64):
        assert ex.deblend_settings(dict(nthresh=n))['nthresh'] == n
    for bad in (dict(nthresh=24), dict(nthresh=0), dict(nthresh=3), dict(nthresh=128), dict(nthresh=32.5), dict(mincont=1.5),
                dict(mincont=float('nan')), dict(mincont=-1e-9)):
        with pytest.raises(ValueError):
            ex.deblend_settings(bad)
    p = z._lib.zm_deblend_params()
    z._lib.lib().zm_deblend_params_default(C.byref(p))
    assert dict(nthresh=p.nthresh, mincont=p.mincont) == ex.DEBLEND_DEFAULTS
    q = ex.deblend_params(dict(nthresh=8, mincont=0.25))
    assert (q.nthresh, q.mincont) == (8, 0.25)
    assert z._lib.EXTRACT_DEBLEND == 2 and z._lib.EXTRACT_CHAIN == 1
    with pytest.raises(ValueError):                                          # SubtractionJob refuses before any GPU work
        importlib.import_module('zuds-pipeline_amd.nightly').SubtractionJob({}, {}, detect=True, deblend=dict(nthresh=24))
    with pytest.raises(ValueError):
        importlib.import_module('zuds-pipeline_amd.nightly').SubtractionJob({}, {}, deblend=True)


def test_header_cards(tmp_path):
    z = pkg()
    cmod = importlib.import_module('zuds-pipeline_amd.catalog')
    ex = importlib.import_module('zuds-pipeline_amd.extract')
    assert cmod.header_cards() == cmod.HEADER_CARDS and cmod.header_cards(None)[0][:2] == ('ZMDEBLND', False)
    cards = cmod.header_cards(dict(nthresh=16, mincont=0.01))
    assert [c[:2] for c in cards] == [('ZMDEBLND', True), ('ZMDBNTHR', 16), ('ZMDBMINC', 0.01), ('ZMCLEAN', False)]
    tab = ex.with_parent(np.zeros(3, dtype=ex.TABLE_DTYPE).view(np.recarray), np.array([1, 1, 2], np.int32))
    assert tab.dtype.names == ex.TABLE_DTYPE.names + ('PARENT_NUMBER',) and tab['PARENT_NUMBER'].tolist() == [1, 1, 2]
    for db in (None, dict(nthresh=16, mincont=0.01)):
        cat = z.PipelineFITSCatalog()
        cat.basename = 'x.cat'
        cat.data, cat.header, cat.header_comments, cat.deblend = tab, {'SEEING': 2.0}, {}, db
        cat.map_to_local_file(str(tmp_path / ('on.cat' if db else 'off.cat')))
        cat.save()
        back = z.PipelineFITSCatalog.from_file(cat.local_path)
        th = back.table_header
        assert th['ZMCLEAN'] is False and back.data['PARENT_NUMBER'].tolist() == [1, 1, 2]
        if db is None:
            assert th['ZMDEBLND'] is False and 'ZMDBNTHR' not in th and 'ZMDBMINC' not in th and back.deblend is None
        else:
            assert th['ZMDEBLND'] is True and th['ZMDBNTHR'] == 16 and abs(th['ZMDBMINC'] - 0.01) < 1e-15
            assert back.deblend == db
            back.kill_flagged()                                              # a rewrite keeps the cards
            assert z.PipelineFITSCatalog.from_file(cat.local_path).table_header['ZMDEBLND'] is True


def test_deblend_struct_layout_matches_the_header(tmp_path):
    z = pkg()
    structs = {'zm_deblend_params': z._lib.zm_deblend_params, 'zm_extract_params': z._lib.zm_extract_params,
               'zm_object': z._lib.zm_object}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zudsmi.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append(f'  printf("{name} . %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines += ['  printf("ZM_EXTRACT_DEBLEND . %d\\n", ZM_EXTRACT_DEBLEND);', '  return 0;', '}']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines) + '\n')
    exe = tmp_path / 'probe'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        name, field, value = line.split()
        if name == 'ZM_EXTRACT_DEBLEND':
            assert int(value) == z._lib.EXTRACT_DEBLEND
            continue
        cls = structs[name]
        want = C.sizeof(cls) if field == '.' else getattr(cls, field).offset
        assert int(value) == want, (name, field, int(value), want)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in structs.values())
    assert C.sizeof(z._lib.zm_deblend_params) == 16 and C.sizeof(z._lib.zm_extract_params) == 24
