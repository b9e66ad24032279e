"""Host side of the wide table (columns='param'): column lists, FITS_LDAC, struct layouts, the region file, the keys of
sextractor_kws."""
import ctypes as C
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from util import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISOPHOTAL = ['NUMBER', 'X_IMAGE', 'Y_IMAGE', 'X_WORLD', 'Y_WORLD', 'XMIN_IMAGE', 'XMAX_IMAGE', 'YMIN_IMAGE', 'YMAX_IMAGE',
             'ISOAREA_IMAGE', 'A_IMAGE', 'B_IMAGE', 'THETA_IMAGE', 'ELONGATION', 'FWHM_IMAGE', 'FLUX_ISO', 'FLUX_MAX',
             'FLUX_APER', 'FLUXERR_APER', 'FLAGS', 'FLAGS_WEIGHT', 'IMAFLAGS_ISO']


def ex():
    pkg()
    return importlib.import_module('zuds-pipeline_amd.extract')


def wide_table(n=6, goodcut=False):
    rng = np.random.default_rng(9)
    dt = ex().PARAM_DTYPE.descr + ([('GOODCUT', 'u1')] if goodcut else [])
    tab = np.zeros(n, dtype=dt)
    for name in tab.dtype.names:
        tab[name] = rng.integers(0, 1 << 12, n) if tab.dtype[name].kind in 'iu' else rng.normal(0, 1e3, n)
    tab['NUMBER'] = np.arange(1, n + 1)
    tab['XWIN_WORLD'], tab['YWIN_WORLD'] = rng.uniform(0, 360, n), rng.uniform(-90, 90, n)
    if goodcut:
        tab['GOODCUT'] = np.arange(n) % 2
    return tab


def test_column_lists():
    e = ex()
    names = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'sextractor_param_names.json')))
    assert len(names) == 32 and 'MAG_AUTO' in names and 'YWIN_WORLD' in names
    wide = [c for c, _, _ in e.PARAM_COLUMNS]
    assert not set(names) - set(wide), set(names) - set(wide)
    assert {'KRON_RADIUS', 'FLAGS_AUTO', 'FLAGS_WIN'} <= set(wide) and len(set(wide)) == len(wide)
    assert [c for c, _, _ in e.CATALOG_COLUMNS] == ISOPHOTAL == wide[:len(ISOPHOTAL)]
    assert e.TABLE_DTYPE.names == tuple(ISOPHOTAL) and e.PARAM_DTYPE.names == tuple(wide)
    z = pkg()
    f0, f1 = ({f for f, _ in c._fields_} for c in (z._lib.zm_object, z._lib.zm_object_ext))
    assert all(f in f0 for _, f, _ in e.CATALOG_COLUMNS) and all(f in f1 for _, f, _ in e.EXT_COLUMNS)
    with pytest.raises(ValueError):
        e._split_params('everything', {})


def test_wide_table_round_trips_through_fits_ldac(tmp_path):
    z = pkg()
    tab = wide_table()
    tab['ERRA_WORLD'][:2] = np.nan
    cat = z.PipelineFITSCatalog()
    cat.basename = 'sub.w.cat'
    cat.data = tab
    cat.header = {'SEEING': 2.0}
    cat.map_to_local_file(str(tmp_path / cat.basename))
    cat.save()
    back = z.PipelineFITSCatalog.from_file(cat.local_path)
    assert back.data.dtype.names == tab.dtype.names
    for name in tab.dtype.names:
        assert back.data[name].dtype == tab[name].dtype and np.array_equal(back.data[name], tab[name], equal_nan=True)
    assert back.table_header['ZMMASKTY'] == 'NONE' and back.table_header['ZMDEBLND'] is False
    # the isophotal table's file says nothing about a mask type
    narrow = z.PipelineFITSCatalog()
    narrow.basename = 'sub.n.cat'
    narrow.data = np.zeros(2, dtype=ex().TABLE_DTYPE)
    narrow.map_to_local_file(str(tmp_path / narrow.basename))
    narrow.save()
    assert 'ZMMASKTY' not in z.PipelineFITSCatalog.from_file(narrow.local_path).table_header


def test_new_struct_layouts_match_the_header(tmp_path):
    z = pkg()
    structs = {'zm_measure_params': z._lib.zm_measure_params, 'zm_object_ext': z._lib.zm_object_ext}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zudsmi.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append(f'  printf("{name} . %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines) + '\n')
    exe = tmp_path / 'probe'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        name, field, value = line.split()
        cls = structs[name]
        want = C.sizeof(cls) if field == '.' else getattr(cls, field).offset
        assert int(value) == want, (name, field, int(value), want)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in structs.values())
    p = z._lib.zm_measure_params()
    z._lib.lib().zm_measure_params_default(C.byref(p))
    assert (p.kron_fact, p.kron_min_radius, p.filter) == (2.5, 3.5, 1)


@pytest.mark.parametrize('goodcut', [False, True])
def test_region_file_is_the_references_text(tmp_path, goodcut):
    z = pkg()
    cat = z.PipelineFITSCatalog()
    cat.basename = 'sub.r.cat'
    cat.data = wide_table(5, goodcut)
    cat.field = 762
    cat.map_to_local_file(str(tmp_path / cat.basename))
    reg = z.PipelineRegionFile.from_catalog(cat)
    assert reg.basename == 'sub.r.reg' and reg.local_path == str(tmp_path / 'sub.r.reg') and reg.field == 762
    assert reg.catalog is cat and cat.regionfile is reg
    # the reference's loop (zuds/catalog.py:52-64), restated
    want = ('global color=green dashlist=8 3 width=1 font="helvetica 10 normal" select=1 highlite=1 dash=0 fixed=0 '
            'edit=1 move=1 delete=1 include=1 source=1\n' + 'icrs\n')
    for r in cat.data:
        color = ('green' if r['GOODCUT'] else 'red') if goodcut else 'blue'
        want += f'point({r["XWIN_WORLD"]},{r["YWIN_WORLD"]}) # color={color}\n'
    assert open(reg.local_path, 'rb').read() == want.encode()


def test_region_file_needs_the_windowed_world_columns(tmp_path):
    z = pkg()
    cat = z.PipelineFITSCatalog()
    cat.basename = 'sub.i.cat'
    cat.data = np.zeros(3, dtype=ex().TABLE_DTYPE)
    cat.map_to_local_file(str(tmp_path / cat.basename))
    with pytest.raises(ValueError, match='XWIN_WORLD'):
        z.PipelineRegionFile.from_catalog(cat)


def test_phot_autoparams_only_with_the_wide_table():
    sx = importlib.import_module('zuds-pipeline_amd.sextractor')
    with pytest.raises(ValueError):
        sx.extraction_settings({'PHOT_AUTOPARAMS': [2.5, 3.5]}, None)          # the default path: as before
    rest, second = sx.measurement_settings({'PHOT_AUTOPARAMS': [2.0, 4.0], 'DETECT_THRESH': 2.0})
    assert rest == {'DETECT_THRESH': 2.0} and second == dict(kron_fact=2.0, kron_min_radius=4.0)
    assert sx.measurement_settings({'phot_autoparams': '2.5,3.5'})[1] == dict(kron_fact=2.5, kron_min_radius=3.5)
    assert sx.measurement_settings(None) == ({}, {})
    for bad in ([2.5], [2.5, 3.5, 1.0], [2.5, -1.0]):
        with pytest.raises(ValueError):
            sx.measurement_settings({'PHOT_AUTOPARAMS': bad})


def test_cuts_and_detections_read_a_wide_table_unchanged():
    z = pkg()
    fo = importlib.import_module('zuds-pipeline_amd.filterobjects')
    n = 4
    wide, narrow = np.zeros(n, dtype=ex().PARAM_DTYPE), np.zeros(n, dtype=ex().TABLE_DTYPE)
    for t in (wide, narrow):
        t['A_IMAGE'], t['B_IMAGE'], t['FWHM_IMAGE'] = [1.2, 2.1, 1.2, 1.2], 1.0, 2.2
        t['FLUX_APER'], t['FLUXERR_APER'] = 100.0, [10.0, 10.0, 25.0, 10.0]
    a = fo.column_cuts(wide, 2.0, np.zeros(n), np.ones(n), 1.1)
    b = fo.column_cuts(narrow, 2.0, np.zeros(n), np.ones(n), 1.1)
    assert list(a[0]) == list(b[0]) == [1, 0, 0, 1] and a[1] == b[1]
    cat = z.PipelineFITSCatalog()
    cat.data = wide
    cat.image = object()
    assert len(z.Detection.from_catalog(cat, filter=False)) == n


MASK_RULE = "mask='correct' needs columns='param': masking belongs to the second pass"
BAD_OPTIONS = [        # (keywords, message of extract_options and SubtractionJob, message of sextractor._extract)
    (dict(mask='correct'), MASK_RULE, MASK_RULE),
    (dict(columns='wide'), "columns='wide': one of ('isophotal', 'param')", "columns='wide': 'isophotal' or 'param'"),
    (dict(deblend=dict(nthresh=3)), 'deblend: nthresh=3 must be a power of two in 2 .. 64', None),
    (dict(deblend=dict(mincont=2)), 'deblend: mincont=2.0 must lie in [0, 1]', None),
    (dict(clean=dict(param=0)), 'clean: param=0.0 must be finite and lie in [0.1, 10]', None),
    (dict(deblend=dict(levels=8)), "deblend: unknown keys ['levels'] (nthresh, mincont)", None),
]


class _Image:
    header, header_comments, ismapped, basename = {}, {}, False, 'x.fits'


@pytest.mark.parametrize('kw,message,object_layer', BAD_OPTIONS, ids=[repr(kw) for kw, _, _ in BAD_OPTIONS])
def test_bad_options_raise_the_same_text_from_every_door(kw, message, object_layer):
    """One bad option at a time through ``extract_options`` (and ``_split_params``, which the engine's calls go through),
    the object layer (``sextractor._extract`` and, for the settings it takes, ``extraction_settings``) and
    ``SubtractionJob(detect=True)``: the whole text of the ValueError, as it has read since each option arrived."""
    e = ex()
    sx = importlib.import_module('zuds-pipeline_amd.sextractor')
    nightly = importlib.import_module('zuds-pipeline_amd.nightly')
    call = dict(catalog_type='FITS_LDAC', weight=np.ones((4, 4)))
    doors = [(lambda: e.extract_options(**kw), message),
             (lambda: sx._extract(_Image(), call, np.zeros((4, 4), np.float32), None, **kw), object_layer or message),
             (lambda: nightly.SubtractionJob({}, {}, detect=True, **kw), message)]
    if 'deblend' in kw or 'clean' in kw:
        doors.append((lambda: sx.extraction_settings(None, None, **kw), message))
    else:
        doors.append((lambda: e._split_params(kw.get('columns', 'isophotal'), {}, kw.get('mask')), message))
    for door, text in doors:
        with pytest.raises(ValueError) as err:
            door()
        assert str(err.value) == text
