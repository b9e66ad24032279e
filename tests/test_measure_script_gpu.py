"""``scripts/dosub.py --detect --param-columns``: the wide catalog on disk and the region file behind the cuts."""
import os

import numpy as np
import pytest

from test_catalog_gpu import _scene, load_script  # noqa: F401  (the synthetic epoch and the drivers' job files)
from util import pkg, synth

pytestmark = pytest.mark.gpu


def test_dosub_param_columns_writes_the_wide_catalog_and_the_region_file(tmp_path, engine, monkeypatch, capsys):
    z, s = pkg(), synth()
    d = str(tmp_path)
    refims, _ = _scene(z, s, d, 640, 600, 3, 4300, '201912', fwhm=2.0)
    refname = os.path.join(d, 'ref.000651_c03_q1_zg.fits')
    z.ReferenceImage.from_images(refims, refname, sci_swarp_kws={'COMBINE_TYPE': 'WEIGHTED'})
    _, spaths = _scene(z, s, d, 640, 600, 1, 4400, '202003', fwhm=2.6)
    script = load_script('dosub')
    monkeypatch.setattr(script, 'MAX_DETS', 10 ** 6)
    assert script.main([os.path.join(d, 'none.txt'), refname, '--param-columns']) == 2          # needs --detect
    jobs = os.path.join(d, 'images.txt')
    with open(jobs, 'w') as f:
        f.write(spaths[0] + '\n')
    assert script.main([jobs, refname, '--detect', '--param-columns']) == 0
    assert 'Traceback' not in capsys.readouterr().out
    sub = z.sub_name(spaths[0], refname)
    cat = z.PipelineFITSCatalog.from_file(sub.replace('.fits', '.cat'))
    tab = cat.data
    ex = __import__('importlib').import_module('zuds-pipeline_amd.extract')
    assert set(ex.PARAM_DTYPE.names) <= set(tab.dtype.names) and 'GOODCUT' in tab.dtype.names
    assert cat.table_header['ZMMASKTY'] == 'NONE' and len(tab) > 0
    assert np.isfinite(tab['XWIN_WORLD']).all() and np.isfinite(tab['ERRA_WORLD']).all()
    # a window that fell back carries the isophotal position; no other one does
    fell = (tab['FLAGS_WIN'] & 1) != 0
    assert np.array_equal(tab['XWIN_IMAGE'][fell], tab['X_IMAGE'][fell]) and (tab['XWIN_IMAGE'][~fell] != tab['X_IMAGE'][~fell]).all()
    lines = open(sub.replace('.fits', '.reg')).read().splitlines()
    assert len(lines) == 2 + len(tab) and lines[1] == 'icrs'
    want = [f'point({r["XWIN_WORLD"]},{r["YWIN_WORLD"]}) # color={"green" if r["GOODCUT"] else "red"}' for r in tab]
    assert lines[2:] == want
