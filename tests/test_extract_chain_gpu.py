"""The host chain around the extraction kernels, through both doors: ``Engine.extract`` (host planes) and
``Engine.extract_dev`` (device planes, the caller's ``segm``) in all 12 combinations of ``deblend`` off / on, ``clean`` off /
on and the three tables ('isophotal'; 'param'; 'param' with ``mask='correct'``), on one scene, ``halo_pair`` of
tests/clean_scenes.py (160 x 160): deblending splits its pair of stars, CLEAN folds the bumps on the galaxy's halo.

The kernels are pinned to the restatements elsewhere (tests/test_extract_gpu.py, test_deblend_gpu.py, test_clean_gpu.py,
test_measure_gpu.py, test_mask_gpu.py); what is held here is what the host code between them decides: which entry point
runs, which columns the table carries and in which order, that the second pass sees the final map, and that the two doors
agree byte for byte.

The first pass's columns inside a wide table are those of the narrow table of the same (deblend, clean), byte for byte.
A masked second pass replaces FLUX_APER / FLUXERR_APER and may set FLAGS bit 1 (value 1: the first pass sets 2, 4, 8
and 16 only), so there these two columns are left out and FLAGS is compared with bit 1 cleared."""
import importlib
import itertools

import numpy as np
import pytest

import clean_scenes as cs

pytestmark = pytest.mark.gpu

SCENE, NX, NY = 'halo_pair', 160, 160
DEBLEND = dict(nthresh=32, mincont=0.005)
TABLES = (('isophotal', None), ('param', None), ('param', 'correct'))
COMBOS = list(itertools.product((False, True), (False, True), TABLES))
ISOPHOTAL = ['NUMBER', 'X_IMAGE', 'Y_IMAGE', 'X_WORLD', 'Y_WORLD', 'XMIN_IMAGE', 'XMAX_IMAGE', 'YMIN_IMAGE', 'YMAX_IMAGE',
             'ISOAREA_IMAGE', 'A_IMAGE', 'B_IMAGE', 'THETA_IMAGE', 'ELONGATION', 'FWHM_IMAGE', 'FLUX_ISO', 'FLUX_MAX',
             'FLUX_APER', 'FLUXERR_APER', 'FLAGS', 'FLAGS_WEIGHT', 'IMAFLAGS_ISO']
SECOND = ['MAG_AUTO', 'MAGERR_AUTO', 'FLUX_AUTO', 'FLUXERR_AUTO', 'XWIN_IMAGE', 'YWIN_IMAGE', 'XWIN_WORLD', 'YWIN_WORLD',
          'AWIN_IMAGE', 'BWIN_IMAGE', 'ERRAWIN_IMAGE', 'ERRBWIN_IMAGE', 'ERRTHETAWIN_IMAGE', 'ERRA_WORLD', 'ERRB_WORLD',
          'ERRTHETA_WORLD', 'KRON_RADIUS', 'FLAGS_AUTO', 'FLAGS_WIN']
MASKED = ['NREPL_AUTO', 'NLOST_AUTO', 'NREPL_APER', 'NLOST_APER', 'NREPL_WIN', 'NLOST_WIN']


def names(deblend, clean, columns, mask):
    return tuple(ISOPHOTAL + (SECOND if columns == 'param' else []) + (MASKED if mask else [])
                 + (['PARENT_NUMBER'] if deblend else []) + (['NMERGED'] if clean else []))


class Doors:
    """Both doors on the scene's planes; the device plane that takes the map is poisoned before every call."""

    def __init__(self, engine):
        hipmem = importlib.import_module('zuds-pipeline_amd.hipmem')
        self.engine = engine
        self.img, self.sigma, kw = cs.scene(SCENE)
        assert not kw and self.img.shape == (NY, NX)
        self.dev = []
        for arr in (self.img, self.sigma):
            d = hipmem.DeviceBuffer(arr.nbytes)
            d.upload(np.ascontiguousarray(arr))
            self.dev.append(d)
        self.dseg = hipmem.DeviceBuffer(NX * NY * 4)

    def __call__(self, deblend, clean, columns, mask, **more):
        kw = dict(deblend=DEBLEND if deblend else False, clean=clean, columns=columns, mask=mask, **more)
        host = self.engine.extract(self.img, self.sigma, full=True, **kw)
        self.dseg.upload(np.full((NY, NX), -7, np.int32))
        dtab, dfound = self.engine.extract_dev(self.dev[0].ptr, self.dev[1].ptr, None, None, NX, NY, segm=self.dseg.ptr, **kw)
        return host, dtab, dfound, self.dseg.download(np.int32, (NY, NX))


@pytest.fixture(scope='module')
def doors(engine):
    return Doors(engine)


@pytest.fixture(scope='module')
def runs(doors):
    return {(db, cl, cols, mask): doors(db, cl, cols, mask) for db, cl, (cols, mask) in COMBOS}


def test_the_scene_splits_and_absorbs(runs):
    plain, split = runs[False, False, 'isophotal', None][0], runs[True, False, 'isophotal', None][0]
    merged, both = runs[False, True, 'isophotal', None][0], runs[True, True, 'isophotal', None][0]
    print(f'{SCENE}: {plain["nfound"]} objects, {split["nfound"]} deblended, {merged["nfound"]} cleaned, {both["nfound"]} both')
    assert split['nfound'] > plain['nfound'] and (split['table']['FLAGS'] & 2).any()
    assert merged['nfound'] < plain['nfound'] and merged['table']['NMERGED'].max() > 1
    assert both['nfound'] < split['nfound'] and both['table']['NMERGED'].max() > 1 and (both['table']['FLAGS'] & 2).any()
    assert len({r['nfound'] for r in (plain, split, merged, both)}) == 4
    assert len({r['segm'].tobytes() for r in (plain, split, merged, both)}) == 4


@pytest.mark.parametrize('deblend,clean,table', COMBOS)
def test_both_doors_every_combination(runs, deblend, clean, table):
    columns, mask = table
    host, dtab, dfound, dsegm = runs[deblend, clean, columns, mask]
    tab = host['table']
    assert host['status'] == 0 and host['nfound'] == dfound == len(tab) > 0
    assert tab.dtype.names == dtab.dtype.names == names(deblend, clean, columns, mask)
    assert tab.dtype == dtab.dtype and tab.tobytes() == dtab.tobytes()
    assert host['segm'].tobytes() == dsegm.tobytes()
    assert set(host) == {'table', 'segm', 'filtered', 'nfound', 'status'} | ({'ext'} if columns == 'param' else set()) \
        | ({'maskrows'} if mask else set())
    narrow = runs[deblend, clean, 'isophotal', None][0]
    assert host['segm'].tobytes() == narrow['segm'].tobytes() and host['nfound'] == narrow['nfound']
    assert host['filtered'].tobytes() == narrow['filtered'].tobytes()
    for c in narrow['table'].dtype.names:
        if mask and c in ('FLUX_APER', 'FLUXERR_APER'):
            continue
        if mask and c == 'FLAGS':
            assert np.array_equal(tab[c] & ~1, narrow['table'][c]) and not (narrow['table'][c] & 1).any()
            continue
        assert tab[c].tobytes() == narrow['table'][c].tobytes(), c
    if mask and not clean:                                # before CLEAN the halo's bumps lie inside the galaxy's footprints
        assert (tab['NREPL_AUTO'] + tab['NREPL_APER'] + tab['NREPL_WIN']).any()


def test_fewer_rows_than_objects_in_the_widest_call(runs, doors):
    """max_objects one below the number found, deblended, cleaned, wide and masked: the leading rows of the full table,
    the same map."""
    full = runs[True, True, 'param', 'correct'][0]
    n = full['nfound'] - 1
    assert n >= 1
    host, dtab, dfound, dsegm = doors(True, True, 'param', 'correct', max_objects=n)
    assert host['nfound'] == dfound == n + 1 and len(host['table']) == len(dtab) == n and host['status'] == 0
    assert host['table'].dtype == full['table'].dtype
    assert host['table'].tobytes() == dtab.tobytes() == full['table'][:n].tobytes()
    assert host['segm'].tobytes() == dsegm.tobytes() == full['segm'].tobytes()
