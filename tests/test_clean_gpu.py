"""zm_extract_clean and zm_clean_decide (csrc/clean.hip) against the numpy restatement (tests/clean_ref.py) on the GPU.

The per-object sums F, T and m, the decisions (``into``, ``root``), the segmentation map, every integer column,
PARENT_NUMBER and NMERGED are compared bit for bit.  The float columns are held to the bounds of
tests/test_extract_gpu.py, figures printed before anything is asserted: 10 x the difference between the restatement's
forward and reversed summation order, plus ``extract_ref.LIBM_ULPS`` spacings for THETA_IMAGE and FWHM_IMAGE; FLUX_APER and
FLUXERR_APER to the aperture kernel's existing pin (rtol 1e-10, atol 1e-9).  Every row is compared in every column: the
NaN / +inf / -inf pattern of a float column must equal the restatement's, and outside the poisoned scenes every float must
be finite.  The scenes of ``clean_scenes.PLANES`` - the frame's edges, bad pixels, a flag plane, non-finite pixels, and a
shred beside a 3 x 3 hole that CLEAN folds into the star whose wing the hole lies in, once in the frame's corner - run
deblended at nthresh 32 and at nthresh 8 (tests/test_clean_ref.py: their gaps, and that the planes change the map).

Outcomes of the scenes (restatement and GPU alike): ``halo`` with seeds 1, 2, 3 goes from 6 / 16 / 15 objects to 3, the
galaxy and the two stars, with smallest relative gaps 0.51 / 0.18 / 0.24; ``stars40`` keeps its 23 objects, ``two_equal``
its two, and both equal the call without CLEAN bit for bit; ``halo_pair`` (``halo`` 2 and a pair 6 px apart) goes from 18
deblended objects to 5, both members of the pair among them with FLAGS bit 2, and from 17 to 4 without deblending.  With ``param`` 0.5 and 2 the decisions are compared on
tables whose gap exceeds ``clean_ref.GAP_MIN`` (tests/test_clean_ref.py checks that they do).
"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import clean_ref as cr
import clean_scenes as cs
import deblend_scenes as ds
import extract_ref as xr
from test_clean_ref import chain_table
from test_extract_gpu import APER_COLUMNS

pytestmark = pytest.mark.gpu

DEBLEND = dict(nthresh=32, mincont=0.005)


def run(engine, name, deblend=False, **more):
    """``deblend``: False, True (nthresh 32) or another nthresh."""
    img, sigma, kw = cs.scene(name)
    db = dict(DEBLEND, nthresh=32 if deblend is True else int(deblend)) if deblend else False
    return engine.extract(img, sigma, full=True, deblend=db, clean=more.pop('clean', True), **kw, **more)


def int_columns(deblend):
    return xr.INT_COLUMNS + (['PARENT_NUMBER'] if deblend else []) + ['NMERGED']


def compare(engine, name, deblend=False, finite=True, **more):
    """``finite``: every float of both tables must be finite (every scene but the poisoned ones).  Otherwise the NaN / inf
    pattern of every float column must equal the restatement's; no row and no column is left out either way."""
    got = run(engine, name, deblend, **more)
    ref, rev = cs.reference(name, deblend), cs.reference(name, deblend, reverse=True)
    assert got['status'] == 0
    ds.assert_same_plane(got['filtered'], ref['filtered'])
    assert np.array_equal(got['segm'], ref['segm']), 'segmentation map'
    t, r = got['table'], ref['table']
    assert got['nfound'] == len(r) == len(t)
    assert ('PARENT_NUMBER' in t.dtype.names) == bool(deblend)
    for c in int_columns(deblend):
        assert np.array_equal(t[c], r[c]), c
    worst, bounds, fails = ds.float_columns(t, r, rev['table'], APER_COLUMNS, finite)
    print(f'clean {name} deblend={deblend}: {len(ref["pre"]["table"])} -> {len(r)} objects, gap {ref["gap"]:.3g}; column '
          f'measured (order bound; libm allowance in spacings): '
          + ', '.join(f'{c} {worst[c]:.3g} ({bounds[c]:.3g}; {xr.LIBM_ULPS.get(c, 0)})' for c in xr.FLOAT_COLUMNS))
    assert not fails, fails
    return got, ref


# ---- k_cl_stats through the full call -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['shapes1', 'shapes5', 'shapes9', 'halo2'])
def test_object_sums_bit_for_bit(engine, name):
    """F in the fixed order of k_ex_measure, T at the first pixel of the largest f, m the k-th largest f - t for k = 1, 5,
    9: an object of exactly k pixels, a plateau, a box beyond 32 x 32 and one round of lanes, a noise plane that varies."""
    got = run(engine, name)
    ref = cs.reference(name)
    F, T, m = engine.clean_stats()
    assert len(F) == len(ref['F']) == len(ref['pre']['table']) and len(F) >= 4
    print(f'{name}: F {F[:4]}, T {T[:4]}, m {m[:4]}')
    assert F.tobytes() == ref['F'].tobytes(), 'F'
    assert T.tobytes() == ref['T'].tobytes(), 'T'
    assert m.tobytes() == ref['m'].tobytes(), 'm'
    if name.startswith('shapes'):
        k = cs.scene(name)[2]['detect_minarea']
        npix = ref['pre']['table']['ISOAREA_IMAGE']
        assert npix.min() == k and 36 in npix and 1440 in npix                # exactly k pixels; the plateau; 40 x 36
        assert not ref['into'].any() and got['nfound'] == len(F)


# ---- zm_clean_decide ------------------------------------------------------------------------------------------------
def to_rows(zuds, rows):
    out = np.zeros(len(rows), np.dtype(zuds._lib.zm_object))
    for c in cr.ROW.names:
        out[c] = rows[c]
    return out


def decide_both(engine, zuds, rows, F, T, m, param=1.0):
    into, root = engine.clean_decide(to_rows(zuds, rows), F, T, m, minarea=5, clean=dict(param=param))
    rinto, rroot, gap = cr.decide(rows, F, T, m, param)
    return into, root, rinto, rroot, gap


@pytest.mark.parametrize('param', [1.0, 0.5, 2.0])
@pytest.mark.parametrize('n', cs.TABLE_SIZES)
def test_decisions_on_random_tables(engine, zuds, n, param):
    rows, F, T, m = cs.random_table(n, cs.TABLE_SEED + n)
    into, root, rinto, rroot, gap = decide_both(engine, zuds, rows, F, T, m, param)
    print(f'n {n} param {param}: {int((rinto > 0).sum())} absorbed, {int(((rinto > 0) & (rroot != rinto)).sum())} through a '
          f'chain, gap {gap:.3g}')
    assert param == 1.0 or gap > cr.GAP_MIN
    assert np.array_equal(into, rinto), 'into'
    assert np.array_equal(root, rroot), 'root'
    if n >= 255:
        assert (rinto > 0).any()


@pytest.mark.parametrize('param', [1.0, 0.5, 2.0])
def test_a_chain_of_three(engine, zuds, param):
    rows, F, T, m = chain_table()
    if param == 2.0:                                      # a steeper wing: lower profiles at the same places
        m = np.array([1e-3, 1e-4, 3.0], np.float32)
    elif param == 0.5:                                    # a shallower one: fainter absorbers, or val passes 1e10
        F, m = np.array([200.0, 5e3, 5e4]), np.array([1.0, 0.5, 3.0], np.float32)
    into, root, rinto, rroot, gap = decide_both(engine, zuds, rows, F, T, m, param)
    assert gap > cr.GAP_MIN
    assert rinto.tolist() == [2, 3, 0] and rroot.tolist() == [3, 3, 3]       # C absorbs B, B absorbs A, C does not reach A
    assert into.tolist() == [2, 3, 0] and root.tolist() == [3, 3, 3]


def pair_table(sep, F=(3000.0, 3000.0)):
    """Two round objects ``sep`` apart, a = 2 and 1: the zone ends at 10 (2 + 1) = 30."""
    rows = np.zeros(2, cr.ROW)
    rows['number'] = [1, 2]
    rows['x_image'], rows['y_image'] = [50.0, 50.0 + sep], [50.0, 50.0]
    rows['a_image'] = rows['b_image'] = [2.0, 1.0]
    rows['x2'] = rows['y2'] = [4.0, 1.0]
    rows['npix'] = [60, 12]
    rows['first'] = [100, 40]
    return rows, np.array(F), np.full(2, 6.0, np.float32), np.full(2, 1e-3, np.float32)


def test_equal_flux_zone_edge_and_non_absorbers(engine, zuds):
    # equal F: the smaller NUMBER counts as the larger, whichever way round the two lie
    rows, F, T, m = pair_table(12.0)
    into, root, rinto, rroot, _ = decide_both(engine, zuds, rows, F, T, m)
    assert into.tolist() == rinto.tolist() == [0, 1] and root.tolist() == rroot.tolist() == [1, 1]
    rows['x_image'] = rows['x_image'][::-1].copy()
    into, root, rinto, rroot, _ = decide_both(engine, zuds, rows, F, T, m)
    assert into.tolist() == rinto.tolist() == [0, 1]
    # just inside and just outside the zone of 10 (a_i + a_j) = 30: the profile would pass at either distance
    for sep, want in ((30.0 - 1e-9, [0, 1]), (30.0, [0, 0]), (30.0 + 1e-9, [0, 0])):
        rows, F, T, m = pair_table(sep, F=(1e6, 3000.0))
        m[:] = 1e-6
        into, root, rinto, rroot, _ = decide_both(engine, zuds, rows, F, T, m)
        assert into.tolist() == rinto.tolist() == want, sep
    # alpha <= 0: an object whose model amplitude lies below its threshold absorbs nothing ...
    rows, F, T, m = pair_table(5.0, F=(100.0, 20.0))
    assert not cr.model(rows, F, T, 1.0)['ok'][0]
    into, root, rinto, rroot, _ = decide_both(engine, zuds, rows, F, T, m)
    assert into.tolist() == rinto.tolist() == [0, 0]
    # ... but is absorbed like any other
    rows, F, T, m = chain_table()
    F[0], m[0] = 1.0, 0.1
    assert not cr.model(rows, F, T, 1.0)['ok'][0]
    into, root, rinto, rroot, _ = decide_both(engine, zuds, rows, F, T, m)
    assert into.tolist() == rinto.tolist() == [2, 3, 0]


def test_decide_refuses_bad_input(engine, zuds):
    rows, F, T, m = chain_table()
    for bad in (dict(param=0.05), dict(param=float('nan')), dict(exponent=1.0)):
        with pytest.raises(ValueError):
            engine.clean_decide(to_rows(zuds, rows), F, T, m, clean=bad)
    L, lib = zuds._lib.lib(), zuds._lib
    zr = to_rows(zuds, rows)
    cl = lib.zm_clean_params()
    L.zm_clean_params_default(C.byref(cl))
    out = np.zeros(3, np.int32)
    args = lambda r, n=3, k=5: (engine.ctx, n, r.ctypes.data, F.ctypes.data, T.ctypes.data, m.ctypes.data, k, C.byref(cl),
                                out.ctypes.data, out.ctypes.data)
    assert L.zm_clean_decide(*args(zr)) == 0
    assert L.zm_clean_decide(*args(zr, n=0)) != 0 and b'zm_clean_decide' in L.zm_last_error()
    assert L.zm_clean_decide(*args(zr, k=10)) != 0 and b'npix' in L.zm_last_error()      # npix 9 < minarea 10
    wrong = zr.copy()
    wrong['number'] = [1, 3, 2]
    assert L.zm_clean_decide(*args(wrong)) != 0 and b'number' in L.zm_last_error()
    cl.param = 11.0
    assert L.zm_clean_decide(*args(zr)) != 0 and b'bad parameters' in L.zm_last_error()
    assert L.zm_clean_decide(engine.ctx, 3, zr.ctypes.data, F.ctypes.data, T.ctypes.data, m.ctypes.data, 5, None, None, None) != 0


# ---- full calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('deblend', [False, True])
@pytest.mark.parametrize('seed', [1, 2, 3])
def test_halo(engine, seed, deblend):
    got, ref = compare(engine, f'halo{seed}', deblend)
    t = got['table']
    assert len(ref['pre']['table']) == {1: 6, 2: 16, 3: 15}[seed] and len(t) == 3
    for cx, cy, *_ in cs.HALO_SOURCES:
        assert (np.hypot(t['X_IMAGE'] - 1.0 - cx, t['Y_IMAGE'] - 1.0 - cy) < 1.0).sum() == 1
    assert sorted(t['NMERGED'].tolist()) == [1, 1, len(ref['pre']['table']) - 2]
    plain = run(engine, f'halo{seed}', deblend, clean=False)
    assert len(plain['table']) == len(ref['pre']['table']) and 'NMERGED' not in plain['table'].dtype.names
    assert np.array_equal(plain['segm'] > 0, got['segm'] > 0)                 # pixels change hands, none appears or goes


def test_deblended_pair_survives_clean(engine):
    """Deblending splits the pair, CLEAN folds the halo's 13 bumps into the galaxy and keeps both members of the pair,
    with their FLAGS bit 2 and their common PARENT_NUMBER; without deblending the pair is one row."""
    got, ref = compare(engine, 'halo_pair', True)
    t = got['table']
    assert len(ref['pre']['table']) == 18 and len(t) == 5 and ref['pre']['nsplit'] == 1
    pair = [int(np.argmin(np.hypot(t['X_IMAGE'] - 1.0 - x, t['Y_IMAGE'] - 1.0 - 38.0))) for x in (40.0, 46.0)]
    assert pair[0] != pair[1] and (t['FLAGS'][pair] & 2).all() and t['PARENT_NUMBER'][pair[0]] == t['PARENT_NUMBER'][pair[1]]
    assert (t['NMERGED'][pair] == 1).all() and sorted(t['NMERGED'].tolist()) == [1, 1, 1, 1, 14]
    assert not (np.delete(t['FLAGS'], pair) & 2).any()
    got, ref = compare(engine, 'halo_pair', False)
    assert len(ref['pre']['table']) == 17 and len(got['table']) == 4 and not (got['table']['FLAGS'] & 2).any()


def test_deblended_field_is_left_alone(engine):
    got, ref = compare(engine, 'noisy_field', True)
    plain = run(engine, 'noisy_field', True, clean=False)
    assert len(got['table']) == 20 and got['segm'].tobytes() == plain['segm'].tobytes()
    for c in plain['table'].dtype.names:                                      # PARENT_NUMBER and FLAGS bit 2 among them
        assert got['table'][c].tobytes() == plain['table'][c].tobytes(), c
    assert (got['table']['FLAGS'] & 2).any() and (got['table']['NMERGED'] == 1).all()


@pytest.mark.parametrize('name', ['stars40', 'two_equal'])
def test_where_nothing_is_absorbed_the_call_equals_the_one_without(engine, name):
    got, ref = compare(engine, name)
    plain = run(engine, name, clean=False)
    assert not ref['into'].any() and len(got['table']) == {'stars40': 23, 'two_equal': 2}[name]
    assert got['segm'].tobytes() == plain['segm'].tobytes() and got['nfound'] == plain['nfound']
    assert got['filtered'].tobytes() == plain['filtered'].tobytes()
    for c in plain['table'].dtype.names:
        assert got['table'][c].tobytes() == plain['table'][c].tobytes(), c
    assert (got['table']['NMERGED'] == 1).all()
    if name == 'two_equal':
        F, _, _ = engine.clean_stats()
        assert F[0] == F[1]


def test_wide_table_reads_the_new_map(engine):
    img, sigma, kw = cs.scene('halo2')
    iso = run(engine, 'halo2')
    wide = run(engine, 'halo2', columns='param')
    t = wide['table']
    assert len(t) == 3 and np.array_equal(wide['segm'], iso['segm']) and t.dtype.names[-1] == 'NMERGED'
    for c in iso['table'].dtype.names:
        assert t[c].tobytes() == iso['table'][c].tobytes(), c
    assert np.isfinite(t['FLUX_AUTO']).all() and (t['FLUX_AUTO'] > 0).all()
    # the second pass measured the merged galaxy: its Kron flux exceeds that of the largest piece before CLEAN
    before = engine.extract(img, sigma, columns='param', **kw)[0]
    gal = int(np.argmax(t['NMERGED']))
    assert t['ISOAREA_IMAGE'][gal] > before['ISOAREA_IMAGE'].max()
    assert abs(t['XWIN_IMAGE'][gal] - 1.0 - 80.3) < 1.0 and abs(t['YWIN_IMAGE'][gal] - 1.0 - 79.6) < 1.0
    both = run(engine, 'halo2', True, columns='param')['table']
    assert both.dtype.names[-2:] == ('PARENT_NUMBER', 'NMERGED') and len(both) == 3


def test_fewer_rows_than_objects_before_clean(engine):
    """CLEAN sees all 16 objects of the pass before whatever max_objects is; max_objects truncates the final table alone."""
    full = run(engine, 'halo2')
    for cap in (2, 5):
        part = run(engine, 'halo2', max_objects=cap)
        n = min(cap, 3)
        assert len(part['table']) == n and part['nfound'] == 3 and part['status'] == 0
        assert part['table'].tobytes() == full['table'][:n].tobytes()
        assert np.array_equal(part['segm'], full['segm'])
    none = run(engine, 'halo2', max_objects=0)
    assert len(none['table']) == 0 and none['nfound'] == 3 and np.array_equal(none['segm'], full['segm'])
    part = run(engine, 'stars40', max_objects=7)                              # nothing absorbed: the other path
    whole = run(engine, 'stars40')
    assert len(part['table']) == 7 and part['nfound'] == 23 and part['table'].tobytes() == whole['table'][:7].tobytes()
    assert np.array_equal(part['segm'], whole['segm'])


def test_limits_runs_and_entry_points(engine):
    hipmem = importlib.import_module('zuds-pipeline_amd.hipmem')
    one = np.full((1, 1), 10.0, np.float32)
    for minarea, n in ((1, 1), (5, 0)):
        r = engine.extract(one, np.ones_like(one), full=True, clean=True, detect_minarea=minarea)
        assert len(r['table']) == n == r['nfound'] and int(r['segm'][0, 0]) == n and r['status'] == 0
        assert 'NMERGED' in r['table'].dtype.names
    empty = np.zeros((40, 56), np.float32)
    r = engine.extract(empty, np.ones_like(empty), full=True, clean=True, deblend=True)
    assert len(r['table']) == 0 and r['nfound'] == 0 and not r['segm'].any()
    img, sigma, _ = cs.scene('halo3')
    a, b = run(engine, 'halo3'), run(engine, 'halo3')
    assert a['table'].tobytes() == b['table'].tobytes() and a['segm'].tobytes() == b['segm'].tobytes()
    bufs = []
    for arr in (img, sigma):
        d = hipmem.DeviceBuffer(arr.nbytes)
        d.upload(np.ascontiguousarray(arr))
        bufs.append(d)
    dseg = hipmem.DeviceBuffer(a['segm'].nbytes)
    dtab, nfound = engine.extract_dev(bufs[0].ptr, bufs[1].ptr, None, None, 160, 160, segm=dseg.ptr, clean=True)
    assert nfound == 3 and dtab.dtype == a['table'].dtype and dtab.tobytes() == a['table'].tobytes()
    assert np.array_equal(dseg.download(np.int32, a['segm'].shape), a['segm'])
    for bad in (dict(param=0.01), dict(param=float('inf')), dict(beta=1.0)):
        with pytest.raises(ValueError):
            engine.extract(img, sigma, clean=bad)


@pytest.mark.parametrize('nthresh', cs.PLANES_NTHRESH)
@pytest.mark.parametrize('name', cs.PLANES)
def test_edges_bad_pixels_flags_and_poison(engine, name, nthresh):
    """CLEAN over the scenes with edges, bad pixels, flags and poison (clean_ref.clean(..., bad=, flag=)), deblended at
    nthresh 32 and 8.  Stars are not each other's shreds: only the shred beside the hole is absorbed."""
    got, ref = compare(engine, name, nthresh, finite=name not in ds.POISON_SCENES, clean=dict(param=1.0))
    t = got['table']
    if name in cs.SHREDS:
        assert t['NMERGED'].tolist() == ([2, 1] if nthresh == 32 else [2]) and t['FLAGS_WEIGHT'][0] == 1
        assert ((t['XMIN_IMAGE'][0], t['YMIN_IMAGE'][0]) == (1, 1)) == (name == 'shred_corner')
    else:
        assert len(t) == ds.EXPECT[name][4] and (t['NMERGED'] == 1).all()


def test_planes_on_the_device_and_two_runs(engine):
    hipmem = importlib.import_module('zuds-pipeline_amd.hipmem')
    img, sigma, kw = cs.scene('shred_corner')
    flag = (np.arange(48 * 48, dtype=np.int32).reshape(48, 48) % 5 == 0) * 8
    a, b = (run(engine, 'shred_corner', True, flag=flag) for _ in range(2))
    assert a['table'].tobytes() == b['table'].tobytes() and a['segm'].tobytes() == b['segm'].tobytes()
    assert a['table']['NMERGED'].tolist() == [2, 1] and a['table']['IMAFLAGS_ISO'].tolist() == [8, 8]
    bufs = []
    for arr, dt in ((img, np.float32), (sigma, np.float32), (kw['bad'], np.uint8), (flag, np.int32)):
        arr = np.ascontiguousarray(arr, dt)
        d = hipmem.DeviceBuffer(arr.nbytes)
        d.upload(arr)
        bufs.append(d)
    dseg = hipmem.DeviceBuffer(a['segm'].nbytes)
    dtab, nfound = engine.extract_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 48, 48, segm=dseg.ptr, deblend=DEBLEND,
                                      clean=True, filter=False)
    assert nfound == 2 and dtab.dtype == a['table'].dtype and dtab.tobytes() == a['table'].tobytes()
    assert np.array_equal(dseg.download(np.int32, a['segm'].shape), a['segm'])


# ---- through the layers ---------------------------------------------------------------------------------------------
from test_deblend_gpu import blended_subtraction                             # noqa: E402,F401  (the fixture: one small subtraction)


def test_candidates_on_a_resident_subtraction(blended_subtraction, engine):
    import torch
    sc = blended_subtraction
    ref, sci, f = sc['ref'], sc['ims'][3], sc['frames'][3]
    dmod = importlib.import_module('zuds-pipeline_amd.device')
    chain = dmod.DeviceSubtraction(sci.wcs, ref.wcs, device=0, engine=engine)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to('cuda:0')
    args = (t(f['img'], np.float32), t(sci.rms_image.data, np.float32), t(f['mask'], np.int32),
            t(sci.weight_image.data, np.float32), t(ref.data, np.float32), t(ref.rms_image.data, np.float32),
            t(ref.mask_image.data, np.int32))
    torch.cuda.synchronize()
    chain.run(*args, seeing=2.0, nreg_side=1, hotpants_kws={'ko': 0, 'bgo': 0},
              ref_flxscale=float(ref.header.get('FLXSCALE', 1.0)))
    ptab, nplain, pseg = chain.extract()
    ctab, nclean, cseg = chain.extract(clean=True)
    btab, nboth, _ = chain.extract(clean=dict(param=1.0), deblend=True)
    cand, ncand = chain.candidates(2.0, clean=True)
    chain.stream.synchronize()
    engine.set_stream(0)
    assert 'NMERGED' in ctab.dtype.names and 'NMERGED' not in ptab.dtype.names and 'PARENT_NUMBER' not in ctab.dtype.names
    assert btab.dtype.names[-2:] == ('PARENT_NUMBER', 'NMERGED')
    assert nclean <= nplain and int(ctab['NMERGED'].sum()) == nplain and ncand == nclean
    assert torch.equal(pseg > 0, cseg > 0)
    if nclean == nplain:
        assert torch.equal(pseg, cseg)
    assert 'GOODCUT' in cand.dtype.names and 'NMERGED' in cand.dtype.names and len(cand) <= nclean
    print(f'candidates: {nplain} objects, {nclean} after CLEAN, {nboth} deblended and cleaned')


def test_dosub_detect_clean_writes_the_cards(blended_subtraction, engine, monkeypatch, capsys):
    from test_catalog_gpu import load_script
    sc = blended_subtraction
    z, d = sc['z'], sc['d']
    script = load_script('dosub')
    monkeypatch.setattr(script, 'MAX_DETS', 10 ** 6)
    jobs = os.path.join(d, 'images.txt')
    with open(jobs, 'w') as f:
        f.write(sc['ims'][3].local_path + '\n')
    assert script.main([jobs, sc['refname'], '--clean']) == 2                 # needs --detect
    capsys.readouterr()
    assert script.main([jobs, sc['refname'], '--detect', '--clean', '--clean-param', '1.5']) == 0
    out = capsys.readouterr().out
    assert 'cat: ' in out and 'Traceback' not in out
    cat = z.PipelineFITSCatalog.from_file(z.sub_name(sc['ims'][3].local_path, sc['refname']).replace('.fits', '.cat'))
    th = cat.table_header
    assert th['ZMCLEAN'] is True and th['ZMCLNPAR'] == 1.5 and th['ZMDEBLND'] is False and cat.clean == dict(param=1.5)
    assert 'NMERGED' in cat.data.dtype.names and 'GOODCUT' in cat.data.dtype.names
    assert 'PARENT_NUMBER' not in cat.data.dtype.names and (cat.data['NMERGED'] >= 1).all()
