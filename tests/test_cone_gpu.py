"""The resident sky index and its two queries (csrc/skyindex.hip) against tests/cone_ref.py on the smallest scenes that
can break them.  ``idx``, ``count``, ``offsets`` and ``cat_idx`` are compared exactly - every query, every slot - which the
restatement's two preconditions allow (no pair in the band 0.999 r .. 1.001 r; rows of one query are the same position or
clearly apart in separation: asserted on every scene, and proven against a KD-tree by tests/test_cone_ref.py).

``sep`` alone has a tolerance: ``assoc_ref.SEP_TOL_ARCSEC``, 16 eps64 radians of chord.  It carries over from
tests/test_associate_gpu.py because the unit-vector, chord and separation formulas are the same functions (sky_cells.h),
and the worst-case derivation there (14.5 eps64) does not depend on the scene.  tests/measure_cone_tolerance.py repeats
the 50-digit measurement on these scenes."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import assoc_ref as ar
import cone_ref as cr
from util import pkg

pytestmark = pytest.mark.gpu


def xm():
    return importlib.import_module('zuds-pipeline_amd.crossmatch')


def src():
    return importlib.import_module('zuds-pipeline_amd.source')


@functools.lru_cache(maxsize=None)
def scene(name):
    out = cr.scene(name)
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def knn_want(name, r, k):
    return cr.knn_ref(*scene(name), r, k, what=f'{name} at {r}')


@functools.lru_cache(maxsize=None)
def within_want(name, r):
    return cr.within_ref(*scene(name), r, what=f'{name} at {r}')


def check_knn(got, want, what):
    idx, sep, count = got
    widx, wsep, wcount = want
    assert idx.dtype == np.int32 and count.dtype == np.int32 and sep.dtype == np.float64
    assert idx.shape == widx.shape and np.array_equal(idx, widx), what
    assert np.array_equal(count, wcount), what
    hit = widx >= 0
    assert np.isnan(sep[~hit]).all() and not np.isnan(sep[hit]).any(), what
    err = np.abs(sep[hit] - wsep[hit]).max(initial=0.0)
    print(f'{what}: largest |sep - restatement| = {err:.3e} arcsec = {err / (ar.EPS64 * ar.ARCSEC_PER_RAD):.2f} eps64 rad '
          f'(bound {ar.SEP_K})')
    assert err <= ar.SEP_TOL_ARCSEC, what


def check_within(got, want, what):
    offsets, cat_idx = got
    assert offsets.dtype == np.int64 and cat_idx.dtype == np.int32
    assert np.array_equal(offsets, want[0]) and np.array_equal(cat_idx, want[1]), what


@pytest.mark.parametrize('name', cr.SCENES)
def test_scenes(engine, name):
    ra, dec, cra, cdec = scene(name)
    with xm().SkyIndex(cra, cdec, cr.R_KNN, engine=engine) as ix:
        assert ix.stats()['rows'] == int((np.isfinite(cra) & np.isfinite(cdec)).sum())
        for r in (cr.R_KNN, cr.R_NAME):                  # r equal to max_radius, and 1.5 on an index built for 30
            for k in (1, 3, 8):
                check_knn(ix.knn(ra, dec, r, k), knn_want(name, r, k), f'{name} r={r} k={k}')
            check_within(ix.within(ra, dec, r), within_want(name, r), f'{name} r={r}')


@pytest.mark.parametrize('k', range(1, 9))
def test_every_k_on_queries_with_0_1_k_minus_1_k_k_plus_1_and_many_rows(engine, k):
    ra, dec, cra, cdec = scene('counts')
    with xm().SkyIndex(cra, cdec, cr.R_KNN, engine=engine) as ix:
        got = ix.knn(ra, dec, cr.R_KNN, k)
    want = knn_want('counts', cr.R_KNN, k)
    check_knn(got, want, f'counts k={k}')
    assert {0, 1, k - 1, k, k + 1, 40} <= set(got[2].tolist()) and (got[2] > k).any()
    assert (got[0][got[2] == 0] == -1).all() and np.isnan(got[1][got[2] == 0]).all()


def test_exact_duplicates_come_in_row_order(engine):
    ra, dec, cra, cdec = scene('duplicates')
    with xm().SkyIndex(cra, cdec, cr.R_KNN, engine=engine) as ix:
        for k in (2, 3, 4, 8):
            idx, sep, count = ix.knn(ra, dec, cr.R_KNN, k)
            check_knn((idx, sep, count), knn_want('duplicates', cr.R_KNN, k), f'duplicates k={k}')
            assert idx[0][:min(k, 3)].tolist() == [0, 2, 5][:k] and idx[1][:min(k, 5)].tolist() == [1, 4, 6, 8, 9][:k]
            assert sep[0][0] == sep[0][1] and (sep[1][:min(k, 5)] == 0.0).all()


@pytest.mark.parametrize('name', ['field', 'wrap', 'ra90', 'north', 'south'])
def test_k_1_is_zm_crossmatch_bit_for_bit(engine, name):
    ra, dec, cra, cdec, r = ar.xm_scene(name)
    widx, wsep = src().crossmatch(ra, dec, cra, cdec, r, engine=engine)
    for rmax in (r, 30.0):                               # the cell size does not show in the result
        with xm().SkyIndex(cra, cdec, rmax, engine=engine) as ix:
            idx, sep, count = ix.knn(ra, dec, r, 1)
        assert np.array_equal(idx[:, 0], widx) and (widx >= 0).sum() >= 10
        hit = widx >= 0
        assert sep[hit, 0].tobytes() == wsep[hit].tobytes() and np.isnan(sep[~hit, 0]).all()
        assert np.array_equal(count > 0, hit)


def test_empty_and_single_row_inputs(engine):
    ra, dec = np.array([10.0, 10.0, 50.0]), np.array([5.0, 5.0 + 1.0 / 3600, 5.0])
    with xm().SkyIndex([], [], 30.0, engine=engine) as ix:              # m = 0
        assert ix.stats() == dict(rows=0, cells=0, capacity=64, probe_max=0)
        idx, sep, count = ix.knn(ra, dec, 30.0, 3)
        assert idx.shape == (3, 3) and (idx == -1).all() and np.isnan(sep).all() and not count.any()
        offsets, cat_idx = ix.within(ra, dec, 30.0)
        assert offsets.tolist() == [0, 0, 0, 0] and cat_idx.size == 0
        idx, sep, count = ix.knn([], [], 30.0, 3)                       # n = 0 as well
        assert idx.shape == (0, 3) and count.shape == (0,)
    with xm().SkyIndex([10.0], [5.0], 30.0, engine=engine) as ix:      # m = 1
        assert ix.stats()['rows'] == 1 and ix.stats()['cells'] == 1 and ix.stats()['probe_max'] == 1
        for k in range(1, 9):
            idx, sep, count = ix.knn(ra, dec, 30.0, k)
            assert idx[:, 0].tolist() == [0, 0, -1] and (idx[:, 1:] == -1).all() and count.tolist() == [1, 1, 0]
            one = ar.separation(ra[1:2], dec[1:2], [10.0], [5.0])[0, 0]                 # (1 arcsec)
            assert sep[0, 0] == 0.0 and abs(sep[1, 0] - one) <= ar.SEP_TOL_ARCSEC and np.isnan(sep[2]).all()
        offsets, cat_idx = ix.within(ra, dec, 1.5)
        assert offsets.tolist() == [0, 1, 2, 2] and cat_idx.tolist() == [0, 0]
        offsets, cat_idx = ix.within([], [], 1.5)                       # n = 0
        assert offsets.tolist() == [0] and cat_idx.size == 0


def test_the_radius_and_k_are_checked(engine):
    z = pkg()
    ra, dec, cra, cdec = scene('counts')
    with xm().SkyIndex(cra, cdec, 30.0, engine=engine) as ix:
        with pytest.raises(z.ZMError, match='30') as e:
            ix.knn(ra, dec, 30.5, 3)
        assert '30.5' in str(e.value) and b'30.5' in z._lib.lib().zm_last_error()
        with pytest.raises(z.ZMError, match='45'):
            ix.within(ra, dec, 45.0)
        for r in (0.0, -1.0, np.nan):
            with pytest.raises(z.ZMError, match='radius'):
                ix.knn(ra, dec, r, 3)
        for k in (0, 9, -1):
            with pytest.raises(z.ZMError, match='k must be'):
                ix.knn(ra, dec, 30.0, k)
        check_knn(ix.knn(ra, dec, 30.0, 3), knn_want('counts', 30.0, 3), 'after the errors')      # the index is unharmed
    for rmax in (0.1, 4000.0, np.nan):
        with pytest.raises(z.ZMError, match='max_radius'):
            xm().SkyIndex(cra, cdec, rmax, engine=engine)


def test_within_writes_nothing_past_the_capacity(engine):
    import torch
    ra, dec, cra, cdec = scene('field')
    woff, widx = within_want('field', cr.R_KNN)
    npairs = int(woff[-1])
    assert npairs > 2000
    L = engine.L
    d_ra, d_dec = torch.from_numpy(np.array(ra)).cuda(), torch.from_numpy(np.array(dec)).cuda()
    canary = -7
    with xm().SkyIndex(cra, cdec, cr.R_KNN, engine=engine) as ix:
        for cap in (0, npairs - 1, npairs, 1000):
            off = torch.full((ra.size + 1,), -1, dtype=torch.int64, device='cuda')
            out = torch.full((npairs + 64,), canary, dtype=torch.int32, device='cuda')
            torch.cuda.synchronize()
            n = C.c_int64(0)
            rc = L.zm_cone_within_dev(engine.ctx, ix._handle(), ra.size, d_ra.data_ptr(), d_dec.data_ptr(), cr.R_KNN, cap,
                                      off.data_ptr(), out.data_ptr(), C.byref(n))
            assert rc == 0 and n.value == npairs
            engine.synchronize()
            assert np.array_equal(off.cpu().numpy(), woff)               # always complete
            got = out.cpu().numpy()
            assert np.array_equal(got[:cap], widx[:cap]) and (got[cap:] == canary).all(), cap
        # the Python form retries once with room for all: a first list that is too short (1024 < npairs) is invisible
        check_within(ix.within(ra, dec, cr.R_KNN), (woff, widx), 'retry')
        off, idx, n = ix.within_dev(d_ra, d_dec, cr.R_KNN, capacity=10)
        torch.cuda.synchronize()
        assert n == npairs and np.array_equal(idx.cpu().numpy()[:n], widx) and np.array_equal(off.cpu().numpy(), woff)


def test_one_index_serves_many_queries_and_every_run_gives_the_same_bytes(engine):
    import torch
    ra, dec, cra, cdec = scene('field')
    with xm().SkyIndex(cra, cdec, cr.R_KNN, engine=engine) as ix:
        stats = ix.stats()
        first = None
        for n, r, k in ((ra.size, cr.R_KNN, 3), (17, cr.R_NAME, 2), (101, 10.0, 8), (ra.size, cr.R_KNN, 3)):
            got = ix.knn(ra[:n], dec[:n], r, k)
            check_knn(got, cr.knn_ref(ra[:n], dec[:n], cra, cdec, r, k, check=False), f'n={n} r={r} k={k}')
            check_within(ix.within(ra[:n], dec[:n], r), cr.within_ref(ra[:n], dec[:n], cra, cdec, r, check=False), f'n={n} r={r}')
            if first is None:
                first = got
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, got))         # the same query again: the same bytes
        assert ix.stats() == stats                                                 # nothing was rebuilt
        # host and device forms
        d_ra, d_dec = torch.from_numpy(np.array(ra)).cuda(), torch.from_numpy(np.array(dec)).cuda()
        dev = ix.knn_dev(d_ra, d_dec, cr.R_KNN, 3)
        engine.synchronize()
        assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(first, dev))
        off, idx, n = ix.within_dev(d_ra, d_dec, cr.R_KNN)
        engine.synchronize()
        hoff, hidx = ix.within(ra, dec, cr.R_KNN)
        assert off.cpu().numpy().tobytes() == hoff.tobytes() and idx.cpu().numpy()[:n].tobytes() == hidx.tobytes()
    # a second index of the same rows, built from device arrays: the order inside a cell may differ, the results may not
    with xm().SkyIndex(torch.from_numpy(np.array(cra)).cuda(), torch.from_numpy(np.array(cdec)).cuda(), cr.R_KNN, engine=engine) as ix2:
        assert ix2.stats()['rows'] == stats['rows'] and ix2.stats()['cells'] == stats['cells']
        again = ix2.knn(ra, dec, cr.R_KNN, 3)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
        assert all(a.tobytes() == b.tobytes() for a, b in zip((hoff, hidx), ix2.within(ra, dec, cr.R_KNN)))


def test_stats_and_a_closed_index(engine):
    ra, dec, cra, cdec = scene('nonfinite')
    ix = xm().SkyIndex(cra, cdec, cr.R_KNN, engine=engine)
    st = ix.stats()
    assert st['rows'] == cra.size - 4 and 1 <= st['cells'] <= st['rows'] and st['probe_max'] >= 1
    assert st['capacity'] >= 2 * cra.size and st['capacity'] & (st['capacity'] - 1) == 0
    ix.close()
    ix.close()
    with pytest.raises(ValueError, match='closed'):
        ix.knn(ra, dec, 1.5, 1)
