"""The kernel fit's stamp rejection and every fit parameter against the hotpants oracle.

The scenes of tests/hp_scenes.py (transients on the brightest stars, noise maps that vary over the frame) make the
fit reject stamps for up to eight rounds, walk the substamp lists to their ends and let regions converge at different
rounds; tests/test_oracle_rejection.py proves that on the CPU, with the margins that rule out ties.  Here the GPU fit
runs the same cases: every product through ``compare()`` of test_subtract_gpu.py at its tolerances, plus the summary's
chi2 against the oracle's.

CHI2_TOL: the two fp64 CPU implementations (oracle/hotpants.py and oracle/cport/zm_hotpants.c, sums in different
orders) differ in chi2 by at most 3.5e-9 (relative) over these cases; ten times that is below the 1e-6 that
test_oracle_cport.py asks of them, so 1e-6 it is.  No basis needed a pixel tolerance of its own.
"""
import numpy as np
import pytest

import hp_scenes as hs
from test_subtract_gpu import compare
from util import pkg

pytestmark = pytest.mark.gpu

CHI2_TOL = 1e-6
SUMMARY = ('nstamps_total', 'nstamps_used', 'niter', 'ncoeff', 'kernel_sum', 'chi2', 'nmasked')


def ncoeff(kw):
    nc = sum((d + 1) * (d + 2) // 2 for d in kw.get('deg', (6, 4, 2)))
    ko, bgo = kw['ko'], kw['bgo']
    return 1 + (nc - 1) * (ko + 1) * (ko + 2) // 2 + (bgo + 1) * (bgo + 2) // 2


def run_case(engine, name, **more):
    kw = hs.case_kw(name)
    d, n, info, rd = compare(engine, hs.case_data(name), chi2_tol=CHI2_TOL, **more, **kw)
    assert info['status'] == 0 and info['retries'] == 0 and info['ncoeff'] == ncoeff(kw)
    return info


@pytest.mark.parametrize('nss', [1, 3, 8])
@pytest.mark.parametrize('scene', ['tr5', 'tr9', 'step'])
def test_rejection_branches(engine, scene, nss):
    """Regions of 8 / 5 / 2 rounds side by side, rejections in the eighth round, stamps on their 2nd and 3rd substamp,
    stamps that run out at nss and at an empty centre before it - at one, three and eight substamps per stamp.  In
    ``step`` the science noise map jumps tenfold at column 96: vbar spans two decades and decides who is rejected."""
    info = run_case(engine, f'{scene}-nss{nss}')
    assert info['niter'] == max(r[0] for r in hs.EXPECT[f'{scene}-nss{nss}'])


@pytest.mark.parametrize('name', ['ks0.5', 'ks1.0', 'ks4.0', 'ft5', 'ft200'])
def test_rejection_settings(engine, name):
    run_case(engine, name)


def test_block_wide_rejection_kernel(engine):
    """272 cells in one region (k_hp_reject instead of k_hp_reject_wave), eight rounds, 47 stamps lost."""
    info = run_case(engine, 'wide')
    assert info['niter'] >= 3 and info['nstamps_used'] < info['nstamps_total']


@pytest.mark.parametrize('name, tol', [('ko0', 1e-5), ('ko4', 1e-5), ('ko5', 2e-4), ('bgo2', 1e-5)])
def test_incremental_build_at_its_other_shapes(engine, name, tol):
    """The retained normal matrix loses and gains stamps with one spatial term, with the reference's orders, with
    more than 16 spatial terms (the per-pair build) and with six background terms."""
    info = run_case(engine, name, tol=tol)
    assert info['niter'] >= 4


def test_factorisation_forms_under_rejection(engine, monkeypatch):
    """Eight live rounds under every form of the factorisation, and repeated after a time-out of the first attempt:
    the same bits."""
    data, kw = hs.case_data('tr5-nss3'), hs.case_kw('tr5-nss3')
    d0, n0, i0, _ = compare(engine, data, chi2_tol=CHI2_TOL, **kw)
    assert i0['niter'] == 8 and i0['retries'] == 0 and i0['status'] == 0
    for var, val, retries in (('ZM_CHOL_FORM', 'lat', 0), ('ZM_CHOL_FORM', 'tp', 0), ('ZM_CHOL_FORM', 'df', 0),
                              ('ZM_CHOL_SPIN_LIMIT', '0', None)):
        monkeypatch.setenv(var, val)
        d, n, i = engine.subtract(*data, **kw)
        monkeypatch.delenv(var)
        assert i['status'] == 0 and i['nunsolved'] == 0 and (retries is None or i['retries'] == retries), (var, val)
        assert np.array_equal(d0, d) and np.array_equal(n0, n), (var, val)
        for k in SUMMARY:
            assert i0[k] == i[k], (var, val, k)


@pytest.mark.parametrize('order', [('batch-1', 'batch-5', 'tr5-nss3'), ('tr5-nss3', 'batch-5', 'batch-1')])
def test_batch_of_jobs_that_leave_at_different_rounds(engine, order):
    """Jobs of 1, 5 and 8 rounds in one batch (the per-round job tables shrink as they leave): each like the oracle's
    and bit for bit its lone subtraction's."""
    kw = hs.case_kw(order[0])
    assert all(hs.case_kw(n) == kw for n in order)
    frames = [hs.case_data(n) for n in order]
    got = engine.subtract_batch(frames, **kw)
    rounds = []
    for data, g in zip(frames, got):
        compare(engine, data, got=g, chi2_tol=CHI2_TOL, **kw)
        d, n, info = engine.subtract(*data, **kw)
        assert np.array_equal(d, g[0]) and np.array_equal(n, g[1]) and info == g[2]
        rounds.append(info['niter'])
    assert sorted(rounds) == [1, 5, 8]


@pytest.mark.parametrize('name', ['basis-4', 'basis-8-0', 'basis-3-2-2-1', 'basis-0', 'basis-limit'])
def test_bases(engine, name):
    """One to four Gaussians, degrees 0 to 8, two unknowns, and a Gram tile filled to its last row."""
    info = run_case(engine, name)
    if name == 'basis-0':
        assert info['ncoeff'] == 2
    if name == 'basis-limit':
        assert info['ncoeff'] == 1 + 52 * 3 + 10


def test_basis_over_the_gram_tile_is_refused(engine):
    z = pkg()
    with pytest.raises(z.ZMError):
        engine.subtract(*hs.case_data('basis-limit'), **dict(hs.case_kw('basis-limit'), **hs.OVER_LIMIT))


def test_noise_maps_that_vary_on_a_clean_scene(engine):
    """vbar differs from stamp to stamp.  (The scene whose tenfold step in the science noise map decides who is
    rejected - test_the_noise_maps_decide_who_is_rejected of test_oracle_rejection.py - is the ``step`` scene of
    test_rejection_branches.)"""
    run_case(engine, 'noise-clean')
