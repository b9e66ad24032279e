"""The later rounds' update of the retained normal matrix: every form of it gives the same bits.

A rejection round takes the changed cells out of the unscaled normal matrix with the Gram matrices and spatial terms
they had and puts them back with the new ones (k_hp_build_blk / k_hp_build_blk_b, sign 2; k_hp_build beyond 16 spatial
terms).  The update stages all changed cells of a region once per workgroup and sums out of LDS; the sums, their order
and their roundings are those of the two-pass form, so the products are compared with ``np.array_equal`` and the
summary fields with ``==`` - between the forms of the factorisation, between one context used back to back and fresh
ones, and between a batch and lone subtractions.  Every scene also goes through ``compare()`` against the oracle at
the tolerances of test_subtract_rejection_gpu.py.
"""
import numpy as np
import pytest

import hp_scenes as hs
from test_subtract_gpu import compare
from test_subtract_rejection_gpu import CHI2_TOL, SUMMARY
from util import pkg

pytestmark = pytest.mark.gpu

# (pixel tolerance against the oracle: test_incremental_build_at_its_other_shapes)
TOL = {'ko5': 2e-4}


def same(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
    for k in SUMMARY:
        assert a[2][k] == b[2][k], (what, k)


def against_oracle(engine, name):
    kw = hs.case_kw(name)
    data = hs.case_data(name)
    d, n, info, _ = compare(engine, data, tol=TOL.get(name, 1e-5), chi2_tol=CHI2_TOL, **kw)
    assert info['status'] == 0 and info['retries'] == 0
    assert info['niter'] == max(r[0] for r in hs.EXPECT[name])
    return data, kw, (d, n, info)


@pytest.mark.parametrize('name', ['tr9-nss3', 'tr5-nss1', 'step-nss3', 'ko4', 'ko0', 'bgo2', 'wide', 'basis-limit',
                                  'ks4.0'])
def test_default_form_against_tp_and_lat(engine, monkeypatch, name):
    """Regions that converge at different rounds, a leave pass only (stamps dropped without replacement), 722 unknowns
    in one region, one spatial term, six background terms, a change list of more cells than one staging chunk, a Gram
    tile filled to its last row, and regions with no or a single update."""
    data, kw, ref = against_oracle(engine, name)
    for form in ('tp', 'lat'):
        monkeypatch.setenv('ZM_CHOL_FORM', form)
        got = engine.subtract(*data, **kw)
        monkeypatch.delenv('ZM_CHOL_FORM')
        assert got[2]['status'] == 0 and got[2]['retries'] == 0, form
        same(ref, got, form)


def test_one_context_back_to_back(engine):
    """8 rounds, 5 and 4 rounds, 1 and 2 rounds, 8 rounds again on one context: each like the same case on a fresh
    engine (nothing of a fit - flag words, retained matrices, old Gram matrices - leaks into the next one)."""
    z = pkg()
    order = ('tr5-nss3', 'batch-5', 'ks4.0', 'tr5-nss3')
    fresh = {}
    for name in set(order):
        e = z.Engine(0)
        try:
            fresh[name] = e.subtract(*hs.case_data(name), **hs.case_kw(name))
        finally:
            e.close()
    e = z.Engine(0)
    try:
        for k, name in enumerate(order):
            got = e.subtract(*hs.case_data(name), **hs.case_kw(name))
            assert got[2]['niter'] == max(r[0] for r in hs.EXPECT[name])
            same(fresh[name], got, (k, name))
    finally:
        e.close()
    for name in set(order):
        compare(engine, hs.case_data(name), got=fresh[name], chi2_tol=CHI2_TOL, **hs.case_kw(name))


def test_more_than_16_spatial_terms(engine, monkeypatch):
    """``ko5``: 21 spatial terms, the per-pair build (k_hp_build) - like the oracle's, and the same under ``tp``."""
    data, kw, ref = against_oracle(engine, 'ko5')
    monkeypatch.setenv('ZM_CHOL_FORM', 'tp')
    got = engine.subtract(*data, **kw)
    monkeypatch.delenv('ZM_CHOL_FORM')
    same(ref, got, 'tp')


def test_batch_against_lone(engine):
    """Jobs of 1, 5 and 8 rounds in one batch (k_hp_build_blk_b): bit for bit the lone subtractions."""
    order = ('batch-1', 'batch-5', 'tr5-nss3')
    kw = hs.case_kw(order[0])
    assert all(hs.case_kw(n) == kw for n in order)
    frames = [hs.case_data(n) for n in order]
    got = engine.subtract_batch(frames, **kw)
    for name, data, g in zip(order, frames, got):
        compare(engine, data, got=g, chi2_tol=CHI2_TOL, **kw)
        lone = engine.subtract(*data, **kw)
        same(lone, g, name)
        assert lone[2] == g[2], name
