"""``nightly._detect`` with a stand-in chain (no GPU): the order in which the subtraction's own verdict and the detection
step are asked, and what each failure leaves in the result."""
import importlib

import numpy as np
import pytest

from util import pkg


def table(n, ngood):
    t = np.zeros(n, dtype=[('X_WORLD', 'f8'), ('Y_WORLD', 'f8'), ('GOODCUT', 'u1')]).view(np.recarray)
    t['X_WORLD'], t['Y_WORLD'] = np.arange(n) + 10.0, np.arange(n) - 5.0
    t['GOODCUT'][:ngood] = 1
    return t


class Chain(object):
    def __init__(self, cat=None, result_error=None, cuts_error=None, stamps_error=None):
        self.cat, self.result_error, self.cuts_error, self.stamps_error = cat, result_error, cuts_error, stamps_error
        self.calls = []

    def result(self):
        self.calls.append('result')
        if self.result_error:
            raise self.result_error

    def candidates(self, seeing, wcs=None):
        self.calls.append('candidates')
        if self.cuts_error:
            raise self.cuts_error
        return self.cat, len(self.cat) + 3

    def stamps(self, ra, dec, sci, ref, ref_flxscale=1.0, sci_flxscale=1.0):
        self.calls.append('stamps')
        if self.stamps_error:
            raise self.stamps_error
        n = len(ra)
        return np.ones((n, 3, 63, 63), np.float32), np.ones((n, 3)), np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)


def job(nm, **kw):
    return nm.SubtractionJob(dict(seeing=2.4, wcs=None, img=None), dict(img=None), tag=7, detect=True, **kw)


def test_the_subtraction_s_verdict_comes_first_and_is_not_caught():
    z = pkg()
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    ch = Chain(cat=table(4, 2), result_error=z.ZMError('zm_median_mad2: every pixel is masked'))
    out = dict(tag=7)
    with pytest.raises(z.ZMError, match='every pixel is masked'):
        nm._detect(ch, job(nm, stamps=True), out)
    assert ch.calls == ['result'] and out == dict(tag=7)


def test_a_failure_of_the_cuts_leaves_the_products_and_says_so():
    z = pkg()
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    ch = Chain(cuts_error=z.ZMError('zm_candidate_cuts: sigma must be positive'))
    out = dict(tag=7, diff='kept')
    nm._detect(ch, job(nm, stamps=True), out)
    assert ch.calls == ['result', 'candidates']
    assert out == dict(tag=7, diff='kept', cat=None, detect_error='zm_candidate_cuts: sigma must be positive')


def test_stamps_of_the_good_rows_and_the_three_ways_to_get_none():
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    cat = table(5, 3)
    out = {}
    ch = Chain(cat=cat)
    nm._detect(ch, job(nm, stamps=True), out)
    assert out['cat'] is cat and out['nfound'] == 8 and out['stamps']['blocks'].shape == (3, 3, 63, 63)
    assert np.array_equal(out['stamps']['ra'], [10.0, 11.0, 12.0]) and np.array_equal(out['stamps']['dec'], [-5.0, -4.0, -3.0])
    # not asked for
    out, ch = {}, Chain(cat=cat)
    nm._detect(ch, job(nm), out)
    assert set(out) == {'cat', 'nfound'} and 'stamps' not in ch.calls
    # over the limit: the catalog, no stamps, and stamps never called
    out, ch = {}, Chain(cat=cat)
    nm._detect(ch, job(nm, stamps=True, max_detections=2), out)
    assert out['too_many'] is True and 'stamps' not in out and 'stamps' not in ch.calls and out['cat'] is cat
    # exactly at the limit is fine
    out = {}
    nm._detect(Chain(cat=cat), job(nm, stamps=True, max_detections=3), out)
    assert 'stamps' in out and 'too_many' not in out
    # a detection whose stamp misses the reference's grid: the catalog stays, stamps_error says why
    out = {}
    nm._detect(Chain(cat=cat, stamps_error=ValueError('stamp 1 does not overlap the grid')), job(nm, stamps=True), out)
    assert out['cat'] is cat and 'stamps' not in out and 'does not overlap the grid' in out['stamps_error']
    # no good row: empty blocks, the engine is not asked
    out, ch = {}, Chain(cat=table(4, 0))
    nm._detect(ch, job(nm, stamps=True), out)
    assert out['stamps']['blocks'].shape == (0, 3, 63, 63) and 'stamps' not in ch.calls


def test_stamps_need_detect():
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    with pytest.raises(ValueError):
        nm.SubtractionJob({}, {}, stamps=True)
    j = nm.SubtractionJob({}, {})
    assert (j.detect, j.stamps, j.max_detections) == (False, False, 50)
