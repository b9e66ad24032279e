"""The rejection scenes of tests/hp_scenes.py in the oracle alone (no GPU): each one reaches the branch of the stamp
rejection it is committed for, and no decision in it is a near tie.

Branches, read off the trace that ``oracle.hotpants.fit_region`` keeps on request:

* a - at least 5 rounds in one region while another region converges earlier;
* b - all 8 rounds, with a rejection in the eighth;
* c - a stamp that moves to its 2nd and to its 3rd substamp;
* d_nss / d_short - a stamp that runs out of substamps at ``a >= nss`` / at a ``(-1, -1)`` centre before ``nss``
  (its cell holds fewer candidates than ``nss``);
* f - a round in which one region rejects nothing and another rejects something.

(A region that loses every stamp through rejection does not exist for ks >= 0: the limit ``m + ks s`` is at least the
clipped mean, which is at least the smallest merit, so the stamp with the smallest merit always stays - DESIGN.md.)

Margin: in every round no merit lies within 1e-6 (relative) of the rejection limit and none within 1e-6 of a 3-sigma
boundary of ``clipped_moments``.  This is a condition on the inputs: with it a GPU fit that picks other stamps cannot
be excused as a tie.  The C port (oracle/cport/zm_hotpants.c), which sums in another order, must find the same counts
on every scene and the same chi2 to 1e-6.
"""
import numpy as np
import pytest

import hp_scenes as hs
from oracle import cport

EXPECT = hs.EXPECT
MIN_ROUNDS = {'wide': 3, 'ko0': 4, 'ko4': 4, 'ko5': 4, 'bgo2': 4}        # what the GPU cases of these scenes ask for

_runs = {}


def oracle_run(name):
    """One traced oracle run per case, shared by the tests of this module and left unchanged."""
    if name not in _runs:
        _runs[name] = hs.run_oracle(hs.case_data(name), **hs.case_kw(name))
    return _runs[name]


def rejected_set(info):
    return {(ri, rec['round'], si) for ri, tr in enumerate(info['traces']) for rec in (tr or [])[1:]
            for si in rec['rejected']}


def test_every_case_is_listed():
    assert set(EXPECT) == set(hs.CASES)


@pytest.mark.parametrize('name', list(hs.CASES))
def test_scene_reaches_its_branch_with_margin(name):
    _, _, info = oracle_run(name)
    kw = hs.case_kw(name)
    assert hs.summary(info) == EXPECT[name]
    reach = hs.branches(info['traces'], kw.get('nss', 3))
    assert hs.CASES[name]['reach'] <= reach, (sorted(hs.CASES[name]['reach']), sorted(reach))
    assert 'e' not in reach
    assert max(r[0] for r in EXPECT[name]) >= MIN_ROUNDS.get(name, 1)
    assert hs.margin(info['traces'], kw.get('ks', 2.0)) > 1e-6


def test_the_branches_are_all_reached_by_some_scene():
    reach = set().union(*(c['reach'] for c in hs.CASES.values()))
    assert reach == {'a', 'b', 'c', 'd_nss', 'd_short', 'f'}


def test_trace_changes_no_result_and_describes_the_rounds():
    from oracle import hotpants as ohp
    sci, srms, ref, rrms, bpm = hs.case_data('step-nss3')
    kw = hs.case_kw('step-nss3')
    d0, n0, i0 = ohp.subtract(sci, ref, srms, rrms, bpm, **kw)
    d1, n1, i1 = oracle_run('step-nss3')
    assert 'traces' not in i0 and i0['regions'] == i1['regions'] and i0['nmasked'] == i1['nmasked']
    assert np.array_equal(d0, d1) and np.array_equal(n0, n1)
    for reg, tr in zip(i1['regions'], i1['traces']):
        cands, recs = tr[0]['cands'], tr[1:]
        assert len(recs) == reg['niter'] and recs[-1]['live'] == reg['fitted']
        assert float(np.mean(recs[-1]['merits'])) == reg['chi2']
        for rec in recs:
            assert [cands[si][a] for si, a in zip(rec['live'], rec['active'])] == rec['centres']
            assert rec['rejected'] == [si for si, m in zip(rec['live'], rec['merits']) if m > rec['limit']]
            assert len(rec['clips']) == 3 and len(rec['vbar']) == len(rec['live'])


def test_ft_values_select_different_stamps():
    a, b = EXPECT['ft5'], EXPECT['ft200']
    assert [r[1] for r in a] != [r[1] for r in b]


def test_the_noise_maps_decide_who_is_rejected():
    """vbar spans more than an order of magnitude between the stamps of the stepped scene, and the stamps it rejects
    are not those of the same scene under constant maps."""
    _, _, step = oracle_run('step-nss3')
    _, _, flat = oracle_run('batch-5')
    vb = [v for tr in step['traces'] for v in tr[1]['vbar']]
    assert max(vb) > 10.0 * min(vb)
    assert len({round(v, 9) for tr in flat['traces'] for v in tr[1]['vbar']}) == 1
    assert rejected_set(step) != rejected_set(flat)
    # ... and under the varying maps without a step every stamp has a vbar of its own
    _, _, var = oracle_run('noise-clean')
    vb = [v for tr in var['traces'] for v in tr[1]['vbar']]
    assert len({round(v, 9) for v in vb}) == len(vb)


def test_batch_jobs_need_different_numbers_of_rounds():
    rounds = [max(r[0] for r in EXPECT[n]) for n in ('batch-1', 'batch-5', 'tr5-nss3')]
    assert rounds == [1, 5, 8]


@pytest.fixture(scope='module')
def c():
    return cport.load()


@pytest.mark.parametrize('name', list(hs.CASES))
def test_c_port_agrees_on_the_rejection_scenes(c, name):
    """The counts equal, chi2 to the 1e-6 of test_oracle_cport.py (measured: 3.5e-9 at most)."""
    sci, srms, ref, rrms, bpm = hs.case_data(name)
    d0, n0, i0 = oracle_run(name)
    d1, n1, i1 = c.hotpants(sci, ref, srms, rrms, bpm, **hs.case_kw(name))
    assert np.array_equal(d0 == 1e-30, d1 == 1e-30) and i0['nmasked'] == i1['nmasked']
    for a, b in zip(i0['regions'], i1['regions']):
        assert a is not None and b is not None
        for k in ('nstamps_total', 'nstamps_used', 'niter', 'ncoeff'):
            assert a[k] == b[k], k
        assert b['kernel_sum'] == pytest.approx(a['kernel_sum'], rel=1e-8)
        assert b['chi2'] == pytest.approx(a['chi2'], rel=1e-6)
