"""Every instance of the convolution (hp_apply.hip) against the oracle, on scenes that can tell the taps apart.

hp_apply.hip compiles 40 instances: ``k_hp_apply<HWK>`` (the tile form) and ``k_hp_apply_w<HWK>`` (the wave form, with
``k_hp_kbasis`` and ``k_hp_ktable``) for kernel half widths 1 .. 20, each with a geometry of its own (lanes per block
row, pixels per lane, blocks per workgroup, tile pitch).  ``ZM_APPLY_FORM`` forces either form at every half width
while the kernel has at most 15 spatial terms.  The scenes are those of tests/conv_scenes.py: a kernel and a template
variance without symmetry, of which tests/test_conv_scenes.py shows that mirrored, transposed or shifted taps move
most pixels of both products.

Every comparison is ``test_subtract_gpu.compare``, unchanged: fill pattern, ``nmasked`` and the fit summary exactly,
``diff`` to 1e-5 (|I| + |I - D|) + 1e-4, ``noise`` to 2e-5 relative plus 1e-5.  The oracle's answer to a scene is
computed once (conv_scenes) and handed to ``compare`` in place of a run of its own; the stand-in refuses any other
input than the scene it was computed for.
"""
import numpy as np
import pytest

import conv_scenes as cs
import hp_scenes
from oracle import hotpants as ohp
from test_subtract_gpu import compare

pytestmark = pytest.mark.gpu

FORMS = ('wave', 'tile')
SUMMARY = ('status', 'nstamps_total', 'nstamps_used', 'niter', 'ncoeff', 'kernel_sum', 'chi2', 'nmasked')


def default_form(hwk):
    """launch_apply's rule at ko <= 4: the wave form where a block fills at least 60 % of a wave's lanes and columns
    and the half width is at least 4."""
    step = 2 * hwk + 1
    lpr = max(64 // step, 1)
    r = -(-step // lpr)
    eff = (100 * step * lpr // 64) * step // (lpr * r)
    return 'wave' if eff >= 60 and hwk >= 4 else 'tile'


def test_the_dispatch_rule_by_half_width():
    wave = [h for h in range(1, 21) if default_form(h) == 'wave']
    assert wave == list(range(4, 16)) + [19, 20]


def against(monkeypatch, data, kw, answer):
    """``compare`` reads the oracle through ``ohp.subtract``: give it the answer computed before."""
    sci, srms, ref, rrms, bpm = data

    def cached(a, b, c, d, e, **k):
        assert a is sci and b is ref and c is srms and d is rrms and e is bpm and k == kw
        return answer
    monkeypatch.setattr(ohp, 'subtract', cached)


_runs = {}


def gpu_run(engine, monkeypatch, hwk, form):
    """The products of ``case(hwk)`` under ``ZM_APPLY_FORM=form`` (None: unset), computed once."""
    if (hwk, form) not in _runs:
        data, kw = cs.case(hwk)
        if form is None:
            monkeypatch.delenv('ZM_APPLY_FORM', raising=False)
        else:
            monkeypatch.setenv('ZM_APPLY_FORM', form)
        _runs[hwk, form] = engine.subtract(*data, **kw)
    return _runs[hwk, form]


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('hwk', range(1, 21))
def test_every_instance_against_the_oracle(engine, monkeypatch, hwk, form):
    data, kw = cs.case(hwk)
    got = gpu_run(engine, monkeypatch, hwk, form)
    against(monkeypatch, data, kw, cs.oracle(hwk))
    compare(engine, data, got=got, **kw)


@pytest.mark.parametrize('hwk', [3, 8, 17, 19])
def test_the_default_form_is_the_one_the_rule_predicts(engine, monkeypatch, hwk):
    """No variable set: bit for bit the forced run of tile, wave, tile, wave - and not the other form's."""
    assert default_form(hwk) == dict([(3, 'tile'), (8, 'wave'), (17, 'tile'), (19, 'wave')])[hwk]
    d, n, info = gpu_run(engine, monkeypatch, hwk, None)
    fd, fn, finfo = gpu_run(engine, monkeypatch, hwk, default_form(hwk))
    assert np.array_equal(d, fd) and np.array_equal(n, fn) and info == finfo


def test_more_than_15_spatial_terms_fall_back_to_the_tile_form(engine, monkeypatch):
    """ko = 5 (21 spatial terms) at half width 8, where the wave form is the default: the register path of
    ``k_hp_ktable`` holds 15, so the default run and both settings of the variable are the tile instance (held to the
    oracle above) - the same bits in both products, the same summary."""
    data = cs.asymmetric(640, 600, seed=58, nstars=600)
    kw = cs.settings(8, nsx=6, nsy=6, nrx=1, nry=1, ko=5, bgo=0)
    monkeypatch.delenv('ZM_APPLY_FORM', raising=False)
    d0, n0, i0 = engine.subtract(*data, **kw)
    assert i0['status'] == 0 and i0['ncoeff'] == 1 + 48 * 21 + 1 and i0['nstamps_used'] >= 21
    assert (d0 != np.float32(1e-30)).mean() > 0.6
    for form in FORMS:
        monkeypatch.setenv('ZM_APPLY_FORM', form)
        d, n, i = engine.subtract(*data, **kw)
        assert np.array_equal(d, d0) and np.array_equal(n, n0), form
        assert i == i0, form


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('layout', cs.LAYOUTS)
@pytest.mark.parametrize('hwk', [2, 8, 12])
def test_ragged_and_exact_blocks(engine, monkeypatch, hwk, layout, form):
    """Region widths and heights of residue 0, 1 and STEP - 1 modulo the block (tests/test_conv_scenes.py asserts
    them); 'thirds' has a last column and row of regions larger than the others."""
    data, kw = cs.ragged(hwk, layout)
    monkeypatch.setenv('ZM_APPLY_FORM', form)
    got = engine.subtract(*data, **kw)
    against(monkeypatch, data, kw, cs.ragged_oracle(hwk, layout))
    compare(engine, data, got=got, **kw)


@pytest.mark.parametrize('form', FORMS)
def test_nonfinite_template_noise_counts_as_zero_variance(engine, monkeypatch, form):
    data, kw = cs.nonfinite(6)
    monkeypatch.setenv('ZM_APPLY_FORM', form)
    got = engine.subtract(*data, **kw)
    assert np.isfinite(got[1]).all()
    against(monkeypatch, data, kw, cs.nonfinite_oracle(6))
    compare(engine, data, got=got, **kw)


@pytest.mark.parametrize('form', FORMS)
def test_normalised_to_the_template(engine, monkeypatch, form):
    data, kw = cs.case(6)
    kw = dict(kw, normalize=1)
    monkeypatch.setenv('ZM_APPLY_FORM', form)
    got = engine.subtract(*data, **kw)
    against(monkeypatch, data, kw, cs.normalized_oracle(6))
    compare(engine, data, got=got, **kw)


@pytest.mark.parametrize('name', ['basis-8-0', 'basis-limit'])
def test_other_bases_through_the_tile_form(engine, monkeypatch, name):
    """9 and 7 distinct 1-D filters instead of 7 (and 64 rows at the limit): the tile form sizes its evaluation
    scratch in LDS by them.  Half width 5 runs the wave form by default."""
    monkeypatch.setenv('ZM_APPLY_FORM', 'tile')
    compare(engine, hp_scenes.case_data(name), **hp_scenes.case_kw(name))
