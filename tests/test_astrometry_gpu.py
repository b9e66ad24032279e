"""zm_astrom_solve / zm_astrom_solve_dev (csrc/astrometry.hip) against the restatement tests/astrom_ref.py on the
smallest scenes that can break them (tests/astrom_scenes.py).

Every scene keeps its distance from the decisions that hang on a comparison of reals: no separation within 1e-3 (relative)
of the cross-id radius, no chi2 within 1e-6 of the clip bound, no offset within 1e-9 of the edge of a vote bin or of the
window - asserted by ``astrom_scenes.reference``.  Under that rule the discrete results are compared exactly: ``match``,
``used``, ``status``, ``nmatch``, ``nused``, ``rounds``, ``vote_peak``, ``vote_runner_up``, and ``shift`` (the same fp64
expression of the same integers) to the bit.

The solved header and ``rms`` have a tolerance, TOL = 2^-30 arcsec (9.3e-10), measured, not chosen:
tests/measure_astrom_tolerance.py solves the last fit of every scene here with mpmath at 50 digits, with the restatement
and with fp64 normal equations (what the kernel does).  Seen through the test's own measure - the largest sky separation
on a 9 x 9 grid of pixels, evaluated in fp64 - the normal equations are off by at most 2.04e-10 arcsec from the 50-digit
header (the restatement by the same 2.04e-10: at this level the measure is dominated by the rounding of a right ascension
of up to 360 degrees, 2e-10 arcsec per ulp, not by the solve) and by 2.4e-11 arcsec in ``rms``.  4 x 2.04e-10 = 8.2e-10,
rounded up to a power of two: 2^-30.  ``chi2`` is held to what that bound lets it move (``chi2_bound``).  The kernel's
largest deviation on these scenes, measured on an MI355X: 2.04e-10 arcsec in the header, 5.6e-12 in ``rms``.
("Astrometric refit".)"""
import ctypes as C
import importlib

import numpy as np
import pytest

import astrom_ref as am
import astrom_scenes as sc

pytestmark = pytest.mark.gpu
TOL = 2.0 ** -30                                            # arcsec; see the docstring
EXPECTED = dict(empty='AMBIGUOUS', exactly_enough='OK', one_too_few='TOO_FEW', rows_65='OK', rows_300='OK',
                stars_far_away='OK', shift_inside_window='OK', two_equal_peaks='AMBIGUOUS', across_ra_zero='OK',
                near_the_pole='OK', duplicate_stars='OK', nonfinite_rows='OK', a_row_returns='OK', vote_skipped='OK',
                top_of_the_list='OK', fine_bins='OK', one_round='NOT_CONVERGED', singular='SINGULAR')


def scamp():
    return importlib.import_module('zuds-pipeline_amd.scamp')


def product_wcs(w):
    pkg = importlib.import_module('zuds-pipeline_amd')
    return pkg.WCS(w.crpix, w.crval, w.cd, w.pv1 if w.has_pv else None, w.pv2 if w.has_pv else None, w.naxis)


def oracle_wcs(w):
    from util import to_oracle_wcs
    return to_oracle_wcs(w)


_solved = {}


def solved(engine, name):
    """The host entry point on a scene, once per session."""
    if name not in _solved:
        (wcs_list, dets, ref, params), _ = sc.reference(name)
        _solved[name] = scamp().solve([product_wcs(w) for w in wcs_list], dets, ref, engine=engine, **params)
    return _solved[name]


def weight_sum(w0, det, ref, want):
    """Sum of the weights of the rows the last fit used (arcsec^-2)."""
    rows = np.flatnonzero(want['used'] != 0)
    if rows.size == 0:
        return 0.0
    pixscale = 3600.0 * np.sqrt(abs(np.linalg.det(np.asarray(w0.cd).reshape(2, 2))))
    sd, sig = np.asarray(det[2], np.float64)[rows], np.asarray(ref[2], np.float64)[want['match'][rows]]
    return float(np.sum(1.0 / ((sd * pixscale) ** 2 + sig ** 2)))


def chi2_bound(chi2, wsum, nused):
    """What TOL allows ``chi2 = sum w (r1^2 + r2^2)`` to move.  Two headers within TOL of each other on the grid give
    every row residuals within d = TOL of each other per axis, so with Cauchy-Schwarz
    |sum w ((r + e)^2 - r^2)| <= 2 sqrt(sum w r^2) sqrt(sum w e^2) + sum w e^2 <= 2 sqrt(chi2) sqrt(2 W d^2) + 2 W d^2
    (W: the sum of the weights of the rows used); the sum itself is rounded nused + 2 times in another order."""
    return 2.0 * np.sqrt(2.0 * chi2 * wsum) * TOL + 2.0 * wsum * TOL ** 2 + (nused + 2) * 2.0 ** -52 * chi2


def compare(got_w, got_i, want, wsum=0.0):
    assert got_i['status'] == am.STATUS[want['status']]
    for k in ('nmatch', 'nused', 'rounds', 'vote_peak', 'vote_runner_up'):
        assert got_i[k] == want[k], k
    assert np.float64(got_i['shift'][0]).tobytes() == np.float64(want['shift'][0]).tobytes()
    assert np.float64(got_i['shift'][1]).tobytes() == np.float64(want['shift'][1]).tobytes()
    assert got_i['match'].dtype == np.int32 and np.array_equal(got_i['match'], want['match'])
    assert got_i['used'].dtype == np.uint8 and np.array_equal(got_i['used'], want['used'])
    sep = am.grid_separation(oracle_wcs(got_w), want['wcs'])
    drms = max(abs(got_i['rms'][0] - want['rms'][0]), abs(got_i['rms'][1] - want['rms'][1]))
    print(f'grid separation {sep:.3e} arcsec, rms difference {drms:.3e} arcsec (bound {TOL:.3e})')
    assert sep <= TOL and drms <= TOL
    if want['status'] in (am.OK, am.NOT_CONVERGED):
        assert got_w.has_pv and np.array_equal(got_w.cd, want['wcs'].cd) and np.array_equal(got_w.crpix, want['wcs'].crpix)
        bound = chi2_bound(want['chi2'], wsum, want['nused'])
        print(f"chi2 {want['chi2']:.6e}: difference {abs(got_i['chi2'] - want['chi2']):.3e} (bound {bound:.3e})")
        assert abs(got_i['chi2'] - want['chi2']) <= bound


@pytest.mark.parametrize('name', sorted(sc.SCENES))
def test_scene_against_the_restatement(engine, name):
    (wcs_list, dets, ref, _), want = sc.reference(name)
    got_w, got_i = solved(engine, name)
    assert len(got_w) == len(want)
    for w, i, r, w0, det in zip(got_w, got_i, want, wcs_list, dets):
        compare(w, i, r, weight_sum(w0, det, ref, r))
    if name in EXPECTED:
        assert got_i[0]['status'] == EXPECTED[name]


def test_the_scenes_show_what_they_are_for(engine):
    """The properties the scenes were built for, read from the GPU's answers."""
    _, i = solved(engine, 'batch_of_three')
    assert [v['status'] for v in i] == ['OK', 'AMBIGUOUS', 'OK'] and [v['match'].size for v in i] == [70, 0, 130]
    _, i = solved(engine, 'shift_outside_window')
    assert i[0]['status'] != 'OK'
    _, i = solved(engine, 'shift_inside_window')
    assert -60.0 < i[0]['shift'][0] < -58.0
    _, i = solved(engine, 'two_equal_peaks')
    assert i[0]['vote_peak'] == i[0]['vote_runner_up'] == 30
    _, i = solved(engine, 'duplicate_stars')
    assert i[0]['match'].max() < 40                          # the copies sit at 40 .. 43 and are never chosen
    _, i = solved(engine, 'nonfinite_rows')
    assert (i[0]['match'][[4, 9, 17, 23, 30]] == -1).all() and not np.isin(i[0]['match'], [5, 6]).any()
    for name in ('rows_65', 'rows_300'):
        _, i = solved(engine, name)
        assert i[0]['nmatch'] - i[0]['nused'] == 5           # the planted outliers, and only they
    _, want = sc.reference('a_row_returns')
    assert want[0]['returned'] >= 1
    _, i = solved(engine, 'a_row_returns')
    assert i[0]['nmatch'] - i[0]['nused'] == 1
    _, i = solved(engine, 'top_of_the_list')
    assert i[0]['vote_peak'] < 48 < i[0]['nmatch']
    w, i = solved(engine, 'degree1_tan')
    assert not w[0].pv1[4:].any() and w[0].pv1[3] == 0.0
    w, i = solved(engine, 'one_round')                      # NOT_CONVERGED returns the last solution, not the header it was given
    assert i[0]['rounds'] == 1 and w[0].has_pv and w[0].pv1[0] != 0.0 and i[0]['rms'][0] > 0.0
    (wl, _, _, _), _ = sc.reference('singular')
    w, i = solved(engine, 'singular')                       # SINGULAR leaves the header as it was given
    assert i[0]['nmatch'] == i[0]['nused'] == 8 and not w[0].has_pv and np.array_equal(w[0].cd, wl[0].cd)
    _, i = solved(engine, 'fine_bins')
    assert i[0]['vote_peak'] == 150                         # every detection voted, whichever piece it came through LDS in
    _, i = solved(engine, 'empty')
    assert i[0]['rounds'] == 0 and i[0]['match'].size == 0


@pytest.mark.parametrize('name', ['rows_300', 'batch_of_three', 'degree3_tpv'])
def test_same_bits_twice_and_from_device_arrays(engine, name):
    import torch
    (wcs_list, dets, ref, params), _ = sc.reference(name)
    wl = [product_wcs(w) for w in wcs_list]
    w1, i1 = solved(engine, name)
    w2, i2 = scamp().solve(wl, dets, ref, engine=engine, **params)
    dev = torch.device('cuda', 0)
    cols = [torch.from_numpy(np.concatenate([np.asarray(d[k], np.float64) for d in dets])).to(dev) for k in range(4)]
    offsets = np.concatenate([[0], np.cumsum([np.asarray(d[0]).size for d in dets])]).astype(np.int32)
    rd = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev) for v in ref]
    w3, i3 = scamp().solve_dev(wl, offsets, *cols, *rd, engine=engine, **params)
    torch.cuda.synchronize()
    for wa, ia, others in zip(w1, i1, zip(zip(w2, i2), zip(w3, i3))):
        for wb, ib in others:
            for k in ('crpix', 'crval', 'cd', 'pv1', 'pv2'):
                assert np.asarray(getattr(wa, k)).tobytes() == np.asarray(getattr(wb, k)).tobytes(), k
            for k in ('status', 'nmatch', 'nused', 'rounds', 'vote_peak', 'vote_runner_up'):
                assert ia[k] == ib[k], k
            for k in ('shift', 'rms'):
                assert np.asarray(ia[k]).tobytes() == np.asarray(ib[k]).tobytes(), k
            assert np.float64(ia['chi2']).tobytes() == np.float64(ib['chi2']).tobytes()
            mb, ub = (ib[k].cpu().numpy() if hasattr(ib[k], 'cpu') else ib[k] for k in ('match', 'used'))
            assert np.array_equal(ia['match'], mb) and np.array_equal(ia['used'], ub)


def test_bad_arguments(engine):
    lib = importlib.import_module('zuds-pipeline_amd._lib')
    (wcs_list, dets, ref, _), _ = sc.reference('exactly_enough')
    wl = [product_wcs(w) for w in wcs_list]
    for bad in (dict(degree=0), dict(degree=4), dict(match_resol=-1.0), dict(crossid_radius=0.0, match_resol=0.0),
                dict(position_maxerr=60.0, match_resol=0.5), dict(crossid_radius=0.1)):
        with pytest.raises(lib.ZMError):
            scamp().solve(wl, dets, ref, engine=engine, **bad)
    # through the C ABI: a negative count and offsets that do not ascend
    L = engine.L
    p = scamp().astrom_params()
    w0 = (lib.zm_wcs * 2)(lib.wcs_struct(wl[0]), lib.wcs_struct(wl[0]))
    res = (lib.zm_astrom_result * 2)()
    x = np.zeros(8)
    match, used = np.zeros(8, np.int32), np.zeros(8, np.uint8)
    star = np.zeros(1)

    def call(nframes, offsets, m):
        off = np.asarray(offsets, np.int32)
        return L.zm_astrom_solve(engine.ctx, nframes, w0, off.ctypes.data, x.ctypes.data, x.ctypes.data, x.ctypes.data,
                                 x.ctypes.data, m, star.ctypes.data, star.ctypes.data, star.ctypes.data, C.byref(p), res,
                                 match.ctypes.data, used.ctypes.data)

    assert call(-1, [0, 4, 8], 1) != 0 and b'nframes' in L.zm_last_error()
    assert call(2, [0, 4, 8], -1) != 0
    assert call(2, [0, 6, 4], 1) != 0 and b'ascend' in L.zm_last_error()
    assert call(2, [-1, 4, 8], 1) != 0
    assert call(0, [0], 1) == 0
