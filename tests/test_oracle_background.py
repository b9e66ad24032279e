"""Known-answer tests of the background oracle (no GPU)."""
import numpy as np
from scipy.interpolate import CubicSpline

from oracle import background as oback


def test_natural_spline_matches_scipy():
    rng = np.random.default_rng(1)
    nodes = rng.normal(100, 3, (7, 5))
    up = oback.expand(nodes, 5 * 32, 7 * 32, 32)
    # reference: natural cubic splines along y then x through the mesh centres
    yc = (np.arange(7) + 0.5) * 32 - 0.5
    xc = (np.arange(5) + 0.5) * 32 - 0.5
    rows = CubicSpline(yc, nodes, axis=0, bc_type='natural', extrapolate=True)(np.arange(7 * 32))
    ref = CubicSpline(xc, rows, axis=1, bc_type='natural', extrapolate=True)(np.arange(5 * 32))
    np.testing.assert_allclose(up, ref, rtol=0, atol=1e-9)


def test_flat_noise_field_recovers_level_and_sigma():
    rng = np.random.default_rng(2)
    img = rng.normal(150.0, 5.0, (512, 512))
    bkg, rms, mean, sig, bo, so = oback.background(img, None, 128)
    assert abs(mean - 150.0) < 0.1 and abs(sig - 5.0) < 0.1
    assert np.abs(bkg - 150.0).max() < 0.5
    assert np.abs(rms - 5.0).max() < 0.3


def test_stars_do_not_bias_the_mode():
    rng = np.random.default_rng(3)
    img = rng.normal(100.0, 4.0, (256, 256))
    img[rng.uniform(size=img.shape) < 0.05] += rng.uniform(20, 2000)   # 5 % bright pixels
    _, _, mean, sig, _, _ = oback.background(img, None, 128)
    assert abs(mean - 100.0) < 0.5 and abs(sig - 4.0) < 0.5


def test_masked_mesh_is_filled():
    rng = np.random.default_rng(4)
    img = rng.normal(50.0, 2.0, (384, 384))
    w = np.ones_like(img)
    w[128:256, 128:256] = 0
    back, sigm = oback.mesh_maps(img, w, 128)
    assert back[1, 1] == -oback.BIG
    bo, so = oback.filter_maps(back, sigm, 3)
    assert abs(bo[1, 1] - 50.0) < 0.5


def test_histogram_median_merge_path_equals_sequential_walk():
    # host-side check of the search the kernel uses in place of backguess's walk
    rng = np.random.default_rng(0)
    for trial in range(300):
        n = int(rng.integers(1, 200))
        h = rng.integers(0, 6, n) * (rng.uniform(size=n) < 0.7)
        lcut = int(rng.integers(0, n))
        hcut = int(rng.integers(lcut, n))
        ref = oback.histogram_median_walk(h, lcut, hcut)
        P = np.concatenate([[0], np.cumsum(h)])   # P[i+1] = inclusive prefix at i
        p0 = lambda i: 0 if i < 0 else int(P[i + 1])
        T = hcut - lcut + 1
        lo, hi = 0, T
        while lo < hi:
            a = (lo + hi + 1) >> 1
            La = p0(lcut + a - 2) - p0(lcut - 1)
            Hb = p0(hcut) - p0(hcut - (T - a))
            if La < Hb:
                lo = a
            else:
                hi = a - 1
        a, b = lo, T - lo
        lowsum = p0(lcut + a - 1) - p0(lcut - 1)
        highsum = p0(hcut) - p0(hcut - b)
        ihigh, ilow = hcut - b, lcut + a
        if ihigh >= 0:
            den = 2.0 * max(int(h[ilow]), int(h[ihigh]))
            med = ihigh + 0.5 + ((highsum - lowsum) / den if den > 0 else 0.0)
        else:
            med = 0.0
        assert med == ref, (trial, med, ref)


def narrowing_median(h, lcut, hcut):
    """Host emulation of the search in ``backguess_wave`` (csrc/background.hip): 64 candidates per round, one per
    lane, ``step = (span + 63) >> 6``, the count of leading trues, and the same ``lo`` / ``hi`` updates."""
    P = np.concatenate([[0], np.cumsum(h)])       # P[i + 1] = inclusive prefix at i
    p0 = lambda i: 0 if i < 0 else int(P[i + 1])
    T = hcut - lcut + 1
    base_lo, top = p0(lcut - 1), p0(hcut)
    lo, hi = 0, T
    rounds = 0
    while hi > lo:
        rounds += 1
        assert rounds <= 64
        span = hi - lo
        step = (span + 63) >> 6
        oks = []
        for lane in range(64):
            a = lo + (lane + 1) * step
            ok = False
            if a <= hi:
                La = p0(lcut + a - 2) - base_lo
                Hb = top - p0(hcut - (T - a))
                ok = La < Hb
            oks.append(ok)
        k = sum(oks)
        assert all(oks[:k]) and not any(oks[k:])      # the ballot is k leading trues: the predicate is monotone
        nlo = lo + k * step
        nhi = lo + (k + 1) * step - 1
        lo = nlo if nlo < hi else hi
        hi = nhi if nhi < hi else hi
        if lo > hi:
            hi = lo
    a, b = lo, T - lo
    lowsum = p0(lcut + a - 1) - base_lo
    highsum = top - p0(hcut - b)
    ihigh, ilow = hcut - b, lcut + a
    if ihigh < 0:
        return 0.0
    ha = int(h[ilow]) if ilow < len(h) else 0          # the oracle's guard; the kernel's prefix array has 4096 entries
    den = 2.0 * max(ha, int(h[ihigh]))
    return ihigh + 0.5 + ((highsum - lowsum) / den if den > 0 else 0.0)


def test_64_ary_narrowing_loop_equals_sequential_walk():
    """The loop the kernel runs, not its binary-search restatement: on full and on sparse histograms (long runs of
    lowsum == highsum ties), all-zero windows and single-bin windows, lengths 1 .. 4096, cuts over the whole range."""
    rng = np.random.default_rng(7)
    lengths = [1, 2, 3, 63, 64, 65, 127, 128, 129, 4095, 4096]
    cases = 0
    for empty in (0.0, 0.5, 0.9, 0.99):
        for trial in range(560):
            n = lengths[trial] if trial < len(lengths) else int(np.exp(rng.uniform(0, np.log(4096.999))))
            h = rng.integers(1, 40, n) * (rng.uniform(size=n) >= empty)
            kind = trial % 7
            lcut = int(rng.integers(0, n))
            hcut = int(rng.integers(lcut, n))
            if kind == 0:
                lcut, hcut = 0, n - 1                 # the first iteration's window
            elif kind == 1:
                hcut = lcut                           # a single bin
            elif kind == 2:
                h[lcut:hcut + 1] = 0                  # nothing inside the window
            assert narrowing_median(h, lcut, hcut) == oback.histogram_median_walk(h, lcut, hcut), \
                (empty, trial, n, lcut, hcut)
            cases += 1
    assert cases >= 2000


# ---- the branch census (oracle.background trace hook) and the scenes of tests/mesh_scenes.py -----------------------
import pytest                      # noqa: E402

import mesh_scenes as ms           # noqa: E402


def test_trace_changes_no_result():
    for name, ((nx, ny), mesh) in (('crowded', ms.GEOMETRIES[2]), ('poisson3', ms.GEOMETRIES[0]),
                                   ('nearly_constant', ms.GEOMETRIES[3]), ('constant_42.1_nan', ms.GEOMETRIES[5])):
        img, wgt, c = ms.scene(name, nx, ny, mesh)
        t = {}
        a = oback.mesh_maps(img.astype(np.float64), wgt, mesh)
        b = oback.mesh_maps(img.astype(np.float64), wgt, mesh, trace=t)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        n = t['meshes']
        assert n == a[0].size and t.get('bad', 0) + t.get('mode', 0) + t.get('median', 0) + t.get('sig0', 0) == n
        assert len(t['iterations']) == len(t['empty_bin_share']) == n - t.get('bad', 0)
    img, wgt, mesh, nbad = ms.good_fraction('ragged', 'weight0', True)
    t = {}
    a = oback.mesh_maps(img.astype(np.float64), wgt.astype(np.float64), mesh)
    b = oback.mesh_maps(img.astype(np.float64), wgt.astype(np.float64), mesh, trace=t)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and t['bad'] == nbad == (a[0] == -oback.BIG).sum()


@pytest.mark.parametrize('name', list(ms.SCENES))
def test_scene_takes_the_branch_it_is_there_for(name):
    for (nx, ny), mesh in ms.GEOMETRIES:
        _, _, c = ms.scene(name, nx, ny, mesh)
        assert ms.census_ok(name, c, mesh), (name, nx, ny, mesh, {k: v for k, v in c.items() if not isinstance(v, list)})


@pytest.mark.parametrize('where,how,short', ms.GOOD_FRACTION_CASES)
def test_good_fraction_pairs_sit_on_the_boundary(where, how, short):
    img, wgt, mesh, nbad = ms.good_fraction(where, how, short)
    assert ms.census(img, wgt, mesh)['bad'] == nbad
    if how == 'tiny':
        # the same answer whether the float32 plane or its float64 copy is handed over
        t = {}
        oback.mesh_maps(img.astype(np.float64), wgt, mesh, trace=t)
        assert t.get('bad', 0) == nbad


def test_oracle_commutes_with_powers_of_two():
    img, _, _ = ms.scene('crowded', 512, 512, 64)
    b0, r0, m0, s0, _, _ = oback.background(img.astype(np.float64), None, 64)
    for s in (2.0 ** -30, 2.0 ** 20):
        b, r, m, sg, _, _ = oback.background((img * np.float32(s)).astype(np.float64), None, 64)
        assert np.array_equal(b, s * b0) and np.array_equal(r, s * r0) and m == s * m0 and sg == s * s0
