"""What tests/seeing_scenes.py says about its scenes, asserted from oracle/detect.py on the CPU, and the proof that the
scenes can fail: restatements of the star finder and of the moments with one slip each (a window short of a pixel or a
row, swapped centroid axes, a wrapping window; a wrong tie rule, a wrong comparison at ``hi``, box corners left out)
differ from the oracle on at least one scene - by 100 x the tolerance of tests/test_seeing_gpu.py where the output is
a float, in the list itself where it is one.  The slips are made in a copy of the logic here, never in ``oracle/``."""
import functools

import numpy as np
import pytest

import seeing_scenes as ss
from oracle import detect as odet


@functools.lru_cache(maxsize=None)
def moments(name):
    return ss.MOMENTS[name]()


@functools.lru_cache(maxsize=None)
def traces(name):
    sc = moments(name)
    with np.errstate(all='ignore'):
        return tuple(ss.trace(sc.img, int(x), int(y), sc.half) for x, y in zip(sc.x, sc.y))


@functools.lru_cache(maxsize=None)
def oracle_moments(name):
    sc = moments(name)
    with np.errstate(all='ignore'):
        return np.array([odet.star_fwhm(sc.img, int(x), int(y), sc.half) for x, y in zip(sc.x, sc.y)], np.float64)


@functools.lru_cache(maxsize=None)
def oracle_stars(name, with_map):
    sc = ss.FINDER[name]()
    with np.errstate(invalid='ignore'):
        stars, n = odet.find_stars(sc.img, sc.bad if with_map else None, sc.lo, sc.hi, sc.iso, sc.border, nmax=10 ** 6)
    assert n == len(stars)
    return [(int(x), int(y), float(v)) for x, y, v in stars]


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


# ------------------------------------------------------------------------------------------------- the moments scenes
@pytest.mark.parametrize('name', list(ss.MOMENTS))
def test_the_trace_is_the_oracle_and_the_preconditions_hold(name):
    sc = moments(name)
    ny, nx = sc.img.shape
    assert sc.img.dtype == np.float32 and nx != ny and max(nx, ny) <= 520
    assert np.abs(sc.x).max() <= 10 ** 6 and np.abs(sc.y).max() <= 10 ** 6 and sc.x.dtype == sc.y.dtype == np.int32
    ref = oracle_moments(name)
    nfinite = 0
    for k, t in enumerate(traces(name)):
        where = f'{name} star {k} at ({sc.x[k]}, {sc.y[k]})'
        assert same([t.fwhm, t.cx, t.cy], ref[k]), where
        assert ss.stop_round_is_safe(t), (where, t.steps)
        assert ss.exit_is_safe(t), (where, t.exit, t.margin)
        assert ss.is_tame(t), (where, t.steps)
        if np.isfinite(t.fwhm):
            nfinite += 1
            assert t.fwhm >= 1.4, where                     # (nothing collapses: the chaotic regime returns 1e-13)
            if name in ss.WINDOW_SCENES:
                assert t.corner >= 1e-3, (where, t.corner)
    print(f'{name}: {len(ref)} stars, {nfinite} finite; exits {sorted({t.exit for t in traces(name)})}; '
          f'rounds {min(t.rounds for t in traces(name))} .. {max(t.rounds for t in traces(name))}')


def test_every_exit_and_the_cap_are_taken():
    got = tuple(t.exit for t in traces('exits'))
    assert got == ss.EXITS_WANT
    t = traces('exits')
    assert t[7].rounds == 25 and t[9].rounds == 25          # the criterion met in the last round; the cap itself
    assert t[8].rounds == 3 and np.isfinite(t[8].fwhm)      # the width of round 2 is kept
    assert all(np.isnan(t[k].fwhm) for k in range(7))
    assert (t[0].cx, t[0].cy) == (15.0, 15.0) and (t[1].cx, t[1].cy) == (45.0, 16.0)
    assert abs(t[3].cx - 1.0) < 1e-9 and abs(t[3].cy - 15.0) < 1e-9
    assert np.isnan(t[6].cx) and np.isnan(t[6].cy)
    # windows without a pixel: NaN, and the centroid is the start pixel
    sc, tr = moments('stars-outside'), traces('stars-outside')
    far = [k for k in range(len(sc.x)) if abs(int(sc.x[k])) == 10 ** 6 or abs(int(sc.y[k])) == 10 ** 6]
    assert len(far) == 6
    for k in far:
        assert np.isnan(tr[k].fwhm) and (tr[k].cx, tr[k].cy) == (float(sc.x[k]), float(sc.y[k])) and tr[k].exit == 's0'


def test_known_answers_of_the_constant_frame():
    """The window alone decides: 4.186 for the whole 5 x 5 window, 9.242 for the 11 x 11 corner of the 21 x 21 one."""
    assert traces('flat-half2')[0].fwhm == pytest.approx(4.186, abs=5e-4)
    assert traces('flat-half10')[5].fwhm == pytest.approx(9.242, abs=5e-4)
    assert abs(traces('flat-half10')[5].cx - 5.0) < 1e-5 and abs(traces('flat-half10')[5].cy - 5.0) < 1e-5
    # the well-sampled stars come back as planted
    for k, (cx, cy, _, fwhm) in enumerate(ss.INTERIOR):
        t = traces('stars-interior')[k]
        assert abs(t.fwhm / fwhm - 1) < 0.02 and abs(t.cx - cx) < 0.05 and abs(t.cy - cy) < 0.05


# -------------------------------------------------------------------------------------------------- the finder scenes
def test_the_finder_scenes_hold_what_they_say():
    xy = lambda name, m=True: sorted((x, y) for x, y, _ in oracle_stars(name, m))      # noqa: E731
    assert xy('rules') == ss.RULES_WANT
    assert xy('poison') == ss.POISON_WANT and xy('poison', False) == ss.POISON_WANT_NOMAP
    assert len(xy('cap')) == 40 and len({v for _, _, v in oracle_stars('cap', True)}) == 40
    assert (1, 1) in xy('iso1-border1', False) and (1, 1) not in xy('iso1-border1')
    assert {(24, 1), (1, 20), (24, 20), (6, 10), (11, 10), (6, 14), (12, 14), (16, 6), (15, 10), (17, 10)} \
        == set(xy('iso1-border1'))
    assert {(3, 3), (22, 3), (3, 18), (22, 18)} <= set(xy('iso1-border3')) and len(xy('iso1-border3')) == 11
    assert xy('iso32-border32') == [(32, 167), (70, 120), (103, 153), (132, 92), (197, 32)]
    assert xy('iso32-border32', False) == sorted(xy('iso32-border32') + [(32, 32), (197, 167)])
    assert xy('iso32-border40') == [(40, 40), (40, 159), (70, 120), (103, 153), (132, 92), (189, 40), (189, 159)]
    assert xy('seam-255') == []
    assert xy('seam-256') == [(254, 2), (254, 23)]
    assert xy('seam-257') == [(254, 2), (254, 23), (255, 5), (255, 26)]
    assert xy('seam-513') == [(254, 2), (254, 23), (255, 5), (255, 26), (256, 8), (256, 29), (257, 11), (510, 14),
                              (511, 17), (511, 32)]
    for name in ss.FINDER:
        if name.startswith('tiny'):
            sc = ss.FINDER[name]()
            ny, nx = sc.img.shape
            one = nx == 2 * sc.border + 1 and ny == 2 * sc.border + 1
            assert xy(name) == ([(sc.border, sc.border)] if one else []), name
    for name, f in ss.FINDER.items():
        sc = f()
        assert max(sc.img.shape) <= 520 and sc.img.dtype == np.float32
        fin = sc.img[np.isfinite(sc.img)]
        whole = fin == np.round(fin)
        assert whole.all() if name != 'rules' else (~whole).sum() == 2


def test_the_end_to_end_fields():
    img, bad, saturate = ss.lattice_field()
    yy, xx = np.mgrid[:260, :260]
    sub = img - (150.0 + 0.05 * xx + 0.03 * yy).astype(np.float32)
    stars, n = odet.find_stars(sub, bad, 90.0, 0.5 * saturate - 170.0, nmax=10 ** 6)
    assert n == 356 > 300                                    # 361 less four under the bad block and the blob
    assert len({v for _, _, v in stars}) == n
    assert abs(odet.seeing(sub, bad, 90.0, 0.5 * saturate - 170.0) / ss.TRUTH - 1) < 0.03
    for equal in (False, True):
        f = ss.sparse_field(equal) - np.float32(100.0)
        stars, n = odet.find_stars(f, None, 60.0, 3e38, nmax=10 ** 6)
        peaks = np.array([v for _, _, v in stars])
        assert n == 30
        assert (np.abs(peaks - 5500.0) < 20.0).all() if equal else (np.diff(np.sort(peaks)) > 0).all()


# ------------------------------------------------------------------------------------------------------- sensitivity
def star_fwhm_with(slip, img, x, y, half=10, maxit=25):
    """The moments as the kernel walks them - element e of the (2 half + 1)^2 window is pixel (x - half + e % side,
    y - half + e // side), kept when it is inside the frame - with one slip: 'pixel' (the last element is never
    reached), 'row' (the last row), 'swap' (cx and cy change places on output), 'wrap' (an index outside the frame
    wraps round instead of being skipped), or None."""
    img = np.asarray(img, dtype=np.float64)
    ny, nx = img.shape
    side = 2 * half + 1
    e = np.arange(side * side - (1 if slip == 'pixel' else side if slip == 'row' else 0))
    jj, ii = y - half + e // side, x - half + e % side
    if slip == 'wrap':
        I = img[jj % ny, ii % nx]
    else:
        keep = (ii >= 0) & (ii < nx) & (jj >= 0) & (jj < ny)
        jj, ii = jj[keep], ii[keep]
        I = img[jj, ii]
    cx, cy, s2 = float(x), float(y), 4.0
    out = np.nan
    with np.errstate(all='ignore'):
        for _ in range(maxit):
            w = np.exp(-0.5 * ((ii - cx) ** 2 + (jj - cy) ** 2) / s2) * I
            s0 = w.sum()
            if not s0 > 0:
                break
            cx, cy = (w * ii).sum() / s0, (w * jj).sum() / s0
            w = np.exp(-0.5 * ((ii - cx) ** 2 + (jj - cy) ** 2) / s2) * I
            t0 = w.sum()
            if not t0 > 0:
                break
            m2 = 0.5 * ((w * (ii - cx) ** 2).sum() + (w * (jj - cy) ** 2).sum()) / t0
            if not m2 > 0:
                break
            inv = 1.0 / m2 - 1.0 / s2
            if not inv > 0:
                break
            ns2 = 1.0 / inv
            done = abs(ns2 - s2) <= 1e-8 * ns2
            s2 = ns2
            out = ss.K_FWHM * np.sqrt(s2)
            if done:
                break
    return (out, cy, cx) if slip == 'swap' else (out, cx, cy)


def moments_differ(got, ref, factor):
    """Whether any of (fwhm, cx, cy) is off by more than ``factor`` x the tolerance, or NaN where the other is not."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if (np.isnan(got) != np.isnan(ref)).any():
        return True
    with np.errstate(invalid='ignore'):
        d = np.abs(got - ref)
    tol = factor * np.array([ss.RTOL_FW * abs(ref[0]), ss.ATOL_C, ss.ATOL_C])
    return bool((d > tol).any())


def test_the_moments_scenes_tell_a_wrong_window_from_the_right_one():
    kills = {slip: [] for slip in ('pixel', 'row', 'swap', 'wrap')}
    for name in ss.MOMENTS:
        sc, ref = moments(name), oracle_moments(name)
        for slip in (None,) + tuple(kills):
            got = [star_fwhm_with(slip, sc.img, int(x), int(y), sc.half) for x, y in zip(sc.x, sc.y)]
            hit = [k for k in range(len(got)) if moments_differ(got[k], ref[k], 1 if slip is None else 100)]
            if slip is None:
                assert not hit, (name, hit)          # the restatement itself is within the tolerance of the oracle
            elif hit:
                kills[slip].append(f'{name} ({len(hit)} of {len(got)} stars)')
    for slip, where in kills.items():
        print(f'{slip:>5}: {", ".join(where) or "survives"}')
    assert all(kills.values()), kills
    # the extent of the window shows where the scenes were built for it
    assert any(w.startswith('flat-half2 ') for w in kills['pixel']) and any(w.startswith('broad-half64') for w in kills['row'])
    assert any(w.startswith('stars-clipped') for w in kills['wrap'])


def find_stars_with(slip, img, bad, lo, hi, iso, border):
    """The star finder pixel by pixel with one slip: 'tie' (> where >= belongs: an earlier equal pixel no longer
    hides a later one), 'hi' (<= where < belongs), 'corner' (the four corners of the box are not looked at), or None."""
    img = np.asarray(img, dtype=np.float32)
    ny, nx = img.shape
    out = []
    with np.errstate(invalid='ignore'):
        for y in range(border, ny - border):
            for x in range(border, nx - border):
                v = img[y, x]
                if not v > lo or not (v <= hi if slip == 'hi' else v < hi):
                    continue
                ok = True
                for dy in range(-iso, iso + 1):
                    for dx in range(-iso, iso + 1):
                        if slip == 'corner' and abs(dx) == iso and abs(dy) == iso:
                            continue
                        n = img[y + dy, x + dx]
                        if n != n or (bad is not None and bad[y + dy, x + dx]):
                            ok = False
                        elif (dx or dy):
                            earlier = dy < 0 or (dy == 0 and dx < 0)
                            if (n > v if slip == 'tie' else n >= v) if earlier else n > v:
                                ok = False
                        if not ok:
                            break
                    if not ok:
                        break
                if ok:
                    out.append((x, y, float(v)))
    out.sort(key=lambda t: (-t[2], t[1], t[0]))
    return out


def test_the_finder_scenes_tell_a_wrong_rule_from_the_right_one():
    kills = {slip: [] for slip in ('tie', 'hi', 'corner')}
    for name, f in ss.FINDER.items():
        sc = f()
        for with_map in ((True, False) if sc.bad is not None else (False,)):
            ref = oracle_stars(name, with_map)
            for slip in (None,) + tuple(kills):
                got = find_stars_with(slip, sc.img, sc.bad if with_map else None, sc.lo, sc.hi, sc.iso, sc.border)
                if slip is None:
                    assert got == ref, name
                elif got != ref:
                    kills[slip].append(name + ('' if with_map or sc.bad is None else ' without its map'))
    for slip, where in kills.items():
        print(f'{slip:>6}: {", ".join(where) or "survives"}')
    assert all(kills.values()), kills
    assert 'rules' in kills['tie'] and 'rules' in kills['hi'] and 'rules' in kills['corner'] and 'poison' in kills['corner']
    assert any(w.startswith('seam') for w in kills['tie']) and 'iso32-border32' in kills['corner']
