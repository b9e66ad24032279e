"""The seeing estimate on the GPU - ``k_find_stars``, ``k_star_fwhm`` (``csrc/detect.hip``), both routes of
``seeing.py`` - and the host route of the dipole cut (``k_negpix``), on the scenes of tests/seeing_scenes.py against
``oracle/detect.py``.  tests/test_seeing_scenes.py shows on the CPU that these comparisons can fail.

Tolerances.  Star lists, peaks and every route-to-route comparison: exact.  Moments: ``fw`` relative, ``cx`` / ``cy``
absolute, against the float64 oracle.  ``python tests/measure_seeing_tolerance.py`` evaluates the same iteration at 50
digits (mpmath) on every moments scene; the oracle's own error is at most

    FWHM 2.69e-15 relative (stars-clipped),  centroid 8.89e-13 px (exits: the centroid sent 99 px away)

(stars-interior 1.45e-15 / 8.80e-15, stars-outside 1.12e-15 / 8.83e-14, flat-half2|3|10 below 3.9e-16 / 1.1e-14,
broad-half31|32|64 below 2.9e-16 / 3.1e-14).  8 x the largest, rounded up to one digit, is ``seeing_scenes.RTOL_FW`` =
3e-14 and ``ATOL_C`` = 8e-12, far below the suite's ceilings of rtol 1e-9 and atol 1e-8 (tests/test_detect_gpu.py),
so the scenes are held to the former.  Either figure stands only because no star of a scene has a step of its
iteration within 1 % of the 1e-8 at which it stops (tests/seeing_scenes.py): one round more or less is 2.5e-9.
``abs(seeing / truth - 1) < 0.03`` is DESIGN.md's "+-3 % on synthetic fields".

Nothing here depends on which thread wins the atomic in ``k_find_stars``: lists are compared sorted, the overflow
test asks for membership."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import cuts_ref as cref
import seeing_scenes as ss
from oracle import detect as odet
from util import pkg

pytestmark = pytest.mark.gpu
CANARY = -7


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


@contextlib.contextmanager
def on_a_stream(engine):
    """The engine bound to a torch stream that is current, as ``measure_seeing_dev`` asks of its caller."""
    import torch
    stream = torch.cuda.Stream('cuda:0')
    engine.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            yield stream
        stream.synchronize()
    finally:
        engine.set_stream(0)


@functools.lru_cache(maxsize=None)
def finder(name):
    return ss.FINDER[name]()


@functools.lru_cache(maxsize=None)
def moments(name):
    return ss.MOMENTS[name]()


@functools.lru_cache(maxsize=None)
def oracle_stars(name, with_map):
    sc = finder(name)
    with np.errstate(invalid='ignore'):
        stars, n = odet.find_stars(sc.img, sc.bad if with_map else None, sc.lo, sc.hi, sc.iso, sc.border, nmax=10 ** 6)
    assert n == len(stars)
    return tuple((int(x), int(y), np.float32(v).view(np.uint32).item()) for x, y, v in stars)


@functools.lru_cache(maxsize=None)
def oracle_moments(name):
    sc = moments(name)
    with np.errstate(all='ignore'):
        ref = np.array([odet.star_fwhm(sc.img, int(x), int(y), sc.half) for x, y in zip(sc.x, sc.y)], np.float64)
    ref.setflags(write=False)
    return ref


def raw_find(engine, img, bad, lo, hi, iso, border, max_out, device=False, room=64):
    """The C entry point itself: (rc, n, xs, ys, pk) with ``max_out + room`` entries that start as the canary."""
    ny, nx = img.shape
    size = max(max_out, 0) + room
    xs, ys, pk = np.full(size, CANARY, np.int32), np.full(size, CANARY, np.int32), np.full(size, CANARY, np.float32)
    n = C.c_int(CANARY)
    b8 = None if bad is None else np.ascontiguousarray(bad).astype(np.uint8)
    if device:
        import torch
        d_img, d_bad = dev(img), (None if b8 is None else dev(b8))
        torch.cuda.synchronize()
        rc = engine.L.zm_find_stars_dev(engine.ctx, d_img.data_ptr(), None if d_bad is None else d_bad.data_ptr(), nx, ny,
                                        lo, hi, iso, border, max_out, xs.ctypes.data, ys.ctypes.data, pk.ctypes.data,
                                        C.byref(n))
    else:
        rc = engine.L.zm_find_stars(engine.ctx, img.ctypes.data, None if b8 is None else b8.ctypes.data, nx, ny, lo, hi,
                                    iso, border, max_out, xs.ctypes.data, ys.ctypes.data, pk.ctypes.data, C.byref(n))
    return rc, n.value, xs, ys, pk


def sorted_stars(n, xs, ys, pk):
    order = np.lexsort((xs[:n], ys[:n], -pk[:n].astype(np.float64)))
    return tuple((int(xs[k]), int(ys[k]), pk[k].view(np.uint32).item()) for k in order)


def raw_moments(engine, img, x, y, half, device=False):
    """(rc, fw, cx, cy): outputs start as the canary."""
    ny, nx = img.shape
    k = len(x)
    x, y = np.ascontiguousarray(x, np.int32), np.ascontiguousarray(y, np.int32)
    fw, cx, cy = np.full(k + 1, float(CANARY)), np.full(k + 1, float(CANARY)), np.full(k + 1, float(CANARY))
    if device:
        import torch
        d_img = dev(img)
        torch.cuda.synchronize()
        rc = engine.L.zm_star_fwhm_dev(engine.ctx, d_img.data_ptr(), nx, ny, k, x.ctypes.data, y.ctypes.data, half,
                                       fw.ctypes.data, cx.ctypes.data, cy.ctypes.data)
    else:
        rc = engine.L.zm_star_fwhm(engine.ctx, img.ctypes.data, nx, ny, k, x.ctypes.data, y.ctypes.data, half,
                                   fw.ctypes.data, cx.ctypes.data, cy.ctypes.data)
    assert fw[k] == cx[k] == cy[k] == CANARY                 # nothing is written past the last star
    return rc, fw[:k], cx[:k], cy[:k]


def worst_errors(fw, cx, cy, ref):
    """(largest relative error of fw, largest absolute error of cx / cy) over the entries that are finite in the
    oracle; the NaN pattern must be the oracle's."""
    got = np.stack([fw, cx, cy], axis=1)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (np.argwhere(np.isnan(got) != np.isnan(ref)).tolist())
    with np.errstate(invalid='ignore'):
        e_fw = np.nanmax(np.abs(fw - ref[:, 0]) / np.abs(ref[:, 0]), initial=0.0)
        e_c = max(np.nanmax(np.abs(cx - ref[:, 1]), initial=0.0), np.nanmax(np.abs(cy - ref[:, 2]), initial=0.0))
    return float(e_fw), float(e_c)


# ---------------------------------------------------------------------------------------------------- the star finder
@pytest.mark.parametrize('name', list(ss.FINDER))
def test_star_list_equals_the_oracles_on_every_finder_scene(engine, name):
    z = pkg()
    sc = finder(name)
    for with_map in ((True, False) if sc.bad is not None else (False,)):
        want = oracle_stars(name, with_map)
        for device in (False, True):
            rc, n, xs, ys, pk = raw_find(engine, sc.img, sc.bad if with_map else None, sc.lo, sc.hi, sc.iso, sc.border,
                                         4096, device)
            z._lib.check(rc, 'zm_find_stars')
            print(f'{name}, map {with_map}, device planes {device}: {n} stars, the oracle {len(want)}')
            assert n == len(want)
            assert sorted_stars(n, xs, ys, pk) == want       # x, y and the bits of the peak
            assert (xs[n:] == CANARY).all() and (ys[n:] == CANARY).all() and (pk[n:] == CANARY).all()


@pytest.mark.parametrize('max_out', [1, 39, 40, 41])
def test_a_full_list_reports_its_true_length_and_writes_no_further(engine, max_out):
    z = pkg()
    sc = finder('cap')
    want = {(x, y): p for x, y, p in oracle_stars('cap', False)}
    assert len(want) == 40
    for device in (False, True):
        rc, n, xs, ys, pk = raw_find(engine, sc.img, None, sc.lo, sc.hi, sc.iso, sc.border, max_out, device)
        z._lib.check(rc, 'zm_find_stars')
        m = min(max_out, 40)
        got = [(int(xs[k]), int(ys[k])) for k in range(m)]
        print(f'max_out {max_out}, device planes {device}: out_n {n}, {len(set(got))} distinct entries of {m}')
        assert n == 40
        assert len(set(got)) == m and all(g in want for g in got)
        assert all(pk[k].view(np.uint32).item() == want[got[k]] for k in range(m))
        assert (xs[m:] == CANARY).all() and (ys[m:] == CANARY).all() and (pk[m:] == CANARY).all()


def test_the_finder_refuses_what_it_cannot_do(engine):
    z = pkg()
    sc = finder('cap')
    for iso, border, max_out, msg in ((0, 12, 64, 'border >= isolation >= 1'), (33, 40, 64, 'border >= isolation >= 1'),
                                      (5, 4, 64, 'border >= isolation >= 1'), (5, 12, 0, 'bad sizes')):
        for device in (False, True):
            rc, n, xs, ys, pk = raw_find(engine, sc.img, None, sc.lo, sc.hi, iso, border, max_out, device)
            assert rc != 0 and n == CANARY and (xs == CANARY).all()
            with pytest.raises(z.ZMError, match=msg):
                z._lib.check(rc, 'zm_find_stars')
    ny, nx = sc.img.shape
    xs, ys, pk, n = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(64, np.float32), C.c_int(0)
    for args in ((None, ys.ctypes.data, pk.ctypes.data, C.byref(n)), (xs.ctypes.data, None, pk.ctypes.data, C.byref(n)),
                 (xs.ctypes.data, ys.ctypes.data, None, C.byref(n)), (xs.ctypes.data, ys.ctypes.data, pk.ctypes.data, None)):
        rc = engine.L.zm_find_stars(engine.ctx, sc.img.ctypes.data, None, nx, ny, sc.lo, sc.hi, 5, 12, 64, *args)
        with pytest.raises(z.ZMError, match='null argument'):
            z._lib.check(rc, 'zm_find_stars')


# -------------------------------------------------------------------------------------------------------- the moments
@pytest.mark.parametrize('name', list(ss.MOMENTS))
def test_moments_equal_the_oracles_on_every_moments_scene(engine, name):
    z = pkg()
    sc = moments(name)
    ref = oracle_moments(name)
    rc, fw, cx, cy = raw_moments(engine, sc.img, sc.x, sc.y, sc.half)
    z._lib.check(rc, 'zm_star_fwhm')
    e_fw, e_c = worst_errors(fw, cx, cy, ref)
    print(f'{name}: {len(fw)} stars, {int(np.isfinite(fw).sum())} finite; fw off by {e_fw:.2e} relative '
          f'(tolerance {ss.RTOL_FW:.0e}), cx / cy by {e_c:.2e} px (tolerance {ss.ATOL_C:.0e})')
    assert e_fw <= ss.RTOL_FW and e_c <= ss.ATOL_C
    rc, fw_d, cx_d, cy_d = raw_moments(engine, sc.img, sc.x, sc.y, sc.half, device=True)
    z._lib.check(rc, 'zm_star_fwhm_dev')
    for a, b in ((fw, fw_d), (cx, cx_d), (cy, cy_d)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize('nstar', [0, 1, 65])
def test_moments_of_no_star_one_star_and_more_than_a_wave_of_them(engine, nstar):
    z = pkg()
    sc = moments('stars-clipped')
    pick = np.arange(nstar) % len(sc.x)
    ref = oracle_moments('stars-clipped')[pick]
    for device in (False, True):
        rc, fw, cx, cy = raw_moments(engine, sc.img, sc.x[pick], sc.y[pick], sc.half, device)
        z._lib.check(rc, 'zm_star_fwhm')
        e_fw, e_c = worst_errors(fw, cx, cy, ref.reshape(nstar, 3))
        print(f'nstar {nstar}, device plane {device}: fw off by {e_fw:.2e} (tolerance {ss.RTOL_FW:.0e}), '
              f'cx / cy by {e_c:.2e} px (tolerance {ss.ATOL_C:.0e})')
        assert e_fw <= ss.RTOL_FW and e_c <= ss.ATOL_C


@pytest.mark.parametrize('half', [1, 65])
def test_a_window_the_kernel_is_not_built_for_is_refused(engine, half):
    z = pkg()
    sc = moments('stars-interior')
    for device in (False, True):
        rc, fw, cx, cy = raw_moments(engine, sc.img, sc.x, sc.y, half, device)
        assert rc != 0 and (fw == CANARY).all()
        with pytest.raises(z.ZMError, match='zm_star_fwhm: bad sizes'):
            z._lib.check(rc, 'zm_star_fwhm')


# --------------------------------------------------------------------------------------------------------- the routes
def both_routes(engine, img, bad, saturate):
    """((seeing, nused), stars handed to the moments) of ``measure_seeing`` and of ``measure_seeing_dev``."""
    z = pkg()
    out = []
    for name, device in (('zm_star_fwhm', False), ('zm_star_fwhm_dev', True)):
        real, seen = getattr(engine.L, name), []

        def spy(ctx, img_, nx, ny, k, x, y, *rest, real=real, seen=seen):
            seen.append((np.ctypeslib.as_array(C.cast(x, C.POINTER(C.c_int32)), (k,)).copy(),
                         np.ctypeslib.as_array(C.cast(y, C.POINTER(C.c_int32)), (k,)).copy()))
            return real(ctx, img_, nx, ny, k, x, y, *rest)
        setattr(engine.L, name, spy)
        try:
            if device:
                with on_a_stream(engine):
                    got = z.seeing.measure_seeing_dev(dev(img), None if bad is None else dev(bad.astype(np.uint8)),
                                                      saturate, engine=engine)
            else:
                got = z.seeing.measure_seeing(img, bad, saturate, engine=engine)
        finally:
            setattr(engine.L, name, real)
        assert len(seen) == 1
        out.append((got, seen[0]))
    return out


def oracle_route(engine, img, bad, saturate, cap=None):
    """The oracle's stars and seeing on the background-subtracted plane the engine returns, with the thresholds of
    ``measure_seeing``; ``cap``: the threshold doubles while the oracle counts more stars than that.
    Returns (seeing, finite count, [(x, y)] of the stars used, lo)."""
    z = pkg()
    wgt = None if bad is None else np.where(bad, 0.0, 1.0).astype(np.float32)
    _, _, sub, (bmean, bsig) = engine.background(img, wgt, want=('sub',))
    lo = float(z.seeing.NSIGMA * max(bsig, 1e-6))
    hi = float(0.5 * saturate - bmean) if saturate else 3.0e38
    while True:
        stars, n = odet.find_stars(sub, bad, np.float32(lo), np.float32(hi), z.seeing.ISOLATION, z.seeing.BORDER,
                                   z.seeing.NMAX)
        if cap is None or n <= cap:
            break
        lo *= 2.0
    with np.errstate(all='ignore'):
        fw = np.array([odet.star_fwhm(sub, int(x), int(y), z.seeing.HALF)[0] for x, y, _ in stars])
    return float(np.nanmedian(fw)), int(np.isfinite(fw).sum()), [(int(x), int(y)) for x, y, _ in stars], lo


@pytest.mark.parametrize('masked', [True, False])
def test_both_routes_use_the_oracles_300_brightest_and_agree_to_the_bit(engine, masked):
    img, bad, saturate = ss.lattice_field()
    if not masked:
        bad, saturate = None, None
    (host, host_stars), (devr, dev_stars) = both_routes(engine, img, bad, saturate)
    want, nfinite, stars, _ = oracle_route(engine, img, bad, saturate)
    err = abs(host[0] / want - 1)
    print(f'masked {masked}: seeing {host[0]!r} from {host[1]} stars (device planes: {devr[0]!r} from {devr[1]}); the '
          f'oracle {want!r} from {nfinite} of {len(stars)}: off by {err:.2e} (tolerance {ss.RTOL_FW:.0e}); '
          f'truth {ss.TRUTH}: off by {abs(host[0] / ss.TRUTH - 1):.2e} (tolerance 0.03)')
    assert host == devr and isinstance(host[0], float)                    # the same float, the same count
    assert np.array_equal(host_stars[0], dev_stars[0]) and np.array_equal(host_stars[1], dev_stars[1])
    assert len(stars) == 300 and list(zip(host_stars[0].tolist(), host_stars[1].tolist())) == stars
    assert host[1] == nfinite <= 300
    assert err <= ss.RTOL_FW
    assert abs(host[0] / ss.TRUTH - 1) < 0.03


def test_a_full_list_doubles_the_threshold_until_it_fits(engine, monkeypatch):
    z = pkg()
    monkeypatch.setattr(z.seeing, 'CAP', 8)
    img = ss.sparse_field()
    want, nfinite, stars, lo = oracle_route(engine, img, None, None, cap=8)
    assert 0 < len(stars) <= 8
    (host, host_stars), (devr, dev_stars) = both_routes(engine, img, None, None)
    err = abs(host[0] / want - 1)
    print(f'CAP 8: the threshold ends at {lo:.6g} with {len(stars)} stars; seeing {host[0]!r}, the oracle {want!r}: off '
          f'by {err:.2e} (tolerance {ss.RTOL_FW:.0e})')
    assert host == devr and host[1] == nfinite
    assert list(zip(host_stars[0].tolist(), host_stars[1].tolist())) == stars
    assert list(zip(dev_stars[0].tolist(), dev_stars[1].tolist())) == stars
    assert err <= ss.RTOL_FW
    # stars of one height: no threshold keeps some of them, the loop ends with none - and says so
    flat = ss.sparse_field(equal=True)
    with pytest.raises(RuntimeError, match='Unable to find any stars'):
        z.seeing.measure_seeing(flat, engine=engine)
    with on_a_stream(engine):
        with pytest.raises(RuntimeError, match='Unable to find any stars'):
            z.seeing.measure_seeing_dev(dev(flat), engine=engine)


# --------------------------------------------------------------------------------- the host route of the dipole cut
def host_negpix(engine, img, x, y, med, sig):
    z = pkg()
    ny, nx = img.shape
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    out = np.full(x.size + 1, CANARY, np.int32)
    z._lib.check(engine.L.zm_negpix_test(engine.ctx, img.ctypes.data, nx, ny, x.size, x.ctypes.data, y.ctypes.data,
                                         float(med), float(sig), out.ctypes.data), 'zm_negpix_test')
    assert out[-1] == CANARY
    return out[:-1]


def test_host_dipole_route_on_positions_that_are_not_finite_or_far_outside(engine):
    """The list of tests/test_candidate_cuts_gpu.py::test_positions_that_are_not_finite_or_far_outside and more of its
    kind, with a dipole in the frame's corner - where a NaN converted to 0 would look - and one at the in-frame row."""
    z = pkg()
    img, rms, mask, _, _ = cref.field(cref.SEEDS[1])
    img = img.copy()
    ny, nx = img.shape
    img[1, 1], img[1, 2] = -70.0, 80.0
    img[49, 49], img[49, 50] = -70.0, 80.0
    img[ny - 2, nx - 2], img[ny - 2, nx - 3] = -70.0, 80.0
    nan, inf = np.nan, np.inf
    x = np.array([nan, 30.0, inf, -inf, 1e300, -1e300, 3e9, -3e9, 1e5, 40.0, nx + 7.0, -6.6, 50.0,
                  nan, nan, 2.0, inf, -inf, 2.0, 2.0 ** 31, -2.0 ** 31, 2.0 ** 32 + 2, 2.0 ** 63, 2.0, nx - 1.0])
    y = np.array([30.0, nan, 30.0, 30.0, 30.0, 30.0, 30.0, -3e9, 1e5, 1e18, 30.0, 30.0, 50.0,
                  nan, 2.0, nan, 2.0, 2.0, inf, 2.0, 2.0, 2.0 ** 32 + 2, 2.0, 2.0, ny - 1.0])
    want = cref.candidate_cuts(img, rms, mask, x, y, z.BAD_SUM)
    assert want['NEGPIX'].tolist() == [0] * 12 + [1] + [0] * 10 + [1, 1]
    assert np.array_equal(odet.negpix(img, x, y, want['IMMED'], want['IMSIG']), want['NEGPIX'])
    import torch
    d = [dev(img), dev(rms), dev(mask.astype(np.int32))]
    torch.cuda.synchronize()
    device = z.pixel_cuts_dev(engine, d[0], d[1], d[2], x, y, bad_bits=z.BAD_SUM)
    immed, immad = engine.median_mad(img)
    raw = host_negpix(engine, img, x, y, immed, 1.48 * (immad / 1.4826))
    host = z.pixel_cuts(img, rms, (mask & z.BAD_SUM) != 0, x, y, engine=engine)
    print(f'NEGPIX of {x.size} positions: zm_negpix_test {raw.tolist()}, pixel_cuts {host["NEGPIX"].tolist()}, '
          f'device route {device["NEGPIX"].tolist()}')
    assert np.array_equal(raw, want['NEGPIX'])
    assert np.array_equal(host['NEGPIX'], want['NEGPIX'])
    assert np.array_equal(device['NEGPIX'], want['NEGPIX'])
    assert raw[12] == 1 and raw[-1] == 1 and raw[-2] == 1


def test_host_dipole_route_compares_strictly_at_five_sigma(engine):
    """(v - med) / sig in float32 against -5 and +5: a pixel at exactly 5 sigma is no hit, one float32 spacing beyond
    is.  med and sig are powers of two, so that the quotient is the planted number."""
    f = np.float32
    for med, sig in ((0.0, 1.0), (2.0, 4.0), (-8.0, 0.5)):
        at = (f(med) - f(5) * f(sig), f(med) + f(5) * f(sig))
        past = (np.nextafter(at[0], f(-np.inf)), np.nextafter(at[1], f(np.inf)))
        img = np.full((40, 56), med, np.float32)
        cases = ((at[0], at[1]), (past[0], at[1]), (at[0], past[1]), (past[0], past[1]))
        x, y = [], []
        for k, (lo, hi) in enumerate(cases):
            img[20, 8 + 13 * k], img[20, 9 + 13 * k] = lo, hi
            x.append(9.0 + 13 * k)                              # 1-based: the negative pixel itself
            y.append(21.0)
        got = host_negpix(engine, img, x, y, med, sig)
        want = odet.negpix(img, x, y, med, sig)
        print(f'med {med}, sig {sig}: at / at, past / at, at / past, past / past -> {got.tolist()}')
        assert want.tolist() == [0, 0, 0, 1] and np.array_equal(got, want)
