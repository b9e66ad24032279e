"""The restatement of the masked second pass (tests/mask_ref.py) against closed forms, on the CPU.

The scene is a float32 image that is exactly point-symmetric about the pixel (20, 18) (a Gaussian plus noise, averaged
with its own point reflection), an object centred on that pixel, and foreign blocks painted into the map by hand.  Every
committed scene of tests/mask_scenes.py also passes the census the GPU tests start with.
"""
import numpy as np
import pytest

import mask_ref as kr
import mask_scenes as ms
import measure_ref as mr

NX, NY, CX, CY = 41, 37, 20, 18
OBJ = dict(number=1, xc=float(CX), yc=float(CY), x2=2.3, y2=1.9, xy=0.2, fwhm=3.6, a=1.6, b=1.3, theta=20.0)
RADIUS = 3.0


def symmetric():
    yy, xx = np.mgrid[0:NY, 0:NX].astype(np.float64)
    g = 400.0 * np.exp(-0.5 * ((xx - CX) ** 2 / 2.4 + (yy - CY) ** 2 / 2.0 + 0.1 * (xx - CX) * (yy - CY)))
    n = np.random.default_rng(3).normal(0.0, 0.5, (NY, NX))
    img = (g + n).astype(np.float32)
    img = ((img.astype(np.float64) + img[::-1, ::-1]) / 2.0).astype(np.float32)
    assert np.array_equal(img, img[::-1, ::-1])
    return img, np.ones((NY, NX), np.float32)


def own_map():
    yy, xx = np.mgrid[0:NY, 0:NX]
    return (np.hypot(xx - CX, yy - CY) < 3.2).astype(np.int32)


def painted(cells, label=2, add=50.0):
    """(image, map) with the pixels ``cells`` (j, i) given to another object and made brighter."""
    img, sigma = symmetric()
    seg = own_map()
    for j, i in cells:
        seg[j, i] = label
        img[j, i] += add
    return img, sigma, seg


BLOCK = [(j, i) for j in range(16, 20) for i in range(22, 25)]          # right of the centre; mirrors: columns 16 .. 18


def in_kron(o, R, cells):
    D = o['x2'] * o['y2'] - o['xy'] ** 2
    oo = dict(o, cxx=o['y2'] / D, cyy=o['x2'] / D, cxy=-2.0 * o['xy'] / D)
    return [c for c in cells if mr._r2(oo, float(c[1]), float(c[0])) <= R * R]


def touches(cx, cy, r, cells):
    """The cells whose square reaches inside the circle (a positive overlap)."""
    return [c for c in cells if np.hypot(max(abs(c[1] - cx) - 0.5, 0.0), max(abs(c[0] - cy) - 0.5, 0.0)) < r]


def plain(img, sigma, reverse=False, **kw):
    b = np.zeros(img.shape, bool)
    out = dict(mr.kron(img, sigma, b, OBJ, reverse=reverse, **kw))
    out.update(mr.window(img, sigma, b, OBJ, reverse=reverse))
    return out


def masked(img, sigma, seg, typ, reverse=False, bad=None, **kw):
    return kr.measure(img, sigma, bad, seg, [OBJ], typ, aper_radius=RADIUS, reverse=reverse, **kw)[0]


@pytest.mark.parametrize('reverse', [False, True])
def test_correct_on_a_symmetric_image_gives_the_bits_of_the_image_without_the_neighbour(reverse):
    clean_img, sigma = symmetric()
    img, _, seg = painted(BLOCK)
    want = plain(clean_img, sigma, reverse)
    aper = kr.aperture(clean_img, sigma, np.zeros(img.shape, bool), own_map(), OBJ, kr.CORRECT, RADIUS, reverse)
    got = masked(img, sigma, seg, kr.CORRECT, reverse)
    for f in ('flux_auto', 'fluxerr_auto', 'kron_radius', 'xwin_image', 'ywin_image', 'x2win', 'y2win', 'xywin', 'niter_win'):
        assert got[f] == want[f], f
    assert got['flux_aper'] == aper['flux_aper'] and got['fluxerr_aper'] == aper['fluxerr_aper']
    # and the neighbour did change the unmasked sums: the equality above is the replacement's doing
    assert plain(img, sigma, reverse)['flux_auto'] > want['flux_auto'] + 100.0
    assert got['nrepl_auto'] == len(in_kron(OBJ, got['kron_radius'], BLOCK)) > 0 and got['nlost_auto'] == 0
    assert got['nrepl_aper'] == len(touches(CX, CY, RADIUS, BLOCK)) > 0 and got['nlost_aper'] == 0
    r = 4.0 * got['sigma_win']
    assert got['nrepl_win'] == len(touches(got['xwin_image'] - 1.0, got['ywin_image'] - 1.0, r, BLOCK)) > 0
    assert got['nlost_win'] == 0
    assert got['npix_auto'] == want['npix_auto'] and got['nskip_auto'] == 0


def test_blank_is_the_unmasked_sum_minus_the_sum_over_the_block():
    img, sigma, seg = painted(BLOCK)
    kw = dict(kron_fact=0.1)                                 # KRON_RADIUS is the floor of 3.5 with and without the block
    res = {}
    for rev in (False, True):
        res[rev] = (plain(img, sigma, rev, **kw), masked(img, sigma, seg, kr.BLANK, rev, **kw),
                    kr.aperture(img, sigma, np.zeros(img.shape, bool), own_map(), OBJ, kr.BLANK, RADIUS, rev))
    p, m, a = res[False]
    assert p['kron_radius'] == m['kron_radius'] == 3.5
    cells = in_kron(OBJ, 3.5, BLOCK)
    block = sum(float(img[j, i]) for j, i in cells)
    order = 10.0 * (abs(p['flux_auto'] - res[True][0]['flux_auto']) + abs(m['flux_auto'] - res[True][1]['flux_auto']))
    assert abs(m['flux_auto'] - (p['flux_auto'] - block)) <= order + 2.0 * kr.EPS * p['absflux']
    assert m['nlost_auto'] == len(cells) > 0 and m['nrepl_auto'] == 0 and m['npix_auto'] == p['npix_auto'] - len(cells)
    assert m['fluxerr_auto'] == np.sqrt(float(m['npix_auto']))            # sigma = 1: an exact sum
    # the aperture: every block pixel times its overlap, taken from the unmasked aperture of the same map
    _, _, _, _, frac = kr._overlap(float(CX), float(CY), RADIUS, NX, NY)
    i0, _, j0, _ = kr._overlap(float(CX), float(CY), RADIUS, NX, NY)[:4]
    tcells = touches(CX, CY, RADIUS, BLOCK)
    part = sum(frac[j - j0, i - i0] * float(img[j, i]) for j, i in tcells)
    order = 10.0 * (abs(a['flux_aper'] - res[True][2]['flux_aper']) + abs(m['flux_aper'] - res[True][1]['flux_aper']))
    total = float((np.abs(frac) * np.abs(img[j0:j0 + frac.shape[0], i0:i0 + frac.shape[1]])).sum())
    assert abs(m['flux_aper'] - (a['flux_aper'] - part)) <= order + 2.0 * kr.EPS * total
    assert m['nlost_aper'] == len(tcells) > 0 and m['nrepl_aper'] == 0 and m['nap'] == a['nap']


def test_a_block_whose_mirror_is_foreign_too_is_lost_and_counted():
    mirror = [(2 * CY - j, 2 * CX - i) for j, i in BLOCK]
    img, sigma, seg = painted(BLOCK + mirror)
    got = masked(img, sigma, seg, kr.CORRECT)
    both = BLOCK + mirror
    assert got['nrepl_auto'] == 0 and got['nlost_auto'] == len(in_kron(OBJ, got['kron_radius'], both)) > 0
    assert got['nrepl_aper'] == 0 and got['nlost_aper'] == len(touches(CX, CY, RADIUS, both)) > 0
    blank = masked(img, sigma, seg, kr.BLANK)
    for f in ('flux_auto', 'flux_aper', 'kron_radius', 'nlost_auto', 'nlost_aper', 'xwin_image', 'ywin_image'):
        assert got[f] == blank[f], f                         # nothing to replace with: CORRECT is BLANK here


def test_a_mirror_off_the_frame_is_lost():
    img, sigma = symmetric()
    o = dict(OBJ, xc=2.0, yc=18.0)                           # 2 px from the left edge: mirrors of columns 5 .. 7 are -1 .. -3
    yy, xx = np.mgrid[0:NY, 0:NX]
    seg = (np.hypot(xx - 2, yy - 18) < 2.5).astype(np.int32)
    cells = [(j, i) for j in range(17, 20) for i in range(5, 8)]
    for j, i in cells:
        seg[j, i] = 2
    bmap = np.zeros(img.shape, bool)
    k = kr.kron(img, sigma, bmap, seg, o, kr.CORRECT)
    a = kr.aperture(img, sigma, bmap, seg, o, kr.CORRECT, 4.0)
    off = [c for c in cells if 2 * 2 - c[1] < 0]
    assert k['nrepl_auto'] == len(in_kron(o, k['kron_radius'], [c for c in cells if c not in off]))
    assert k['nlost_auto'] == len(in_kron(o, k['kron_radius'], off)) > 0
    assert a['nlost_aper'] == len(touches(2, 18, 4.0, off)) > 0
    assert a['nrepl_aper'] == len(touches(2, 18, 4.0, [c for c in cells if c not in off]))
    v, s, lost, how = kr.planes(img, sigma, bmap, seg, 1, 2.0, 18.0, kr.CORRECT)
    assert all(how[j, i] == kr.LOST for j, i in off) and lost.sum() == len(off)
    # a centre that is not finite has no mirror anywhere
    assert (kr.planes(img, sigma, bmap, seg, 1, np.nan, 18.0, kr.CORRECT)[3][seg == 2] == kr.LOST).all()


def ring_cells(n, inner, outer):
    """n pixels in raster order at a distance in [inner, outer) from the centre, all on the right half, so that their
    mirrors are clean."""
    yy, xx = np.mgrid[0:NY, 0:NX]
    d = np.hypot(xx - CX, yy - CY)
    jj, ii = np.nonzero((d >= inner) & (d < outer) & (xx > CX))
    assert len(jj) >= n
    return list(zip(jj[:n].tolist(), ii[:n].tolist()))


@pytest.mark.parametrize('typ', [kr.BLANK, kr.CORRECT])
def test_the_crowded_thresholds_from_both_sides(typ):
    img, sigma = symmetric()
    base = masked(img, sigma, own_map(), typ, kron_fact=0.1)
    ntot, nap = base['npix_auto'], base['nap']
    assert base['crowded'] == 0 and base['flags_auto'] & kr.AUTO_CROWDED == 0
    # Kron: pixels between the aperture and the ellipse's edge; 10 (nrepl + nlost) > npix + nlost = ntot
    o = dict(OBJ)
    yy, xx = np.mgrid[0:NY, 0:NX]
    D = o['x2'] * o['y2'] - o['xy'] ** 2
    r2 = mr._r2(dict(o, cxx=o['y2'] / D, cyy=o['x2'] / D, cxy=-2.0 * o['xy'] / D), xx.astype(float), yy.astype(float))
    far = np.hypot(xx - CX, yy - CY) > RADIUS + 1.0
    jj, ii = np.nonzero((r2 <= 3.5 ** 2) & far & (xx > CX))
    for k, flag in ((ntot // 10, 0), (ntot // 10 + 1, 1)):
        cells = list(zip(jj[:k].tolist(), ii[:k].tolist()))
        assert len(cells) == k
        im, sg, seg = painted(cells)
        got = masked(im, sg, seg, typ, kron_fact=0.1)
        assert got['nrepl_auto'] + got['nlost_auto'] == k and got['npix_auto'] + got['nlost_auto'] == ntot
        assert bool(got['flags_auto'] & kr.AUTO_CROWDED) == bool(flag) == (10 * k > ntot)
        assert got['nrepl_aper'] + got['nlost_aper'] == 0 and got['crowded'] == flag
    # the aperture: 10 (nrepl + nlost) > nap, with the Kron ellipse made wide enough to stay below its own tenth
    inside = ring_cells(nap // 10 + 1, 0.5, RADIUS)          # centres inside the circle: a positive overlap
    for k, flag in ((nap // 10, 0), (nap // 10 + 1, 1)):
        im, sg, seg = painted(inside[:k])
        got = masked(im, sg, seg, typ, kron_fact=0.1, kron_min=6.0)
        assert got['nap'] == nap and got['nrepl_aper'] + got['nlost_aper'] == k
        assert 10 * (got['nrepl_auto'] + got['nlost_auto']) <= got['npix_auto'] + got['nlost_auto']
        assert got['aper_crowded'] == flag == int(10 * k > nap) and got['crowded'] == flag
        assert got['flags_auto'] & kr.AUTO_CROWDED == 0


def test_own_bad_pixels_are_replaced_and_an_unknown_type_is_refused():
    img, sigma = symmetric()
    clean = plain(img, sigma)
    bad = np.zeros(img.shape, np.uint8)
    bad[:, CX + 1] = 1
    img2 = img.copy()
    img2[CY + 1, CX - 2] = np.nan                            # its mirror (CY - 1, CX + 2) is good
    got = masked(img2, sigma, own_map(), kr.CORRECT, bad=bad)
    assert got['flux_auto'] == clean['flux_auto'] and got['nlost_auto'] == 0 and got['nrepl_auto'] > 7
    assert masked(img2, sigma, own_map(), kr.BLANK, bad=bad)['nlost_auto'] == got['nrepl_auto']
    with pytest.raises(ValueError):
        masked(img, sigma, own_map(), 'none')


@pytest.mark.parametrize('typ', [kr.BLANK, kr.CORRECT])
@pytest.mark.parametrize('name', ms.NAMES)
def test_every_committed_scene_passes_the_census(name, typ):
    sc = ms.scene(name)
    rows = kr.measure(sc['img'], sc['sigma'], sc['bad'], sc['seg'], ms.objects(sc['rows']), typ, **sc['kw'])
    kr.census(rows)
    assert len(rows) == len(sc['rows']) >= 1
    if name in ms.CLEAN_SCENES:
        assert all(r[f] == 0 for r in rows for f in ('nrepl_auto', 'nlost_auto', 'nrepl_aper', 'nlost_aper', 'nrepl_win', 'nlost_win'))
    else:
        assert any(r['nlost_auto'] + r['nrepl_auto'] for r in rows)


def test_what_the_scenes_are_there_for():
    c = {n: kr.measure(s['img'], s['sigma'], s['bad'], s['seg'], ms.objects(s['rows']), kr.CORRECT, **s['kw'])
         for n, s in ((n, ms.scene(n)) for n in ms.NAMES)}
    assert all(r['nrepl_auto'] and r['nrepl_aper'] + r['nrepl_win'] for r in c['pair'])
    assert c['corner'][0]['nlost_win'] > 0                   # mirrors off the frame
    assert c['both_foreign'][0]['nlost_auto'] >= 20 and c['both_foreign'][0]['nrepl_auto'] > 0
    assert c['bad_column'][0]['nrepl_auto'] > 10 and ms.scene('bad_column')['seg'].max() == 1
    w = c['wide_window_small_kron']
    assert (2 * int(4.0 * w[0]['sigma_win'])) ** 2 > 256 and w[1]['npix_auto'] + w[1]['nlost_auto'] < 64
    d = c['deblended']
    assert len(d) == 12 and sum(1 for r in ms.scene('deblended')['rows'] if r['flags'] & 2) >= 2
    assert sum(1 for r in d if r['nrepl_auto']) >= 2
