"""The mesh background kernels against the oracle in every regime of the statistic (tests/mesh_scenes.py): the median
branch, sparse histograms, capped levels, sigma under 0.1 bins, constant meshes, BACK_MINGOODFRAC and WEIGHT_THRESH at
their edges, frames scaled by 2^-30 and 2^20 - on the fast path with 16-byte and with scalar loads, the generic
statistics kernel and the generic filter.  Every comparison starts with the census condition of its scene.

Tolerance: ``A |ref| + B rms_ref`` at every pixel of every map, nothing left out, no absolute
term.  ``|ref|`` and ``rms_ref`` are the oracle's maps with the spline's terms summed without cancellation
(``mesh_scenes.envelope``); ``rms_ref`` is floored by the float32 spacing of the reference value, and where it is 0
(constant frames) the bound is the A term alone.  A and B come from the oracle alone
(tests/measure_mesh_tolerances.py): A = 4 x its float32 floor, B = 2 x its sensitivity to the last bit of the mesh
mean and sigma that the quantisation rounds to float.
"""
import functools

import numpy as np
import pytest

import mesh_scenes as ms
from oracle import background as oback
from util import assert_close_masked, pkg, synth

pytestmark = pytest.mark.gpu

A = 1.62e-5       # 4 x 4.04e-06 (crowded, 512 x 512 at mesh 33)
B = 0.16          # 2 x 0.0799 (poisson400, 560 x 540 at mesh 16)


def spacing32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _reference(key, mesh, fsize):
    """oracle.background.background of a scene, once per module; key: ('scene', name, nx, ny) or ('gf', where, how,
    short)."""
    img, wgt = _planes(key, mesh)
    ny, nx = img.shape
    bkg, rms, mean, sig, bo, so = oback.background(img.astype(np.float64),
                                                   None if wgt is None else wgt.astype(np.float64), mesh, fsize)
    return bkg, rms, mean, sig, ms.envelope(bo, nx, ny, mesh), ms.envelope(so, nx, ny, mesh)


def _planes(key, mesh):
    if key[0] == 'scene':
        img, wgt, _ = ms.scene(key[1], key[2], key[3], mesh)
        return img, wgt
    img, wgt, _, _ = ms.good_fraction(*key[1:])
    return img, wgt


def _units(err, tol):
    """Worst error in units of the tolerance; where the tolerance is 0 the error has to be 0."""
    assert not err[tol == 0].any(), 'a value that has to be exact is not'
    pos = tol > 0
    return float((err[pos] / tol[pos]).max()) if pos.any() else 0.0


def compare(engine, key, mesh, fsize, label):
    img, wgt = _planes(key, mesh)
    r_bkg, r_rms, r_mean, r_sig, env_b, env_r = _reference(key, mesh, fsize)
    bkg, rms, sub, stats = engine.background(img, wgt, mesh=mesh, filtersize=fsize)

    def unit(ref):
        return np.where(env_r > 0, np.maximum(env_r, spacing32(ref)), 0.0)
    tol_b = A * env_b + B * unit(r_bkg)
    tol_r = A * env_r + B * unit(r_rms)
    worst = {'bkg': _units(np.abs(bkg - r_bkg), tol_b), 'rms': _units(np.abs(rms - r_rms), tol_r)}
    # sub = img - bkg in float: the background's tolerance and the rounding of the difference
    i64 = img.astype(np.float64)
    fin = np.isfinite(i64)
    r_sub = i64 - r_bkg
    assert np.array_equal(np.isnan(sub), np.isnan(i64)) and np.array_equal(np.isposinf(sub), np.isposinf(i64))
    worst['sub'] = _units(np.abs(sub[fin] - r_sub[fin]), (tol_b + A * np.abs(r_sub))[fin])
    usig = max(r_sig, float(spacing32(r_mean))) if r_sig > 0 else 0.0
    worst['backmean'] = _units(np.abs(np.array([stats[0] - r_mean])), np.array([A * abs(r_mean) + B * usig]))
    worst['backsig'] = _units(np.abs(np.array([stats[1] - r_sig])), np.array([(A + B) * r_sig]))
    print('REGIME %s mesh %d filter %d: worst error / tolerance %s' % (
        label, mesh, fsize, ' '.join('%s %.3g' % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, (label, mesh, fsize, worst)


@pytest.mark.parametrize('geometry', ms.GEOMETRIES, ids=lambda g: '%dx%d@%d' % (g[0][0], g[0][1], g[1]))
@pytest.mark.parametrize('name', list(ms.SCENES))
def test_regime_matches_oracle(engine, name, geometry):
    (nx, ny), mesh = geometry
    _, _, census = ms.scene(name, nx, ny, mesh)
    assert ms.census_ok(name, census, mesh), census
    compare(engine, ('scene', name, nx, ny), mesh, 3, '%s %dx%d' % (name, nx, ny))


@pytest.mark.parametrize('name', list(ms.SCENES))
def test_regime_without_the_median_filter(engine, name):
    """BACK_FILTERSIZE 1: a single wrong mesh is not voted away by its neighbours.  The scenes take turns at the
    geometries."""
    (nx, ny), mesh = ms.GEOMETRIES[list(ms.SCENES).index(name) % len(ms.GEOMETRIES)]
    _, _, census = ms.scene(name, nx, ny, mesh)
    assert ms.census_ok(name, census, mesh), census
    compare(engine, ('scene', name, nx, ny), mesh, 1, '%s %dx%d' % (name, nx, ny))


@pytest.mark.parametrize('where,how,short', ms.GOOD_FRACTION_CASES)
def test_good_fraction_and_weight_threshold_edges(engine, where, how, short):
    """A mesh with exactly area / 2 samples is kept, one with a sample less is dropped and filled from its neighbours:
    on a full mesh and on the clipped areas of the last column, the last row and the corner; bad pixels made by
    weights of 0, by NaN / +inf / 1e30 / -1e30 values, and by weights AT the threshold beside weights above it."""
    img, wgt, mesh, nbad = ms.good_fraction(where, how, short)
    assert ms.census(img, wgt, mesh)['bad'] == nbad
    for fsize in (3, 1):
        compare(engine, ('gf', where, how, short), mesh, fsize, 'good fraction %s %s %s' % (where, how, short))


# ---- metamorphic: no reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize('geometry', [ms.GEOMETRIES[0], ms.GEOMETRIES[3], ms.GEOMETRIES[4]],
                         ids=lambda g: '%dx%d@%d' % (g[0][0], g[0][1], g[1]))
@pytest.mark.parametrize('name', ['crowded', 'poisson400'])
def test_power_of_two_scaling_is_exact(engine, name, geometry):
    """Every operation of the statistic commutes with a power of two (float quantisation, fp64 moments, thresholds in
    bins, the relative EPS), and so does the oracle, exactly: s * image gives s * maps, bit for bit."""
    (nx, ny), mesh = geometry
    img, _, census = ms.scene(name, nx, ny, mesh)
    assert ms.census_ok(name, census, mesh), census
    wgt = np.ones_like(img)
    wgt[5::23, 3::19] = 0                       # the weights stay as they are
    bkg, rms, _, stats = engine.background(img, wgt, mesh=mesh)
    for s in (2.0 ** -30, 2.0 ** -7, 2.0 ** 9, 2.0 ** 20):
        sb, sr, _, ss = engine.background(img * np.float32(s), wgt, mesh=mesh)
        assert np.array_equal(sb, bkg * np.float32(s)) and np.array_equal(sr, rms * np.float32(s)), (name, s)
        assert ss[0] == stats[0] * s and ss[1] == stats[1] * s, (name, s, ss, stats)


def _tile(block, reps):
    return np.ascontiguousarray(np.tile(block, (reps, reps)))


def _within_spacings(a, v, k):
    return bool((np.abs(a.astype(np.float64) - float(v)) <= k * float(np.spacing(np.float32(abs(v))))).all())


def test_position_independence_aligned(engine):
    """One 64 x 64 block of the crowded scene, tiled 8 x 8: 64 meshes with the same pixels.  Without the median
    filter every mesh has the value the block returns alone, as a single-mesh frame: the two global values (medians
    of the 64 mesh values) are that value, float for float.  The pixels are the fp32 spline through 64 equal nodes,
    ``dx1 (dy1 V + dy V) + dx (dy1 V + dy V)``: two convex combinations, each of which can move the value by one
    float spacing (two roundings of half a spacing), so every pixel is within 2 spacings of V - not the same float.
    Measured on an MI355X: the global values equal; rms equal at every pixel; bkg off V at 13041 of 262144 pixels,
    by 2 spacings at the most.  (A mesh that had read one wrong pixel would be off by hundreds of spacings.)"""
    img, _, _ = ms.scene('crowded', 512, 512, 64)
    block = np.array(img[64:128, 384:448])
    assert ms.census(block, None, 64)['median'] == 1            # the block is on the median branch
    b1, r1, _, s1 = engine.background(block, None, mesh=64, filtersize=1)
    assert (b1 == b1[0, 0]).all() and (r1 == r1[0, 0]).all() and s1[0] == b1[0, 0] and s1[1] == r1[0, 0]
    bkg, rms, _, stats = engine.background(_tile(block, 8), None, mesh=64, filtersize=1)
    assert stats[0] == s1[0] and stats[1] == s1[1]
    print('REGIME tiled 64: pixels off the single-mesh value: bkg %d rms %d of %d, worst %.3g / %.3g spacings' % (
        (bkg != b1[0, 0]).sum(), (rms != r1[0, 0]).sum(), bkg.size,
        np.abs(bkg - b1[0, 0]).max() / np.spacing(b1[0, 0]), np.abs(rms - r1[0, 0]).max() / np.spacing(r1[0, 0])))
    assert _within_spacings(bkg, b1[0, 0], 2) and _within_spacings(rms, r1[0, 0], 2)


def test_position_independence_unaligned(engine):
    """The same with a 61 x 61 block in a frame of 488 x 488 at mesh 61: scalar loads, row starts off the 16-byte
    grid.  Against the oracle within the tolerance; the same value in all 64 meshes: the global values are the value
    of the block alone, and every pixel is within 4 float spacings of it: at a mesh size that is no power of two the
    spline weights dy and 1 - dy are rounded themselves and their sum misses 1 by up to half a spacing of 1, which is
    up to one more spacing of V in each of the two convex combinations (see above)."""
    img, _, _ = ms.scene('crowded', 512, 512, 64)
    block = np.array(img[64:125, 384:445])
    frame = _tile(block, 8)
    assert ms.census(frame, None, 61)['median'] == 64
    b1, r1, _, s1 = engine.background(block, None, mesh=61, filtersize=1)
    bkg, rms, _, stats = engine.background(frame, None, mesh=61, filtersize=1)
    r_bkg, r_rms, r_mean, r_sig, bo, so = oback.background(frame.astype(np.float64), None, 61, 1)
    assert (bo == bo[0, 0]).all() and (so == so[0, 0]).all()
    tol_b = A * abs(r_mean) + B * r_sig
    tol_r = (A + B) * r_sig
    assert abs(stats[0] - r_mean) <= tol_b and abs(stats[1] - r_sig) <= tol_r
    assert np.abs(bkg - r_bkg).max() <= tol_b and np.abs(rms - r_rms).max() <= tol_r
    assert stats[0] == s1[0] == b1[0, 0] and stats[1] == s1[1] == r1[0, 0]
    print('REGIME tiled 61: worst %.3g / %.3g spacings off the single-mesh value' % (
        np.abs(bkg - b1[0, 0]).max() / np.spacing(b1[0, 0]), np.abs(rms - r1[0, 0]).max() / np.spacing(r1[0, 0])))
    assert _within_spacings(bkg, b1[0, 0], 4) and _within_spacings(rms, r1[0, 0], 4)


# ---- the variance statistic (1 / weight), which feeds the weight rescale -----------------------------------------
def _weight_maps(nx, ny):
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:ny, 0:nx]
    flat = np.full((ny, nx), 0.04, np.float32)
    flat[:, 128:] = 0.025                                   # flat inside every 64 px mesh
    two = np.where(rng.uniform(size=(ny, nx)) < 0.5, 0.02, 0.05).astype(np.float32)
    smooth = (1.0 / (40.0 * (1.0 + 0.3 * np.sin(xx / 41.0) * np.cos(yy / 57.0)))).astype(np.float32)
    u = rng.uniform(size=(ny, nx))
    smooth[u < 0.30] = 0
    smooth[(u < 0.51) & (xx < 128)] = 0                     # 51 % of the pixels gone in the first two mesh columns
    return {'flat': flat, 'two_valued': two, 'smooth': smooth}


@pytest.mark.parametrize('which', ['flat', 'two_valued', 'smooth'])
def test_variance_statistic_through_the_weight_rescale(engine, which):
    from test_coadd_gpu import oracle_coadd
    z, s = pkg(), synth()
    nx, ny, mesh = 300, 280, 64
    base = s.tan_wcs(nx, ny)
    f = s.make_frame(nx, ny, 77, s.tan_wcs(nx, ny), sky=160.0, noise=5.0, nstars=30, nbad=0)
    f['wgt'] = _weight_maps(nx, ny)[which]
    with np.errstate(divide='ignore'):
        var = np.where(f['wgt'] > 1e-30, 1.0 / np.where(f['wgt'] > 0, f['wgt'], 1), 0.0)
    c = ms.census(var, f['wgt'], mesh)
    if which == 'flat':
        assert c['sig0'] == c['meshes']
    elif which == 'two_valued':
        assert c['median'] > 0 and c['bad'] == 0
    else:
        assert c['bad'] >= 5 and c['meshes'] - c['bad'] >= 8 and c['sig0'] == 0
    p = z.coadd_params(combine='WEIGHTED', subtract_back=True, rescale_weights=True, back_size=mesh)
    g_img, g_wgt, _, _ = engine.coadd([f], base, p, want_mask=False)
    r_img, r_wgt, _, _, _ = oracle_coadd([f], base, 'WEIGHTED', True, True, mesh=mesh)
    both = (g_wgt > 0) & (r_wgt > 0)
    assert both.mean() > 0.4 and ((g_wgt > 0) != (r_wgt > 0)).mean() < 1e-4
    assert_close_masked(g_wgt[both], r_wgt[both], 2e-3, 0, 'rescaled weights, %s' % which, max_bad_frac=1e-4)
