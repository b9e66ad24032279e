"""Scenes for the mesh background statistic, one builder per regime of ``backguess`` (plain helper module).

Every builder is seeded, returns float32 planes ``(img, wgt or None)`` for a frame of nx x ny pixels, and comes with
the census condition (``oracle.background.mesh_maps(trace=...)``) that a test asserts before it compares anything:
the condition says which branch of the statistic the scene is there for, so a later edit of a recipe cannot make
its test vacuous.  ``tests/test_oracle_background.py`` checks every condition without a GPU;
``tests/test_background_regimes_gpu.py`` checks it again in front of each comparison.
"""
import functools

import numpy as np

from oracle import background as oback

# (nx, ny), mesh: what each geometry is there for in csrc/background.hip
GEOMETRIES = [
    ((512, 512), 64),     # fast path, 16-byte loads
    ((512, 512), 128),    # fast path, 16-byte loads, the largest fast mesh
    ((509, 487), 64),     # fast path, scalar loads, ragged last column and row
    ((512, 512), 33),     # fast path, scalar loads, mesh size not a multiple of 4
    ((600, 560), 256),    # generic statistics kernel (mesh area above 16384 px)
    ((560, 540), 16),     # 1190 meshes: generic filter kernel
]


def _rng(seed=1):
    return np.random.default_rng(seed)


def _stars(img, rng, n, sigma=2.0, flux=(50.0, 5e4)):
    """n circular Gaussians of total flux log-uniform in ``flux``, pixel-centre sampled, added in place; their
    density rises linearly from 0 at the left edge to twice the mean at the right edge."""
    ny, nx = img.shape
    xs = nx * np.sqrt(rng.uniform(size=n))
    ys = rng.uniform(0, ny, n)
    fl = np.exp(rng.uniform(np.log(flux[0]), np.log(flux[1]), n))
    r = int(np.ceil(5 * sigma)) + 1
    for x, y, f in zip(xs, ys, fl):
        x0, x1 = max(int(x) - r, 0), min(int(x) + r + 1, nx)
        y0, y1 = max(int(y) - r, 0), min(int(y) + r + 1, ny)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        img[y0:y1, x0:x1] += f / (2 * np.pi * sigma * sigma) * np.exp(
            -0.5 * ((xx - x) ** 2 + (yy - y) ** 2) / (sigma * sigma))


def gaussian(nx, ny, mesh=None):
    return _rng().normal(180.0, 6.0, (ny, nx)).astype(np.float32), None


def crowded(nx, ny, mesh=None):
    """Sky 180, noise 6, 6000 stars per 512 x 512 px (sigma 2 px, flux 50 .. 5e4): the median branch, and the mode
    branch beside it.  (At a uniform density the 128 and 256 px meshes are all on the median branch; with the
    density gradient of ``_stars`` every mesh size has both.)"""
    rng = _rng()
    img = rng.normal(180.0, 6.0, (ny, nx))
    _stars(img, rng, int(round(6000 * nx * ny / (512.0 * 512.0))))
    return img.astype(np.float32), None


def poisson3(nx, ny, mesh=None):
    return _rng().poisson(3, (ny, nx)).astype(np.float32), None


def poisson400(nx, ny, mesh=None):
    return _rng().poisson(400, (ny, nx)).astype(np.float32), None


def two_valued(nx, ny, mesh=None):
    return (10.0 + (_rng().uniform(size=(ny, nx)) < 0.5)).astype(np.float32), None


def nearly_constant(nx, ny, mesh=None):
    img = np.full((ny, nx), 42.0, np.float32)
    img[::37, ::11] += 1.0
    return img, None


CONSTANTS = (42.1, 1e-3, -7.3e4, 0.0)


def constant(value, poison=None):
    """An exactly constant frame; ``poison``: None, np.nan or np.inf - one such pixel in every mesh."""
    def build(nx, ny, mesh):
        img = np.full((ny, nx), value, np.float32)
        if poison is not None:
            img[mesh // 3::mesh, mesh // 2::mesh] = poison
        return img, None
    return build


def scaled(factor):
    def build(nx, ny, mesh=None):
        img, _ = gaussian(nx, ny)
        return (img * np.float32(factor)).astype(np.float32), None
    return build


# ---- the magnitudes a tolerance is stated in --------------------------------------------------------------------
def _spline_matrix(n, npix, mesh):
    eye = np.eye(n)
    return oback._spline_eval_axis(eye, oback.spline_derivs(eye), npix, mesh)        # (npix, n)


def envelope(nodes, nx, ny, mesh):
    """``oracle.background.expand`` is linear in the nodes: ``Wy @ nodes @ Wx.T``.  This is ``|Wy| @ |nodes| @ |Wx|.T``:
    the magnitude of the map with its terms summed without cancellation, which is what the rounding error of an fp32
    evaluation is proportional to.  Never below ``|expand(nodes)|``; on a smooth map of one sign within a few per
    cent of it; where the spline of a rough map swings through zero it stays at the size of the nodes around."""
    nby, nbx = nodes.shape
    wy = np.abs(_spline_matrix(nby, ny, mesh))
    wx = np.abs(_spline_matrix(nbx, nx, mesh))
    return wy @ np.abs(nodes) @ wx.T


# ---- census -----------------------------------------------------------------------------------------------------
def census(img, wgt, mesh):
    """The branch census of a frame (see ``oracle.background.mesh_maps``), every count present."""
    t = {}
    oback.mesh_maps(np.asarray(img, np.float64), None if wgt is None else np.asarray(wgt, np.float64), mesh, trace=t)
    for k in ('meshes', 'bad', 'mode', 'median', 'sig0', 'lowsig', 'it100', 'capped'):
        t.setdefault(k, 0)
    t.setdefault('iterations', [])
    t.setdefault('empty_bin_share', [])
    return t


def cond_crowded(c, mesh):
    return c['bad'] == 0 and c['median'] >= 0.4 * c['meshes'] and c['mode'] >= 0.1 * c['meshes']


def cond_poisson3(c, mesh):
    return c['bad'] == 0 and min(c['empty_bin_share']) >= 0.9


def cond_poisson400(c, mesh):
    # 128 x 128 meshes: every histogram has all 4096 levels
    return c['bad'] == 0 and c['mode'] + c['median'] == c['meshes'] and (mesh != 128 or c['capped'] == c['meshes'])


def cond_two_valued(c, mesh):
    return c['median'] == c['meshes']


def cond_nearly_constant(c, mesh):
    return c['bad'] == 0 and c['lowsig'] == c['meshes']


def cond_constant(c, mesh):
    return c['sig0'] == c['meshes']


def cond_any(c, mesh):
    return c['bad'] == 0 and c['mode'] + c['median'] == c['meshes']


# name -> (builder, census condition): the scenes that go through every geometry
SCENES = {
    'crowded': (crowded, cond_crowded),
    'poisson3': (poisson3, cond_poisson3),
    'poisson400': (poisson400, cond_poisson400),
    'two_valued': (two_valued, cond_two_valued),
    'nearly_constant': (nearly_constant, cond_nearly_constant),
    'scaled_2^-30': (scaled(2.0 ** -30), cond_any),
    'scaled_2^20': (scaled(2.0 ** 20), cond_any),
    'negated': (scaled(-1.0), cond_any),
}
for _v in CONSTANTS:
    SCENES['constant_%g' % _v] = (constant(_v), cond_constant)
    SCENES['constant_%g_nan' % _v] = (constant(_v, np.nan), cond_constant)
    SCENES['constant_%g_inf' % _v] = (constant(_v, np.inf), cond_constant)


# ---- BACK_MINGOODFRAC and WEIGHT_THRESH at their edges --------------------------------------------------------------
# A mesh is kept when n >= area / 2 of its pixels are samples (area: the clipped area of a ragged mesh).  Each scene is
# a pair: `exact` has meshes with exactly area / 2 samples (all kept), `short` has one sample less in each (all
# dropped).  Entries: name -> ((nx, ny), mesh, half-mesh regions [(y0, y1, x0, x1)], one more pixel per region, how).
_HALVES = {
    # 512 x 512 at 64: the first mesh, upper half
    'full': ((512, 512), 64, [(0, 32, 0, 64)], [(32, 0)]),
    # 300 x 280 at 64: a mesh of the last column (64 x 44), of the last row (24 x 64) and the corner (24 x 44)
    'ragged': ((300, 280), 64, [(0, 32, 256, 300), (256, 268, 0, 64), (256, 268, 256, 300)],
               [(32, 256), (268, 0), (268, 299)]),
}
BAD_VALUES = (np.nan, np.inf, 1e30, -1e30)


def good_fraction(where, how, short):
    """-> (img, wgt, mesh, number of meshes the oracle must drop).  how: 'weight0' (weight 0 against weight 1),
    'values' (NaN, +inf, 1e30, -1e30 in turn, no weight map), 'tiny' (weight 1e-30, not a sample, against
    1.1e-30, a sample)."""
    (nx, ny), mesh, regions, extra = _HALVES[where]
    img = _rng().normal(180.0, 6.0, (ny, nx)).astype(np.float32)
    sel = np.zeros((ny, nx), bool)
    for y0, y1, x0, x1 in regions:
        sel[y0:y1, x0:x1] = True
        # the mesh around the region stands 20 counts (3 sigma) above its neighbours: kept, it returns its own level;
        # dropped, it is filled with theirs - far apart, where two meshes of one sky differ by a few per cent of sigma
        my, mx = y0 // mesh * mesh, x0 // mesh * mesh
        img[my:my + mesh, mx:mx + mesh] += np.float32(20.0)
    if short:
        for y, x in extra:
            sel[y, x] = True
    wgt = None
    if how == 'weight0':
        wgt = np.where(sel, 0.0, 1.0).astype(np.float32)
    elif how == 'tiny':
        wgt = np.where(sel, np.float32(1e-30), np.float32(1.1e-30)).astype(np.float32)
    else:
        img[sel] = np.resize(np.array(BAD_VALUES, np.float32), int(sel.sum()))
    return img, wgt, mesh, (len(regions) if short else 0)


GOOD_FRACTION_CASES = [(w, h, s) for w in ('full', 'ragged') for h in ('weight0', 'values', 'tiny')
                       for s in (False, True)]


@functools.lru_cache(maxsize=None)
def scene(name, nx, ny, mesh):
    """-> (img, wgt, census); cached, the arrays are read-only."""
    build, _ = SCENES[name]
    img, wgt = build(nx, ny, mesh)
    img.setflags(write=False)
    return img, wgt, census(img, wgt, mesh)


def census_ok(name, c, mesh):
    return SCENES[name][1](c, mesh)
