"""Scenes for the deblending tests: the smallest inputs at which each part of the operator can go wrong.

Test infrastructure.  Every scene is (img, sigma, keyword arguments of the extraction).  The keyword arguments may carry
``bad`` (uint8 plane) and ``flag`` (int32 plane), which ``Engine.extract`` takes under the same names, and ``nthresh`` /
``mincont``; ``name@N`` is the scene ``name`` deblended with ``nthresh=N``.  Every finite pixel has ``|v| <= 1e6``; the
scenes of ``POISON_SCENES`` carry NaN, +inf or -inf in ``img`` or NaN, 0 or -1 in ``sigma``.  ``reference(name)`` computes
the numpy restatement once per process (forward and reversed member order).

The groups added for the tree kernel's indexing ("Deblending", *Tests*): ``NTHRESH_SCENES`` (every accepted
``nthresh``), ``BOX_SCENES`` (bounding boxes around ``DB_CELLS`` in every aspect ratio, 8-connectivity through a diagonal),
``EDGE_SCENES`` (right and bottom edge, the four corners, frames that are one object, one-column and one-row frames),
``BAD_SCENES`` (bad and flag planes) and ``POISON_SCENES``.  ``EXPECT`` holds (box width, box height, pixels of the largest
first-pass object, first-pass objects, final objects) of every one of them; tests/test_deblend_ref.py asserts it.
"""
import functools

import numpy as np

import deblend_ref as dr


def gaussians(nx, ny, items, base=0.0):
    y, x = np.mgrid[:ny, :nx]
    img = np.full((ny, nx), base, np.float64)
    for cx, cy, amp, width in items:
        img += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * width * width))
    return img


def pair(sep):
    """48 x 48, sigma = 1: amplitudes 200 and 150, width 1.1, ``sep`` pixels apart."""
    img = gaussians(48, 48, [(20, 24, 200.0, 1.1), (20 + sep, 24, 150.0, 1.1)])
    return img.astype(np.float32), np.ones((48, 48), np.float32), {}


def contrast(amp):
    """A primary of amplitude 1000 and width 2.5 with a companion of width 1.1, 12 px away."""
    img = gaussians(64, 64, [(24, 32, 1000.0, 2.5), (36, 32, float(amp), 1.1)])
    return img.astype(np.float32), np.ones((64, 64), np.float32), {}


def nested():
    """Three peaks in one component at x = 20, 25 and 34: the split of the close two survives the merge with the third."""
    img = gaussians(64, 64, [(20, 32, 300.0, 1.3), (25, 32, 250.0, 1.3), (34, 32, 200.0, 1.3)])
    return img.astype(np.float32), np.ones((64, 64), np.float32), {}


def plateaus():
    """Two mesas of 50, 8 x 10 px each, joined by a 4-row bridge of 10; integers, no filter: every tie rule decides."""
    img = np.zeros((32, 48), np.float32)
    img[10:20, 6:14] = 50.0
    img[10:20, 30:38] = 50.0
    img[13:17, 14:30] = 10.0
    return img, np.ones_like(img), dict(filter=False)


def sigma_step():
    """A 2x step in sigma across a blend: T is the threshold at the peak pixel, level 0 is still the whole object."""
    img = gaussians(56, 40, [(22, 20, 400.0, 1.6), (31, 20, 300.0, 1.6)])
    sigma = np.ones((40, 56), np.float32)
    sigma[:, 27:] = 2.0
    return img.astype(np.float32), sigma, {}


def noisy_field():
    """128 x 128, 25 stars on noise 1, fixed seed; several land in one component.  One realisation of such a field: 15
    objects before and 20 after, three parents split, one of them in four.  (The prototype the issue quotes had its own
    seed and amplitudes, which are not recorded, and gave 18 -> 24 with one parent split in six; the difference is the
    scene's, the operator is the one stated.)"""
    rng = np.random.default_rng(20261019)
    x, y = rng.uniform(8, 120, 25), rng.uniform(8, 120, 25)
    amp = 10 ** rng.uniform(1.2, 2.8, 25)
    img = gaussians(128, 128, list(zip(x, y, amp, np.full(25, 1.4)))) + rng.normal(0.0, 1.0, (128, 128))
    return img.astype(np.float32), np.ones((128, 128), np.float32), {}


def lone_star():
    """Amplitude 5000 under noise 3 on 96 x 96: the noise on its wings must not shred it."""
    rng = np.random.default_rng(5)
    img = gaussians(96, 96, [(47.3, 48.6, 5000.0, 1.5)]) + rng.normal(0.0, 3.0, (96, 96))
    return img.astype(np.float32), np.full((96, 96), 3.0, np.float32), {}


def all_above():
    """512 x 512, every pixel above the threshold, two broad peaks: one object far beyond any LDS tile."""
    img = gaussians(512, 512, [(170, 250, 400.0, 40.0), (350, 260, 300.0, 40.0)], base=10.0)
    return img.astype(np.float32), np.ones((512, 512), np.float32), dict(filter=False)


def spiral_with_knots():
    """test_extract_gpu's spiral, a bright knot at either end of the arm: long chains, one leftover pixel per round."""
    from test_extract_gpu import spiral
    arm = spiral(512)
    img = np.where(arm, 100.0, 0.0).astype(np.float32)
    img[0, 0:40] = 20000.0                                # the outer end: the arm starts along the first row
    ys, xs = np.nonzero(arm[250:262, 250:262])            # the inner end: the arm's pixels at the centre
    img[250 + ys, 250 + xs] = 20000.0
    return img, np.ones_like(img), dict(filter=False)


def edge():
    """A blend that touches the frame's left and top edges."""
    img = gaussians(40, 32, [(1, 2, 300.0, 1.3), (8, 2, 250.0, 1.3)])
    return img.astype(np.float32), np.ones((32, 40), np.float32), {}


def just_too_small():
    """Two rows with two peaks each: 9 = 2 x minarea - 1 pixels (it cannot hold two branches of minarea pixels and is not
    examined) and 11 pixels (two branches of five around one low pixel: it splits at mincont 0)."""
    img = np.zeros((24, 40), np.float32)
    img[8, 4:13] = [90, 80, 70, 60, 6, 60, 70, 80, 90]
    img[16, 4:15] = [90, 80, 70, 60, 50, 6, 50, 60, 70, 80, 90]
    return img, np.ones_like(img), dict(filter=False, detect_minarea=5, mincont=0.0)


def box(width):
    """A 32-row block of ``width`` columns above the threshold with two peaks, no filter: the bounding box has exactly
    32 x width pixels (1024: the largest that the kernel keeps in LDS; 1056: the smallest that goes to global memory)."""
    img = np.zeros((48, 56), np.float32)
    img[8:40, 10:10 + width] = 10.0 + gaussians(width, 32, [(9, 15, 300.0, 2.0), (22, 17, 240.0, 2.0)])
    return img, np.ones_like(img), dict(filter=False)


DB_CELLS = 1024                      # box pixels up to which k_db_tree keeps an object's planes in LDS


def deep_saddle():
    """Two narrow stars of amplitude 30000 and 20000, 6 px apart: the saddle lies far above sqrt(P T), the one upper
    threshold of nthresh = 2, so the pair stays one object there and splits at 32; at 64 its few hundred pixels occupy
    more than 40 of the 64 levels."""
    img = gaussians(48, 48, [(20, 24, 3e4, 1.5), (26, 24, 2e4, 1.5)])
    return img.astype(np.float32), np.ones((48, 48), np.float32), {}


def fine_saddle():
    """The mesas of ``plateaus`` with a bridge of 46: P / T = 50 / 1.5, so the highest threshold is 47.3 at nthresh 64 and
    44.8 at 32.  The bridge lies between the two: 64 levels tell it from the mesas and split them, 32 do not."""
    img, sigma, kw = plateaus()
    img[13:17, 14:30] = 46.0
    return img, sigma, kw


def framed(blk):
    """``blk`` with 3 columns of sky to its left and right and 2 rows above, 3 below: the frame is a few pixels larger
    than the box, and the box starts at no multiple of 4."""
    h, w = blk.shape
    img = np.zeros((h + 5, w + 6), np.float32)
    img[2:2 + h, 3:3 + w] = blk
    return img, np.ones_like(img), dict(filter=False)


def strip(bw, bh, peaks=2):
    """A line of ``max(bw, bh)`` pixels above the threshold, ``min(bw, bh)`` = 1, 2 or 3 wide: 10 + two peaks of 300 and
    240 (``peaks=1``: one of 300).  The 2- and 3-wide ones are cut at 45 % of their length, in the wing between the seeds,
    down to a connection through one diagonal step: [v 0 (0)] above [0 v (v)]."""
    n, wide = max(bw, bh), min(bw, bh)
    t = np.arange(n, dtype=np.float64)
    tops = [(0.27 * n, 300.0), (0.71 * n, 240.0)] if peaks == 2 else [(0.4 * n, 300.0)]
    prof = 10.0 + sum(a * np.exp(-(t - c) ** 2 / (2.0 * (n / 24.0) ** 2)) for c, a in tops)
    blk = prof[:, None] + 0.25 * np.arange(wide)[None, :]
    if wide > 1:
        r = int(0.45 * n)
        blk[r - 1, 1:] = 0.0
        blk[r, :1] = 0.0
    return framed((blk.T if bw > bh else blk).astype(np.float32))


def block(bw, bh):
    """A ``bw`` x ``bh`` block above the threshold, 10 + two peaks of 300 and 240 along its longer side."""
    a, b = (0.28, 0.45), (0.70, 0.55)
    if bh > bw:
        a, b = a[::-1], b[::-1]
    tops = [(a[0] * bw, a[1] * bh, 300.0, 2.0), (b[0] * bw, b[1] * bh, 240.0, 2.0)]
    return framed((10.0 + gaussians(bw, bh, tops)).astype(np.float32))


def whole_frame(nx, ny):
    """Every pixel of the frame above the threshold, two peaks: one object that touches all four edges."""
    img = 10.0 + gaussians(nx, ny, [(0.3 * nx, 0.4 * ny, 300.0, 2.5), (0.72 * nx, 0.6 * ny, 240.0, 2.5)])
    return img.astype(np.float32), np.ones((ny, nx), np.float32), dict(filter=False)


def frame_line(nx, ny):
    """A frame of one row or one column, 5 + peaks of 100 and 80 at pixels 10 and 29 of 40."""
    t = np.arange(40, dtype=np.float64)
    prof = 5.0 + 100.0 * np.exp(-(t - 10) ** 2 / 8.0) + 80.0 * np.exp(-(t - 29) ** 2 / 8.0)
    img = prof.reshape(ny, nx).astype(np.float32)
    return img, np.ones_like(img), dict(filter=False)


def blend_at(nx, ny, stars):
    img = gaussians(nx, ny, [(x, y, a, 1.3) for x, y, a in stars])
    return img.astype(np.float32), np.ones((ny, nx), np.float32), dict(filter=False)


# (33 x 31 = 1023 lies on the LDS side as 31 x 33 does; 32 x 33 = 1056 is the block beyond the limit that is taller than
# wide, beside the 33 x 32 of ``box(33)``)
BOX_SHAPES = {True: [(1024, 1), (1, 1024), (2, 512), (512, 2), (64, 16), (16, 64), (3, 341), (31, 33), (33, 31)],      # LDS form
              False: [(1025, 1), (1, 1025), (2, 513), (3, 342), (32, 33)]}                                              # global form
BOX_SCENES = {f'box{w}x{h}': (lambda w=w, h=h: strip(w, h) if min(w, h) <= 3 else block(w, h))
              for shapes in BOX_SHAPES.values() for w, h in shapes}
SINGLE_LINES = {'line1024': lambda: strip(1024, 1, peaks=1), 'line1025': lambda: strip(1025, 1, peaks=1)}
EDGE_SCENES = {
    'edge_right': lambda: blend_at(40, 32, [(38, 16, 300.0), (31, 16, 250.0)]),
    'edge_bottom': lambda: blend_at(40, 32, [(16, 30, 300.0), (16, 23, 250.0)]),
    'corners': lambda: blend_at(48, 40, [(1, 1, 300.0), (8, 2, 250.0), (46, 1, 300.0), (46, 8, 250.0),
                                         (1, 38, 300.0), (2, 31, 250.0), (46, 38, 300.0), (39, 37, 250.0)]),
    'frame37x29': lambda: whole_frame(37, 29), 'frame31x29': lambda: whole_frame(31, 29),
    'frame1x40': lambda: frame_line(1, 40), 'frame40x1': lambda: frame_line(40, 1)}

# ---- bad pixels, flags, poison: 48 x 48, two stars (4000 and 3000, width 2.5) at (17, 24) and (28, 24) unless said otherwise
HOLE1, HOLE9 = (slice(24, 25), slice(11, 12)), (slice(23, 26), slice(9, 12))        # in the left star's wing, 6 .. 8 px out
SADDLE, PEAK = (slice(24, 25), slice(22, 23)), (slice(24, 25), slice(17, 18))
POISONS = {'imgnan': ('img', np.nan), 'imgpinf': ('img', np.inf), 'imgninf': ('img', -np.inf),
           'signan': ('sigma', np.nan), 'sig0': ('sigma', 0.0), 'signeg': ('sigma', -1.0)}


def masked(kind, use_filter, planes=True, poison=None):
    """The scenes of bad pixels (``planes=False``: the same image without its bad and flag planes and without poison).
    ``poison``: a key of POISONS, written at the place of the bad byte instead of it; those scenes measure with an
    aperture of radius 7, which reaches the poisoned pixels, so that FLUX_APER / FLUXERR_APER become non-finite."""
    stars = [(17, 24, 4000.0, 2.5), (28, 24, 3000.0, 2.5)]
    if kind in ('diag', 'cut'):                           # three stars; the line runs between the second and the third
        stars = [(14, 24, 400.0, 2.0), (23, 24, 300.0, 2.0), (32, 24, 350.0, 2.0)]
    elif kind == 'edge':
        stars = [(17, 2, 4000.0, 2.5), (28, 2, 3000.0, 2.5)]
    img = gaussians(48, 48, stars).astype(np.float32)
    sigma = np.ones((48, 48), np.float32)
    bad, flag = np.zeros((48, 48), np.uint8), None
    y, x = np.mgrid[:48, :48]
    if kind in ('saddle', 'peak', 'hole1', 'hole9'):
        bad[dict(saddle=SADDLE, peak=PEAK, hole1=HOLE1, hole9=HOLE9)[kind]] = 1
    elif kind == 'diag':                                  # one pixel thick: the two sides touch diagonally across it
        bad[x - y == 3] = 1
    elif kind == 'cut':                                   # two pixels thick: they do not touch
        bad[(x - y == 3) | (x - y == 4)] = 1
    elif kind == 'edge':                                  # part of the first row under the blend
        bad[0, 14:26] = 1
    elif kind == 'flags':                                 # flags on the right star alone, and on the hole
        bad[HOLE9] = 1
        flag = np.zeros((48, 48), np.int32)
        flag[HOLE9] = 0x40
        flag[22:27, 27:30] = 0x10
        flag[24, 28] |= 0x40000000
    kw = dict(filter=use_filter)
    if poison is not None:
        plane, value = POISONS[poison]
        if planes:
            (img if plane == 'img' else sigma)[bad != 0] = value
        kw['aper_radius'] = 7.0
    elif planes:
        kw['bad'] = bad
        if flag is not None:
            kw['flag'] = flag
    return img, sigma, kw


BAD_KINDS = ('saddle', 'peak', 'diag', 'cut', 'hole1', 'hole9', 'edge', 'flags')
BAD_SCENES = {f'bad_{kind}.f{int(f)}': (lambda kind=kind, f=f: masked(kind, f)) for kind in BAD_KINDS for f in (False, True)}
POISON_SCENES = {f'{p}_{kind}.f{int(f)}': (lambda kind=kind, f=f, p=p: masked(kind, f, poison=p))
                 for p in POISONS for kind in ('saddle', 'hole9') for f in (False, True)}


def unmasked(name):
    """(img, sigma, kw) of a scene of BAD_SCENES or POISON_SCENES without its planes and without its poison."""
    head, f = name.split('.f')
    p, kind = head.split('_')
    return masked(kind, bool(int(f)), planes=False, poison=None if p == 'bad' else p)


# (box width, box height, pixels) of the largest first-pass object, first-pass objects, final objects (nthresh 32)
EXPECT = {'box1024x1': (1024, 1, 1024, 1, 2), 'box1x1024': (1, 1024, 1024, 1, 2), 'box2x512': (2, 512, 1022, 1, 2),
          'box512x2': (512, 2, 1022, 1, 2), 'box64x16': (64, 16, 1024, 1, 2), 'box16x64': (16, 64, 1024, 1, 2),
          'box3x341': (3, 341, 1020, 1, 2), 'box31x33': (31, 33, 1023, 1, 2), 'box1025x1': (1025, 1, 1025, 1, 2),
          'box1x1025': (1, 1025, 1025, 1, 2), 'box2x513': (2, 513, 1024, 1, 2), 'box3x342': (3, 342, 1023, 1, 2),
          'box33x31': (33, 31, 1023, 1, 2), 'box32x33': (32, 33, 1056, 1, 2),
          'line1024': (1024, 1, 1024, 1, 1), 'line1025': (1025, 1, 1025, 1, 1),
          'edge_right': (13, 9, 95, 1, 2), 'edge_bottom': (9, 13, 95, 1, 2), 'corners': (13, 7, 74, 4, 8),
          'frame37x29': (37, 29, 1073, 1, 2), 'frame31x29': (31, 29, 899, 1, 2), 'frame1x40': (1, 40, 40, 1, 2),
          'frame40x1': (40, 1, 40, 1, 2),
          'bad_saddle.f0': (30, 19, 501, 1, 2), 'bad_saddle.f1': (32, 21, 545, 1, 2), 'bad_peak.f0': (30, 19, 501, 1, 2),
          'bad_peak.f1': (32, 21, 545, 1, 2), 'bad_diag.f0': (31, 13, 342, 1, 3), 'bad_diag.f1': (31, 13, 358, 1, 3),
          'bad_cut.f0': (25, 13, 219, 2, 3), 'bad_cut.f1': (25, 13, 229, 2, 3), 'bad_hole1.f0': (30, 19, 501, 1, 2),
          'bad_hole1.f1': (32, 21, 545, 1, 2), 'bad_hole9.f0': (30, 19, 493, 1, 2), 'bad_hole9.f1': (32, 21, 537, 1, 2),
          'bad_edge.f0': (30, 12, 314, 1, 2), 'bad_edge.f1': (32, 13, 339, 1, 2), 'bad_flags.f0': (30, 19, 493, 1, 2),
          'bad_flags.f1': (32, 21, 537, 1, 2)}
EXPECT.update({name: EXPECT['bad_' + name.split('_')[1]] for name in POISON_SCENES})       # poison at the bad byte's place
# final objects per nthresh (32 included): what the sweep must find
NTHRESH_OBJECTS = {'pair5': {2: 1, 4: 2, 8: 2, 16: 2, 32: 2, 64: 2}, 'pair8': {2: 2, 4: 2, 8: 2, 16: 2, 32: 2, 64: 2},
                   'nested': {2: 2, 4: 2, 8: 3, 16: 3, 32: 3, 64: 3},
                   'noisy_field': {2: 18, 4: 18, 8: 19, 16: 19, 32: 20, 64: 20},
                   'deep_saddle': {2: 1, 4: 1, 8: 1, 16: 2, 32: 2, 64: 2},
                   'fine_saddle': {2: 1, 4: 1, 8: 1, 16: 1, 32: 1, 64: 2}}
NTHRESH = (2, 4, 8, 16, 64)                                # 32 is every other scene
NTHRESH_SCENES = [f'{name}@{n}' for name in NTHRESH_OBJECTS for n in NTHRESH]

SCENES = {**BOX_SCENES, **SINGLE_LINES, **EDGE_SCENES, **BAD_SCENES, **POISON_SCENES,
          'deep_saddle': deep_saddle, 'fine_saddle': fine_saddle,
          'pair3': lambda: pair(3), 'pair4': lambda: pair(4), 'pair5': lambda: pair(5), 'pair6': lambda: pair(6),
          'pair8': lambda: pair(8), 'contrast20': lambda: contrast(20), 'contrast60': lambda: contrast(60),
          'nested': nested, 'plateaus': plateaus, 'sigma_step': sigma_step, 'noisy_field': noisy_field,
          'lone_star': lone_star, 'all_above': all_above, 'spiral_with_knots': spiral_with_knots, 'edge': edge,
          'just_too_small': just_too_small, 'box1024': lambda: box(32), 'box1056': lambda: box(33)}


@functools.lru_cache(maxsize=None)
def scene(name):
    if '@' in name:                                       # name@N: the scene deblended with nthresh = N
        base, n = name.split('@')
        img, sigma, kw = scene(base)
        return img, sigma, dict(kw, nthresh=int(n))
    img, sigma, kw = SCENES[name]()
    for a in (img, sigma, kw.get('bad'), kw.get('flag')):
        if a is not None:
            a.setflags(write=False)
    return img, sigma, kw


def split_kw(kw):
    """(extraction keywords, deblending keywords) of a scene's keyword arguments."""
    ex = {k: v for k, v in kw.items() if k not in ('nthresh', 'mincont')}
    db = {k: v for k, v in kw.items() if k in ('nthresh', 'mincont')}
    return ex, db


@functools.lru_cache(maxsize=None)
def reference(name, reverse=False):
    img, sigma, kw = scene(name)
    ex, db = split_kw(kw)
    ref_kw = dict(detect_thresh=ex.get('detect_thresh', 1.5), detect_minarea=ex.get('detect_minarea', 5),
                  use_filter=ex.get('filter', True), satur_level=ex.get('satur_level', 50000.0),
                  aper_radius=ex.get('aper_radius', 3.0))
    return dr.deblend(img, sigma, ex.get('bad'), ex.get('flag'), reverse=reverse, **db, **ref_kw)


# ---- the comparison both GPU test files make ------------------------------------------------------------------------
def assert_same_plane(got, ref):
    """The filtered plane, byte for byte; where the restatement itself holds a NaN (``filter=False`` over a NaN pixel) the
    other side must hold a NaN too: NaN payloads are not part of the convention."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), 'filtered plane: NaN pattern'
    zero = np.float32(0)
    assert np.where(nan, zero, got).tobytes() == np.where(nan, zero, ref).tobytes(), 'filtered plane'


def float_columns(t, r, rev, aper_columns, finite=True):
    """(worst difference, bound, failures) per float column of the GPU table ``t`` against the restatement ``r`` (``rev``:
    its reversed summation order).  No row and no column is left out: the NaN / +inf / -inf pattern of every column must
    equal the restatement's exactly, and every finite entry is held to 10 x the order difference plus the libm
    allowance (FLUX_APER / FLUXERR_APER: rtol 1e-10 + atol 1e-9).  ``finite``: every entry must be finite on both sides."""
    import extract_ref as xr
    bounds = xr.order_bounds(r, rev)
    worst, fails = {}, []
    for c in xr.FLOAT_COLUMNS:
        a, b = np.asarray(t[c], np.float64), np.asarray(r[c], np.float64)
        for what, test in (('NaN', np.isnan), ('+inf', np.isposinf), ('-inf', np.isneginf)):
            assert np.array_equal(test(a), test(b)), f'{c}: {what} pattern {a} / {b}'
        ok = np.isfinite(b)
        if finite:
            assert ok.all() and np.isfinite(a).all(), c
        diff = np.abs(a[ok] - b[ok])
        allow = 1e-10 * np.abs(b[ok]) + 1e-9 if c in aper_columns else bounds[c] + xr.libm_allowance(c, b[ok])
        worst[c] = float(diff.max()) if len(diff) else 0.0
        if (diff > allow).any():
            fails.append((c, worst[c], bounds[c]))
    return worst, bounds, fails


def occupied_levels(name):
    """The distinct values of L among the members of every first-pass object of a scene, at the scene's nthresh."""
    img, sigma, kw = scene(name)
    ex, db = split_kw(kw)
    first = reference(name)['first']
    filt, seg = np.asarray(first['filtered'], np.float32), first['segm']
    thr = np.float32(ex.get('detect_thresh', 1.5)) * sigma
    out = []
    for k in range(1, seg.max() + 1):
        ys, xs = np.nonzero(seg == k)
        f = filt[ys, xs]
        i = int(np.argmax(f))
        out.append(np.unique(dr.pixel_levels(f, dr.thresholds(f[i], thr[ys[i], xs[i]], db.get('nthresh', 32)))))
    return out
