"""Named geometries for the resampler (numpy and the oracle only, no GPU).

A scene is ``Scene(win, wout, img, wgt, mask)``: the input frame with its WCS and the output grid.  The
frames come from ``synth.make_frame`` (stars, noise, bad pixels with zero weight, mask bits 0 and 8); a
few pixels also carry mask bits 16, 20 and 30, which do not fit the 16-bit box-OR plane of the kernels
(``ZM_BOX_RAW``).  Outputs are at most 260 x 260 pixels, inputs at most 420 on a side, and every output
spans at least three 64 x 32 tiles along both axes.  ``tests/test_resample_scenes.py`` asserts from the
oracle alone what is said about a scene here; ``tests/test_resample_geometry_gpu.py`` runs the scenes
through the kernels; ``tests/measure_resample_tolerance.py`` prints the table ``BOUNDS`` is taken from.

What a scene is for
  crval_offset         TPV on both sides, tangent points 40 arcsec apart: the 3 x 3 rotation between the
                       tangent frames is not the identity
  across_ra_zero       CRVAL1 359.995 against 0.004
  near_pole            dec 89.99, tangent points 90 degrees apart in RA: the frames are turned by a quarter
                       against each other and the rotation matrix is far from the identity
  tpv_degree7_radial   ZTF's PV terms plus degree 5, 6, 7 terms and PV?_3 / PV?_11, reference pixel 1400 px
                       off the frame so that the high degrees move pixels by tenths of a pixel
  tpv_to_tan, tan_to_tpv   TPV on one side only (input, output)
  rot90, rot180, rot270    quarter turns with the dither (0.37, -0.41): tall tile footprints, a lattice
                       that runs backwards
  rot90_exact          a quarter turn without dither: integer positions, a pure copy
  mirrored, mirrored_rot90  det CD of the opposite sign
  finer_2x, coarser_2x, coarser_3x   scale changes, dithers that keep the positions off the integers; the coarser
                       ones are turned by 0.2 degrees so that the fractions sweep every fp32 rounding case of a
                       140 and a 200 px wide tile footprint
  quarter_shift, half_shift    0.25 and 0.5 px on both axes: fractions every fp32 step represents exactly

Flip budget.  A pixel is *near a decision* when its oracle position lies within ``delta = 2 delta0`` (the
scene's emulated position error, ``BOUNDS``) of a snap threshold (fraction 1e-5 or 1 - 1e-5) on either
axis, or, for NEAREST, of a half-integer.  Only such pixels may differ in validity or mask; their share of
the covered pixels is at most 1e-3 in every scene (asserted on the CPU).  One combination is exempt by
construction: NEAREST on ``half_shift`` puts every position on a half-integer, where the pick depends on
the last bit of the fp64 map; there the kernel has to return one of the tied pixels for every output
(``nearest_candidates``).
"""
import functools
from typing import NamedTuple

import numpy as np

from oracle import resample as oresample
from oracle.wcs import map_out_to_in
from util import oracle_coadd, synth, to_oracle_wcs

SCENES = ('crval_offset', 'across_ra_zero', 'near_pole', 'tpv_degree7_radial', 'tpv_to_tan', 'tan_to_tpv',
          'rot90', 'rot180', 'rot270', 'rot90_exact', 'mirrored', 'mirrored_rot90',
          'finer_2x', 'coarser_2x', 'coarser_3x', 'quarter_shift', 'half_shift')
OTHER_KERNEL_SCENES = ('crval_offset', 'rot90', 'mirrored', 'coarser_2x', 'half_shift')
EXACT = {'rot90_exact': 0.0, 'quarter_shift': 0.25, 'half_shift': 0.5}      # the fraction of every position
QUADRANT = ('rot90', 'rot270', 'rot90_exact', 'mirrored_rot90', 'near_pole')
ROTATED_FRAMES = ('crval_offset', 'across_ra_zero', 'near_pole')          # tangent frames differ
DITHER = (0.37, -0.41)
SCALE_DITHER = (0.3183, -0.4142)

KINDS = {'LANCZOS3': oresample.LANCZOS3, 'BILINEAR': oresample.BILINEAR, 'NEAREST': oresample.NEAREST}
RTOL, ATOL, WTOL = 2e-5, 2e-5, 5e-5          # the parity bounds of tests/test_resample_gpu.py
MAX_EXCLUDED = 1e-3

# Printed by tests/measure_resample_tolerance.py: (delta0 in px, value bound, weight bound), the bounds in
# units of (RTOL |ref| + ATOL std(img)) and of WTOL |ref|.  A bound is 1 where the fp32 emulation of the
# kernel's positions stays inside the existing tolerance, and 4 x the emulated deviation where it does not.
BOUNDS = {
    'crval_offset':       (9.57e-06, 1.0, 1.0),
    'across_ra_zero':     (6.89e-06, 1.0, 1.0),
    'near_pole':          (1.02e-05, 1.0, 1.0),
    'tpv_degree7_radial': (1.43e-05, 5.58, 1.0),
    'tpv_to_tan':         (2.08e-05, 7.73, 1.0),
    'tan_to_tpv':         (1.88e-05, 6.27, 1.0),
    'rot90':              (3.67e-06, 1.0, 1.0),
    'rot180':             (2.75e-06, 1.0, 1.0),
    'rot270':             (3.67e-06, 1.0, 1.0),
    'rot90_exact':        (2.96e-12, 1.0, 1.0),
    'mirrored':           (1.03e-05, 1.0, 1.0),
    'mirrored_rot90':     (3.67e-06, 1.0, 1.0),
    'finer_2x':           (1.67e-06, 1.0, 1.0),
    'coarser_2x':         (2.09e-05, 1.0, 1.0),
    'coarser_3x':         (2.11e-05, 1.0, 1.0),
    'quarter_shift':      (2.96e-12, 1.0, 1.0),
    'half_shift':         (2.96e-12, 1.0, 1.0),
}


class Scene(NamedTuple):
    win: object
    wout: object
    img: np.ndarray
    wgt: np.ndarray
    mask: np.ndarray


def _turn(w, deg, mirror=False):
    """``w`` with its CD matrix turned by a multiple of 90 degrees (exact 0 / +-1 factors) and, with ``mirror``,
    the x axis flipped first."""
    q = (deg // 90) % 4
    r = np.array([[1, 0], [0, 1]]) if q == 0 else np.array([[0, -1], [1, 0]]) if q == 1 else \
        np.array([[-1, 0], [0, -1]]) if q == 2 else np.array([[0, 1], [-1, 0]])
    m = np.diag([-1.0, 1.0]) if mirror else np.eye(2)
    w.cd = w.cd @ m @ r
    return w


def _scaled(w, factor):
    w.cd = w.cd * factor
    return w


def _high_tpv(w, amp):
    """Degree 5 - 7 and radial terms on top of ZTF's: with (u, v) around 0.4 degrees every term moves a pixel by a
    few hundredths to a few tenths of a pixel (2.8e-4 degrees) at ``amp`` = 1."""
    k = np.arange(17, 39)
    k = k[k != 23]
    rng = np.random.default_rng(77)
    for pv in (w.pv1, w.pv2):
        pv[k] = amp * rng.uniform(-1.0, 1.0, k.size) * np.where(k < 24, 1e-3, np.where(k < 31, 2e-3, 4e-3))
        pv[3] = amp * 1e-4 * rng.uniform(0.5, 1.0)
        pv[11] = -amp * 3e-4 * rng.uniform(0.5, 1.0)
    return w


def _wcs_pair(name):
    s = synth()
    ra0, dec0 = s.ZTF_CRVAL
    if name == 'crval_offset':
        # 31 arcsec along RA on the sky and 25.3 along dec: 40 arcsec
        off = (ra0 + 31.0 / 3600.0 / np.cos(np.deg2rad(dec0)), dec0 + 25.3 / 3600.0)
        return (s.ztf_wcs(220, 200, dx=0.37, dy=-0.41, rot_deg=0.3, tpv=True),
                s.ztf_wcs(200, 190, tpv=True, crval=off))
    if name == 'across_ra_zero':
        return (s.ztf_wcs(220, 200, dx=1.37, dy=-0.41, rot_deg=-0.2, tpv=True, crval=(359.995, dec0)),
                s.ztf_wcs(200, 190, tpv=True, crval=(0.004, dec0)))
    if name == 'near_pole':
        return (s.ztf_wcs(230, 230, dx=0.37, dy=-0.41, tpv=False, crval=(10.0, 89.99)),
                s.ztf_wcs(200, 190, tpv=False, crval=(100.0, 89.99)))
    if name == 'tpv_degree7_radial':
        win = _high_tpv(s.ztf_wcs(220, 200, dx=2.37, dy=-1.41, rot_deg=0.05, tpv=True), 0.25)
        wout = _high_tpv(s.ztf_wcs(200, 190, tpv=True), -0.15)
        for w in (win, wout):
            w.crpix = w.crpix + np.array([-1400.0, 1300.0])
        return win, wout
    if name == 'tpv_to_tan':
        return s.ztf_wcs(220, 200, dx=0.37, dy=-0.41, rot_deg=0.2, tpv=True), s.ztf_wcs(200, 190, tpv=False)
    if name == 'tan_to_tpv':
        return s.ztf_wcs(220, 200, dx=0.37, dy=-0.41, rot_deg=0.2, tpv=False), s.ztf_wcs(200, 190, tpv=True)
    if name in ('rot90', 'rot180', 'rot270'):
        deg = int(name[3:])
        return (_turn(s.ztf_wcs(200, 210, dx=DITHER[0], dy=DITHER[1], tpv=(deg == 180)), deg),
                s.ztf_wcs(200, 190, tpv=(deg == 180)))
    if name == 'rot90_exact':
        return _turn(s.tan_wcs(190, 200), 90), s.tan_wcs(200, 190)
    if name == 'mirrored':
        return _turn(s.ztf_wcs(220, 200, dx=DITHER[0], dy=DITHER[1], rot_deg=0.2, tpv=True), 0, True), \
            s.ztf_wcs(200, 190, tpv=True)
    if name == 'mirrored_rot90':
        return _turn(s.ztf_wcs(200, 210, dx=DITHER[0], dy=DITHER[1], tpv=False), 90, True), s.ztf_wcs(200, 190, tpv=False)
    if name == 'finer_2x':
        return s.tan_wcs(150, 140, dx=SCALE_DITHER[0], dy=SCALE_DITHER[1]), s.tan_wcs(260, 250, scale=2.81e-4 / 2)
    if name == 'coarser_2x':
        return (s.ztf_wcs(420, 400, dx=SCALE_DITHER[0], dy=SCALE_DITHER[1], rot_deg=0.2, tpv=False),
                _scaled(s.ztf_wcs(200, 190, tpv=False), 2.0))
    if name == 'coarser_3x':
        return (s.ztf_wcs(420, 400, dx=SCALE_DITHER[0], dy=SCALE_DITHER[1], rot_deg=0.2, tpv=False),
                _scaled(s.ztf_wcs(136, 130, tpv=False), 3.0))
    if name in ('quarter_shift', 'half_shift'):
        d = EXACT[name]
        return s.tan_wcs(210, 200, dx=d, dy=d), s.tan_wcs(200, 190)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene(name):
    win, wout = _wcs_pair(name)
    nx, ny = win.naxis
    seed = 4100 + SCENES.index(name)
    f = synth().make_frame(nx, ny, seed, win, nstars=max(40, nx * ny // 900), nbad=nx * ny // 300)
    mask = f['mask'].copy()
    rng = np.random.default_rng(seed + 1000)
    n = 12
    xs, ys = rng.integers(0, nx, n), rng.integers(0, ny, n)
    mask[ys, xs] |= np.array([1 << 16, 1 << 20, 1 << 30], np.int32)[np.arange(n) % 3]
    for a in (f['img'], f['wgt'], mask):
        a.setflags(write=False)
    return Scene(win, wout, f['img'], f['wgt'], mask)


def positions(name):
    """The oracle's 0-based input positions of every output pixel."""
    return _positions(name)


@functools.lru_cache(maxsize=None)
def _positions(name):
    sc = scene(name)
    onx, ony = sc.wout.naxis
    px, py = oresample.positions(to_oracle_wcs(sc.wout), to_oracle_wcs(sc.win), onx, ony)
    px.setflags(write=False)
    py.setflags(write=False)
    return px, py


@functools.lru_cache(maxsize=None)
def reference(name, kernel='LANCZOS3'):
    """(px, py, img, wgt, mask) of the oracle, computed once per session and read-only."""
    sc = scene(name)
    px, py = _positions(name)
    out = oresample.resample(sc.img, sc.wgt, px, py, KINDS[kernel], 1.0, sc.mask)
    for a in out:
        a.setflags(write=False)
    return (px, py) + tuple(out)


def covered(name, kernel='LANCZOS3'):
    sc = scene(name)
    px, py = _positions(name)
    nx, ny = sc.win.naxis
    if kernel == 'NEAREST':
        return oresample.position_on_frame(px, nx) & oresample.position_on_frame(py, ny)
    return oresample.coverage(px, py, nx, ny, KINDS[kernel])


def near_decision(name, kernel='LANCZOS3'):
    """Output pixels whose oracle position is within 2 delta0 of a snap threshold (or, NEAREST, of a half-integer)
    on either axis."""
    delta = 2.0 * BOUNDS[name][0]
    out = None
    for p in _positions(name):
        fr = p - np.floor(p)
        if kernel == 'NEAREST':
            near = np.abs(fr - 0.5) <= delta
        else:
            near = (np.abs(fr - oresample.SNAP) <= delta) | (np.abs(fr - (1.0 - oresample.SNAP)) <= delta)
        out = near if out is None else out | near
    return out


def nearest_candidates(name):
    """NEAREST with every tie broken both ways: the oracle at positions moved by -+1e-6 px along either axis, four
    (img, wgt, mask) triples.  For ``half_shift``, where every position is a tie."""
    sc = scene(name)
    px, py = _positions(name)
    e = 1e-6
    return [oresample.resample(sc.img, sc.wgt, px + sx * e, py + sy * e, oresample.NEAREST, 1.0, sc.mask)
            for sx in (-1, 1) for sy in (-1, 1)]


# ---- the kernel's positions in numpy float32 ------------------------------------------------------------------------

LSTEP, TW = 16, 64
# (tile rows, support_lo, support_hi) of the kernels' tile headers: k_resample with six and with two taps, the
# nearest-neighbour kernel
GEOMETRY = {'LANCZOS3': (32, -2, 3), 'BILINEAR': (32, 0, 1), 'NEAREST': (16, 0, 0)}


def emulated_positions(name, kernel='LANCZOS3'):
    sc = scene(name)
    return emulate_map(sc.win, sc.wout, kernel)


def emulate_map(win, wout, kernel='LANCZOS3'):
    """What the kernels make of a position: fp64 lattice nodes every 16 output pixels, the origin of the tile's
    bounding box subtracted, rounded to fp32, bilinear in fp32 along x and then along y (k_resample's statement
    order, every operation rounded on its own).  Returns absolute 0-based positions in fp64."""
    onx, ony = wout.naxis
    th, lo, hi = GEOMETRY[kernel]
    lnx, lny = (onx - 1) // LSTEP + 2, (ony - 1) // LSTEP + 2
    gy, gx = np.mgrid[0:lny, 0:lnx].astype(np.float64)
    nxp, nyp = map_out_to_in(to_oracle_wcs(wout), to_oracle_wcs(win), 1.0 + gx * LSTEP, 1.0 + gy * LSTEP)
    nxp, nyp = nxp - 1.0, nyp - 1.0
    ex, ey = np.empty((ony, onx)), np.empty((ony, onx))
    f32 = np.float32
    align = 4 if th == 32 else 2
    for oy0 in range(0, ony, th):
        for ox0 in range(0, onx, TW):
            rows = np.minimum(oy0 // LSTEP + np.arange(th // LSTEP + 1), lny - 1)
            cols = np.minimum(ox0 // LSTEP + np.arange(TW // LSTEP + 1), lnx - 1)
            bx, by = nxp[np.ix_(rows, cols)], nyp[np.ix_(rows, cols)]
            bx0 = (int(np.floor(bx.min())) + lo - 1) & ~(align - 1)
            by0 = int(np.floor(by.min())) + lo - 1
            rx, ry = (bx - bx0).astype(f32), (by - by0).astype(f32)
            h, w = min(th, ony - oy0), min(TW, onx - ox0)
            ty, tx = np.mgrid[0:h, 0:w]
            cell, crow = tx >> 4, ty >> 4
            fx, fy = ((tx & 15) / 16.0).astype(f32), ((ty & 15) / 16.0).astype(f32)
            res = []
            for r in (rx, ry):
                a0, a1 = r[crow, cell], r[crow, cell + 1]
                b0, b1 = r[crow + 1, cell], r[crow + 1, cell + 1]
                pa = a0 + fx * (a1 - a0)
                pb = b0 + fx * (b1 - b0)
                res.append(pa + fy * (pb - pa))
            assert res[0].dtype == f32
            ex[oy0:oy0 + h, ox0:ox0 + w] = res[0].astype(np.float64) + bx0
            ey[oy0:oy0 + h, ox0:ox0 + w] = res[1].astype(np.float64) + by0
    return ex, ey


@functools.lru_cache(maxsize=None)
def emulation(name):
    """(delta0, value deviation, weight deviation) of the emulated positions against the exact ones: delta0 the
    largest position error over the covered pixels of all three kernels' tile geometries, the deviations those of
    the LANCZOS3 products at the emulated positions from ``reference(name)`` in units of the existing bounds."""
    sc = scene(name)
    px, py, r_img, r_wgt, _ = reference(name)
    d0 = 0.0
    for kernel in KINDS:
        ex, ey = emulated_positions(name, kernel)
        c = covered(name, kernel)
        d0 = max(d0, float(np.abs(ex - px)[c].max()), float(np.abs(ey - py)[c].max()))
    ex, ey = emulated_positions(name, 'LANCZOS3')
    e_img, e_wgt, _ = oresample.resample(sc.img, sc.wgt, ex, ey, oresample.LANCZOS3, 1.0, None)
    both = (e_wgt > 0) & (r_wgt > 0)
    tol = RTOL * np.abs(r_img[both]) + ATOL * float(np.std(sc.img))
    dv = float((np.abs(e_img[both] - r_img[both]) / tol).max())
    dw = float((np.abs(e_wgt[both] - r_wgt[both]) / (WTOL * np.abs(r_wgt[both]))).max())
    return d0, dv, dw


def bound_for(dev):
    """The rule of the table: the existing bound where the emulation stays inside it, else 4 x the emulated
    deviation."""
    return 1.0 if dev <= 1.0 else 4.0 * dev


# ---- stacks for the fused coadd kernels --------------------------------------------------------------------------------

# 'turned': the stack the quarter turn belongs to; its tall footprints do not fit the fixed slot of k_coadd_fused_own, so
# the plan takes k_coadd_fused_dma with or without ZM_FF_FORM.  'upright': every footprint fits, k_coadd_fused_own runs.
STACKS = {'turned': ('crval_offset', 'rot90', 'mirrored'), 'upright': ('crval_offset', 'tan_to_tpv', 'mirrored')}
STACK_RTOL, STACK_ATOL = 3e-5, 3e-5 * 5.0            # the value bound of tests/test_coadd_gpu.py


@functools.lru_cache(maxsize=None)
def stack(which):
    """(frames, wout): three views of one star field on the output grid of ``crval_offset`` - that scene's input
    (tangent point 40 arcsec away, TPV), the mirrored frame of ``mirrored`` (TPV) and the quarter turn of ``rot90``
    (TAN) or the TAN frame of ``tan_to_tpv`` - with zero points 25.6, 25.9, 26.2.

    Stars of 1e3 to 2e4 counts.  The positions of these geometries are off by up to 1e-5 px (``BOUNDS``), which moves
    the steep flanks of a brighter star by more than the absolute term of the coadd bound (3e-5 x the noise of 5): at
    5e4 counts the emulated positions alone put 7 pixels of the turned CLIPPED stack beyond it, the same 7 the kernels
    do.  At 2e4 the emulation stays inside the bound on every pixel (tests/test_resample_scenes.py)."""
    s = synth()
    wout = scene('crval_offset').wout
    onx, ony = wout.naxis
    rng = np.random.default_rng(4300)
    xs, ys = rng.uniform(-30, onx + 30, 70), rng.uniform(-30, ony + 30, 70)
    fl = np.exp(rng.uniform(np.log(1e3), np.log(2e4), 70))
    ra, dec = wout.all_pix2world(xs, ys, 0)
    frames = []
    for i, name in enumerate(STACKS[which]):
        w = scene(name).win
        nx, ny = w.naxis
        f = s.make_frame(nx, ny, 4300 + i, w, star_sky=(ra, dec, fl), magzp=25.6 + 0.3 * i, nbad=nx * ny // 300)
        f['mask'][rng.integers(0, ny, 8), rng.integers(0, nx, 8)] |= 1 << 17
        for a in (f['img'], f['wgt'], f['mask']):
            a.setflags(write=False)
        frames.append(f)
    return tuple(frames), wout


@functools.lru_cache(maxsize=None)
def stack_reference(which, kind):
    """oracle_coadd of the stack: (img, wgt, mask, resampled values, resampled weights)."""
    frames, wout = stack(which)
    return oracle_coadd(list(frames), wout, kind)


def stack_emulation(which, kind):
    """The largest deviation of the coadd at emulated positions from ``stack_reference``, in units of the coadd bound
    (``STACK_RTOL |ref| + STACK_ATOL``), over the pixels valid in both."""
    from oracle import combine as ocombine
    frames, wout = stack(which)
    r_img, r_wgt = stack_reference(which, kind)[:2]
    vals, wgts = [], []
    for f in frames:
        ex, ey = emulate_map(f['wcs'], wout)
        fs = oresample.flux_scale(to_oracle_wcs(f['wcs']), to_oracle_wcs(wout), f['flxscale'])
        o, w, _ = oresample.resample(f['img'], f['wgt'], ex, ey, oresample.LANCZOS3, fs)
        vals.append(o)
        wgts.append(w)
    e_img, e_wgt, _ = ocombine.combine(np.array(vals), np.array(wgts), kind)
    both = (e_wgt > 0) & (r_wgt > 0)
    return float((np.abs(e_img - r_img)[both] / (STACK_RTOL * np.abs(r_img[both]) + STACK_ATOL)).max())
