"""A numpy restatement of the fake-source injection (``zuds-pipeline_amd/fakes.py``, ``csrc/inject.hip``), independent of
the library: the profile of a fake goes through the explicit 1-D interpolation matrices of ``psf_ref.interp_matrix``
(the kernel walks six taps per axis), the fakes are added one at a time in index order (the kernel launches layers), and
the layers come from an O(n^2) longest-path computation (the library hashes cells).

Every function takes ``T``, the type of its arithmetic: ``numpy.float64`` is the restatement the GPU is held to,
``numpy.longdouble`` the same statements in extended precision, which ``tests/measure_inject_tolerance.py`` compares
against the float64 run to set the tolerances below.  Which pixels lie in a box, in the frame or inside the core radius
is decided in float64 in both.

Definitions the kernel and this file share (include/zudsmi.h, DESIGN.md "Fake sources"):
  * ``ix = floor(x + 0.5)``, ``fx = x - ix``; ``P_ij`` = the model interpolated at ``(i - fx, j - fy)`` (taps of
    ``psf_ref.taps``; the model is 0 outside its grid); box ``|i|, |j| <= half + 3`` clipped to the frame;
  * image: box pixels inside the frame with ``v = flux P_ij != 0`` become ``float32(float64(img) + v)``; nothing else is
    written;
  * rms (given, gain > 0): the same pixels with ``v > 0`` and a finite positive rms become
    ``float32(sqrt(rms^2 + v / gain))``;
  * ``out_sum = flux * sum(P_ij)`` over the pixels written; flags as ``ZM_INJ_*``;
  * layer = 1 + the largest layer among the earlier fakes with ``|ix_a - ix_b| <= 2 (half + 3)`` in x and in y; 0 for a
    position that is not finite.

Tolerances (GPU against the float64 run of this file).  tests/measure_inject_tolerance.py prints the largest difference
between the float64 and the longdouble run of this file on the scenes of tests/inject_scenes.py; each constant is 4 x that,
rounded up to a power of two (the project's convention).  Nothing the GPU produced enters them; tests/test_inject_ref.py
holds them to the script's output.
  INJ_TOL    ``flux * P`` of a written pixel, relative to ``|img| + |flux P|``: the slack of the pixel rule below
  SUM_RTOL   ``out_sum``, relative
  RMS_TOL    the new rms of a pixel the rms rule writes, relative to it: the slack of the pixel rule on the rms plane

The pixel rule for a float32 output (``pixel_rule``): a pixel passes if it equals ``float32(want64)`` bit for bit; it also
passes if it is that value's float32 neighbour on the side of ``want64`` and ``want64`` lies within the slack of the midpoint
between the two.  At most ``MAX_NEAR`` pixels of a scene may need the second clause.
"""
import numpy as np

import psf_ref as pr

INJ_TOL = 2.0 ** -46
SUM_RTOL = 2.0 ** -49
RMS_TOL = 2.0 ** -46
# what tests/measure_inject_tolerance.py printed: the largest float64 - longdouble differences behind the constants above
MEASURED = dict(inj=2.261e-15, sum_rel=4.333e-16, rms_rel=1.96e-15)
MAX_NEAR = 8

CLIPPED, OUTSIDE, BAD, NONFINITE, BADPOS = 1, 2, 4, 8, 16
PAD = 3
F64 = np.float64


def profile(model, x, y, T=F64):
    """P over the whole box of a fake at the finite position (x, y): array [2 m + 1, 2 m + 1], entry (j + m, i + m), with
    m = half + 3, and (ix, iy, fx, fy) in float64."""
    model = np.asarray(model, dtype=T)
    w = model.shape[0]
    half = (w - 1) // 2
    m = half + PAD
    ixd, iyd = float(np.floor(x + 0.5)), float(np.floor(y + 0.5))
    fx, fy = float(x) - ixd, float(y) - iyd
    off = np.arange(-m, m + 1).astype(T)
    Mx, _, _ = pr.interp_matrix(off - T(fx) + T(half), w, T)
    My, _, _ = pr.interp_matrix(off - T(fy) + T(half), w, T)
    return My @ model @ Mx.T, ixd, iyd, fx, fy


def inject(img, x, y, flux, model, rms=None, mask=None, bad_bits=0, gain=0.0, core_radius=6.0, T=F64):
    """The fakes added one at a time in index order.  Returns a dict: ``img`` / ``rms`` (new float32 planes; rms None when
    none was given), ``out_sum`` (T), ``flags`` (int32), and per pixel of the LAST write ``nwrites`` (int), ``base`` (the
    float32 value before it), ``v`` (T); the same for the rms plane as ``rms_nwrites``, ``rms_base``, ``rms_want`` (T, the
    unrounded new rms)."""
    img = np.array(img, dtype=np.float32)
    ny, nx = img.shape
    rms = None if rms is None else np.array(rms, dtype=np.float32)
    model = np.asarray(model)
    half = (model.shape[0] - 1) // 2
    m = half + PAD
    x, y, flux = (np.atleast_1d(np.asarray(v, dtype=F64)) for v in (x, y, flux))
    n = x.size
    out_sum = np.zeros(n, dtype=T)
    flags = np.zeros(n, np.int32)
    nwrites = np.zeros((ny, nx), np.int64)
    base = np.zeros((ny, nx), np.float32)
    vlast = np.zeros((ny, nx), dtype=T)
    rms_nwrites = np.zeros((ny, nx), np.int64)
    rms_base = np.zeros((ny, nx), np.float32)
    rms_want = np.zeros((ny, nx), dtype=T)
    jj, ii = np.meshgrid(np.arange(-m, m + 1), np.arange(-m, m + 1), indexing='ij')
    for s in range(n):
        if not (np.isfinite(x[s]) and np.isfinite(y[s]) and np.isfinite(flux[s])):
            flags[s], out_sum[s] = BADPOS, np.nan
            continue
        P, ixd, iyd, fx, fy = profile(model, x[s], y[s], T)
        px, py = ixd + ii.astype(F64), iyd + jj.astype(F64)
        inside = (px >= 0) & (py >= 0) & (px < nx) & (py < ny)
        fl = 0
        if not inside.all():
            fl |= CLIPPED
        if not inside.any():
            flags[s] = fl | OUTSIDE
            continue
        cx, cy = px[inside].astype(np.int64), py[inside].astype(np.int64)
        if mask is not None:
            ddx, ddy = ii.astype(F64) - fx, jj.astype(F64) - fy
            core = (ddx * ddx + ddy * ddy <= float(core_radius) * float(core_radius))[inside]
            if ((np.asarray(mask)[cy, cx].astype(np.int64) & int(bad_bits)) != 0)[core].any():
                fl |= BAD
        v = T(flux[s]) * P[inside]
        wr = v != 0
        cx, cy, v, Pw = cx[wr], cy[wr], v[wr], P[inside][wr]
        old = img[cy, cx]
        if not np.isfinite(old).all():
            fl |= NONFINITE
        with np.errstate(invalid='ignore', over='ignore'):
            img[cy, cx] = (old.astype(T) + v).astype(np.float32)
        nwrites[cy, cx] += 1
        base[cy, cx] = old
        vlast[cy, cx] = v
        out_sum[s] = T(flux[s]) * Pw.sum(dtype=T)
        flags[s] = fl
        if rms is not None and gain > 0:
            sg = rms[cy, cx]
            with np.errstate(invalid='ignore'):
                ok = (v > 0) & np.isfinite(sg) & (sg > 0)
            want = np.sqrt(sg[ok].astype(T) * sg[ok].astype(T) + v[ok] / T(gain))
            rms[cy[ok], cx[ok]] = want.astype(np.float32)
            rms_nwrites[cy[ok], cx[ok]] += 1
            rms_base[cy[ok], cx[ok]] = sg[ok]
            rms_want[cy[ok], cx[ok]] = want
    return dict(img=img, rms=rms, out_sum=out_sum, flags=flags, nwrites=nwrites, base=base, v=vlast, rms_nwrites=rms_nwrites,
                rms_base=rms_base, rms_want=rms_want)


def layers(x, y, half):
    """(layer int32 [n], number of layers) by the definition: every earlier fake is looked at."""
    x, y = np.atleast_1d(np.asarray(x, dtype=F64)), np.atleast_1d(np.asarray(y, dtype=F64))
    n = x.size
    sep = 2.0 * (half + PAD)
    fin = np.isfinite(x) & np.isfinite(y)
    with np.errstate(invalid='ignore'):
        ix, iy = np.floor(x + 0.5), np.floor(y + 0.5)
    lay = np.zeros(n, np.int32)
    for k in range(n):
        if not fin[k]:
            continue
        with np.errstate(invalid='ignore', over='ignore'):
            hit = fin[:k] & (np.abs(ix[:k] - ix[k]) <= sep) & (np.abs(iy[:k] - iy[k]) <= sep)
        lay[k] = 1 + (lay[:k][hit].max() if hit.any() else 0)
    return lay, int(lay.max()) if n else 0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.view(np.uint32) == b.view(np.uint32)


def pixel_rule(got, want64, slack):
    """(passes, needed the second clause) per pixel: ``got`` float32 against the unrounded ``want64`` (float64) with the
    absolute ``slack`` of the second clause.  A value that is not finite passes when both are NaN, or the same infinity."""
    got = np.asarray(got, dtype=np.float32)
    want64 = np.asarray(want64, dtype=F64)
    with np.errstate(over='ignore', invalid='ignore'):
        r = want64.astype(np.float32)
        exact = same_bits(got, r) | (np.isnan(got) & np.isnan(r))
        side = np.where(want64 > r.astype(F64), np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        nb = np.nextafter(r, side)
        mid = 0.5 * (r.astype(F64) + nb.astype(F64))
        near = ~exact & (want64 != r.astype(F64)) & np.isfinite(want64) & same_bits(got, nb) & (np.abs(want64 - mid) <= slack)
    return exact | near, near
