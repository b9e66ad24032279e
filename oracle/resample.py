"""Resample-to-reference-WCS restatement (oracle; test infrastructure).

Operator definition from the reference: ``RESAMPLING_TYPE LANCZOS3``,
``OVERSAMPLING 0``, ``INTERPOLATE N``, ``FSCALASTRO_TYPE FIXED``,
``FSCALE_KEYWORD FLXSCALE`` (``zuds/astromatic/makecoadd/default.swarp:51-67``),
``WEIGHT_THRESH 1e-30`` (``default.swarp:19``); called for coadds from
``zuds/coadd.py:133,156`` and for single-image alignment from
``zuds/swarp.py:157-204`` (``HasWCS.aligned_to`` ``zuds/fitsfile.py:290-314``).

Arithmetic (SWarp >= 2.38 ``interpolate.c`` as published; adopted conventions):

* taps: for fractional offset d from the floor pixel, offsets k = -2..+3,
  ``t_k = sin(x_k) / x_k**2`` with ``x_k = -pi/3 (d - k)`` and alternating
  sign, i.e. ``sinc(d-k) sinc((d-k)/3)`` up to a common factor; each 1-D 6-vector
  is normalised to unit sum;
* ``d < 1e-5`` (or ``d > 1 - 1e-5``: snapped to the next pixel) gives a delta;
* the variance plane is interpolated with the same (unsquared) taps;
* an output pixel is *bad* (value 0, weight 0) when a tap with non-zero weight
  falls outside the input frame - per axis: the 6-tap footprint, or for a delta
  kernel (every other tap is exactly 0) its centre pixel only, so that identity /
  integer-shift alignments keep their borders, as SWarp's edge-truncated kernels
  do - when any tap with non-zero weight lands on a bad input pixel
  (weight <= WEIGHT_THRESH, or a value that is NaN or +-inf), when the interpolated variance is <= 0, or when it
  is >= BADVAR_TEST (below);
* flux: ``out = interp * fscale``, variance ``* fscale**2`` where ``fscale`` =
  FLXSCALE x (A_out / A_in) (fixed pixel-area ratio).

Non-finite values and the bad-tap rule (the convention the HIP kernels follow): an input pixel is bad when its
weight is at or below WEIGHT_THRESH or when its value is not finite (NaN, +inf, -inf; ZTF frames carry NaN
pixels, ``zuds/constants.py:59``), with or without a weight map and for every kernel, NEAREST included.  A bad
input pixel takes part as value 0 and variance BIGVAR.  An output is bad when its interpolated variance, in the
units of 1 / weight (var_scale / weight on the device; this function's callers fold var_scale into ``wgt``), is
``>= BADVAR_TEST = 1e14``: that is how the kernels tell a BIGVAR tap from good ones under any non-zero tap, and
there is no cheap exact alternative.  It also makes a good pixel whose weight lies between WEIGHT_THRESH and about
1e-14 (a variance of 1e14 and more, in the same units) bad, where SWarp's ``WEIGHT_THRESH 1e-30`` alone would keep
it; realistic ZTF weights (1e-4 to 1e-1) sit ten decades away from that edge.

Integer masks go through the same footprint (``mask.swarp`` keeps
``RESAMPLING_TYPE LANCZOS3``): output mask = bitwise OR of every input mask
pixel whose tap weight is non-zero.  Chosen convention, see DESIGN.md.

Round 6: the two places where SWarp's own behaviour is known to differ from the conventions above are
OPTIONS (defaults unchanged), so that a pixel-for-pixel comparison with real SWarp output can pick them:

* ``edge='truncate'`` (``EDGE_TRUNCATE``): SWarp's interpolation truncates the kernel at the frame edge - an output
  pixel whose POSITION lies on the input frame (nearest input pixel on the frame) is computed from the taps that
  are on the frame, the others dropped, nothing renormalised (flux falls off over the last three pixels, the
  interpolated variance with it, so the weight grows: SWarp's weight maps show that rim); a dropped tap is not a
  bad pixel.  Default ``edge='zero'``: such pixels get value 0 / weight 0 (=> bit 16).
* ``mask_resample='lanczos_round'``: SWarp resamples an integer mask as the image it is (``mask.swarp:25`` changes
  the combine type, not ``RESAMPLING_TYPE LANCZOS3``): the interpolated value of the integers, rounded to the
  nearest integer (half to even, fp32 storage) - bit patterns that mean nothing where neighbouring pixels
  differ; no weights are involved (``WEIGHT_TYPE NONE``).  Default ``'or'``.
"""
import numpy as np

from .wcs import map_out_to_in

LANCZOS3, BILINEAR, NEAREST = 3, 1, 0
SNAP = 1e-5
BIGVAR = 1e30
BADVAR_TEST = 1e14      # an interpolated variance at or above this: a bad tap was hit (module docstring)
WEIGHT_THRESH = 1e-30


def lanczos3_taps(d):
    """Unit-sum Lanczos-3 taps for fractional offsets d in [SNAP, 1-SNAP].

    Returns array (..., 6) for pixel offsets k = -2..3 from the floor pixel.
    """
    d = np.asarray(d, dtype=np.float64)
    k = np.arange(-2, 4, dtype=np.float64)
    x = (d[..., None] - k)                      # distance in pixels
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.sin(np.pi * x) * np.sin(np.pi * x / 3.0) / (x * x)
    t = np.where(x == 0.0, np.pi * np.pi / 3.0, t)
    return t / t.sum(axis=-1, keepdims=True)


def split_position(p):
    """0-based continuous position -> (floor index, taps-ready fraction, delta?)."""
    i = np.floor(p)
    d = p - i
    up = d > 1.0 - SNAP
    i = np.where(up, i + 1, i)
    d = np.where(up, 0.0, d)
    delta = d < SNAP
    d = np.where(delta, 0.0, d)
    return i.astype(np.int64), d, delta


def on_frame(i, delta, n, kind):
    """Do the non-zero taps of one axis lie on the frame?  i: floor index, delta: snapped
    (delta kernel: only the centre tap at i is non-zero), n: axis length."""
    nt, off = (6, -2) if kind == LANCZOS3 else (2, 0)
    full = (i + off >= 0) & (i + off + nt <= n)
    centre = (i >= 0) & (i < n)
    return np.where(delta, centre, full)


EDGE_ZERO, EDGE_TRUNCATE = 'zero', 'truncate'
MASK_OR, MASK_LANCZOS_ROUND = 'or', 'lanczos_round'


def position_on_frame(p, n):
    """EDGE_TRUNCATE: the pixel nearest to the position lies on the axis of length n."""
    j = np.floor(p + 0.5)
    return (j >= 0) & (j < n)


def coverage(px, py, nx, ny, kind=LANCZOS3, edge=EDGE_ZERO):
    """Boolean map of the output pixels that get a value: all non-zero taps on the nx x ny frame (EDGE_ZERO) or
    the position itself on the frame (EDGE_TRUNCATE)."""
    if edge == EDGE_TRUNCATE:
        return position_on_frame(px, nx) & position_on_frame(py, ny)
    ix, _, ddx = split_position(px)
    iy, _, ddy = split_position(py)
    return on_frame(ix, ddx, nx, kind) & on_frame(iy, ddy, ny, kind)


def taps_for(d, delta, kind):
    if kind == LANCZOS3:
        t = lanczos3_taps(np.where(delta, 0.5, d))
        dl = np.zeros(6)
        dl[2] = 1.0
        t = np.where(delta[..., None], dl, t)
        return t, -2
    if kind == BILINEAR:
        t = np.stack([1.0 - d, d], axis=-1)
        return t, 0
    raise ValueError(kind)


def positions(wout, win, onx, ony):
    """0-based input positions of every output pixel: arrays (ony, onx)."""
    yo, xo = np.mgrid[1:ony + 1, 1:onx + 1].astype(np.float64)
    xi, yi = map_out_to_in(wout, win, xo, yo)
    return xi - 1.0, yi - 1.0


def resample(img, wgt, px, py, kind=LANCZOS3, fscale=1.0, mask=None,
             chunk=256, edge=EDGE_ZERO, mask_resample=MASK_OR, debug=None):
    """Resample ``img`` (and weight map ``wgt`` = 1/var, may be None = all 1).

    px, py: 0-based input positions per output pixel.  Returns
    (out_img, out_wgt, out_mask_or_None), float64 / int64.  ``edge`` / ``mask_resample``: module docstring.
    ``debug``: a dict that receives 'mask_float', the interpolated mask before rounding (tests compare a device that
    evaluates fp32 table taps with it: the integers agree except within rounding distance of a half), and 'vacc', the
    interpolated variance of every covered output without a bad tap (0 elsewhere; not for NEAREST).
    """
    img = np.asarray(img, dtype=np.float64)
    ny, nx = img.shape
    if wgt is None:
        var = np.ones_like(img)
    else:
        w = np.asarray(wgt, dtype=np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            var = np.where(w > WEIGHT_THRESH, 1.0 / np.where(w > 0, w, 1.0), BIGVAR)
    # a non-finite value is a bad input pixel: value 0, variance BIGVAR
    finite = np.isfinite(img)
    img = np.where(finite, img, 0.0)
    var = np.where(finite, var, BIGVAR)
    bad_in = var >= BIGVAR
    oshape = px.shape
    out = np.zeros(oshape)
    outw = np.zeros(oshape)
    outm = None if mask is None else np.zeros(oshape, dtype=np.int64)
    if kind == NEAREST:
        ix = np.floor(px + 0.5).astype(np.int64)
        iy = np.floor(py + 0.5).astype(np.int64)
        ok = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
        ixc = np.clip(ix, 0, nx - 1)
        iyc = np.clip(iy, 0, ny - 1)
        v = var[iyc, ixc]
        good = ok & ~bad_in[iyc, ixc] & (v > 0) & (v < BADVAR_TEST)
        out = np.where(good, img[iyc, ixc] * fscale, 0.0)
        with np.errstate(divide='ignore'):
            outw = np.where(good, 1.0 / (v * fscale * fscale), 0.0)
        if mask is not None:
            outm = np.where(ok, mask[iyc, ixc], 0).astype(np.int64)
        return out, outw, outm

    for r0 in range(0, oshape[0], chunk):
        sl = slice(r0, min(r0 + chunk, oshape[0]))
        ix, dx, ddx = split_position(px[sl])
        iy, dy, ddy = split_position(py[sl])
        tx, off = taps_for(dx, ddx, kind)
        ty, _ = taps_for(dy, ddy, kind)
        nt = tx.shape[-1]
        x0 = ix + off
        y0 = iy + off
        trunc = edge == EDGE_TRUNCATE
        if trunc:
            inb = position_on_frame(px[sl], nx) & position_on_frame(py[sl], ny)
        else:
            inb = on_frame(ix, ddx, nx, kind) & on_frame(iy, ddy, ny, kind)
        acc = np.zeros(ix.shape)
        vacc = np.zeros(ix.shape)
        anybad = np.zeros(ix.shape, dtype=bool)
        macc = np.zeros(ix.shape, dtype=np.int64)
        mflt = np.zeros(ix.shape)
        for r in range(nt):
            yy = np.clip(y0 + r, 0, ny - 1)
            for c in range(nt):
                xx = np.clip(x0 + c, 0, nx - 1)
                wt = ty[..., r] * tx[..., c]
                if trunc:           # taps off the frame are dropped: they add nothing and flag nothing
                    wt = np.where((y0 + r >= 0) & (y0 + r < ny) & (x0 + c >= 0) & (x0 + c < nx), wt, 0.0)
                acc += wt * img[yy, xx]
                vacc += wt * np.where(bad_in[yy, xx], 0.0, var[yy, xx])
                nz = wt != 0.0
                anybad |= nz & bad_in[yy, xx]
                if mask is not None:
                    macc |= np.where(nz, mask[yy, xx], 0)
                    mflt += wt * mask[yy, xx]            # (the mask as the image SWarp takes it for)
        good = inb & ~anybad & (vacc > 0) & (vacc < BADVAR_TEST)
        if debug is not None:
            debug.setdefault('vacc', np.zeros(oshape))[sl] = np.where(inb & ~anybad, vacc, 0.0)
        if mask is not None and mask_resample == MASK_LANCZOS_ROUND:
            macc = np.rint(mflt).astype(np.int64)
            if debug is not None:
                debug.setdefault('mask_float', np.zeros(oshape))[sl] = np.where(inb, mflt, 0.0)
        out[sl] = np.where(good, acc * fscale, 0.0)
        with np.errstate(divide='ignore', invalid='ignore'):
            outw[sl] = np.where(good, 1.0 / (vacc * fscale * fscale), 0.0)
        if mask is not None:
            outm[sl] = np.where(inb, macc, 0)
    return out, outw, outm


def flux_scale(win, wout, flxscale=1.0):
    """FLXSCALE x fixed pixel-area ratio A_out / A_in (FSCALASTRO_TYPE FIXED).

    A_in at the input frame centre, A_out at the output pixel the centre maps to.
    """
    a_in = win.pixel_area()
    cx = (win.naxis[0] + 1) / 2.0
    cy = (win.naxis[1] + 1) / 2.0
    xo, yo = map_out_to_in(win, wout, np.float64(cx), np.float64(cy))
    a_out = wout.pixel_area(float(xo), float(yo))
    return flxscale * a_out / a_in
