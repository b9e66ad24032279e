"""Helpers shared by the tests (the only place product and oracle meet)."""
import importlib

import numpy as np

from oracle import background as oback
from oracle import combine as ocombine
from oracle import resample as oresample
from oracle.wcs import WCS as OWCS


def pkg():
    return importlib.import_module('zuds-pipeline_amd')


def synth():
    return importlib.import_module('zuds-pipeline_amd.synth')


def to_oracle_wcs(w):
    return OWCS(w.crpix, w.crval, w.cd, w.pv1 if w.has_pv else None,
                w.pv2 if w.has_pv else None, w.naxis)


def assert_close_masked(got, ref, rtol, atol, what='', max_bad_frac=0.0):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    tol = atol + rtol * np.abs(ref)
    bad = err > tol
    frac = bad.mean() if bad.size else 0.0
    if frac > max_bad_frac:
        i = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError(
            f'{what}: {bad.sum()} / {bad.size} elements off (frac {frac:.3e} > '
            f'{max_bad_frac:.1e}); worst at {i}: got {got[i]!r} ref {ref[i]!r}')


def oracle_coadd(frames, wout, kind, subtract_back=False, rescale=False,
                 clip_sigma=4.0, clip_ampfrac=0.3, mesh=128):
    onx, ony = wout.naxis
    ow = to_oracle_wcs(wout)
    vals, wgts, masks, cov = [], [], [], []
    for f in frames:
        wi = to_oracle_wcs(f['wcs'])
        px, py = oresample.positions(ow, wi, onx, ony)
        img = f['img'].astype(np.float64)
        wgt = None if f.get('wgt') is None else f['wgt'].astype(np.float64)
        if subtract_back or rescale:
            bkg, rms, bmean, bsig, _, _ = oback.background(img, wgt, mesh)
            if rescale and wgt is not None:
                with np.errstate(divide='ignore'):
                    var = np.where(wgt > 1e-30, 1.0 / np.where(wgt > 0, wgt, 1), 0.0)
                vb, vs = oback.mesh_maps(var, wgt, mesh)
                vbf, _ = oback.filter_maps(vb, vs, 3)
                level = oback.fqmedian(vbf.ravel())
                if level > 0 and bsig > 0:
                    wgt = wgt / (bsig * bsig / level)
            if subtract_back:
                img = img - bkg
        fs = oresample.flux_scale(wi, ow, f.get('flxscale', 1.0))
        o, w, m = oresample.resample(img, wgt, px, py, oresample.LANCZOS3, fs,
                                     f.get('mask'))
        vals.append(o)
        wgts.append(w)
        if m is not None:
            masks.append(m)
            nx, ny = f['wcs'].naxis
            cov.append(oresample.coverage(px, py, nx, ny))
    out, ow_, _ = ocombine.combine(np.array(vals), np.array(wgts), kind, clip_sigma, clip_ampfrac)
    om = None
    if masks:
        om, ocov = ocombine.combine_masks(np.array(masks), np.array(cov), 'AND')
    return out, ow_, om, np.array(vals), np.array(wgts)
