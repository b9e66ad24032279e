"""Measures, on the CPU and against the oracle alone, the two coefficients of the tolerance of
tests/test_background_regimes_gpu.py (``a |ref| + b rms_ref``) and prints the per-scene table of DESIGN.md section 2.

    python tests/measure_mesh_tolerances.py

a: the float32 floor.  The kernels store the filtered node maps as floats and evaluate the spline in fp32; the oracle
   does both in fp64.  Measured: the oracle as it is against the oracle with its node maps rounded to float32 and
   ``expand`` evaluated in float32 numpy, worst |difference| / |ref| over the pixels of both maps, with |ref| taken
   as ``mesh_scenes.envelope`` (the map's magnitude without cancellation between the spline's terms).
b: the oracle's sensitivity to the last bit of the two non-integer inputs of the quantisation.  ``mean32`` and
   ``sig32`` of every mesh are nudged by +-1 float32 ulp (four combinations), the rest of the oracle runs unchanged;
   worst change of the final maps in units of ``rms_ref`` (the envelope of the rms map, floored by the float32
   spacing of the reference value).
   A mesh whose clipped sigma is exactly 0 is not nudged: its variance is an exact zero on every path.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_scenes as ms                      # noqa: E402
from oracle import background as oback        # noqa: E402

f32 = np.float32


def spline_derivs32(a):
    n = a.shape[0]
    d = np.zeros_like(a, dtype=f32)
    if n < 3:
        return d
    u = np.zeros_like(a, dtype=f32)
    for y in range(1, n - 1):
        temp = (f32(-1.0) / (d[y - 1] + f32(4.0))).astype(f32)
        d[y] = temp
        u[y] = temp * (u[y - 1] - f32(6.0) * (a[y + 1] + a[y - 1] - f32(2.0) * a[y]))
    d[n - 1] = 0.0
    for y in range(n - 2, 0, -1):
        d[y] = d[y] * d[y + 1] + u[y]
    d[0] = 0.0
    return (d * f32(1.0 / 6.0)).astype(f32)


def eval_axis32(nodes, derivs, npix, mesh):
    n = nodes.shape[0]
    t = ((np.arange(npix, dtype=f32) + f32(0.5)) * f32(1.0 / mesh) - f32(0.5)).astype(f32)
    if n < 2:
        return np.repeat(nodes[:1], npix, axis=0)
    i0 = np.clip(np.floor(t).astype(np.int64), 0, n - 2)
    dy = (t - i0.astype(f32)).astype(f32)
    dy1 = (f32(1.0) - dy).astype(f32)
    cdy = (dy * dy * dy - dy).astype(f32)
    cdy1 = (dy1 * dy1 * dy1 - dy1).astype(f32)
    shp = (npix,) + (1,) * (nodes.ndim - 1)
    out = (dy1.reshape(shp) * nodes[i0] + dy.reshape(shp) * nodes[i0 + 1]
           + cdy1.reshape(shp) * derivs[i0] + cdy.reshape(shp) * derivs[i0 + 1])
    assert out.dtype == f32
    return out


def expand32(nodes, nx, ny, mesh):
    """oracle.background.expand with float32 nodes and float32 arithmetic throughout."""
    nodes = nodes.astype(f32)
    rows = eval_axis32(nodes, spline_derivs32(nodes), ny, mesh)
    rt = np.ascontiguousarray(rows.T)
    return eval_axis32(rt, spline_derivs32(rt), nx, mesh).T


def stats_nudged(dm, ds):
    """oracle.background.mesh_histogram_stats with mean32 / sig32 moved by dm / ds float32 ulps."""
    def stats(pix):
        n = pix.size
        if n == 0:
            return None
        mean = pix.mean()
        sig = pix.var()
        sig = np.sqrt(sig) if sig > 0 else 0.0
        sel = pix[(pix >= mean - 2.0 * sig) & (pix <= mean + 2.0 * sig)]
        npix = sel.size
        if npix == 0:
            return None
        mean = sel.mean()
        sig = sel.var()
        sig = np.sqrt(sig) if sig > 0 else 0.0
        nlevels = min(int(np.sqrt(2.0 / np.pi) * oback.QUANTIF_NSIGMA / oback.QUANTIF_AMIN * npix + 1),
                      oback.QUANTIF_NMAXLEVELS)
        mean32, sig32 = f32(mean), f32(sig)
        if sig32 > 0:
            if dm:
                mean32 = np.nextafter(mean32, f32(np.inf * dm))
            if ds:
                sig32 = np.nextafter(sig32, f32(np.inf * ds))
        qscale = f32(2.0 * oback.QUANTIF_NSIGMA * np.float64(sig32) / nlevels) if sig32 > 0 else f32(1.0)
        qzero = f32(np.float64(mean32) - oback.QUANTIF_NSIGMA * np.float64(sig32))
        cste = f32(0.499999 - np.float64(qzero / qscale))
        b = np.trunc(pix.astype(f32) / qscale + cste).astype(np.int64)
        b = b[(b >= 0) & (b < nlevels)]
        histo = np.bincount(b, minlength=nlevels).astype(np.int64)
        return dict(mean=float(mean32), sigma=float(sig32), qzero=float(qzero), qscale=float(qscale),
                    nlevels=nlevels, histo=histo)
    return stats


def spacing32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(f32)).astype(np.float64)


def measure(img, wgt, mesh, fsizes=(3, 1)):
    """-> (a ratio, b ratio) of one frame."""
    ny, nx = img.shape
    i64 = img.astype(np.float64)
    w64 = None if wgt is None else wgt.astype(np.float64)
    back, sigm = oback.mesh_maps(i64, w64, mesh)
    # the unnudged copy must be the oracle itself
    keep = oback.mesh_histogram_stats
    try:
        oback.mesh_histogram_stats = stats_nudged(0, 0)
        b0, s0 = oback.mesh_maps(i64, w64, mesh)
        assert np.array_equal(b0, back) and np.array_equal(s0, sigm)
        nudged = []
        for dm in (-1, 1):
            for ds in (-1, 1):
                oback.mesh_histogram_stats = stats_nudged(dm, ds)
                nudged.append(oback.mesh_maps(i64, w64, mesh))
    finally:
        oback.mesh_histogram_stats = keep
    a = b = 0.0
    for fs in fsizes:
        bo, so = oback.filter_maps(back, sigm, fs)
        ref = [oback.expand(bo, nx, ny, mesh), oback.expand(so, nx, ny, mesh)]
        env = [ms.envelope(bo, nx, ny, mesh), ms.envelope(so, nx, ny, mesh)]
        low = [expand32(bo, nx, ny, mesh), expand32(so, nx, ny, mesh)]
        for r, e, l in zip(ref, env, low):
            d = np.abs(l.astype(np.float64) - r)
            nz = e > 0
            assert not d[~nz].any()
            if nz.any():
                a = max(a, float((d[nz] / e[nz]).max()))
        for nb, ns in nudged:
            nbo, nso = oback.filter_maps(nb, ns, fs)
            for r, nodes in zip(ref, (nbo, nso)):
                d = np.abs(oback.expand(nodes, nx, ny, mesh) - r)
                pos = env[1] > 0          # (constant meshes: rms_ref is 0 and nothing may move)
                assert not d[~pos].any()
                if pos.any():
                    b = max(b, float((d[pos] / np.maximum(env[1], spacing32(r))[pos]).max()))
    return a, b


def main():
    worst_a = worst_b = 0.0
    print('| scene | census (all six geometries: bad / mode / median / sig0 / lowsig / capped of meshes) '
          '| worst a ratio | worst b ratio |')
    print('|---|---|---|---|')
    for name in ms.SCENES:
        sa = sb = 0.0
        cen = dict.fromkeys(('meshes', 'bad', 'mode', 'median', 'sig0', 'lowsig', 'capped'), 0)
        for (nx, ny), mesh in ms.GEOMETRIES:
            img, wgt, c = ms.scene(name, nx, ny, mesh)
            assert ms.census_ok(name, c, mesh), (name, nx, ny, mesh)
            for k in cen:
                cen[k] += c[k]
            a, b = measure(img, wgt, mesh)
            sa, sb = max(sa, a), max(sb, b)
        print('| %s | %d / %d / %d / %d / %d / %d of %d | %.3g | %.3g |' % (
            name, cen['bad'], cen['mode'], cen['median'], cen['sig0'], cen['lowsig'], cen['capped'], cen['meshes'],
            sa, sb), flush=True)
        worst_a, worst_b = max(worst_a, sa), max(worst_b, sb)
    for case in ms.GOOD_FRACTION_CASES:
        img, wgt, mesh, nbad = ms.good_fraction(*case)
        a, b = measure(img, wgt, mesh)
        print('| good fraction %s | %d bad | %.3g | %.3g |' % ('/'.join(map(str, case)), nbad, a, b), flush=True)
        worst_a, worst_b = max(worst_a, a), max(worst_b, b)
    print('worst a ratio %.4g -> a = 4 x = %.4g' % (worst_a, 4 * worst_a))
    print('worst b ratio %.4g -> b = 2 x = %.4g' % (worst_b, 2 * worst_b))


if __name__ == '__main__':
    main()
