"""Measures the two bounds tests/test_photcal_ref.py and tests/test_photcal_gpu.py quote, from the restatement's own
error (tests/photcal_ref.py); the GPU is never its own yardstick.  No GPU needed:  python tests/measure_photcal_tolerance.py

1. APCOR_ANALYTIC_TOL.  On a noiseless circular Gaussian the aperture corrections are analytic,
   ``-2.5 log10((1 - exp(-r_ref^2 / 2 s^2)) / (1 - exp(-r_k^2 / 2 s^2)))``.  The restatement sums pixels: each pixel
   holds the integral of the Gaussian over its square, and the exact circle / pixel overlap weights that mean value, so
   what is left is the pixel-integration error - the Gaussian is not constant across the pixels the circle cuts.  It is
   measured here twice: against the analytic value, and against a rendering 64 x oversampled in each axis whose samples
   are summed by the centre rule, over 25 sub-pixel centres.  The bound, one per radius, is 2 x the larger, rounded up
   to one digit.

2. CARD_TOL (kept in tests/photcal_ref.py).  A card is a selected star's magnitude difference.  Its rounding error is
   propagated here from the roundings of the restatement's float64 sums on the end-to-end frame (n eps sum |v frac|, the
   second term of ``aperture_ref.sums_bounds``; its first term is an allowance for the kernel's closed form, not an
   error of the quadrature used here), 1.0857 (b_ref / F_ref + b_k / F_k) per star.  Beside it stands the largest
   difference of a card between that float64 run and ``extended_cards``: the same pipeline on the same frame with every
   sum, logarithm, median and square root in ``numpy.longdouble``.  The tolerance is 4 x the larger of the two, rounded up
   to a power of two.  What the GPU admits in its sums is not part of it.
"""
import functools
import importlib
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import photcal_ref as pr  # noqa: E402
import photcal_scenes as ps  # noqa: E402

RADII = (1.0, 1.5, 2.0, 3.0, 5.0, 7.0, 10.0)
# mag per radius, printed by main() below (the Gaussian has sigma 1.02 px: small apertures cut pixels it varies across)
APCOR_ANALYTIC_TOL = {1.0: 0.4, 1.5: 0.3, 2.0: 0.2, 3.0: 0.03, 5.0: 6e-05, 7.0: 3e-09}


def _erf(v):
    return np.vectorize(math.erf)(v)


def integrated_gaussian(n, cx, cy, flux, fwhm):
    """An n x n image whose pixels hold the integral of a circular Gaussian over their squares."""
    s = fwhm / ps.K_FWHM
    e = np.arange(n + 1) - 0.5
    fx = 0.5 * np.diff(_erf((e - cx) / (s * math.sqrt(2.0))))
    fy = 0.5 * np.diff(_erf((e - cy) / (s * math.sqrt(2.0))))
    return flux * np.outer(fy, fx)


def noiseless_apcor(cx, cy, radii, n=80, flux=1.0e5):
    """``-2.5 log10(F_ref / F_k)`` of the restatement on a noiseless Gaussian of FWHM 2.4 px (the last radius is the
    reference aperture)."""
    img = integrated_gaussian(n, cx, cy, flux, ps.FWHM)
    g = pr.growth(img, [cx], [cy], radii, r_in=14.0, r_out=18.0, kappa=3.0, maxiter=0)
    f = g['flux'][0]
    return [-2.5 * math.log10(f[-1] / fk) for fk in f[:-1]]


def oversampled_apcor(cx, cy, radii, over=64, flux=1.0e5):
    """The same from point samples of the Gaussian on a grid ``over`` times finer, summed by the centre rule."""
    s = ps.FWHM / ps.K_FWHM
    half = int(math.ceil(radii[-1])) + 1
    u = (np.arange(-half * over, half * over) + 0.5) / over
    g = np.exp(-0.5 * (u[None, :] ** 2 + u[:, None] ** 2) / (s * s)) * flux / (2 * math.pi * s * s) / over ** 2
    r2 = u[None, :] ** 2 + u[:, None] ** 2
    f = [float(g[r2 < r * r].sum()) for r in radii]
    return [-2.5 * math.log10(f[-1] / fk) for fk in f[:-1]]


# ---- the end-to-end frames --------------------------------------------------------------------------------------------
E2E_FWHM = 2.0
E2E_NOISE = 4.0
E2E_DITHER = ((0.0, 0.0), (3.4, -2.7), (-2.2, 3.9))


def e2e_wcs(i):
    s = importlib.import_module('zuds-pipeline_amd.synth')
    return s.ztf_wcs(ps.E2E_N, ps.E2E_N, dx=E2E_DITHER[i][0], dy=E2E_DITHER[i][1], tpv=True)


@functools.lru_cache(maxsize=None)
def e2e_catalogue():
    """(ra, dec, mag) of the 60 stars."""
    x, y, mag = ps.e2e_stars()
    ra, dec = e2e_wcs(0).all_pix2world(x, y, 0)
    return np.asarray(ra), np.asarray(dec), mag


@functools.lru_cache(maxsize=None)
def e2e_frame(i):
    """Frame i of three dithered 256 x 256 frames with TPV headers: dict(img, mask, rms, wcs, header, zp, fwhm)."""
    s = importlib.import_module('zuds-pipeline_amd.synth')
    ra, dec, mag = e2e_catalogue()
    w = e2e_wcs(i)
    zp = ps.E2E_ZP[i]
    f = s.make_frame(ps.E2E_N, ps.E2E_N, 7300 + i, w, star_sky=(ra, dec, 10.0 ** (-0.4 * (mag - zp))), fwhm=E2E_FWHM,
                     sky=150.0 + 5 * i, noise=E2E_NOISE, magzp=25.0, bad_block=(60 + 50 * i, 120, 4))
    hdr = dict(f['header'])
    hdr['MAGZP'] = zp
    hdr.pop('APCOR4', None)
    hdr['MJD-OBS'], hdr['OBSJD'] = 58000.0 + i, 2458000.5 + i
    return dict(img=f['img'], mask=f['mask'], rms=np.full(f['img'].shape, E2E_NOISE, np.float32), wcs=w, header=hdr, zp=zp,
                fwhm=E2E_FWHM, saturate=float(hdr['SATURATE']))


def oracle_centroid(sub, ix, iy):
    from oracle import detect as odet
    out = [odet.star_fwhm(sub, int(a), int(b))[1:] for a, b in zip(ix, iy)]
    return np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.float64)


def reference_on_planes(img, mask, rms, wcs, saturate, sub=None, magzp=None, stars=True, **settings):
    """The restatement on numpy planes; ``wcs``: the package's WCS object (projected here by the oracle's).  ``sub``: the
    background-subtracted plane the centroids are taken on (default: the oracle's own mesh background)."""
    from oracle import background as oback
    from util import to_oracle_wcs
    if sub is None:
        bad = (np.asarray(mask) & ps.BAD_BITS) != 0
        bkg = oback.background(np.asarray(img, np.float64), np.where(bad, 0.0, 1.0), 128)[0]
        sub = (np.asarray(img, np.float64) - bkg).astype(np.float32)
    ra, dec, mag = e2e_catalogue()
    x1, y1 = to_oracle_wcs(wcs).sky2pix(ra, dec)
    scale = 3600.0 * math.sqrt(abs(float(np.linalg.det(np.asarray(wcs.cd, np.float64).reshape(2, 2)))))
    return pr.measure(img, sub, (x1 - 1.0, y1 - 1.0), oracle_centroid, rms=rms, mask=mask, bad_bits=ps.BAD_BITS,
                      saturate=saturate, mag=mag if stars else None, magzp=magzp, pixel_scale=scale, **settings)


def e2e_reference(frame):
    return reference_on_planes(frame['img'], frame['mask'], frame['rms'], frame['wcs'], frame['saturate'])


EXTENDED = f'numpy.longdouble, eps {float(np.finfo(np.longdouble).eps):.1e}'


def _median_ld(v):
    s = np.sort(v)
    m = s.size
    return s[m // 2] if m & 1 else (s[m // 2 - 1] + s[m // 2]) / np.longdouble(2)


def extended_cards(frame, ref):
    """The cards of the restatement's run ``ref`` on ``frame`` once more with every sum, logarithm, median and square
    root in ``numpy.longdouble``.  What the two runs share are their inputs: the pixels, the positions, the pixel
    fractions of ``aperture_ref`` (float64 numbers made by a quadrature with float64 nodes), the sky of every star (an
    exact selection) and the sets of pixels and stars the float64 run used - under the scenes' conditions those sets are
    not a matter of rounding.  Returns {card: longdouble}."""
    L = np.longdouble
    img, rms, mask = frame['img'], frame['rms'], frame['mask']
    ny, nx = img.shape
    g, used, radii = ref['growth'], ref['used'], ref['radii']
    xs, ys, sky = ref['x'][used], ref['y'][used], g['sky'][used]
    F = np.zeros((xs.size, len(radii)), dtype=L)
    rmax = radii[-1]
    for s, (xc, yc) in enumerate(zip(xs, ys)):
        i0, i1 = max(math.floor(xc - rmax + 0.5), 0), min(math.ceil(xc + rmax + 0.5), nx)
        j0, j1 = max(math.floor(yc - rmax + 0.5), 0), min(math.ceil(yc + rmax + 0.5), ny)
        ii, jj = (v.ravel() for v in np.meshgrid(np.arange(i0, i1), np.arange(j0, j1)))
        x0, x1, y0, y1 = pr.ar.pixel_edges(ii, jj, xc, yc)
        qx, qy = np.clip(0.0, x0, x1), np.clip(0.0, y0, y1)
        near2 = qx * qx + qy * qy
        dv = img[jj, ii].astype(L) - L(sky[s])
        for k, r in enumerate(radii):
            t = near2 < r * r
            F[s, k] = np.sum(dv[t] * pr.ar.edges_fraction(x0[t], x1[t], y0[t], y1[t], r).astype(L))
    dm = L(-2.5) * np.log10(F[:, -1:] / F[:, :-1])
    cards = {}
    slots = pr.card_slots(tuple(2.0 * r for r in radii[:-1]))
    for k, slot in enumerate(slots):
        v = dm[ref['apcor_stats'][k]['keep'], k]
        med = _median_ld(v)
        cards[f'APCOR{slot}'] = med
        cards[f'APCORUN{slot}'] = L(1.2533) * L(1.4826) * _median_ld(np.abs(v - med)) / np.sqrt(L(v.size))
    k4 = slots.index(4)
    mag = e2e_catalogue()[2]
    zpi = mag[ref['index'][used]].astype(L) + L(2.5) * np.log10(F[:, k4]) - cards['APCOR4']
    v = zpi[ref['zp_stats']['keep']]
    cards['MAGZP'] = _median_ld(v)
    cards['MAGZPRMS'] = L(1.4826) * _median_ld(np.abs(v - cards['MAGZP']))
    cards['MAGZPUNC'] = np.hypot(L(1.2533) * cards['MAGZPRMS'] / np.sqrt(L(v.size)), cards['APCORUN4'])
    # MAGLIM: the aperture noise of every used lattice point
    step = 32
    _, _, _, sig, _ = pr.maglim_sigma(rms, mask, ps.BAD_BITS, pr.APERTURE_RADIUS, step)
    lx, ly = pr.lattice(nx, step, pr.APERTURE_RADIUS), pr.lattice(ny, step, pr.APERTURE_RADIUS)
    px = np.array([a for b in ly for a in lx])
    py = np.array([b for b in ly for a in lx])
    i0, i1, j0, j1, _ = pr.ar.boxes(px, py, pr.APERTURE_RADIUS, nx, ny)
    sap = []
    for k in np.flatnonzero(np.isfinite(sig)):
        ii, jj = (v.ravel() for v in np.meshgrid(np.arange(i0[k], i1[k]), np.arange(j0[k], j1[k])))
        frac = pr.ar.edges_fraction(*pr.ar.pixel_edges(ii, jj, px[k], py[k]), pr.APERTURE_RADIUS).astype(L)
        sap.append(np.sqrt(np.sum(rms[jj, ii].astype(L) ** 2 * frac)))
    cards['MAGLIM'] = cards['MAGZP'] + cards['APCOR4'] - L(2.5) * np.log10(L(5.0) * _median_ld(np.array(sap, dtype=L)))
    return cards


def measure_analytic_tol(report=print):
    """{radius: bound} as the module docstring derives it."""
    radii = list(RADII)
    worst_a, worst_o = np.zeros(len(radii) - 1), np.zeros(len(radii) - 1)
    for fx in np.linspace(0.0, 0.5, 5):
        for fy in np.linspace(0.0, 0.5, 5):
            got = np.array(noiseless_apcor(40.0 + fx, 40.0 + fy, radii))
            ana = np.array([pr.analytic_apcor(r, radii[-1], ps.FWHM) for r in radii[:-1]])
            worst_a = np.maximum(worst_a, np.abs(got - ana))
    for fx, fy in ((0.0, 0.0), (0.5, 0.5), (0.37, 0.19)):
        got = np.array(noiseless_apcor(40.0 + fx, 40.0 + fy, radii))
        ovs = np.array(oversampled_apcor(fx, fy, radii))
        worst_o = np.maximum(worst_o, np.abs(got - ovs))
    tol = {}
    for r, a, o in zip(radii, worst_a, worst_o):
        big = 2.0 * max(a, o)
        digit = 10.0 ** math.floor(math.log10(big))
        tol[r] = float(f'{math.ceil(big / digit) * digit:.0e}')
        report(f'pixel-integration error of APCOR at r = {r:g}: {a:.3e} mag against the analytic curve (25 centres), {o:.3e} '
               f'against the 64 x oversampled rendering (3 centres)')
    return tol


def measure_card_tol(report=print):
    """CARD_TOL as the module docstring derives it."""
    frame = e2e_frame(1)
    ref = e2e_reference(frame)
    g, used = ref['growth'], ref['used']
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = g['round_bound'][used] / np.abs(g['flux'][used])
    own = 1.0857362 * float((rel[:, -1:] + rel[:, :-1]).max())
    ext = extended_cards(frame, ref)
    worst = max(abs(float(np.longdouble(ref['cards'][k]) - v)) for k, v in ext.items())
    which = max(ext, key=lambda k: abs(float(np.longdouble(ref['cards'][k]) - ext[k])))
    tol = 2.0 ** math.ceil(math.log2(4.0 * max(own, worst)))
    report(f'rounding of a card: {own:.3e} mag propagated from the roundings of the float64 sums ({int(used.sum())} stars); '
           f'{worst:.3e} mag between the float64 run and the extended-precision run ({EXTENDED}, {len(ext)} cards, largest '
           f'on {which}); CARD_TOL = 2^{int(math.log2(tol))} = {tol:.3e}')
    return tol


def main():
    print(f'APCOR_ANALYTIC_TOL = {measure_analytic_tol()}')
    measure_card_tol()


if __name__ == '__main__':
    main()
