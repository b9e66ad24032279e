"""What tests/resample_scenes.py says about its scenes, asserted from the oracle alone (no GPU), and the oracle's
inverse map itself against a 50-digit evaluation that goes through (RA, Dec) by spherical trigonometry."""
import mpmath as mp
import numpy as np
import pytest

import resample_scenes as rs
from oracle import resample as oresample
from oracle.wcs import _TPV_TERMS, map_out_to_in
from util import to_oracle_wcs


def owcs(name):
    sc = rs.scene(name)
    return to_oracle_wcs(sc.win), to_oracle_wcs(sc.wout)


@pytest.mark.parametrize('name', rs.SCENES)
def test_sizes_overlap_and_mask_bits(name):
    sc = rs.scene(name)
    onx, ony = sc.wout.naxis
    assert max(onx, ony) <= 260 and max(sc.win.naxis) <= 420
    assert onx > 2 * 64 and ony > 2 * 32                       # three tiles of k_resample along both axes
    assert sc.img.shape == sc.wgt.shape == sc.mask.shape == (sc.win.naxis[1], sc.win.naxis[0])
    share = rs.covered(name).mean()
    assert share >= 0.6, share
    # stars, bad pixels and mask bits on both sides of bit 15, all of which reach the output
    assert (sc.wgt == 0).sum() > 50 and sc.img.max() > 10 * np.std(sc.img)
    assert (sc.mask & 0xffff).any() and (sc.mask >> 16).any()
    r_wgt, r_msk = rs.reference(name)[3], rs.reference(name)[4]
    assert ((r_wgt == 0) & rs.covered(name)).sum() > 50
    assert (r_msk & 0xffff).any() and (r_msk >> 16).any()


@pytest.mark.parametrize('name', rs.SCENES)
def test_rotation_between_the_tangent_frames(name):
    win, wout = owcs(name)
    m = win.frame() @ wout.frame().T
    off = np.abs(m - np.eye(3)).max()
    if name in rs.ROTATED_FRAMES:
        assert off > 1e-6, off
    else:
        assert off < 1e-12, off
    if name == 'crval_offset':
        sep = np.degrees(np.arccos(np.clip(m[2, 2], -1, 1))) * 3600.0
        assert 39.0 < sep < 41.0, sep
    if name == 'across_ra_zero':
        assert win.crval[0] == 359.995 and wout.crval[0] == 0.004
    if name == 'near_pole':
        assert win.crval[1] == wout.crval[1] == 89.99 and abs(wout.crval[0] - win.crval[0]) == 90.0
        assert abs(m[0, 0]) < 1e-3 and abs(m[0, 1]) > 0.999     # east of one frame is north of the other


def tpv_order(pv):
    return max(a + b for k, (a, b, c) in enumerate(_TPV_TERMS) if pv[k] != 0.0 and not c)


def test_tpv_scenes_have_the_terms_they_name():
    win, wout = owcs('tpv_degree7_radial')
    for w in (win, wout):
        assert w.has_pv
        for pv in (w.pv1, w.pv2):
            assert tpv_order(pv) == 7
            assert pv[3] != 0.0 and pv[11] != 0.0
            for deg in (5, 6, 7):
                assert any(pv[k] != 0.0 for k, (a, b, c) in enumerate(_TPV_TERMS) if a + b == deg)
    # the new terms move pixels by far more than the parity tolerance resolves
    sc = rs.scene('tpv_degree7_radial')
    px, py = rs.positions('tpv_degree7_radial')
    low_in, low_out = owcs('tpv_degree7_radial')
    for w in (low_in, low_out):
        for pv in (w.pv1, w.pv2):
            pv[17:] = 0.0
            pv[3] = pv[11] = 0.0
    onx, ony = sc.wout.naxis
    qx, qy = oresample.positions(low_out, low_in, onx, ony)
    moved = np.hypot(px - qx, py - qy)
    assert moved.min() > 1e-3 and moved.max() - moved.min() > 1e-3
    win, wout = owcs('tpv_to_tan')
    assert win.has_pv and not wout.has_pv
    win, wout = owcs('tan_to_tpv')
    assert wout.has_pv and not win.has_pv


@pytest.mark.parametrize('name', ['tpv_degree7_radial', 'tpv_to_tan', 'crval_offset', 'mirrored', 'rot180'])
def test_newton_inverse_converges(name):
    """plane2pix followed by pix2plane gives the plane position back to 1e-12 degrees (3.6e-9 px) all over the frame
    and a margin around it."""
    win, _ = owcs(name)
    nx, ny = win.naxis
    y, x = np.mgrid[-20:ny + 20:7, -20:nx + 20:7].astype(np.float64)
    xi, eta = win.pix2plane(x, y)
    x2, y2 = win.plane2pix(xi, eta)
    assert np.abs(x2 - x).max() < 1e-8 and np.abs(y2 - y).max() < 1e-8
    xi2, eta2 = win.pix2plane(x2, y2)
    assert np.abs(xi2 - xi).max() < 1e-12 and np.abs(eta2 - eta).max() < 1e-12


def jacobian(name):
    """d(px, py) / d(ox, oy) at the centre of an interior tile."""
    px, py = rs.positions(name)
    return np.array([[px[48, 97] - px[48, 96], px[49, 96] - px[48, 96]],
                     [py[48, 97] - py[48, 96], py[49, 96] - py[48, 96]]])


@pytest.mark.parametrize('name', rs.SCENES)
def test_orientation(name):
    px, py = rs.positions(name)
    tile = (slice(32, 64), slice(64, 128))                     # an interior 64 x 32 tile of k_resample
    w, h = np.ptp(px[tile]), np.ptp(py[tile])
    if name in rs.QUADRANT:
        assert h > 1.8 * w, (w, h)
    elif not name.startswith(('finer', 'coarser')):
        assert w > 1.8 * h, (w, h)
    j = jacobian(name)
    det = np.linalg.det(j)
    assert (det < 0) == name.startswith('mirrored'), det
    if name == 'rot180':
        assert j[0, 0] < -0.99 and j[1, 1] < -0.99
    if name == 'rot90':
        assert abs(j[0, 0]) < 0.01 and abs(j[1, 1]) < 0.01
        assert j[0, 1] * jacobian('rot270')[0, 1] < -0.99          # the two quarter turns are opposite
    scale = np.sqrt(abs(det))
    want = {'finer_2x': 0.5, 'coarser_2x': 2.0, 'coarser_3x': 3.0}.get(name, 1.0)
    assert abs(scale / want - 1.0) < 2e-3, scale


@pytest.mark.parametrize('name', sorted(rs.EXACT))
def test_exact_scenes_sit_on_their_fractions(name):
    for p in rs.positions(name):
        fr = p - np.rint(p - rs.EXACT[name]) - rs.EXACT[name]
        assert np.abs(fr).max() < 1e-9
    assert rs.BOUNDS[name][0] < 1e-9
    assert not rs.near_decision(name, 'LANCZOS3').any()


def test_rot90_exact_is_a_transposition():
    """Integer positions: output (x, y) reads input (c - y, x) or (y, c - x): a transposition with one flip."""
    px, py = rs.positions('rot90_exact')
    ix, iy = np.rint(px).astype(int), np.rint(py).astype(int)
    assert np.ptp(ix, axis=1).max() == 0 and np.ptp(iy, axis=0).max() == 0      # x depends on the row only, y on the column
    assert abs(ix[1, 0] - ix[0, 0]) == 1 and abs(iy[0, 1] - iy[0, 0]) == 1
    assert rs.covered('rot90_exact').all()


@pytest.mark.parametrize('name', rs.SCENES)
def test_excluded_share(name):
    """The flip budget as a condition: the pixels near a decision are at most 1e-3 of the covered ones."""
    for kernel in ('LANCZOS3', 'BILINEAR', 'NEAREST'):
        if kernel != 'LANCZOS3' and name not in rs.OTHER_KERNEL_SCENES:
            continue
        cov = rs.covered(name, kernel)
        near = rs.near_decision(name, kernel) & cov
        if kernel == 'NEAREST' and name == 'half_shift':
            assert near.sum() == cov.sum()          # every position is a tie: tests compare with nearest_candidates
            continue
        share = near.sum() / cov.sum()
        assert share <= rs.MAX_EXCLUDED, (kernel, share)


@pytest.mark.parametrize('name', rs.SCENES)
def test_bounds_follow_from_the_emulation(name):
    """BOUNDS is the table tests/measure_resample_tolerance.py prints: delta0 and the 4 x rule, rounded up."""
    d0, dv, dw = rs.emulation(name)
    t0, tv, tw = rs.BOUNDS[name]
    assert d0 <= t0 <= 1.01 * d0 + 1e-15
    for dev, t in ((dv, tv), (dw, tw)):
        want = rs.bound_for(dev)
        assert t == 1.0 if want == 1.0 else want <= t <= 1.01 * want


@pytest.mark.parametrize('which', sorted(rs.STACKS))
def test_stacks_overlap_and_their_emulation_stays_inside_the_coadd_bound(which):
    frames, wout = rs.stack(which)
    assert [f['wcs'] is rs.scene(n).win for f, n in zip(frames, rs.STACKS[which])] == [True] * 3
    for kind in ('WEIGHTED', 'CLIPPED'):
        wgts = rs.stack_reference(which, kind)[4]
        assert ((wgts > 0).sum(axis=0) == 3).mean() > 0.5
        assert rs.stack_emulation(which, kind) <= 1.0


# ---- the oracle's map against spherical trigonometry at 50 digits -------------------------------------------------------

mp.mp.dps = 50


def tpv_index():
    """Exponents (x, y, r) of the forty TPV terms, built degree by degree: x^(d - j) y^j, then r^d after an odd d."""
    terms = [(0, 0, 0)]
    for d in range(1, 8):
        terms += [(d - j, j, 0) for j in range(d + 1)]
        if d % 2:
            terms.append((0, 0, d))
    return terms


def mp_tpv(pv, x, y):
    r = mp.sqrt(x * x + y * y)
    return mp.fsum(mp.mpf(float(p)) * x ** a * y ** b * r ** c for p, (a, b, c) in zip(pv, tpv_index()) if p != 0.0)


def mp_pix2plane(w, x, y):
    dx, dy = mp.mpf(x) - mp.mpf(float(w.crpix[0])), mp.mpf(y) - mp.mpf(float(w.crpix[1]))
    cd = [[mp.mpf(float(v)) for v in row] for row in w.cd]
    u, v = cd[0][0] * dx + cd[0][1] * dy, cd[1][0] * dx + cd[1][1] * dy
    if not w.has_pv:
        return u, v
    return mp_tpv(w.pv1, u, v), mp_tpv(w.pv2, v, u)


def mp_plane2sky(w, xi, eta):
    """Inverse gnomonic projection (Snyder 1987, eq. 20-14, 20-15), radians."""
    x, y = mp.radians(xi), mp.radians(eta)
    a0, d0 = mp.radians(mp.mpf(float(w.crval[0]))), mp.radians(mp.mpf(float(w.crval[1])))
    rho = mp.sqrt(x * x + y * y)
    if rho == 0:
        return a0, d0
    c = mp.atan(rho)
    dec = mp.asin(mp.cos(c) * mp.sin(d0) + y * mp.sin(c) * mp.cos(d0) / rho)
    ra = a0 + mp.atan2(x * mp.sin(c), rho * mp.cos(d0) * mp.cos(c) - y * mp.sin(d0) * mp.sin(c))
    return ra, dec


def mp_sky2plane(w, ra, dec):
    """Gnomonic projection (Snyder 1987, eq. 22-3 to 22-5), degrees."""
    a0, d0 = mp.radians(mp.mpf(float(w.crval[0]))), mp.radians(mp.mpf(float(w.crval[1])))
    cosc = mp.sin(d0) * mp.sin(dec) + mp.cos(d0) * mp.cos(dec) * mp.cos(ra - a0)
    xi = mp.cos(dec) * mp.sin(ra - a0) / cosc
    eta = (mp.cos(d0) * mp.sin(dec) - mp.sin(d0) * mp.cos(dec) * mp.cos(ra - a0)) / cosc
    return mp.degrees(xi), mp.degrees(eta)


def mp_plane2pix(w, xi, eta, guess):
    """Pixel whose plane position is (xi, eta): a root search on the forward map, started at the oracle's answer."""
    def f(x, y):
        a, b = mp_pix2plane(w, x, y)
        return a - xi, b - eta
    x, y = mp.findroot(f, (mp.mpf(float(guess[0])), mp.mpf(float(guess[1]))), tol=mp.mpf(10) ** -40)
    return x, y


def test_tpv_term_table_is_the_registry_order():
    assert tpv_index() == [tuple(t) for t in _TPV_TERMS]


@pytest.mark.parametrize('name', rs.SCENES)
def test_oracle_map_matches_spherical_trigonometry(name):
    """oracle.wcs.map_out_to_in on a dozen output pixels per scene (corners, an off-frame point, random ones) against
    output pixel -> plane -> (RA, Dec) -> input plane -> input pixel at 50 digits: 1e-9 px."""
    win, wout = owcs(name)
    onx, ony = wout.naxis
    rng = np.random.default_rng(rs.SCENES.index(name))
    xo = np.concatenate([[1.0, onx, 1.0, onx, -15.5], rng.uniform(1, onx, 7)])
    yo = np.concatenate([[1.0, 1.0, ony, ony, ony + 9.25], rng.uniform(1, ony, 7)])
    oxi, oyi = map_out_to_in(wout, win, xo, yo)
    worst = 0.0
    for k in range(xo.size):
        xi, eta = mp_pix2plane(wout, float(xo[k]), float(yo[k]))
        ra, dec = mp_plane2sky(wout, xi, eta)
        xi2, eta2 = mp_sky2plane(win, ra, dec)
        x, y = mp_plane2pix(win, xi2, eta2, (oxi[k], oyi[k]))
        # the root is the one next to the oracle's, and it is a root
        a, b = mp_pix2plane(win, x, y)
        assert abs(a - xi2) < mp.mpf(10) ** -30 and abs(b - eta2) < mp.mpf(10) ** -30
        worst = max(worst, abs(float(x - mp.mpf(float(oxi[k])))), abs(float(y - mp.mpf(float(oyi[k])))))
    assert worst < 1e-9, worst
