"""The restatement of tests/lightcurve_ref.py against answers known by hand, the scenes against the conditions the GPU
tests rely on, and the host-side objects of the light-curve layer (``ForcedPhotometry``, ``Source.light_curve``, the CSV,
the ``done`` set difference) against literal values.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

import aperture_ref as ar
import lightcurve_ref as lr
from oracle.wcs import WCS as OWCS
from util import pkg

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_square_on_the_equator_has_great_circle_edges():
    sq = [(9.0, -1.0), (9.0, 1.0), (11.0, 1.0), (11.0, -1.0)]
    # the edge from (9, 1) to (11, 1) is a great circle: at ra = 10 it reaches atan(tan 1 / cos 1) = 1.000152 deg
    top = math.degrees(math.atan(math.tan(math.radians(1.0)) / math.cos(math.radians(1.0))))
    assert 1.00015 < top < 1.00016
    ra = [10.0, 10.5, 9.1, 12.0, 10.0, 10.0, 10.0, 8.9, 190.0, 10.0, np.nan, 10.0]
    dec = [0.0, 0.9, -0.9, 0.0, 1.5, top - 1e-5, top + 1e-5, 0.0, 0.0, -1.0002, 0.0, np.inf]
    want = [True, True, True, False, False, True, False, False, False, False, False, False]
    assert lr.inside_corners(sq, ra, dec).tolist() == want
    # either orientation of the corners
    assert lr.inside_corners(sq[::-1], ra, dec).tolist() == want


def test_square_across_ra_zero():
    sq = [(359.0, -1.0), (359.0, 1.0), (1.0, 1.0), (1.0, -1.0)]
    ra = [0.0, 359.5, 0.5, 360.0, 2.0, 358.0, 180.0, 0.0, -0.5]
    dec = [0.0, 0.5, -0.5, 0.99, 0.0, 0.0, 0.0, 1.1, 0.0]
    want = [True, True, True, True, False, False, False, False, True]
    assert lr.inside_corners(sq, ra, dec).tolist() == want


def test_square_around_the_pole():
    sq = [(0.0, 89.0), (90.0, 89.0), (180.0, 89.0), (270.0, 89.0)]
    # halfway between two corners the edge passes atan(tan 1 cos 45) = 0.70714 deg from the pole
    mid = 90.0 - math.degrees(math.atan(math.tan(math.radians(1.0)) * math.cos(math.radians(45.0))))
    assert 89.2928 < mid < 89.2929
    ra = [123.0, 45.0, 45.0, 0.0, 0.0, 300.0, 77.0, 45.0]
    dec = [89.9, mid + 1e-4, mid - 1e-4, 89.01, 88.99, 90.0, -89.9, 89.2]
    want = [True, True, False, True, False, True, False, False]
    assert lr.inside_corners(sq, ra, dec).tolist() == want


def golden_cases():
    with open(os.path.join(GOLD, 'astropy_wcs.json')) as f:
        return json.load(f)['cases']


def test_footprints_of_the_astropy_golden_file():
    """The restatement's corners are astropy's ``calc_footprint`` rows, and membership in astropy's polygon agrees
    with the pixel-space answer for positions planted 1.5 px either side of it."""
    cases = golden_cases()
    assert len(cases) >= 4
    for c in cases:
        ow = OWCS.from_header(c['header'])
        nx, ny = ow.naxis
        assert nx > 8 and ny > 8
        np.testing.assert_allclose(lr.corners(ow), np.array(c['footprint']), rtol=0, atol=1e-9)
        x, y, inside = lr.planted_pixels(nx, ny)
        off = (x > 1.0 + 1.0) & (x < nx - 1.0) & (y > 1.0 + 1.0) & (y < ny - 1.0) | ~inside      # the 1.5 px positions
        ra, dec = ow.pix2sky(x[off], y[off])
        got = lr.inside_corners(np.array(c['footprint']), ra, dec, lr.centre(ow))
        assert got.tolist() == inside[off].tolist(), c['name']
        assert inside[off].any() and (~inside[off]).any()


@pytest.mark.parametrize('name', lr.FRAMES)
def test_frame_scenes_are_clear_of_the_edges_and_known(name):
    w, ow, ra, dec, known = lr.frame_scene(name)
    lr.assert_clear([ow], ra, dec)
    off, idx = lr.membership([ow], ra, dec)
    assert np.array_equal(np.flatnonzero(known), idx)            # planted through pix2sky: the pixel-space answer
    assert 60 < idx.size < ra.size - 40 and off.tolist() == [0, idx.size]
    d = lr.edge_distance_arcsec([ow], ra, dec)[0]
    assert 0.2 < d.min() < 0.3                                   # the 0.25 px positions, 1 arcsec pixels
    det = float(np.linalg.det(ow.cd))
    assert (det < 0) == (name in ('negdet', 'ra0', 'pole'))
    c = lr.corners(ow)
    if name == 'ra0':
        assert c[:, 0].min() < 1.0 and c[:, 0].max() > 359.0
    if name == 'pole':
        assert lr.inside_corners(c, [0.0], [90.0], lr.centre(ow))[0]
        assert np.ptp(ra[idx]) > 180.0


def test_the_other_scenes_are_clear_of_the_edges():
    ws, ows, planes, ra, dec = lr.batch_scene()
    lr.assert_clear(ows, ra, dec)
    off, idx = lr.membership(ows, ra, dec)
    n = np.diff(off)
    assert (n > 10).all() and n.sum() > ra.size * 0.5 and len({p[0].shape for p in planes}) == 3
    assert planes[1][1] is None and planes[2][2] is None and planes[0][1] is not None and planes[0][2] is not None
    assert np.unique(idx).size < idx.size                         # a source on more than one image
    for k in (63, 64, 65, 300):
        w, ow, ra, dec = lr.count_scene(k)
        lr.assert_clear([ow], ra, dec)
        assert lr.membership([ow], ra, dec)[0].tolist() == [0, k]
    with pytest.raises(AssertionError):                           # the guard does bite: a source on a corner
        c = lr.corners(ows[0])
        lr.assert_clear(ows[:1], c[:1, 0], c[:1, 1])


def test_the_reference_alone_stays_finite_on_the_scenes():
    """Rows whose restated sum is not finite are left out of the comparison with the kernel; on these scenes there is
    none (the NaN-pixel test plants its own)."""
    ws, ows, planes, ra, dec = lr.batch_scene()
    off, idx = lr.membership(ows, ra, dec)
    ref = lr.photometry(ows, planes, ra, dec, off, idx)
    assert np.isfinite(ref['flux']).all() and np.isfinite(ref['fluxerr']).all()
    assert (ref['terms'][4] > 0).all() and (ref['terms'][4] < 49).any()       # every pair has a box, some are clipped
    bf, bv = ar.sums_bounds(ref['terms'])
    assert (bf > 0).all() and np.isfinite(bf).all() and np.isfinite(bv).all()
    a, b = off[1], off[2]
    assert not ref['fluxerr'][a:b].any() and ref['flags'][a:b].any()          # rms None
    assert not ref['flags'][off[2]:].any() and ref['fluxerr'][off[2]:].all()  # mask None
    assert lr.POS_TOL_PX < 1e-7


# ---- the host-side objects ----------------------------------------------------------------------------------------------
def test_forced_photometry_object():
    z = pkg()

    class Im(object):
        header = {'MAGZP': 26.0, 'APCOR4': -0.1}
    p = z.ForcedPhotometry(flux=100.0, fluxerr=4.0, flags=6, ra=1.0, dec=2.0, zp=25.9, obsjd=2458800.5, filtercode='zg',
                           image=Im(), source='s1')
    assert p.snr == 25.0
    assert p.magerr == 1.08573620476 * 4.0 / 100.0
    assert p.mag == -2.5 * 2.0 + 26.0 - 0.1
    assert (p.flags, p.ra, p.dec, p.zp, p.obsjd, p.filtercode, p.source) == (6, 1.0, 2.0, 25.9, 2458800.5, 'zg', 's1')


def test_source_light_curve_columns_and_the_empty_case():
    z = pkg()
    s = z.Source(id='ZUDS20aaaaa', ra=10.0, dec=20.0)
    lc = s.light_curve
    assert len(lc) == 0 and s.forced_photometry == [] and s.unphotometered_images([]) == [] and s.images([]) == []
    cols = ['mjd', 'filter', 'zp', 'zpsys', 'flux', 'fluxerr', 'flags', 'lim_mag', 'id']
    assert lc.colnames == cols
    s.forced_photometry.append(z.ForcedPhotometry(flux=100.0, fluxerr=2.0, flags=0, zp=25.0, obsjd=2458800.5, filtercode='zr'))
    s.forced_photometry.append(z.ForcedPhotometry(flux=-3.0, fluxerr=20.0, flags=8, zp=26.0, obsjd=2458801.75, filtercode='zi',
                                                  id=77))
    lc = s.light_curve
    assert len(lc) == 2 and lc.colnames == cols
    assert lc['mjd'].tolist() == [58800.0, 58801.25] and lc['filter'].tolist() == ['ztfr', 'ztfi']
    assert lc['zpsys'].tolist() == ['ab', 'ab'] and lc['flags'].tolist() == [0, 8] and lc['id'].tolist() == [0, 77]
    assert lc['lim_mag'].tolist() == [-2.5 * math.log10(10.0) + 25.0, -2.5 * math.log10(100.0) + 26.0] == [22.5, 21.0]
    assert lc['flux'].tolist() == [100.0, -3.0] and lc['fluxerr'].tolist() == [2.0, 20.0] and lc['zp'].tolist() == [25.0, 26.0]


def test_csv_round_trip_and_grouping(tmp_path):
    z = pkg()
    lc = z.lightcurve
    assert lc.PHOT_CSV_COLUMNS == ('source_id', 'image_id', 'flux', 'fluxerr', 'flags', 'ra', 'dec', 'zp', 'filtercode', 'obsjd')
    rows = [dict(source_id='src0000002', image_id=12, flux=1.0 / 3.0, fluxerr=2.0 ** -40, flags=5, ra=23.1234567890123,
                 dec=-30.5, zp=26.275, filtercode='zg', obsjd=2458802.5),
            dict(source_id='src0000001', image_id='sub_b.fits', flux=-7.25e-3, fluxerr=float('nan'), flags=0, ra=359.99999,
                 dec=89.5, zp=25.0, filtercode='zr', obsjd=2458801.5),
            dict(source_id='src0000002', image_id=11, flux=5.0, fluxerr=1.0, flags=0, ra=23.1234567890123, dec=-30.5, zp=26.0,
                 filtercode='zr', obsjd=2458800.5)]
    path = tmp_path / 'phot.csv'
    lc.write_phot_csv(path, rows[:2])
    lc.write_phot_csv(path, rows[2:], append=True)
    text = open(path).read().splitlines()
    assert text[0] == 'source_id,image_id,flux,fluxerr,flags,ra,dec,zp,filtercode,obsjd' and len(text) == 4
    assert text[1] == 'src0000002,12,0.3333333333333333,9.094947017729282e-13,5,23.1234567890123,-30.5,26.275,zg,2458802.5'
    back = lc.read_phot_csv(path)
    assert back[0] == rows[0] and back[2] == rows[2]
    assert math.isnan(back[1]['fluxerr']) and {k: v for k, v in back[1].items() if k != 'fluxerr'} == \
        {k: v for k, v in rows[1].items() if k != 'fluxerr'}
    src = z.Source(id='src0000002', ra=23.1234567890123, dec=-30.5)
    groups = lc.light_curves(back, sources=[src])
    assert sorted(groups) == ['src0000001', 'src0000002']
    assert [p.obsjd for p in groups['src0000002']] == [2458800.5, 2458802.5]          # by obsjd within a source
    assert [p.image for p in groups['src0000002']] == [11, 12] and groups['src0000002'][0].source is src
    assert src.forced_photometry == groups['src0000002'] and src.light_curve['mjd'].tolist() == [58800.0, 58802.0]
    assert groups['src0000001'][0].source == 'src0000001'


def test_done_is_a_set_difference_on_pairs():
    lc = pkg().lightcurve
    offsets, src_idx = np.array([0, 3, 3, 7]), np.array([1, 4, 9, 0, 4, 5, 9], np.int32)
    assert lc.pair_keys([0, 2], [4, 9]).tolist() == [4, (2 << 32) + 9]
    o, s = lc.drop_done(offsets, src_idx, {(0, 4), (2, 9), (1, 4), (2, 77)})
    assert o.tolist() == [0, 2, 2, 5] and s.tolist() == [1, 9, 0, 4, 5]
    o, s = lc.drop_done(offsets, src_idx, np.array([[2, 0], [2, 4], [2, 5], [2, 9]]))
    assert o.tolist() == [0, 3, 3, 3] and s.tolist() == [1, 4, 9]
    o, s = lc.drop_done(offsets, src_idx, [])
    assert o.tolist() == offsets.tolist() and s.tolist() == src_idx.tolist()
