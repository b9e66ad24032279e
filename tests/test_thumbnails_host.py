"""Host side of the detection thumbnails (zuds-pipeline_amd/thumbnails.py): the origin rule, the trimmed stamp and its
WCS, the bytes of a ``Thumbnail``, the layout of ``zm_stamp_plane``.  No GPU: ``zm_stamp_origin`` and the WCS helpers are
host code, a plane that is already on the grid is sliced with numpy."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from util import pkg, synth


def origin_restated(x, y, S):
    # astropy.nddata.utils.overlap_slices, restated: the first pixel of a stamp centred on `position` is
    # ceil(position - S / 2), the last one the first + S - 1
    x0 = np.ceil(np.asarray(x, np.float64) - S / 2.0).astype(np.int64)
    return x0, np.ceil(np.asarray(y, np.float64) - S / 2.0).astype(np.int64)


@pytest.mark.parametrize('S', [63, 64, 21, 1, 256])
def test_origin_rule_on_hand_placed_positions(S):
    z, s = pkg(), synth()
    nx, ny = 200, 120
    w = s.tan_wcs(nx, ny)
    x = np.array([50.0, 50.5, 49.5, 0.0, -0.5, nx - 1.0, nx - 0.5, 50.25, -3.0, -10.0, 50.0, 50.0])
    y = np.array([40.0, 40.5, 39.5, 0.0, -0.5, ny - 1.0, ny - 0.5, 40.75, 60.0, -7.0, ny + 5.0, -4.0])
    x0r, y0r = origin_restated(x, y, S)
    # exactly one row of overlap at the top and at the bottom, exactly one column at the left
    x = np.append(x, [50.0, 50.0, 0.0 - (S - 1) / 2.0 + 0.0])
    y = np.append(y, [ny - 1 + S / 2.0 - 0.25, -(S / 2.0) + 0.75, 40.0])
    x0r, y0r = origin_restated(x, y, S)
    assert y0r[-3] == ny - 1 and y0r[-2] + S - 1 == 0
    ra, dec = w.all_pix2world(x, y, 0)
    xx, yy = w.all_world2pix(ra, dec, 0)                 # the float64 positions the library rounds
    x0r, y0r = origin_restated(xx, yy, S)
    x0, y0, st = z.stamp_origin(w, ra, dec, S)
    overlap = (x0r + S > 0) & (x0r < nx) & (y0r + S > 0) & (y0r < ny)
    assert np.array_equal(st == 0, overlap) and overlap.any() and (S >= 21 or not overlap.all())
    assert np.array_equal(x0[overlap], x0r[overlap]) and np.array_equal(y0[overlap], y0r[overlap])
    assert np.all(st[~overlap] == z._lib.STAMP_NO_OVERLAP)
    # integer and half-integer centres: a hair either side of them (the sky round trip moves a position by ~1e-11
    # pixels, so the exact tie is approached from both sides), the first pixel steps where ceil steps
    for c in (50.0, 50.5):
        for nudge in (-1e-7, 1e-7):
            r, d = w.all_pix2world([c + nudge], [40.0 + nudge], 0)
            got = z.stamp_origin(w, r, d, S)
            assert got[0][0] == int(np.ceil(c + nudge - S / 2.0)) and got[1][0] == int(np.ceil(40.0 + nudge - S / 2.0))


def test_no_overlap_and_nan_are_errors():
    z, s = pkg(), synth()
    w = s.tan_wcs(100, 80)
    ra, dec = w.all_pix2world([50.0, -500.0, 50.0], [40.0, 40.0, 4000.0], 0)
    ra = np.append(ra, [np.nan, ra[0]])
    dec = np.append(dec, [dec[0], np.inf])
    _, _, st = z.stamp_origin(w, ra, dec, 63)
    assert list(st) == [0, z._lib.STAMP_NO_OVERLAP, z._lib.STAMP_NO_OVERLAP, z._lib.STAMP_NOT_FINITE, z._lib.STAMP_NOT_FINITE]
    img = np.zeros((80, 100), np.float32)
    for k in (1, 3):
        with pytest.raises(ValueError):
            z.make_stamp(None, ra[k], dec[k], None, None, img, w, save=False)
    with pytest.raises(NotImplementedError, match='matplotlib'):
        z.make_stamp('x.jpg', ra[0], dec[0], None, None, img, w)
    with pytest.raises(z.ZMError):
        z.stamp_origin(w, ra, dec, 257)


@pytest.mark.parametrize('tpv', [False, True])
def test_trimmed_stamp_and_shifted_crpix(tpv):
    z, s = pkg(), synth()
    nx, ny = 300, 260
    w = s.ztf_wcs(nx, ny, rot_deg=0.3, tpv=True) if tpv else s.tan_wcs(nx, ny)
    img = np.arange(nx * ny, dtype=np.float32).reshape(ny, nx)
    for (x, y) in [(150.2, 130.7), (3.0, 4.0), (nx - 2.0, 100.0), (10.0, ny - 1.0), (0.0, 0.0)]:
        ra, dec = w.all_pix2world([x], [y], 0)
        c = z.make_stamp(None, ra[0], dec[0], None, None, img, w, save=False)
        x0, y0 = origin_restated(*w.all_world2pix(ra, dec, 0), 63)
        xa, ya = max(int(x0[0]), 0), max(int(y0[0]), 0)
        xb, yb = min(int(x0[0]) + 63, nx), min(int(y0[0]) + 63, ny)
        assert c.origin == (xa, ya) and c.block_origin == (int(x0[0]), int(y0[0]))
        assert np.array_equal(c.data, img[ya:yb, xa:xb])
        assert c.wcs.naxis == (xb - xa, yb - ya) and c.wcs.has_pv == tpv
        # through the header cards the thumbnail carries
        ws = z.WCS.from_header(dict(c.wcs.to_header(), NAXIS1=xb - xa, NAXIS2=yb - ya))
        jj, ii = np.mgrid[0:yb - ya:7, 0:xb - xa:7]
        r1, d1 = ws.all_pix2world(ii.ravel(), jj.ravel(), 0)
        r2, d2 = w.all_pix2world(xa + ii.ravel(), ya + jj.ravel(), 0)
        # the two differ only in where the integer shift is rounded into x - CRPIX: 4 spacings of the coordinate
        assert np.all(np.abs(r1 - r2) <= 4 * np.spacing(np.abs(r2)))
        assert np.all(np.abs(d1 - d2) <= 4 * np.spacing(np.abs(d2)))


class _Det(object):
    def __init__(self, ra, dec):
        self.ra, self.dec = ra, dec


@pytest.mark.parametrize('tpv', [False, True])
def test_thumbnail_bytes_round_trip(tpv):
    z, s = pkg(), synth()
    nx, ny = 200, 150
    w = s.ztf_wcs(nx, ny, tpv=True) if tpv else s.tan_wcs(nx, ny)
    f = s.make_frame(nx, ny, 5, w)
    image = z.FITSImage()
    image.basename = 'frame.fits'
    image.header = dict(f['header'])
    image.header_comments = {}
    image.data = f['img']
    for (x, y) in [(100.3, 70.1), (2.0, 148.0)]:
        ra, dec = w.all_pix2world([x], [y], 0)
        det = _Det(float(ra[0]), float(dec[0]))
        t = z.Thumbnail.from_detection(det, image)
        cut = z.make_stamp(None, det.ra, det.dec, None, None, image.data, image.wcs, save=False)
        assert t.type == 'new' and t.detection is det and t.image is image
        data, header, _ = z.fits.from_bytes(gzip.decompress(t.bytes))
        assert data.dtype == np.float32 and np.array_equal(data, cut.data)
        assert np.array_equal(t.array, np.flipud(cut.data))
        cards = cut.wcs.to_header()
        assert cards['CRPIX1'] == w.crpix[0] - cut.origin[0] and cards['CRPIX2'] == w.crpix[1] - cut.origin[1]
        for k, v in cards.items():
            assert header[k] == v, k
        assert ('PV1_1' in header) == tpv and header['CTYPE1'] == ('RA---TPV' if tpv else 'RA---TAN')
        assert z.Thumbnail.from_detection(det, image).bytes == t.bytes          # equal stamps, equal bytes
        assert t.bytes[4:8] == b'\0\0\0\0'                                      # gzip mtime = 0


def test_types_follow_the_class_of_the_image_or_its_parent():
    z, s = pkg(), synth()
    w = s.tan_wcs(120, 100)
    f = s.make_frame(120, 100, 6, w)
    ra, dec = w.all_pix2world([60.0], [50.0], 0)
    det = _Det(float(ra[0]), float(dec[0]))
    for cls, typ in ((z.SingleEpochSubtraction, 'sub'), (z.MultiEpochSubtraction, 'sub'), (z.ReferenceImage, 'ref'),
                     (z.ScienceImage, 'new'), (z.ScienceCoadd, 'new')):
        parent = cls()
        parent.basename = 'p.fits'
        parent.header, parent.header_comments, parent.data = dict(f['header']), {}, f['img']
        assert z.Thumbnail.from_detection(det, parent).type == typ
        aligned = z.FITSImage()                          # what aligned_to returns: a plain image with a parent
        aligned.basename = 'a.fits'
        aligned.header, aligned.header_comments, aligned.data = dict(f['header']), {}, f['img']
        aligned.parent_image = parent
        t = z.Thumbnail.from_detection(det, aligned)
        assert t.type == typ and t.image is parent


def test_triplet_of_images_on_one_grid():
    z, s = pkg(), synth()
    w = s.tan_wcs(120, 100)
    imgs = []
    for seed in (1, 2, 3):
        im = z.FITSImage()
        im.basename = f'{seed}.fits'
        f = s.make_frame(120, 100, seed, w)
        im.header, im.header_comments, im.data = dict(f['header']), {}, f['img']
        imgs.append(im)
    ra, dec = w.all_pix2world([4.0], [50.0], 0)          # the stamp hangs over the left edge
    t = z.make_triplet_for_braai(float(ra[0]), float(dec[0]), *imgs)
    assert t.shape == (63, 63, 3)
    x0 = int(np.ceil(4.0 - 31.5))
    for c, im in enumerate(imgs):
        assert np.all(t[:, :-x0, c] == 0)
        block = im.data[50 - 31:50 + 32, 0:63 + x0].astype(np.float64)
        np.testing.assert_allclose(t[:, -x0:, c], block / np.linalg.norm(block), rtol=1e-15)
        assert abs(np.linalg.norm(t[:, :, c]) - 1.0) < 1e-12
    with pytest.raises(NotImplementedError):
        z.make_triplet_for_braai(float(ra[0]), float(dec[0]), *imgs, old_norm=True)


def test_stamp_plane_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of zm_stamp_plane as a C compiler sees it (the probe of
    test_abi.py::test_struct_layouts_match_the_header)."""
    z = pkg()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cls = z._lib.zm_stamp_plane
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zudsmi.h"', 'int main(void) {',
             '  printf("zm_stamp_plane . %zu\\n", sizeof(zm_stamp_plane));']
    for field, _ in cls._fields_:
        lines.append(f'  printf("zm_stamp_plane {field} %zu\\n", offsetof(zm_stamp_plane, {field}));')
    lines += ['  printf("max . %d\\n", ZM_STAMP_MAX);', '  printf("planes . %d\\n", ZM_STAMP_PLANES_MAX);',
              '  printf("status . %d\\n", ZM_STAMP_NOT_FINITE * 10 + ZM_STAMP_NO_OVERLAP);', '  return 0;', '}']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines) + '\n')
    exe = tmp_path / 'probe'
    subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)])
    seen = 0
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        name, field, value = line.split()
        if name == 'zm_stamp_plane':
            want = C.sizeof(cls) if field == '.' else getattr(cls, field).offset
            seen += 1
        else:
            want = {'max': z._lib.STAMP_MAX, 'planes': z._lib.STAMP_PLANES_MAX,
                    'status': z._lib.STAMP_NOT_FINITE * 10 + z._lib.STAMP_NO_OVERLAP}[name]
        assert int(value) == want, (name, field, int(value), want)
    assert seen == len(cls._fields_) + 1


def test_fits_bytes_and_image_table_round_trip(tmp_path):
    z = pkg()
    f = z.fits
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    p = str(tmp_path / 'a.fits')
    f.write(p, a, {'FOO': 'bar', 'X': 1.5})
    assert open(p, 'rb').read() == f.to_bytes(a, {'FOO': 'bar', 'X': 1.5})
    d, h, _ = f.from_bytes(f.to_bytes(a, {'FOO': 'bar', 'X': 1.5}))
    assert np.array_equal(d, a) and h['FOO'] == 'bar' and h['X'] == 1.5
    u = np.array([[0, 65535], [3, 4]], np.uint16)
    assert np.array_equal(f.from_bytes(f.to_bytes(u))[0], u)
    t = np.zeros(3, dtype=[('ra', 'f8'), ('x0', 'i4')])
    t['ra'], t['x0'] = [1.5, 2.5, 3.5], [-1, 0, 7]
    f.write_image_table(p, a, t, {'NDET': 3})
    d, h, tt, th = f.read_image_table(p)
    assert np.array_equal(d, a) and h['EXTEND'] is True and h['NDET'] == 3
    assert list(tt['ra']) == [1.5, 2.5, 3.5] and list(tt['x0']) == [-1, 0, 7] and th['EXTNAME'] == 'STAMPS'
    assert np.array_equal(f.read(p)[0], a)               # the primary HDU reads as any image
