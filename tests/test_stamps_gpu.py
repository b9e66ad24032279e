"""Detection stamps through the C-ABI (zm_stamp_origin / zm_stamps_dev / zm_stamps, csrc/stamps.hip).

The pin is bit identity: a stamp pixel of a plane on another grid is the float32 ``zm_resample_dev`` writes to that grid
pixel (``np.array_equal`` on the uint32 views, zero padding outside the grid), for the geometries of
``tests/test_resample_gpu.py``, both kernels, ``fscale != 1`` and poisoned frames.  Independently of our own resampler the
TPV case is held against ``oracle/resample.py`` with the resampler's existing tolerance.  Norms are held to
``np.linalg.norm`` within 10 x the difference between forward and reversed summation on the same blocks (the extractor's
rule, ``tests/extract_ref.py``)."""
import ctypes as C

import numpy as np
import pytest

from oracle import resample as oresample
from util import assert_close_masked, pkg, synth, to_oracle_wcs

pytestmark = pytest.mark.gpu

KERN = {'LANCZOS3': 3, 'BILINEAR': 1, 'NEAREST': 0}
SIZES = (63, 64, 21, 1, 256)


def _mods():
    import importlib
    return importlib.import_module('zuds-pipeline_amd._lib'), importlib.import_module('zuds-pipeline_amd.hipmem')


def resample_dev(engine, img, win, wout, kernel, fscale):
    """(out_img, out_wgt) of zm_resample_dev(ctx, img, NULL, NULL, &win, &wout, kernel, fscale, ...)."""
    lib, hm = _mods()
    img = np.ascontiguousarray(img, np.float32)
    onx, ony = wout.naxis
    d_in, d_o, d_w = hm.DeviceBuffer(img.nbytes), hm.DeviceBuffer(onx * ony * 4), hm.DeviceBuffer(onx * ony * 4)
    d_in.upload(img)
    a, b = lib.wcs_struct(win), lib.wcs_struct(wout)
    lib.check(engine.L.zm_resample_dev(engine.ctx, d_in.ptr, None, None, C.byref(a), C.byref(b), KERN[kernel],
                                       float(fscale), d_o.ptr, d_w.ptr, None), 'zm_resample_dev')
    engine.synchronize()
    return d_o.download(np.float32, (ony, onx)), d_w.download(np.float32, (ony, onx))


def plane_array(planes, dev_ptrs=None):
    lib, _ = _mods()
    arr = (lib.zm_stamp_plane * len(planes))()
    keep = []
    for p, (img, wcs, fscale, on_grid) in enumerate(planes):
        img = np.ascontiguousarray(img, np.float32)
        keep.append(img)
        arr[p].img = dev_ptrs[p] if dev_ptrs else img.ctypes.data
        arr[p].wcs = lib.wcs_struct(wcs)
        arr[p].fscale = float(fscale)
        arr[p].on_grid = int(on_grid)
    return arr, keep


def stamps(engine, planes, wgrid, x0, y0, S, kernel='LANCZOS3', dev=True, norms=True):
    """(blocks [n, P, S, S], norms [n, P]); planes: (img, wcs, fscale, on_grid)."""
    lib, hm = _mods()
    x0, y0 = np.ascontiguousarray(x0, np.int32), np.ascontiguousarray(y0, np.int32)
    n, P = x0.size, len(planes)
    g = lib.wcs_struct(wgrid)
    out = np.empty((n, P, S, S), np.float32)
    nrm = np.empty((n, P), np.float64)
    if not dev:
        arr, keep = plane_array(planes)
        lib.check(engine.L.zm_stamps(engine.ctx, P, arr, C.byref(g), KERN[kernel], n, x0.ctypes.data, y0.ctypes.data, S,
                                     out.ctypes.data, nrm.ctypes.data if norms else None), 'zm_stamps')
        return out, nrm
    bufs = []
    for img, *_ in planes:
        img = np.ascontiguousarray(img, np.float32)
        b = hm.DeviceBuffer(img.nbytes)
        b.upload(img)
        bufs.append(b)
    arr, keep = plane_array(planes, [b.ptr for b in bufs])
    d_out, d_n = hm.DeviceBuffer(max(out.nbytes, 16)), hm.DeviceBuffer(max(nrm.nbytes, 16))
    lib.check(engine.L.zm_stamps_dev(engine.ctx, P, arr, C.byref(g), KERN[kernel], n, x0.ctypes.data, y0.ctypes.data, S,
                                     d_out.ptr, d_n.ptr if norms else None), 'zm_stamps_dev')
    engine.synchronize()
    if n:
        out, nrm = d_out.download(np.float32, out.shape), d_n.download(np.float64, nrm.shape)
    return out, nrm


def crop(plane, x0, y0, S):
    """Zero-padded S x S crops of a plane: the restatement of Cutout2D(mode='partial', fill_value=0)."""
    ny, nx = plane.shape
    out = np.zeros((len(x0), S, S), plane.dtype)
    for k, (a, b) in enumerate(zip(x0, y0)):
        xa, xb, ya, yb = max(a, 0), min(a + S, nx), max(b, 0), min(b + S, ny)
        if xa < xb and ya < yb:
            out[k, ya - b:yb - b, xa - a:xb - a] = plane[ya:yb, xa:xb]
    return out


def origin_ref(x, y, S):
    """The rule of astropy's overlap_slices, restated: first pixel = ceil(position - S / 2)."""
    return np.ceil(np.asarray(x, float) - S / 2.0).astype(np.int64), np.ceil(np.asarray(y, float) - S / 2.0).astype(np.int64)


def positions(onx, ony, S, seed, nscatter=200):
    """Origins (x0, y0): a seeded scatter, corners, edge mid-points, stamps straddling each edge, twins, heavy overlap,
    tile boundaries (x0 % 64 == 0, y0 % 32 == 0) and one pixel either side."""
    rng = np.random.default_rng(seed)
    x = list(rng.uniform(-0.5, onx - 0.5, nscatter))
    y = list(rng.uniform(-0.5, ony - 0.5, nscatter))
    cx, cy = (onx - 1) / 2.0, (ony - 1) / 2.0
    for px, py in [(0, 0), (onx - 1, 0), (0, ony - 1), (onx - 1, ony - 1),                 # corners
                   (cx, 0), (cx, ony - 1), (0, cy), (onx - 1, cy),                          # edge mid-points
                   (-S / 4.0, cy), (onx - 1 + S / 4.0, cy), (cx, -S / 4.0), (cx, ony - 1 + S / 4.0),   # straddling
                   (cx + 0.3, cy - 0.2), (cx + 0.3, cy - 0.2),                              # twins
                   (cx + 1, cy), (cx + 2, cy + 1), (cx + 3, cy + 2), (cx + 3.5, cy + 2.5)]:  # heavy overlap
        x.append(px)
        y.append(py)
    x0, y0 = origin_ref(x, y, S)
    x0, y0 = list(x0), list(y0)
    for bx in range(0, onx, 64):
        for by in range(0, ony, 32):
            if (bx // 64 + by // 32) % 3 == 0:                                             # a third of the tile corners
                for d in (-1, 0, 1):
                    x0.append(bx + d)
                    y0.append(by + d)
    # stamps that lie off the grid altogether are all zero
    x0 += [-S, onx, 0]
    y0 += [0, 0, ony + 5]
    return np.asarray(x0, np.int32), np.asarray(y0, np.int32)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def geometries():
    s = synth()
    g = {
        'identity': (s.tan_wcs(200, 150), s.tan_wcs(200, 150), 1.0),
        'integer_shift': (s.tan_wcs(160, 120), s.tan_wcs(160, 120, dx=-7.0, dy=4.0), 1.0),
        'half_pixel': (s.tan_wcs(160, 120), s.tan_wcs(160, 120, dx=0.5), 1.0),
        'tpv': (s.ztf_wcs(400, 360, dx=5.3, dy=-8.7, rot_deg=0.1, tpv=True), s.ztf_wcs(420, 380, tpv=True), 0.37),
        'large_rotation': (s.ztf_wcs(300, 300, rot_deg=30.0, tpv=False), s.tan_wcs(220, 200, scale=1.7 * 2.8125e-4), 1.3),
        'disjoint': (s.tan_wcs(128, 128), s.tan_wcs(128, 128, crval=(200.0, -10.0)), 1.0),
    }
    for (nx, ny, onx, ony) in [(33, 17, 31, 19), (65, 129, 67, 15), (1, 1, 5, 5), (7, 7, 1, 1)]:
        g[f'ragged_{nx}x{ny}_{onx}x{ony}'] = (s.tan_wcs(nx, ny, dx=0.3, dy=-0.2), s.tan_wcs(onx, ony), 0.9)
    return g


GEOMS = list(geometries())


def frame_of(win, seed, poison=False):
    s = synth()
    nx, ny = win.naxis
    f = s.make_frame(nx, ny, seed, win, nstars=max(1, nx * ny // 2500))
    if poison:
        f = s.add_nonfinite(f, seed + 1, nscatter=max(3, nx * ny // 400), block=(nx // 3, ny // 3, 7, np.inf),
                            rows=(ny // 2,), cols=(nx // 4,), edges=True)
    return f['img']


def check_identity(engine, img, win, wout, fscale, kernel, S, seed, nscatter=200):
    full, _ = resample_dev(engine, img, win, wout, kernel, fscale)
    x0, y0 = positions(wout.naxis[0], wout.naxis[1], S, seed, nscatter)
    got, _ = stamps(engine, [(img, win, fscale, 0)], wout, x0, y0, S, kernel, norms=False)
    want = crop(full, x0, y0, S)
    if not same_bits(got[:, 0], want):
        bad = np.argwhere(got[:, 0].view(np.uint32) != want.view(np.uint32))
        k, j, i = bad[0]
        raise AssertionError(f'{len(bad)} stamp pixels differ from zm_resample_dev; first: stamp {k} (x0 {x0[k]}, y0 {y0[k]}) '
                             f'pixel ({j}, {i}): {got[k, 0, j, i]!r} vs {want[k, j, i]!r}')
    return full, x0, y0, got


@pytest.mark.parametrize('kernel', ['LANCZOS3', 'BILINEAR'])
@pytest.mark.parametrize('geom', GEOMS)
def test_stamp_pixels_are_the_bits_of_zm_resample_dev(engine, geom, kernel):
    win, wout, fscale = geometries()[geom]
    img = frame_of(win, 31)
    for S in SIZES:
        check_identity(engine, img, win, wout, fscale, kernel, S, seed=100 + S)


@pytest.mark.parametrize('kernel', ['LANCZOS3', 'BILINEAR'])
@pytest.mark.parametrize('geom', ['identity', 'half_pixel', 'tpv', 'large_rotation'])
def test_poisoned_frames_keep_the_bits(engine, geom, kernel):
    """NaN / +-inf pixels (synth.add_nonfinite): the rule of oracle/resample.py arrives through the same prep_pixel."""
    win, wout, fscale = geometries()[geom]
    img = frame_of(win, 32, poison=True)
    assert not np.isfinite(img).all()
    for S in (63, 21):
        full, x0, y0, got = check_identity(engine, img, win, wout, fscale, kernel, S, seed=200 + S)
    assert np.isfinite(got).all()                 # a resampled plane never carries a non-finite value


def test_host_form_two_runs_empty_call_and_4096_stamps(engine):
    win, wout, fscale = geometries()['tpv']
    s = synth()
    sci = frame_of(win, 33)
    other = frame_of(win, 34, poison=True)
    ref = s.make_frame(wout.naxis[0], wout.naxis[1], 35, wout)['img']
    ref[5, 7] = np.nan
    planes = [(sci, win, fscale, 0), (other, win, 1.0, 0), (ref, wout, 1.0, 1)]
    x0, y0 = positions(wout.naxis[0], wout.naxis[1], 63, 7)
    a, na = stamps(engine, planes, wout, x0, y0, 63)
    b, nb = stamps(engine, planes, wout, x0, y0, 63)
    h, nh = stamps(engine, planes, wout, x0, y0, 63, dev=False)
    assert a.tobytes() == b.tobytes() and na.tobytes() == nb.tobytes()
    assert a.tobytes() == h.tobytes() and na.tobytes() == nh.tobytes()
    # each plane of a joint call is what the plane gives alone
    alone, _ = stamps(engine, planes[1:2], wout, x0, y0, 63, norms=False)
    assert same_bits(a[:, 1], alone[:, 0])
    # n = 0: a successful no-op, on both forms
    e, ne = stamps(engine, planes, wout, np.zeros(0, np.int32), np.zeros(0, np.int32), 63)
    assert e.shape == (0, 3, 63, 63)
    stamps(engine, planes, wout, np.zeros(0, np.int32), np.zeros(0, np.int32), 63, dev=False)
    # 4096 stamps in one call
    rng = np.random.default_rng(5)
    X0 = rng.integers(-62, wout.naxis[0], 4096).astype(np.int32)
    Y0 = rng.integers(-62, wout.naxis[1], 4096).astype(np.int32)
    big, _ = stamps(engine, planes, wout, X0, Y0, 63, norms=False)
    full0, _ = resample_dev(engine, sci, win, wout, 'LANCZOS3', fscale)
    full1, _ = resample_dev(engine, other, win, wout, 'LANCZOS3', 1.0)
    assert same_bits(big[:, 0], crop(full0, X0, Y0, 63))
    assert same_bits(big[:, 1], crop(full1, X0, Y0, 63))
    assert same_bits(big[:, 2], crop(ref, X0, Y0, 63))


@pytest.mark.parametrize('S', SIZES)
def test_on_grid_gather_is_numpy_slicing(engine, S):
    s = synth()
    w = s.tan_wcs(150, 97)
    img = s.make_frame(150, 97, 41, w)['img']
    img[::7, ::5] = np.nan
    img[3, 3] = np.inf
    x0, y0 = positions(150, 97, S, 8, nscatter=60)
    got, _ = stamps(engine, [(img, w, 1.0, 1)], w, x0, y0, S, norms=False)
    assert same_bits(got[:, 0], crop(img, x0, y0, S))
    assert np.isnan(got).any()


@pytest.mark.parametrize('kernel', ['LANCZOS3', 'BILINEAR'])
def test_tpv_stamps_agree_with_the_oracle(engine, kernel):
    """Independent pin: oracle/resample.py, the existing resampler tolerance (tests/test_resample_gpu.py:37); every pixel
    valid on both sides is compared - validity itself is fixed by the bit identity above."""
    win, wout, fscale = geometries()['tpv']
    img = frame_of(win, 36)
    kind = {'LANCZOS3': oresample.LANCZOS3, 'BILINEAR': oresample.BILINEAR}[kernel]
    onx, ony = wout.naxis
    px, py = oresample.positions(to_oracle_wcs(wout), to_oracle_wcs(win), onx, ony)
    r_img, r_wgt, _ = oresample.resample(img, None, px, py, kind, fscale, None)
    _, g_wgt = resample_dev(engine, img, win, wout, kernel, fscale)
    x0, y0 = positions(onx, ony, 63, 9)
    got, _ = stamps(engine, [(img, win, fscale, 0)], wout, x0, y0, 63, kernel, norms=False)
    both = (crop(g_wgt, x0, y0, 63) > 0) & (crop(np.asarray(r_wgt), x0, y0, 63) > 0)
    assert both.sum() > 100000
    scale = float(np.std(img)) * abs(fscale)
    assert_close_masked(got[:, 0][both], crop(np.asarray(r_img, np.float64), x0, y0, 63)[both], 2e-5, 2e-5 * scale, 'stamp values')


def test_norms(engine):
    win, wout, fscale = geometries()['tpv']
    s = synth()
    sci = frame_of(win, 37)
    ref = s.make_frame(wout.naxis[0], wout.naxis[1], 38, wout)['img']
    ref[100, 100] = np.nan
    for S in (63, 64, 1, 256):
        x0, y0 = positions(wout.naxis[0], wout.naxis[1], S, 10, nscatter=100)
        x0, y0 = np.append(x0, 100 - S // 2).astype(np.int32), np.append(y0, 100 - S // 2).astype(np.int32)   # holds the NaN
        blocks, norms = stamps(engine, [(sci, win, fscale, 0), (ref, wout, 1.0, 1)], wout, x0, y0, S)
        sq = blocks.astype(np.float64).reshape(len(x0), 2, S * S) ** 2
        want = np.array([[np.linalg.norm(blocks[k, p].astype(np.float64)) for p in range(2)] for k in range(len(x0))])
        fwd, rev = np.sqrt(sq.sum(axis=2)), np.sqrt(sq[:, :, ::-1].sum(axis=2))
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(norms), ~fin) and (~fin).any() and fin[:, 0].all()
        assert np.array_equal(~fin, np.isnan(blocks).any(axis=(2, 3)))      # a block holding NaN gives NaN
        bound = 10.0 * float(np.abs(fwd[fin] - rev[fin]).max())
        diff = float(np.abs(norms[fin] - want[fin]).max())
        print(f'stamp norms S={S}: measured {diff:.3g}, order bound {bound:.3g}')
        assert diff <= bound


def test_origin_rule_matches_the_restatement(engine):
    lib, _ = _mods()
    s = synth()
    w = s.ztf_wcs(420, 380, tpv=True)
    rng = np.random.default_rng(11)
    x, y = rng.uniform(-40, 460, 500), rng.uniform(-40, 420, 500)
    ra, dec = w.all_pix2world(x, y, 0)
    g = lib.wcs_struct(w)
    for S in SIZES:
        x0, y0, st = (np.zeros(500, np.int32) for _ in range(3))
        lib.check(engine.L.zm_stamp_origin(C.byref(g), 500, ra.ctypes.data, dec.ctypes.data, S, x0.ctypes.data,
                                           y0.ctypes.data, st.ctypes.data))
        xx, yy = w.all_world2pix(ra, dec, 0)
        rx, ry = origin_ref(xx, yy, S)
        ok = st == 0
        assert np.array_equal(x0[ok], rx[ok]) and np.array_equal(y0[ok], ry[ok])
        assert np.array_equal(ok, (rx + S > 0) & (rx < 420) & (ry + S > 0) & (ry < 380))


def test_refusals(engine):
    lib, hm = _mods()
    z = pkg()
    s = synth()
    w = s.tan_wcs(64, 64)
    img = np.zeros((64, 64), np.float32)
    buf, out = hm.DeviceBuffer(img.nbytes), hm.DeviceBuffer(4 * 256 * 256)
    buf.upload(img)
    arr, keep = plane_array([(img, w, 1.0, 0)], [buf.ptr])
    g = lib.wcs_struct(w)
    x0 = np.zeros(1, np.int32)

    def call(planes=arr, kernel=3, S=63, xp=x0.ctypes.data, outp=out.ptr, grid=C.byref(g), fn=engine.L.zm_stamps_dev):
        rc = fn(engine.ctx, 1, planes, grid, kernel, 1, xp, x0.ctypes.data, S, outp, None)
        return rc, engine.L.zm_last_error().decode()

    assert call()[0] == 0
    for kw, word in [(dict(kernel=0), 'LANCZOS3'), (dict(S=0), 'size'), (dict(S=257), 'size'), (dict(xp=None), 'null'),
                     (dict(outp=None), 'null'), (dict(planes=None), 'null'), (dict(grid=None), 'null'),
                     (dict(kernel=0, fn=engine.L.zm_stamps), 'LANCZOS3')]:
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    null_img, _ = plane_array([(img, w, 1.0, 0)], [None])
    rc, msg = call(planes=null_img)
    assert rc != 0 and 'image' in msg
    e2 = z.Engine(0)
    try:
        e2.set_conventions(edge='truncate')
        rc = e2.L.zm_stamps_dev(e2.ctx, 1, arr, C.byref(g), 3, 1, x0.ctypes.data, x0.ctypes.data, 63, out.ptr, None)
        assert rc != 0 and 'conventions' in e2.L.zm_last_error().decode()
    finally:
        e2.close()
    with pytest.raises(z.ZMError):
        lib.check(engine.L.zm_stamp_origin(C.byref(g), 1, None, None, 63, x0.ctypes.data, x0.ctypes.data, x0.ctypes.data))
