"""NaN, +-inf and extreme weights on every HIP path, against the oracle's rule for them (oracle/resample.py,
oracle/background.py): a non-finite value is a bad input pixel, an output whose interpolated variance reaches
BADVAR_TEST is bad, a mesh sample needs |p| < BIG.

Real inputs carry such pixels: ZTF frames have NaN pixels (zuds/constants.py:59), and the reference's rms map is inf
on an unmasked zero-weight pixel - the map that the pair alignment takes to the science grid on the default
subtraction route.  The comparisons use the tolerances of test_resample_gpu.py, test_coadd_gpu.py and
test_background_gpu.py; validity must agree exactly except on pixels within the lattice error of the snap (or of
x.5 for NEAREST), and nothing that leaves a kernel may be non-finite."""
import ctypes as C

import numpy as np
import pytest

from oracle import background as oback
from oracle import combine as ocombine
from oracle import resample as oresample
from util import assert_close_masked, pkg, synth, to_oracle_wcs

pytestmark = pytest.mark.gpu

KINDS = {'LANCZOS3': oresample.LANCZOS3, 'BILINEAR': oresample.BILINEAR, 'NEAREST': oresample.NEAREST}
BAD_WEIGHTS = (np.nan, np.inf, -1.0, 1e-30, 1.5e-30, 1e-20, 1e-16, 1e-12)
LATTICE_ERR = 1e-4          # px: the fp32 lattice interpolation of a position against the fp64 oracle


def poison(f, seed, with_w=True):
    """Single NaN / +inf / -inf pixels, a 20 x 20 NaN block, a full NaN row and column, NaN on the four edges (corners
    included) and, with a weight map, the weights of BAD_WEIGHTS at scattered pixels."""
    ny, nx = f['img'].shape
    rng = np.random.default_rng(seed)
    wts = None
    if with_w:
        xs, ys = rng.integers(8, nx - 8, 3 * len(BAD_WEIGHTS)), rng.integers(8, ny - 8, 3 * len(BAD_WEIGHTS))
        wts = [(int(x), int(y), BAD_WEIGHTS[k % len(BAD_WEIGHTS)]) for k, (x, y) in enumerate(zip(xs, ys))]
    return synth().add_nonfinite(f, seed, nscatter=60, block=(nx // 3, ny // 2, 20, np.nan), rows=(ny // 4,),
                                 cols=(2 * nx // 3,), edges=True, weights=wts)


def near_snap(px, py, kernel):
    """Output pixels whose position sits within the lattice error of a snap (or of the x.5 of NEAREST)."""
    def near(p):
        d = p - np.floor(p)
        if kernel == 'NEAREST':
            return np.abs(d - 0.5) < LATTICE_ERR
        return np.minimum(d, 1.0 - d) < oresample.SNAP + LATTICE_ERR
    return near(px) | near(py)


def check_resample(engine, f, win, wout, kernel, with_w, fscale=0.37, max_flip=1e-5):
    img, wgt = f['img'], (f['wgt'] if with_w else None)
    g_img, g_wgt, g_msk = engine.resample(img, win, wout, wgt=wgt, mask=f['mask'], kernel=kernel, fscale=fscale)
    assert np.isfinite(g_img).all() and np.isfinite(g_wgt).all()
    onx, ony = wout.naxis
    px, py = oresample.positions(to_oracle_wcs(wout), to_oracle_wcs(win), onx, ony)
    dbg = {}
    r_img, r_wgt, r_msk = oresample.resample(img.astype(np.float64), None if wgt is None else wgt.astype(np.float64),
                                             px, py, KINDS[kernel], fscale, np.asarray(f['mask'], np.int64),
                                             debug=dbg)
    gv, rv = g_wgt > 0, r_wgt > 0
    flip = gv != rv
    # (a variance within fp32 reach of BADVAR_TEST may land on either side: a weight near 1e-16 under a small tap)
    edge = near_snap(px, py, kernel)
    if 'vacc' in dbg:
        edge |= np.abs(dbg['vacc'] / oresample.BADVAR_TEST - 1.0) < 1e-4
    assert not (flip & ~edge).any(), f'validity differs away from the snap on {int((flip & ~edge).sum())} pixels'
    assert flip.mean() <= max_flip, f'validity differs on {flip.mean():.2e} of the pixels'
    assert (~rv).any() and rv.mean() > 0.3           # the poison is seen, the frame is not lost
    both = gv & rv
    scale = float(np.std(img[np.isfinite(img)])) * abs(fscale)
    vb = max_flip if kernel == 'NEAREST' else 0.0
    assert_close_masked(g_img[both], r_img[both], 2e-5, 2e-5 * scale, 'values', vb)
    # a weight of 1e-12 under a small tap dominates the interpolated variance, and the fp32 taps' absolute error with
    # it: such outputs are held to their validity (above), the others to the weight tolerance
    extreme = np.zeros(img.shape, np.int64)
    if wgt is not None:
        extreme[~(wgt >= 1e-6)] = 1
    reach = oresample.resample(np.zeros(img.shape), None, px, py, KINDS[kernel], 1.0, extreme)[2] != 0
    sel = both & ~reach
    assert_close_masked(g_wgt[sel], r_wgt[sel], 5e-5, 0.0, 'weights', vb)
    assert np.all(g_img[~gv] == 0)
    mm = (g_msk != r_msk).mean()
    assert mm <= max_flip, f'mask differs on {mm:.2e} of the pixels'
    return g_img, g_wgt


def geometry(name, nx=300, ny=260):
    s = synth()
    if name == 'identity':                       # delta taps on both axes
        return s.tan_wcs(nx, ny), s.tan_wcs(nx, ny)
    if name == 'half':                           # six live taps along x, a delta along y
        return s.tan_wcs(nx, ny), s.tan_wcs(nx, ny, dx=0.5)
    if name == 'rotation':                       # fractional dither and rotation
        return s.ztf_wcs(nx, ny, dx=5.3, dy=-8.7, rot_deg=0.1, tpv=True), s.ztf_wcs(nx + 20, ny + 16, tpv=True)
    if name == 'global':                         # 30 degrees and a 1.7x coarser grid: footprints beyond the LDS tile
        return s.ztf_wcs(nx, nx, rot_deg=30.0, tpv=False), s.tan_wcs(220, 200, scale=1.7 * 2.8125e-4)
    raise ValueError(name)


@pytest.mark.parametrize('geom', ['identity', 'half', 'rotation', 'global'])
@pytest.mark.parametrize('with_w', [True, False])
@pytest.mark.parametrize('kernel', ['LANCZOS3', 'BILINEAR', 'NEAREST'])
def test_resample_of_a_poisoned_frame_matches_the_oracle(engine, kernel, with_w, geom):
    win, wout = geometry(geom)
    nx, ny = win.naxis
    f = poison(synth().make_frame(nx, ny, 31, win, nbad=60, nstars=40), 7, with_w)
    check_resample(engine, f, win, wout, kernel, with_w, max_flip=1e-4 if kernel == 'NEAREST' else 1e-5)


def test_resample_with_an_int16_mask_and_single_infinities(engine):
    """zm_resample_i16: the same rule behind the int16 mask entry point; +inf and -inf alone, far from other poison
    (one inf under a Lanczos footprint gave a 6 x 6 patch of +-inf with positive weight)."""
    win, wout = geometry('rotation')
    nx, ny = win.naxis
    f = synth().make_frame(nx, ny, 32, win, nbad=40)
    f = synth().add_nonfinite(f, 0, pixels=[(60, 50, np.inf), (200, 50, -np.inf), (130, 180, np.inf),
                                            (134, 182, np.inf)])
    f['mask'] = f['mask'].astype(np.int16)
    g_img, g_wgt = check_resample(engine, f, win, wout, 'LANCZOS3', True)
    assert (g_wgt > 0).mean() > 0.8


# ---- the pair alignment ------------------------------------------------------------------------------------------

def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


@pytest.fixture
def stream_env(engine):
    import torch
    stream = torch.cuda.Stream('cuda:0')
    engine.set_stream(stream.cuda_stream)
    yield torch, stream
    stream.synchronize()
    engine.set_stream(0)


@pytest.mark.parametrize('geom', ['rotation', 'global', 'integer'])
@pytest.mark.parametrize('kernel', ['LANCZOS3', 'BILINEAR'])
def test_pair_alignment_of_poisoned_planes_equals_the_two_alignments(engine, stream_env, kernel, geom):
    """zm_align_pair_dev with NaN and +-inf in both images (different places in each): every value and the mask equal
    those of two zm_resample_dev calls without weights bit for bit - a bad pixel in one channel leaves the other alone -
    on the LDS path (rotation / dither), the global path (coarser grid) and an integer shift (delta taps, where the LDS
    path multiplies the zero taps too).  The validity of each channel is the oracle's exactly; the values, pinned to
    zm_resample_dev here and through it to the oracle in test_resample_gpu.py, are compared coarsely: the rms map's
    steps from 2-6 to 223.6 at masked pixels cost the fp32 taps more than 2e-5 of the map's spread."""
    torch, stream = stream_env
    z, s = pkg(), synth()
    engine.set_stream(stream.cuda_stream)
    nx, ny = 420, 380
    wref = s.ztf_wcs(nx, ny, tpv=True)
    if geom == 'rotation':
        wsci = s.ztf_wcs(nx + 40, ny - 30, dx=-17.3, dy=9.6, rot_deg=0.4, tpv=True)
    elif geom == 'global':
        wsci = s.ztf_wcs(nx // 2, ny // 2, dx=3.3, dy=-2.1, rot_deg=0.2, tpv=True)
        wsci.cd = np.asarray(wsci.cd) * 2.6
    else:
        wsci = s.ztf_wcs(nx, ny, dx=-7.0, dy=3.0)
    f = s.make_frame(nx, ny, 4243, wref, nstars=60, nbad=80)
    rng = np.random.default_rng(6)
    rms = np.where(f['mask'] != 0, np.float32(223.6068), rng.uniform(2.0, 6.0, (ny, nx))).astype(np.float32)
    a = poison(f, 11, with_w=False)['img']
    b = synth().add_nonfinite(dict(img=rms), 12, nscatter=40, values=(np.inf, np.nan, -np.inf),
                              block=(250, 60, 20, np.inf), cols=(nx // 5,))['img']
    L, W = engine.L, z._lib.wcs_struct
    wa, wb = W(wref), W(wsci)
    onx, ony = wsci.naxis
    K = z._lib.RESAMPLE[kernel]
    with torch.cuda.stream(stream):
        d_a, d_b, d_m = dev(torch, a), dev(torch, b), dev(torch, f['mask'].astype(np.int32))
        o = [torch.empty((ony, onx), dtype=torch.float32, device='cuda') for _ in range(6)]
        m = [torch.empty((ony, onx), dtype=torch.int32, device='cuda') for _ in range(2)]
        z._lib.check(L.zm_resample_dev(engine.ctx, d_a.data_ptr(), None, d_m.data_ptr(), C.byref(wa), C.byref(wb), K,
                                       0.37, o[0].data_ptr(), o[1].data_ptr(), m[0].data_ptr()))
        z._lib.check(L.zm_resample_dev(engine.ctx, d_b.data_ptr(), None, None, C.byref(wa), C.byref(wb), K, 0.61,
                                       o[2].data_ptr(), o[3].data_ptr(), None))
        z._lib.check(L.zm_align_pair_dev(engine.ctx, d_a.data_ptr(), d_b.data_ptr(), d_m.data_ptr(), C.byref(wa),
                                         C.byref(wb), K, 0.37, 0.61, o[4].data_ptr(), o[5].data_ptr(), m[1].data_ptr()))
    stream.synchronize()
    h = [t.cpu().numpy() for t in o]
    for k in range(6):
        assert np.isfinite(h[k]).all(), k
    assert np.array_equal(h[0].view(np.int32), h[4].view(np.int32)), \
        f'channel a: {int((h[0] != h[4]).sum())} pixels differ'
    assert np.array_equal(h[2].view(np.int32), h[5].view(np.int32)), \
        f'channel b: {int((h[2] != h[5]).sum())} pixels differ'
    assert torch.equal(m[0], m[1])
    # each channel's validity is its own: the bad pixels of b do not reach a
    assert ((h[1] > 0) != (h[3] > 0)).any()
    # and the oracle's, per channel (no weight map)
    px, py = oresample.positions(to_oracle_wcs(wsci), to_oracle_wcs(wref), onx, ony)
    edge = near_snap(px, py, kernel)
    for x, fs, ov, ow in ((a, 0.37, h[0], h[1]), (b, 0.61, h[2], h[3])):
        r_img, r_wgt, _ = oresample.resample(x.astype(np.float64), None, px, py, KINDS[kernel], fs)
        flip = (ow > 0) != (r_wgt > 0)
        assert not (flip & ~edge).any() and flip.mean() <= 1e-5
        assert (r_wgt == 0).mean() > 0.02
        both = (ow > 0) & (r_wgt > 0)
        scale = float(np.std(x[np.isfinite(x)])) * fs
        assert_close_masked(ov[both], r_img[both], 2e-5, 2e-5 * scale, 'pair values', max_bad_frac=2e-3)


# ---- the fused coadd ---------------------------------------------------------------------------------------------

FORMS = ({'ZM_COADD_FUSED': '0'}, {}, {'ZM_FF_FORM': 'dma'}, {'ZM_FF_RAW': '0'})


def poisoned_stack(seed=700, nx=420, ny=400):
    s = synth()
    base = s.ztf_wcs(nx, ny, tpv=True)
    rng = np.random.default_rng(seed)
    xs, ys = rng.uniform(5, nx - 5, 50), rng.uniform(5, ny - 5, 50)
    fl = np.exp(rng.uniform(np.log(2e3), np.log(5e4), 50))
    ra, dec = base.all_pix2world(xs, ys, 0)
    frames = []
    for i in range(5):
        w = s.ztf_wcs(nx, ny, dx=rng.uniform(-6, 6), dy=rng.uniform(-6, 6), rot_deg=rng.uniform(-0.2, 0.2), tpv=True)
        frames.append(s.make_frame(nx, ny, seed + i, w, star_sky=(ra, dec, fl), magzp=rng.uniform(25.5, 26.5),
                                   nbad=60))
    frames[0] = poison(frames[0], 1)
    frames[1] = s.add_nonfinite(frames[1], 2, nscatter=30, values=(np.inf, -np.inf))
    frames[2] = s.add_nonfinite(frames[2], 3, edges=True, weights=[(x, y, BAD_WEIGHTS[k % 8]) for k, (x, y) in
                                                                   enumerate(zip(range(20, 400, 19), range(15, 390, 18)))])
    # the rims of the fused items' staged boxes (a 64 x 32 output tile stages about 70 x 38 input pixels: the own
    # slot is 80 x 42): NaN lines that every box crosses near its edges
    frames[3] = s.add_nonfinite(frames[3], 4, rows=tuple(range(3, ny, 37)), cols=tuple(range(5, nx, 71)))
    return frames, base


def oracle_coadd(frames, wout, kind):
    onx, ony = wout.naxis
    ow = to_oracle_wcs(wout)
    vals, wgts = [], []
    for f in frames:
        wi = to_oracle_wcs(f['wcs'])
        px, py = oresample.positions(ow, wi, onx, ony)
        fs = oresample.flux_scale(wi, ow, f.get('flxscale', 1.0))
        o, w, _ = oresample.resample(f['img'].astype(np.float64), f['wgt'].astype(np.float64), px, py,
                                     oresample.LANCZOS3, fs)
        vals.append(o)
        wgts.append(w)
    out, outw, _ = ocombine.combine(np.array(vals), np.array(wgts), kind)
    return out, outw


@pytest.mark.parametrize('kind', ['WEIGHTED', 'AVERAGE', 'CLIPPED', 'MEDIAN'])
def test_fused_coadd_of_poisoned_frames_is_one_result_and_the_oracles(engine, monkeypatch, kind):
    """Every form of the coadd - the materialised k_resample path, the owner-staged fused kernel (the default), the
    LDS-DMA staged one and planes prepped ahead - gives the same bits on a stack with NaN / +-inf pixels, NaN regions
    and edges, NaN lines across the staged boxes and extreme weights; the result is the oracle's."""
    z = pkg()
    frames, wout = poisoned_stack()
    p = z.coadd_params(combine=kind, subtract_back=False, rescale_weights=False)
    res = []
    for form in FORMS:
        with monkeypatch.context() as mp:
            for k, v in form.items():
                mp.setenv(k, v)
            res.append(engine.coadd(frames, wout, p))
            if form.get('ZM_COADD_FUSED') != '0' and kind in ('WEIGHTED', 'AVERAGE'):
                assert engine.query('fused_form') == (1 if form.get('ZM_FF_FORM') == 'dma' else 2)
    for r in res:
        for x in r:
            assert x is None or np.isfinite(x).all()
    for r in res[1:]:
        for x, y, name in zip(res[0], r, ('img', 'wgt', 'mask', 'mask coverage')):
            assert np.array_equal(x, y), f'{name}: {int((x != y).sum())} of {x.size} pixels differ'
    g_img, g_wgt = res[0][0], res[0][1]
    r_img, r_wgt = oracle_coadd(frames, wout, kind)
    gv, rv = g_wgt > 0, r_wgt > 0
    assert (gv != rv).mean() < 2e-4
    both = gv & rv
    assert_close_masked(g_img[both], r_img[both], 3e-5, 3e-5 * 5.0, kind, max_bad_frac=2e-4)
    assert_close_masked(g_wgt[both], r_wgt[both], 1e-4, 0, kind + ' weight', max_bad_frac=2e-4)


# ---- the mesh background -----------------------------------------------------------------------------------------

def bg_frame(nx, ny, seed):
    s = synth()
    f = s.make_frame(nx, ny, seed, s.tan_wcs(nx, ny), sky=180.0, noise=6.0, nstars=60, nbad=200)
    yy, xx = np.mgrid[0:ny, 0:nx]
    f['img'] = (f['img'] + 0.03 * xx - 0.015 * yy + 4 * np.sin(xx / 90.0)).astype(np.float32)
    return f


def bg_cases():
    """(name, mesh, function(img) -> poisoned img)"""
    def scattered(im):
        rng = np.random.default_rng(3)
        ny, nx = im.shape
        im[rng.integers(0, ny, 500), rng.integers(0, nx, 500)] = np.nan
        return im

    def count(n):
        def f(im):                                   # n NaN pixels in mesh (1, 1) of 64 x 64 (BACK_MINGOODFRAC 0.5)
            m = im[64:128, 64:128].reshape(-1).copy()
            m[np.random.default_rng(n).permutation(m.size)[:n]] = np.nan
            im[64:128, 64:128] = m.reshape(64, 64)
            return im
        return f

    def all_nan(im):
        im[128:256, 128:256] = np.nan
        return im

    def wave_share(im):
        # k_mesh_stats_fast loads a 128 x 128 mesh in passes of 16 rows; wave w holds rows 2w and 2w + 1 of every
        # pass: NaN there leaves wave 0 without a sample (and takes the mesh's first pixel, the pivot hint, with it)
        for r0 in range(0, 128, 16):
            im[128 + r0:128 + r0 + 2, 0:128] = np.nan
        return im

    def first_inf(im):
        for y0 in range(0, im.shape[0], 128):
            for x0 in range(0, im.shape[1], 128):
                im[y0, x0] = np.inf if (x0 + y0) % 256 == 0 else -np.inf
        im[300, 301] = np.inf
        im[5, 7] = np.float32(-1e30)                 # exactly the bad-mesh marker
        return im

    return [('scattered', 128, scattered), ('below', 64, count(2048)), ('above', 64, count(2049)),
            ('all_nan', 128, all_nan), ('wave_share', 128, wave_share), ('first_inf', 128, first_inf)]


@pytest.mark.parametrize('with_w', [True, False])
@pytest.mark.parametrize('case', bg_cases(), ids=lambda c: c[0])
def test_background_of_a_poisoned_frame_matches_the_oracle(engine, case, with_w):
    name, mesh, fn = case
    f = bg_frame(512, 384, 17)
    img = fn(f['img'].copy())
    wgt = f['wgt'] if with_w else None
    bkg, rms, sub, stats = engine.background(img, wgt, mesh=mesh)
    r_bkg, r_rms, r_mean, r_sig, r_bo, _ = oback.background(img.astype(np.float64),
                                                            None if wgt is None else wgt.astype(np.float64), mesh)
    assert np.isfinite(bkg).all() and np.isfinite(rms).all() and np.isfinite(stats).all()
    assert np.isfinite(r_bkg).all() and np.isfinite(r_rms).all()
    assert_close_masked(bkg, r_bkg, 2e-5, 1e-3, 'background')
    assert_close_masked(rms, r_rms, 1e-4, 1e-4, 'background rms')
    fin = np.isfinite(img)
    np.testing.assert_allclose(sub[fin], (img - bkg)[fin], atol=1e-4)
    assert abs(stats[0] - r_mean) < 2e-3 and abs(stats[1] - r_sig) < 1e-3
    if name in ('below', 'above') and not with_w:
        # 2048 samples of 4096 keep the mesh, 2047 do not (with the weight map the masked pixels go too)
        assert (r_bo is not None) and ((oback.mesh_maps(img.astype(np.float64), None, mesh)[0][1, 1] > -oback.BIG)
                                       == (name == 'below'))


# ---- the subtraction, end to end ---------------------------------------------------------------------------------

def test_device_subtraction_with_a_poisoned_reference_is_the_same_by_either_alignment(engine, monkeypatch):
    """NaN in the reference image, NaN and inf in its rms map (the map is inf on an unmasked zero-weight pixel):
    the pair alignment (ZM_ALIGN_PAIR=1, the default) and the two separate alignments give the same products, mask and
    fit summary bit for bit, and diff / noise are finite wherever the product mask has no bit 17."""
    import torch
    z, s = pkg(), synth()
    dmod = __import__('importlib').import_module('zuds-pipeline_amd.device')
    from importlib import import_module
    BIG_RMS = import_module('zuds-pipeline_amd.constants').BIG_RMS
    nx = ny = 448
    wref = s.ztf_wcs(nx, ny, tpv=True)
    wsci = s.ztf_wcs(nx, ny, dx=7.4, dy=-5.3, rot_deg=0.08, tpv=True)
    rng = np.random.default_rng(99)
    xs, ys = rng.uniform(-40, nx + 40, 90), rng.uniform(-40, ny + 40, 90)
    fl = np.exp(rng.uniform(np.log(2e3), np.log(1e5), 90))
    ra, dec = wref.all_pix2world(xs, ys, 0)
    ref = s.make_frame(nx, ny, 991, wref, star_sky=(ra, dec, fl), fwhm=2.0, nbad=60)
    sci = s.make_frame(nx, ny, 992, wsci, star_sky=(ra, dec, fl), fwhm=2.0, nbad=60, magzp=25.2)

    def rms_of(w):
        with np.errstate(divide='ignore'):
            return np.where(w > 0, 1.0 / np.sqrt(np.where(w > 0, w, 1.0)), BIG_RMS).astype(np.float32)
    ref = s.add_nonfinite(ref, 5, nscatter=25, values=(np.nan,), block=(200, 150, 20, np.nan))
    ref_rms = rms_of(ref['wgt'])
    ref_rms = s.add_nonfinite(dict(img=ref_rms), 6, nscatter=30, values=(np.nan, np.inf),
                              pixels=[(300, 310, np.inf), (301, 310, np.inf)])['img']
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to('cuda:0')
    args = (t(sci['img'], np.float32), t(rms_of(sci['wgt']), np.float32), t(sci['mask'], np.int32),
            t(sci['wgt'], np.float32), t(ref['img'], np.float32), t(ref_rms, np.float32), t(ref['mask'], np.int32))
    out = {}
    for pair in ('1', '0'):
        monkeypatch.setenv('ZM_ALIGN_PAIR', pair)
        ds = dmod.DeviceSubtraction(wsci, wref, device=0, engine=engine)
        torch.cuda.synchronize()
        diff, noise, submask = ds.run(*args, seeing=2.0, nreg_side=1, hotpants_kws={'ko': 1, 'bgo': 0})
        ds.stream.synchronize()
        engine.set_stream(0)
        info = {k: getattr(ds.info, k) for k, _ in ds.info._fields_}
        out[pair] = (diff.cpu().numpy(), noise.cpu().numpy(), submask.cpu().numpy(), info)
    a, b = out['1'], out['0']
    for x, y, name in zip(a[:3], b[:3], ('diff', 'noise', 'mask')):
        assert np.array_equal(x, y, equal_nan=True), f'{name}: {int((x != y).sum())} pixels differ'
    assert a[3] == b[3]
    assert a[3]['status'] == 0
    diff, noise, submask = a[:3]
    ok = (submask & (1 << 17)) == 0
    assert ok.mean() > 0.5
    assert np.isfinite(diff[ok]).all() and np.isfinite(noise[ok]).all()
