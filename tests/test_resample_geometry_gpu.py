"""The resampling kernels on the geometries of tests/resample_scenes.py, against the oracle's exact positions.

k_resample, the nearest-neighbour kernel, the pair form and both fused coadd kernels take their positions from
resample_dev.h / wcs_math.h; the fused kernels are otherwise only held to k_resample bit for bit.  Here every scene
- tangent points apart, across RA 0, next to the pole, TPV to degree 7 with radial terms, TPV on one side, quarter
turns, mirrored frames, 0.5 x to 3 x pixel scales, exact fractions - is compared with ``oracle.resample.resample`` at
``oracle.wcs.map_out_to_in`` positions (pinned to 50-digit spherical trigonometry in tests/test_resample_scenes.py).

Rules (tests/resample_scenes.py).  Validity (weight > 0) and every mask bit must agree EXACTLY outside the pixels whose
oracle position lies within 2 delta0 of a snap threshold (for NEAREST: of a half-integer); those are at most 1e-3 of
the covered pixels (asserted on the CPU) and none in the exact scenes.  Values agree to bound x (2e-5 |ref| + 2e-5
std(img)), weights to bound x 5e-5 |ref|, with the table of tests/measure_resample_tolerance.py - the kernel's
positions emulated in numpy float32 (fp64 lattice nodes every 16 px, minus the tile's box origin, rounded to fp32,
bilinear in fp32) fed to the oracle; bound = 1 where that emulation stays inside the existing tolerance, else 4 x its
deviation (fp32 tap table 2.4e-7, 36 fp32 products, one contraction difference between numpy and the device):

    scene                 delta0 [px]   emulated values / weights   bound values / weights   MI355X values
    crval_offset            9.57e-06        0.268    0.000              1       1          0.259
    across_ra_zero          6.89e-06        0.271    0.000              1       1          0.275
    near_pole               1.02e-05        0.508    0.000              1       1          0.506
    tpv_degree7_radial      1.43e-05        1.394    0.000              5.58    1          1.387
    tpv_to_tan              2.08e-05        1.930    0.000              7.73    1          1.933
    tan_to_tpv              1.88e-05        1.565    0.000              6.27    1          1.510
    rot90                   3.67e-06        0.439    0.000              1       1          0.373
    rot180                  2.75e-06        0.229    0.000              1       1          0.230
    rot270                  3.67e-06        0.328    0.000              1       1          0.332
    rot90_exact             2.96e-12        0.000    0.000              1       1          0.000
    mirrored                1.03e-05        0.398    0.000              1       1          0.401
    mirrored_rot90          3.67e-06        0.404    0.000              1       1          0.405
    finer_2x                1.67e-06        0.153    0.000              1       1          0.151
    coarser_2x              2.09e-05        0.788    0.000              1       1          0.778
    coarser_3x              2.11e-05        0.967    0.000              1       1          0.967
    quarter_shift           2.96e-12        0.000    0.000              1       1          0.016
    half_shift              2.96e-12        0.000    0.000              1       1          0.017

(last column: what k_resample gave on an MI355X when the table was made, weights at most 0.007, no validity or mask
flip in any scene; BILINEAR at most 0.703, on coarser_2x.)  The three scenes above 1 are the ones with an uncancelled
TPV distortion: what exceeds the bound there is the bilinear interpolation of the map between lattice nodes 16 px apart
(1.4e-5 to 2.1e-5 px), not the fp32 tile-relative positions, which stay inside the existing bound up to the 3 x coarser
grid (a 200 px wide tile footprint; the scale sweep of the measuring script puts the emulation at 1.4 x the bound from
4 x on, where the footprint passes 256 px).
"""
import ctypes as C

import numpy as np
import pytest

import resample_scenes as rs
from oracle import resample as oresample
from util import assert_close_masked, pkg

pytestmark = pytest.mark.gpu


def deviation(got, ref, tol):
    if not got.size:
        return 0.0
    return float((np.abs(got.astype(np.float64) - ref) / tol).max())


def compare(name, kernel, g_img, g_wgt, g_msk, ref=None, std=None, valid_is_nonzero=False):
    """The rules of the module docstring; prints the figures before it asserts."""
    sc = rs.scene(name)
    _, _, r_img, r_wgt, r_msk = rs.reference(name, kernel) if ref is None else (None, None) + tuple(ref)
    _, bv, bw = rs.BOUNDS[name]
    near = rs.near_decision(name, kernel)
    gv = (g_img != 0) if valid_is_nonzero else (g_wgt > 0)
    rv = r_wgt > 0
    both = gv & rv & ~near if kernel == 'NEAREST' else gv & rv
    std = float(np.std(sc.img)) if std is None else std
    dv = deviation(g_img[both], r_img[both], rs.RTOL * np.abs(r_img[both]) + rs.ATOL * std)
    dw = 0.0 if g_wgt is None else deviation(g_wgt[both], r_wgt[both], rs.WTOL * np.abs(r_wgt[both]))
    flips = int(((gv != rv) & ~near).sum())
    mflips = -1 if g_msk is None else int(((g_msk != r_msk) & ~near).sum())
    print(f'{name:20s} {kernel:9s} values {dv:7.3f} / {bv:<5g} weights {dw:7.3f} / {bw:<5g} validity flips {flips} '
          f'mask flips {mflips} near a decision {int(near.sum())} both valid {int(both.sum())}')
    assert both.sum() > 0.5 * rs.covered(name, kernel).sum()
    assert flips == 0, f'validity differs on {flips} pixels away from every decision'
    if g_msk is not None:
        assert mflips == 0, f'mask differs on {mflips} pixels away from every decision'
    assert dv <= bv, f'values: {dv:.3f} x (2e-5 |ref| + 2e-5 std), bound {bv}'
    assert dw <= bw, f'weights: {dw:.3f} x 5e-5 |ref|, bound {bw}'
    assert np.all(g_img[~gv] == 0)


def run(engine, name, kernel):
    sc = rs.scene(name)
    return engine.resample(sc.img, sc.win, sc.wout, wgt=sc.wgt, mask=sc.mask, kernel=kernel)


@pytest.mark.parametrize('name', rs.SCENES)
def test_lanczos3_matches_the_oracle_on_every_geometry(engine, name):
    compare(name, 'LANCZOS3', *run(engine, name, 'LANCZOS3'))


@pytest.mark.parametrize('name', rs.OTHER_KERNEL_SCENES)
def test_bilinear_matches_the_oracle(engine, name):
    compare(name, 'BILINEAR', *run(engine, name, 'BILINEAR'))


@pytest.mark.parametrize('name', [n for n in rs.OTHER_KERNEL_SCENES if n != 'half_shift'])
def test_nearest_matches_the_oracle(engine, name):
    compare(name, 'NEAREST', *run(engine, name, 'NEAREST'))


def test_nearest_on_a_half_pixel_shift_picks_one_of_the_tied_pixels(engine):
    """Every position of ``half_shift`` is a half-integer up to the last bits of the fp64 map, so which neighbour
    NEAREST takes is not defined; each output must be one of the four tied input pixels, with that pixel's value,
    weight and mask together."""
    g_img, g_wgt, g_msk = run(engine, 'half_shift', 'NEAREST')
    ok = np.zeros(g_img.shape, bool)
    for c_img, c_wgt, c_msk in rs.nearest_candidates('half_shift'):
        ok |= (g_img == c_img.astype(np.float32)) & (g_msk == c_msk) & ((g_wgt > 0) == (c_wgt > 0)) & \
            (np.abs(g_wgt - c_wgt) <= rs.WTOL * np.abs(c_wgt))
    print(f'half_shift NEAREST: {int((~ok).sum())} of {ok.size} pixels are none of their four candidates')
    assert ok.all()
    assert (g_wgt > 0).mean() > 0.9


def test_exact_quarter_turn_is_a_copy(engine):
    """``rot90_exact``: integer positions, delta kernels on both axes.  The output is the input transposed and flipped
    along x, bit for bit: values where the input pixel is good (a bad pixel gives 0 and weight 0), the mask everywhere;
    a good pixel keeps its weight (a reciprocal of a reciprocal estimate: 5e-5)."""
    sc = rs.scene('rot90_exact')
    for kernel in ('LANCZOS3', 'BILINEAR', 'NEAREST'):
        g_img, g_wgt, g_msk = run(engine, 'rot90_exact', kernel)
        t_img, t_wgt, t_msk = (a.T[:, ::-1] for a in (sc.img, sc.wgt, sc.mask))
        good = t_wgt > 0
        assert g_img.shape == t_img.shape
        assert np.array_equal(g_wgt > 0, good), kernel
        assert (g_wgt[good] > 0).all() and good.mean() > 0.99
        assert np.array_equal(g_img[good], t_img[good]), kernel
        assert not g_img[~good].any()
        assert np.array_equal(g_msk, t_msk), kernel
        np.testing.assert_allclose(g_wgt[good], t_wgt[good], rtol=rs.WTOL)


@pytest.mark.parametrize('name', ['quarter_shift', 'half_shift'])
def test_exact_fractions_have_no_flip_at_all(engine, name):
    """Fractions 0.25 / 0.5 survive every fp32 step: nothing is near a decision, validity and masks are the oracle's
    on every pixel, for both interpolating kernels."""
    for kernel in ('LANCZOS3', 'BILINEAR'):
        assert not rs.near_decision(name, kernel).any()
        g_img, g_wgt, g_msk = run(engine, name, kernel)
        _, _, r_img, r_wgt, r_msk = rs.reference(name, kernel)
        assert np.array_equal(g_wgt > 0, r_wgt > 0) and np.array_equal(g_msk, r_msk)
        compare(name, kernel, g_img, g_wgt, g_msk)


# ---- the fused kernels against the oracle ---------------------------------------------------------------------------------

FORMS = ({'ZM_COADD_FUSED': '0'}, {'ZM_COADD_FUSED': '1'}, {'ZM_COADD_FUSED': '1', 'ZM_FF_FORM': 'dma'})


@pytest.mark.parametrize('kind', ['WEIGHTED', 'CLIPPED'])
@pytest.mark.parametrize('which', sorted(rs.STACKS))
def test_coadd_of_three_geometries_is_one_result_and_the_oracles(engine, monkeypatch, which, kind):
    """The materialised path (k_resample), the fused coadd as the plan picks it and the LDS-DMA staged form give the
    same bits on frames whose geometry differs in kind (``resample_scenes.STACKS``: k_coadd_fused_own runs on the
    upright stack only), and that result is the oracle's, compared as tests/test_coadd_gpu.py compares a stack."""
    z = pkg()
    frames, wout = rs.stack(which)
    p = z.coadd_params(combine=kind, subtract_back=False, rescale_weights=False)
    res = []
    for form in FORMS:
        with monkeypatch.context() as mp:
            for k, v in form.items():
                mp.setenv(k, v)
            res.append(engine.coadd(frames, wout, p))
            if kind == 'WEIGHTED' and form['ZM_COADD_FUSED'] == '1':
                own = which == 'upright' and form.get('ZM_FF_FORM') != 'dma'
                assert engine.query('fused_form') == (2 if own else 1)
    for r in res[1:]:
        for x, y, what in zip(res[0], r, ('img', 'wgt', 'mask', 'mask coverage')):
            assert np.array_equal(x, y), f'{what}: {int((x != y).sum())} of {x.size} pixels differ'
    g_img, g_wgt, g_msk, _ = res[0]
    r_img, r_wgt, r_msk, vals, wgts = rs.stack_reference(which, kind)
    assert ((wgts > 0).sum(axis=0) == 3).mean() > 0.5          # the three frames overlap on most of the grid
    gv, rv = g_wgt > 0, r_wgt > 0
    both = gv & rv
    print(f'{which} {kind}: validity flips {int((gv != rv).sum())}, mask flips {int((g_msk != r_msk).sum())}, values '
          f'{deviation(g_img[both], r_img[both], 3e-5 * np.abs(r_img[both]) + 3e-5 * 5.0):.3f} x the bound, weights '
          f'{deviation(g_wgt[both], r_wgt[both], 1e-4 * np.abs(r_wgt[both])):.3f}')
    assert (gv != rv).mean() < 2e-4
    assert_close_masked(g_img[both], r_img[both], 3e-5, 3e-5 * 5.0, kind, max_bad_frac=2e-4)
    assert_close_masked(g_wgt[both], r_wgt[both], 1e-4, 0, kind + ' weight', max_bad_frac=2e-4)
    assert (g_msk != r_msk).mean() < 2e-4


# ---- the pair form ----------------------------------------------------------------------------------------------------------

def test_pair_alignment_of_a_half_turn_matches_two_oracle_alignments(engine):
    """One zm_align_pair_dev launch on ``rot180`` (the lattice runs backwards on both axes): the image and an rms map
    against two oracle alignments without weights, each channel under the rules of the module docstring (a pair has
    no weights: a pixel is valid where its value is not 0)."""
    from importlib import import_module
    hipmem = import_module('zuds-pipeline_amd.hipmem')
    z = pkg()
    sc = rs.scene('rot180')
    ny, nx = sc.img.shape
    onx, ony = sc.wout.naxis
    rng = np.random.default_rng(4400)
    rms = rng.uniform(2.0, 6.0, (ny, nx)).astype(np.float32)
    mask = np.ascontiguousarray(sc.mask, dtype=np.int32)
    d_a, d_b, d_m = (hipmem.DeviceBuffer(a.nbytes) for a in (sc.img, rms, mask))
    for d, a in ((d_a, sc.img), (d_b, rms), (d_m, mask)):
        d.upload(a)
    o_a, o_b, o_m = (hipmem.DeviceBuffer(onx * ony * 4) for _ in range(3))
    wa, wb = z._lib.wcs_struct(sc.win), z._lib.wcs_struct(sc.wout)
    engine.synchronize()
    z._lib.check(engine.L.zm_align_pair_dev(engine.ctx, d_a.ptr, d_b.ptr, d_m.ptr, C.byref(wa), C.byref(wb),
                                            z._lib.RESAMPLE['LANCZOS3'], 1.0, 1.0, o_a.ptr, o_b.ptr, o_m.ptr))
    engine.synchronize()
    g_a, g_b = o_a.download(np.float32, (ony, onx)), o_b.download(np.float32, (ony, onx))
    g_m = o_m.download(np.int32, (ony, onx))
    px, py = rs.positions('rot180')
    for src, got, with_mask in ((sc.img, g_a, True), (rms, g_b, False)):
        ref = oresample.resample(src, None, px, py, oresample.LANCZOS3, 1.0, sc.mask)
        compare('rot180', 'LANCZOS3', got, None, g_m if with_mask else None, ref=ref, std=float(np.std(src)),
                valid_is_nonzero=True)
