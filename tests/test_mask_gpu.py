"""zm_extract_measure_masked (csrc/extract_mask.hip) against the numpy restatement (tests/mask_ref.py) on the GPU.

Every scene of tests/mask_scenes.py, both mask types.  A census of the scene on the restatement alone comes first
(mask_ref.census): no mirror within 1e-9 of a rounding tie in any pass, no pixel within 1e-9 of an ellipse's edge, no step
within 1e-6 of the stop threshold, no share within 1e-9 of 0.10.  Then:

integers   npix_auto, nskip_auto, FLAGS_AUTO, FLAGS_WIN, niter_win and every field of zm_object_mask but the two sums:
           bit for bit.
floats     the bounds tests/test_measure_gpu.py derives (its docstring: (i) 10 x forward / reversed summation, (ii) term
           rounding with the sqrt and exp figures, (iii) the overlap's pin), evaluated on the masked restatement by that
           file's own ``term_bounds``.  The masked aperture: (i) plus the overlap's pin, rtol 1e-10 and atol 1e-9 per
           fraction, summed over |v'|; FLUXERR_APER = sqrt(var) inherits (d var) / (2 sqrt(var)) plus one spacing for the
           root.  No tolerance of this file's own.
unchanged  errx2, erry2, errxy (walk 3) equal zm_extract_measure's on the same rows bit for bit.
The measured worst differences are printed per scene before anything is asserted.
"""
import ctypes as C
import importlib
import threading

import numpy as np
import pytest

import mask_ref as kr
import mask_scenes as ms
import test_measure_gpu as tmg
from util import pkg

pytestmark = pytest.mark.gpu

TYPES = [kr.BLANK, kr.CORRECT]


def lib():
    return pkg()._lib


def ex():
    return importlib.import_module('zuds-pipeline_amd.extract')


def as_rows(rows):
    """A ROW array (or a ctypes zm_object array's view) as a contiguous array of zm_object's own dtype."""
    dt = np.dtype(lib().zm_object)
    assert dt.itemsize == ms.ROW.itemsize
    return np.ascontiguousarray(rows).view(dt).copy()


def call(engine, sc, rows, typ, radius=None, dev=None, n=None, mask_type=None):
    """(ext rows, mask rows) of zm_extract_measure_masked[_dev]; typ None: (ext rows, None) of zm_extract_measure."""
    L, _lib = engine.L, lib()
    img, sigma, seg = (np.ascontiguousarray(sc[k]) for k in ('img', 'sigma', 'seg'))
    bad = None if sc['bad'] is None else np.ascontiguousarray(sc['bad'], np.uint8)
    ny, nx = img.shape
    n = len(rows) if n is None else n
    mp = ex().measure_params(sc['kw'].get('kron_fact', 2.5), sc['kw'].get('kron_min', 3.5), True)
    ext = np.zeros(max(len(rows), 1), np.dtype(_lib.zm_object_ext))
    msk = np.zeros(max(len(rows), 1), np.dtype(_lib.zm_object_mask))
    planes = dev if dev is not None else (_lib.ptr(img), _lib.ptr(sigma), _lib.ptr(bad), _lib.ptr(seg))
    args = (engine._ctx, *planes, nx, ny, None, C.byref(mp), n, _lib.ptr(rows), _lib.ptr(ext))
    if typ is None:
        rc = (L.zm_extract_measure_dev if dev is not None else L.zm_extract_measure)(*args)
        return rc, ext[:n], None
    mk = ex().mask_params(typ, sc['kw'].get('aper_radius', 3.0) if radius is None else radius)
    if mask_type is not None:
        mk.type = mask_type
    rc = (L.zm_extract_measure_masked_dev if dev is not None else L.zm_extract_measure_masked)(
        *args, C.byref(mk), _lib.ptr(msk))
    return rc, ext[:n], msk[:n]


def restate(sc, rows, typ, plain_ext):
    objs = ms.objects(rows, ext=plain_ext)
    return [kr.measure(sc['img'], sc['sigma'], sc['bad'], sc['seg'], objs, typ, reverse=rev, cterm=tmg.CTERM, **sc['kw'])
            for rev in (False, True)]


def gpu_scene(engine, name):
    """The scene with its rows as zm_object; ``deblended``: rows and map of zm_extract_deblend itself."""
    if name != 'deblended':
        sc = ms.scene(name)
        return sc, as_rows(sc['rows'])
    img, sigma = ms.deblended_planes()
    got = engine.extract(img, sigma, deblend=True, full=True)
    n = len(got['table'])
    raw = engine.__dict__['_extract_rows'][threading.get_ident()]
    rows = np.frombuffer(raw, dtype=np.dtype(lib().zm_object), count=n).copy()
    assert n == 12 and (got['table']['FLAGS'] & 2).sum() >= 2, 'the scene is meant to hold a deblended pair'
    return dict(img=img, sigma=sigma, bad=None, seg=np.ascontiguousarray(got['segm'], np.int32), kw={}), rows


def compare(engine, name, typ):
    sc, rows = gpu_scene(engine, name)
    rc, plain, _ = call(engine, sc, rows, None)
    assert rc == 0
    fwd, rev = restate(sc, rows, typ, plain)
    kr.census(fwd)
    rc, ext, msk = call(engine, sc, rows, typ)
    assert rc == 0, engine.L.zm_last_error()
    dc = [r['dcentre'] for r in fwd if 'dcentre' in r]
    assert all(d <= 1e-3 for d in dc), 'a windowed position that is not held to anything'
    line, fails = [], []

    def held(field, got, allow_terms):
        a = np.array([r[field] for r in fwd], np.float64)
        o = np.array([r[field] for r in rev], np.float64)
        assert np.isfinite(a).all() and np.isfinite(got).all(), field
        order = 10.0 * float(np.abs(a - o).max())
        allow = order + np.asarray(allow_terms, np.float64)
        diff = np.abs(got - a)
        line.append(f'{field} {float(diff.max()):.3g} ({order:.3g} + {float((allow - order).max()):.3g})')
        if (diff > allow).any():
            fails.append((field, float(diff.max()), float(allow[np.argmax(diff - allow)])))

    for f in kr.FLOAT_FIELDS:
        held(f, ext[f], [tmg.term_bounds(r)[f] for r in fwd])
    held('flux_aper', msk['flux_aper'], [r['dflux'] for r in fwd])
    dvar = 10.0 * max(abs(a['var_aper'] - b['var_aper']) for a, b in zip(fwd, rev))
    held('fluxerr_aper', msk['fluxerr_aper'],
         [(dvar + r['dvar']) / (2.0 * r['fluxerr_aper']) + np.spacing(r['fluxerr_aper']) if r['fluxerr_aper'] > 0 else
          np.sqrt(dvar + r['dvar']) for r in fwd])
    print(f'mask {name} {typ}: {len(fwd)} objects; largest bound on a windowed position {max(dc, default=0.0):.3g} px; '
          f'field measured (order bound + term bound): ' + ', '.join(line))
    for f in kr.INT_FIELDS:
        assert [int(v) for v in ext[f]] == [r[f] for r in fwd], f
    for f in kr.MASK_INT_FIELDS:
        assert [int(v) for v in msk[f]] == [r[f] for r in fwd], f
    assert [int(v) for v in ext['number']] == [int(v) for v in msk['number']] == [r['number'] for r in fwd]
    assert [int(v) for v in ext['nskip_auto']] == [int(v) for v in msk['nlost_auto']]
    assert not fails, fails
    for f in ('errx2', 'erry2', 'errxy'):
        assert ext[f].tobytes() == plain[f].tobytes(), f
    assert np.isnan(ext['xwin_world']).all()
    return sc, rows, plain, ext, msk, fwd


@pytest.mark.parametrize('typ', TYPES)
@pytest.mark.parametrize('name', ms.NAMES)
def test_every_scene_against_the_restatement(engine, name, typ):
    sc, rows, plain, ext, msk, fwd = compare(engine, name, typ)
    # an object with no unusable pixel in any footprint has the unmasked call's row, bit for bit
    quiet = [k for k, r in enumerate(fwd) if r['touched_auto'] + r['touched_win'] + r['touched_aper'] == 0]
    for k in quiet:
        assert ext[k].tobytes() == plain[k].tobytes(), (name, k + 1)
    if name in ms.CLEAN_SCENES:
        assert len(quiet) == len(fwd) and ext.tobytes() == plain.tobytes()
        assert not msk['crowded'].any() and not msk['nrepl_auto'].any() and not msk['nlost_win'].any()
    if name == 'deblended':
        assert len(quiet) >= 6 and (msk['nrepl_auto' if typ == kr.CORRECT else 'nlost_auto'] > 0).sum() >= 4
    if name != 'alone':
        assert any(ext[k].tobytes() != plain[k].tobytes() for k in range(len(fwd)))


def test_blank_and_correct_differ_only_where_something_is_replaced(engine):
    sc, rows = gpu_scene(engine, 'pair')
    _, eb, mb = call(engine, sc, rows, kr.BLANK)
    _, ec, mc = call(engine, sc, rows, kr.CORRECT)
    assert not mb['nrepl_auto'].any() and not mb['nrepl_aper'].any() and not mb['nrepl_win'].any()
    assert (mc['nrepl_auto'] > 0).all() and (ec['flux_auto'] > eb['flux_auto']).all()
    assert (mc['nrepl_auto'] + mc['nlost_auto'] == mb['nlost_auto']).all()


def test_two_runs_and_the_device_form_give_the_same_bits(engine):
    hipmem = importlib.import_module('zuds-pipeline_amd.hipmem')
    sc, rows = gpu_scene(engine, 'wide_window_small_kron')
    bufs = []
    for a in (sc['img'], sc['sigma'], sc['bad'], sc['seg']):
        b = hipmem.DeviceBuffer(a.nbytes)
        b.upload(np.ascontiguousarray(a))
        bufs.append(b)
    for typ in TYPES:
        rc, e1, m1 = call(engine, sc, rows, typ)
        rc2, e2, m2 = call(engine, sc, rows, typ)
        rc3, e3, m3 = call(engine, sc, rows, typ, dev=tuple(b.ptr for b in bufs))
        assert rc == rc2 == rc3 == 0
        assert e1.tobytes() == e2.tobytes() == e3.tobytes() and m1.tobytes() == m2.tobytes() == m3.tobytes()
    # the unmasked call's results are what they were after the masked one ran on the same context
    rc, p1, _ = call(engine, sc, rows, None)
    rc2, p2, _ = call(engine, sc, rows, None, dev=tuple(b.ptr for b in bufs))
    assert rc == rc2 == 0 and p1.tobytes() == p2.tobytes()


def test_no_rows_succeed_and_bad_types_and_radii_are_errors(engine):
    sc, rows = gpu_scene(engine, 'alone')
    L = engine.L
    rc, ext, msk = call(engine, sc, rows, kr.CORRECT, n=0)
    assert rc == 0 and len(ext) == 0
    for kw, text in ((dict(mask_type=0), b'mask type'), (dict(mask_type=3), b'mask type'), (dict(radius=0.0), b'radius'),
                     (dict(radius=-1.0), b'radius'), (dict(radius=512.0), b'radius'), (dict(radius=float('nan')), b'radius')):
        for n in (None, 0):
            rc, _, _ = call(engine, sc, rows, kr.CORRECT, n=n, **kw)
            err = L.zm_last_error()
            assert rc != 0 and b'zm_extract_measure_masked' in err and text in err, (kw, err)
    p = lib().zm_mask_params()
    L.zm_mask_params_default(C.byref(p))
    assert (p.type, p.aper_radius) == (lib().MASK_CORRECT, 3.0)
