"""The real / bogus score on the GPU (csrc/braai.hip) against the float64 reference of tests/braai_ref.py: the kernels
on a tiny network and on VGG6, and the score behind the candidate cuts of the device chain, the nightly pool and the
file route.  Weights come from a seed; the last Dense layer is rescaled so that the scores span [0.05, 0.95] (with plain
Glorot weights every score is 0.5 +- 1e-3 and nothing would be seen).  The tolerance is 8 x the largest difference
between a float32 and a float64 torch forward on the CPU over exactly the inputs of the case (braai_ref.case)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import braai_ref as br
from util import pkg, synth

pytestmark = pytest.mark.gpu

NVGG = 129                     # ZM_RB_CHUNK + 1


def rbmod():
    return importlib.import_module('zuds-pipeline_amd.realbogus')


_MODELS = {}


def model_of(c):
    if c['name'] not in _MODELS:
        _MODELS[c['name']] = rbmod().RBModel(c['json'], c['weights'], name=c['name'])
    return _MODELS[c['name']]


def dev_scores(m, engine, blocks, norms, order=('new', 'ref', 'sub')):
    import torch
    b = torch.from_numpy(np.ascontiguousarray(blocks)).to('cuda:0')
    n = torch.from_numpy(np.ascontiguousarray(norms)).to('cuda:0')
    torch.cuda.synchronize()
    rb = m.score_dev(b, n, order=order, engine=engine)
    engine.synchronize()
    return rb.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def report(what, got, c):
    err = np.abs(got.astype(np.float64) - c['ref'][:len(got)])
    print(f'{what}: n = {len(got)}, tolerance {c["tol"]:.3e}, worst error {err.max():.3e} = {err.max() / c["tol"]:.3f} of it')
    return err


def test_chunk_constant(engine):
    z = pkg()
    assert z._lib.RB_CHUNK + 1 == NVGG
    text = open(z._lib.HERE.parent / 'include' / 'zudsmi.h').read()
    assert f'#define ZM_RB_CHUNK {z._lib.RB_CHUNK}\n' in text


@pytest.mark.parametrize('name', ['tiny', 'tiny_wide'])
def test_tiny_network(engine, name):
    c = br.case(name, 67)
    assert c['ref'].min() <= 0.05 and c['ref'].max() >= 0.95
    m = model_of(c)
    full = dev_scores(m, engine, c['blocks'], c['norms'])
    err = report(name, full, c)
    assert (err <= c['tol']).all()
    for n in (1, 2):
        part = dev_scores(m, engine, c['blocks'][:n], c['norms'][:n])
        assert np.array_equal(bits(part), bits(full[:n])), n
    last = dev_scores(m, engine, c['blocks'][65:], c['norms'][65:])
    assert np.array_equal(bits(last), bits(full[65:]))


@pytest.fixture(scope='module')
def vgg(engine):
    c = br.case('vgg6', NVGG)
    m = model_of(c)
    return c, m, dev_scores(m, engine, c['blocks'], c['norms'])


def test_vgg6_against_the_reference(engine, vgg):
    c, m, full = vgg
    assert c['ref'].min() <= 0.05 and c['ref'].max() >= 0.95
    assert full.dtype == np.float32 and full.shape == (NVGG,)
    err = report('vgg6', full, c)
    assert (err <= c['tol']).all()


def test_vgg6_bits_do_not_depend_on_the_batch(engine, vgg):
    c, m, full = vgg
    for n in (1, 3, 65):
        part = dev_scores(m, engine, c['blocks'][:n], c['norms'][:n])
        assert np.array_equal(bits(part), bits(full[:n])), n
    # other positions: the last 65 (first there, last of the second chunk here), and one from the middle alone
    tail = dev_scores(m, engine, c['blocks'][NVGG - 65:], c['norms'][NVGG - 65:])
    assert np.array_equal(bits(tail), bits(full[NVGG - 65:]))
    one = dev_scores(m, engine, c['blocks'][77:78], c['norms'][77:78])
    assert bits(one)[0] == bits(full)[77]
    # two runs: the same bytes
    assert np.array_equal(bits(dev_scores(m, engine, c['blocks'], c['norms'])), bits(full))


def test_vgg6_host_entry_point_gives_the_same_bytes(engine, vgg):
    c, m, full = vgg
    host = m.score_blocks(c['blocks'], c['norms'], order=('new', 'ref', 'sub'), engine=engine)
    assert np.array_equal(bits(host), bits(full))
    # and the triplet route (normalised on the host in float64, then rounded to float32: not the same bits, the same bound)
    t = m.score_triplets(c['x'][:5], engine=engine)
    assert (np.abs(t.astype(np.float64) - c['ref'][:5]) <= c['tol']).all()


def test_vgg6_channel_order(engine, vgg):
    c, m, full = vgg
    n = 6
    swapped = np.ascontiguousarray(c['blocks'][:n, [2, 1, 0]])
    snorms = np.ascontiguousarray(c['norms'][:n, [2, 1, 0]])
    wrong = dev_scores(m, engine, swapped, snorms)
    assert (np.abs(wrong.astype(np.float64) - full[:n]) > 100 * c['tol']).any()
    undone = dev_scores(m, engine, swapped, snorms, order=('sub', 'ref', 'new'))
    assert np.array_equal(bits(undone), bits(full[:n]))
    # a fourth plane that no channel reads changes nothing
    four = np.concatenate([c['blocks'][:n], np.full((n, 1, 63, 63), 7.0, np.float32)], axis=1)
    fnorms = np.concatenate([c['norms'][:n], np.zeros((n, 1))], axis=1)
    with pytest.raises(ValueError):
        dev_scores(m, engine, four, fnorms)                    # three names for four planes
    L, poc, rb = engine.L, np.array([0, 1, 2], np.int32), np.zeros(n, np.float32)
    z = pkg()
    z._lib.check(L.zm_rb_score(engine.ctx, m.handle(engine), n, four.ctypes.data, fnorms.ctypes.data, 4, poc.ctypes.data,
                               rb.ctypes.data))
    assert np.array_equal(bits(rb), bits(full[:n]))


def test_vgg6_zero_and_infinite_norms_score_nan(engine, vgg):
    c, m, full = vgg
    n = 6
    blocks, norms = c['blocks'][:n].copy(), c['norms'][:n].copy()
    blocks[1, 2] = 0.0
    norms[1, 2] = 0.0                                  # an empty plane: cutout / 0 in the reference
    norms[4, 0] = np.inf
    got = dev_scores(m, engine, blocks, norms)
    assert np.isnan(got[[1, 4]]).all()
    keep = [0, 2, 3, 5]
    assert np.array_equal(bits(got[keep]), bits(full[keep]))
    norms[3, 1] = np.nan
    assert np.isnan(dev_scores(m, engine, blocks, norms)[[1, 3, 4]]).all()


def test_refused_architectures_and_an_empty_batch(engine, vgg):
    import torch
    c, m, full = vgg
    z = pkg()
    rb = rbmod()
    L = engine.L
    layers, blob = rb.pack(m.arch, m.weights)
    out = C.c_void_p()

    def create(edit, in_size=63, in_channels=3):
        arr = (z._lib.zm_rb_layer * len(layers))()
        for k in range(len(layers)):
            C.memmove(C.byref(arr[k]), C.byref(layers[k]), C.sizeof(z._lib.zm_rb_layer))
        edit(arr)
        return L.zm_rb_model_create(engine.ctx, in_size, in_channels, len(arr), arr, blob.ctypes.data, blob.size, C.byref(out))

    def setf(k, **kw):
        def edit(arr):
            for name, v in kw.items():
                setattr(arr[k], name, v)
        return edit
    for edit, word in ((setf(0, ksize=5), b'3 x 3'), (setf(1, stride=2), b'stride'), (setf(0, padding=z._lib.RB_SAME), b'valid'),
                       (setf(1, cout=65), b'output channels'), (setf(3, type=9), b'unsupported layer'),
                       (setf(2, stride=1), b'stride'), (setf(8, w_off=blob.size - 3), b'outside the blob'),
                       (setf(7, cin=1151), b'inputs'), (setf(8, activation=7), b'Dense takes')):
        assert create(edit) != 0
        assert word in L.zm_last_error(), (word, L.zm_last_error())
    assert create(lambda arr: None, in_size=71) != 0 and b'inputs' in L.zm_last_error()       # the shape chain no longer fits
    assert create(lambda arr: None) == 0
    L.zm_rb_model_destroy(out)
    # n = 0 does nothing: the output is not touched
    sentinel = torch.full((4,), 3.5, dtype=torch.float32, device='cuda:0')
    poc = np.array([0, 1, 2], np.int32)
    torch.cuda.synchronize()
    assert L.zm_rb_score_dev(engine.ctx, m.handle(engine), 0, None, None, 3, poc.ctypes.data, sentinel.data_ptr()) == 0
    engine.synchronize()
    assert (sentinel.cpu().numpy() == 3.5).all()
    assert m.score_blocks(np.zeros((0, 3, 63, 63), np.float32), np.zeros((0, 3)), engine=engine).shape == (0,)
    assert L.zm_rb_score_dev(engine.ctx, m.handle(engine), -1, None, None, 3, poc.ctypes.data, sentinel.data_ptr()) != 0
    bad = np.array([0, 1, 3], np.int32)
    assert L.zm_rb_score_dev(engine.ctx, m.handle(engine), 0, None, None, 3, bad.ctypes.data, sentinel.data_ptr()) != 0
    assert b'plane_of_channel' in L.zm_last_error()


# ---- behind the candidate cuts ---------------------------------------------------------------------------------------
ORDER = ('sub', 'new', 'ref')              # planes of DeviceSubtraction.stamps
POC = (1, 2, 0)                            # ... that hold the channels new, ref, sub


@pytest.fixture(scope='module')
def pool_case(engine):
    """The pool-detect scene (two jobs), the tables and stamps of its jobs WITHOUT a model, and a VGG6 whose last layer is
    rescaled over exactly those stamps: reference scores, tolerance and a cut in the widest gap between the scores."""
    import torch
    import test_pool_detect_gpu as pd
    z, s = pkg(), synth()
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    jobs, _ = pd.make_jobs(torch, z, s, 2, detect=True, stamps=True)
    pool = nm.SubtractionPool(1)
    plain = pool.map(jobs)
    pool.close()
    xs = []
    for r in plain:
        assert 'error' not in r and 'stamps' in r and len(r['stamps']['blocks']) >= pd.NTRANS
        xs.append(br.triplets_of(r['stamps']['blocks'], r['stamps']['norms'], POC))
    text, weights, layers, ref, tol = br.model_for(np.concatenate(xs))
    cut = br.choose_cut(ref, tol, groups=np.concatenate([np.full(len(x), j) for j, x in enumerate(xs)]))
    m = rbmod().RBModel(text, weights, name='braai_d6_m9')
    refs, k = [], 0
    for x in xs:
        refs.append(ref[k:k + len(x)])
        k += len(x)
    assert all((r < cut).any() and (r >= cut).any() for r in refs), 'the cut must remove and keep a row of every job'
    return dict(pd=pd, plain=plain, model=m, refs=refs, tol=tol, cut=cut)


def check_table(cat, plain_cat, ref, tol, cut):
    """``cat`` against the reference's chain on the same stamps: filter_table with the reference's scores."""
    alive = plain_cat['GOODCUT'] == 1
    want_good = plain_cat['GOODCUT'].copy()
    want_good[np.flatnonzero(alive)[ref < cut]] = 0
    assert np.array_equal(cat['GOODCUT'], want_good)
    assert (cat['rb'][~alive] == -99).all()
    err = np.abs(cat['rb'][alive] - ref)
    print(f'rb behind the cuts: {alive.sum()} rows, tolerance {tol:.3e}, worst error {err.max():.3e}')
    assert (err <= tol).all()
    for name in plain_cat.dtype.names:
        if name not in ('GOODCUT', 'rb'):
            assert np.array_equal(cat[name], plain_cat[name], equal_nan=True), name


def test_candidates_with_a_model(engine, pool_case, monkeypatch):
    import torch
    z, s = pkg(), synth()
    pc = pool_case
    devmod = importlib.import_module('zuds-pipeline_amd.device')
    jobs, _ = pc['pd'].make_jobs(torch, z, s, 2)
    sci, ref = jobs[0].sci, jobs[0].ref
    ch = devmod.DeviceSubtraction(sci['wcs'], ref['wcs'], engine=engine)
    ch.run(sci['img'], sci['rms'], sci['mask'], sci['wgt'], ref['img'], ref['rms'], ref['mask'], seeing=2.4,
           nreg_side=2, hotpants_kws={'ko': 1, 'bgo': 0})
    none, nfound = ch.candidates(2.4, wcs=sci['wcs'])
    assert none.tobytes() == pc['plain'][0]['cat'].tobytes()
    tab, nfound2 = ch.candidates(2.4, wcs=sci['wcs'], rb_model=pc['model'], sci=sci['img'], ref=ref['img'], rb_cut=pc['cut'])
    assert nfound2 == nfound and tab.dtype == none.dtype
    check_table(tab, none, pc['refs'][0], pc['tol'], pc['cut'])
    # fid names the cut when rb_cut does not; neither is an error, as are missing planes
    by_fid, _ = ch.candidates(2.4, wcs=sci['wcs'], rb_model=pc['model'], sci=sci['img'], ref=ref['img'], fid=3)
    assert np.array_equal(by_fid['rb'], tab['rb'])
    alive = none['GOODCUT'] == 1
    assert np.array_equal(by_fid['GOODCUT'][alive], (~(by_fid['rb'][alive] < 0.6)).astype(np.uint8))
    with pytest.raises(ValueError):
        ch.candidates(2.4, rb_model=pc['model'], sci=sci['img'], ref=ref['img'])
    with pytest.raises(ValueError):
        ch.candidates(2.4, rb_model=pc['model'], rb_cut=0.5)
    # without a model the scoring code is never entered, whatever else is passed, and the table is the same bytes
    def boom(*a, **k):
        raise AssertionError('no model: nothing may be scored')
    monkeypatch.setattr(rbmod().RBModel, 'score_dev', boom)
    monkeypatch.setattr(ch, 'stamps', boom)
    again, _ = ch.candidates(2.4, wcs=sci['wcs'], rb_model=None, sci=sci['img'], ref=ref['img'], fid=3, rb_cut=0.5)
    assert again.tobytes() == none.tobytes() and (again['rb'] == -99).all()


def test_pool_jobs_with_a_model_in_both_lane_forms(engine, pool_case):
    import torch
    z, s = pkg(), synth()
    pc = pool_case
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    survivors = [int((r >= pc['cut']).sum()) for r in pc['refs']]
    jobs, _ = pc['pd'].make_jobs(torch, z, s, 2, detect=True, stamps=True, rb_model=pc['model'], rb_cut=pc['cut'])
    # max_detections counts the rows behind the ML cut: job 0 is allowed exactly its survivors - fewer than reach the network
    jobs[0].max_detections = survivors[0]
    assert survivors[0] < len(pc['refs'][0])
    outs = []
    for pool in (nm.SubtractionPool(1), nm.SubtractionPool(1, batch=2)):
        outs.append(pool.map(jobs))
        pool.close()
    for form in outs:
        for r, p, ref, nsurv in zip(form, pc['plain'], pc['refs'], survivors):
            assert 'error' not in r and 'detect_error' not in r and not r.get('too_many')
            check_table(r['cat'], p['cat'], ref, pc['tol'], pc['cut'])
            for k in ('diff', 'noise', 'mask'):
                assert torch.equal(r[k], p[k]), k
            # the stamps delivered: those of the surviving rows, the bytes the job without a model delivers for them
            keep = ref >= pc['cut']
            assert len(r['stamps']['blocks']) == nsurv == int(keep.sum())
            for k in ('blocks', 'norms', 'x0', 'y0', 'ra', 'dec'):
                assert np.array_equal(r['stamps'][k], p['stamps'][k][keep]), k
    for a, b in zip(*outs):
        assert a['cat'].tobytes() == b['cat'].tobytes()
    # one row fewer is too many, and the products are still delivered
    jobs[0].max_detections = survivors[0] - 1
    pool = nm.SubtractionPool(1)
    r = pool.map(jobs[:1])[0]
    pool.close()
    assert r.get('too_many') is True and 'stamps' not in r and r['cat'].tobytes() == outs[0][0]['cat'].tobytes()
    with pytest.raises(ValueError):
        nm.SubtractionJob(jobs[0].sci, jobs[0].ref, detect=True, rb_model=pc['model'])           # no cut, no filter id
    with pytest.raises(ValueError):
        nm.SubtractionJob(jobs[0].sci, jobs[0].ref, rb_model=pc['model'], fid=1)                 # needs detect


from test_catalog_gpu import scene  # noqa: E402,F401  (the files of a single-epoch subtraction)


@pytest.mark.parametrize('route', ['device', 'host'])
def test_filter_sexcat_with_a_model_on_files(engine, scene, monkeypatch, route):
    z, sub = scene['z'], scene['sub']
    fo = importlib.import_module('zuds-pipeline_amd.filterobjects')
    th = importlib.import_module('zuds-pipeline_amd.thumbnails')
    if route == 'host':
        monkeypatch.setenv('ZM_OBJECT_API', 'host')
    else:
        monkeypatch.delenv('ZM_OBJECT_API', raising=False)
    cat = z.PipelineFITSCatalog.from_image(sub)
    table = cat.data.copy()
    see = sub.header['SEEING']
    pix = z.pixel_cuts(sub.data, sub.rms_image.data, sub.mask_image.boolean.data, table['X_IMAGE'], table['Y_IMAGE'], engine=engine)
    plain = fo.filter_table(table, see, pix)
    rows = table[plain['GOODCUT'] == 1]
    assert len(rows) >= 20

    class At(object):
        def __init__(self, ra, dec):
            self.ra, self.dec = float(ra), float(dec)
    (blocks, norms, _, _, images, _), = th._subtraction_blocks([At(r['X_WORLD'], r['Y_WORLD']) for r in rows], sub, 63)
    assert [t for t, _ in images] == list(ORDER)
    text, weights, layers, ref, tol = br.model_for(br.triplets_of(np.asarray(blocks), np.asarray(norms), POC))
    cut = br.choose_cut(ref, tol)
    m = rbmod().RBModel(text, weights, name='braai_d6_m9')
    fid = sub.fid
    assert fid in (1, 2, 3)                                     # (the FID card of the frames)
    monkeypatch.setattr(sub, 'fid', None, raising=False)
    with pytest.raises(ValueError):
        z.filter_sexcat(cat, quiet=True, rb_model=m)            # no filter id and no cut is given: not guessed
    monkeypatch.setattr(sub, 'fid', fid, raising=False)
    assert 'GOODCUT' not in cat.data.dtype.names
    assert z.filter_sexcat(cat, quiet=True, rb_model=m, rb_cut=cut) is cat
    check_table(cat.data, plain, ref, tol, cut)
    dets = z.Detection.from_catalog(cat, filter=True)
    assert len(dets) == int((ref >= cut).sum()) and all(d.rb_version == 'braai_d6_m9' and d.rb >= cut for d in dets)
