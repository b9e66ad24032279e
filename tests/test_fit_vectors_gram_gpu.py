"""The kernel fit's basis vectors and Gram matrices give the bits they gave before their loops were rewritten.

``tests/golden/fit_vectors_parent.json`` holds, per scene, the SHA-256 of the ``diff`` and ``noise`` planes and the
integer and float fields of the fit summary, recorded by ``tests/golden/make_fit_vectors_golden.py`` from the build of
the commit before the rewrite (twice, in two processes: every scene came out the same both times).  The rewrite keeps
every sum in its order - per output the taps m = 0 .. 2 hwk, per Gram entry the pixels in K order and the eight
slices - so the comparison is for equality.  On a mismatch the planes are set against the oracle's (the fixture holds
digests, not pixels): count and size of the differences tell a last-bit change from a wrong vector.

Scenes: substamp widths of one full strip of eight rows plus a ragged one (15), two strips plus one row (17), 25, and
the benchmark's 49 (six strips plus one row, a 69-pixel patch), each at kernel orders 0, 2, 4 and once with six
background terms; a 2 x 2-region scene whose rejections run the later rounds' list-driven launches of 16 parts; half
width 16 / substamp 38 for the column-chunked form; substamps whose patches touch the frame's edges; and two jobs at
the benchmark's widths through ``SubtractionPool(1, batch=2)`` (the batched kernels) against their lone runs.
"""
import hashlib
import importlib
import json
import pathlib

import numpy as np
import pytest

import hp_scenes as hs
from test_subtract_gpu import COMMON, scene
from util import pkg, synth

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden' / 'fit_vectors_parent.json'


def edge_scene():
    """(3, 7): hw = 10.  Two stars, the brightest of the frame, whose peaks sit at x = hw, at y = hw and at
    (nx - 1 - hw, ny - 1 - hw): the first and the last centre the stamp search may pick, patches from column 0,
    from row 0 and up to the last column and row (oracle/hotpants.py find_substamps, checked on the CPU)."""
    sci, srms, ref, rrms, bpm = scene(nx=256, ny=256, seed=61, nstars=60, nbad=0)
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float64)
    sci, ref = sci.astype(np.float64), ref.astype(np.float64)
    for x, y in ((10, 70), (150, 10), (245, 245)):
        r2 = (xx - x) ** 2 + (yy - y) ** 2
        ref += 6e4 * np.exp(-r2 / (2 * 1.0 ** 2))
        sci += 1.3 * 6e4 / (1 + 0.81) * np.exp(-r2 / (2 * (1.0 + 0.81)))
    return sci.astype(np.float32), srms, ref.astype(np.float32), rrms, bpm


def _plain(r, rss, ko, bgo, seed):
    return (lambda: scene(nx=256, ny=256, seed=seed, nstars=70),
            dict(r=float(r), rss=float(rss), nsx=3, nsy=3, ko=ko, bgo=bgo, **COMMON))


SCENES = {}
for _r, _rss in ((3, 7), (4, 8), (5, 12), (10, 24)):
    for _ko, _bgo in ((0, 0), (2, 0), (4, 0), (2, 2)):
        SCENES[f'r{_r}-rss{_rss}-ko{_ko}-bgo{_bgo}'] = _plain(_r, _rss, _ko, _bgo, 100 + _r)
SCENES['rejected-2x2'] = (lambda: hs.contaminated(nx=256, ny=256, seed=5, nstars=140, ntr=6),
                          dict(hs.BASE, r=4.0, rss=8.0, nsx=3, nsy=3, nrx=2, nry=2, nss=3))
SCENES['big-16-38'] = (lambda: scene(nx=384, ny=384, seed=54, nstars=160, ksig=2.2),
                       dict(r=16.3, rss=38.5, nsx=2, nsy=2, ko=1, bgo=0, **COMMON))
SCENES['edge'] = (edge_scene, dict(r=3.0, rss=7.0, nsx=3, nsy=3, ko=1, bgo=0, **COMMON))
POOL = 'pool-batch2'


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def info_fields(info):
    """The integer fields as they are, the float fields as hex strings (exact, and a NaN compares equal)."""
    out = {}
    for k, v in sorted(info.items()):
        if isinstance(v, (bool, int, np.integer)):
            out[k] = int(v)
        elif isinstance(v, (float, np.floating)):
            out[k] = float(v).hex()
    return out


def record(d, n, info):
    assert d.dtype == np.float32 and n.dtype == np.float32
    return dict(diff=digest(d), noise=digest(n), info=info_fields(info))


def run_scene(engine, name):
    make, kw = SCENES[name]
    data = make()
    return data, kw, engine.subtract(*data, **kw)


def pool_jobs():
    import torch
    from test_nightly_gpu import make_jobs
    # (10 x 10 stamps: the 69-pixel boxes around the bad pixels of these frames leave a smaller frame a stamp or two;
    # the limits of the command line - 5e3 - would take the brighter stars as well)
    jobs = make_jobs(torch, pkg(), synth(), 2, 1024, 1024, 1, {'ko': 1, 'bgo': 0, 'tu': 1e6, 'iu': 1e6}, seed=970)
    for j in jobs:
        j.sci['seeing'] = 4.0                              # -r 2.5 SEEING -rss 6 SEEING: (10, 24)
    return jobs


def run_pool(batch):
    nm = importlib.import_module('zuds-pipeline_amd.nightly')
    pool = nm.SubtractionPool(1, batch=batch) if batch else nm.SubtractionPool(1)
    try:
        res = pool.map(pool_jobs())
    finally:
        pool.close()
    return [record(r['diff'].cpu().numpy(), r['noise'].cpu().numpy(), r['info']) for r in res]


@pytest.fixture(scope='module')
def golden():
    return json.loads(GOLDEN.read_text())


def explain(data, kw, d, n):
    from oracle import hotpants as ohp
    sci, srms, ref, rrms, bpm = data
    rd, rn, _ = ohp.subtract(sci, ref, srms, rrms, bpm, **kw)
    for what, a, b in (('diff', d, rd), ('noise', n, rn)):
        e = np.abs(a.astype(np.float64) - b)
        print(f'{what}: {(a != b.astype(np.float32)).sum()} pixels differ from the oracle, largest {e.max():.3e}')


@pytest.mark.parametrize('name', sorted(SCENES))
def test_scene_gives_the_recorded_bits(engine, golden, name):
    data, kw, (d, n, info) = run_scene(engine, name)
    got, want = record(d, n, info), golden[name]
    if got != want:
        print('info', {k: (got['info'].get(k), v) for k, v in want['info'].items() if got['info'].get(k) != v})
        explain(data, kw, d, n)
    assert got == want
    if name == 'rejected-2x2':
        assert info['niter'] >= 2 and info['nstamps_used'] < info['nstamps_total']


def test_batched_kernels_give_the_bits_of_the_single_call(engine, golden):
    """Two jobs as one batch of launches (k_hp_vectors_b, k_hp_gram_b): the digests recorded from one job at a time."""
    got = run_pool(2)
    assert got == golden[POOL]
