"""The back substitution of the kernel fit gives the bits it gave before its column sweep left the chain's path.

``tests/golden/back_cols_parent.json`` holds, per scene, the SHA-256 of the ``diff`` and ``noise`` planes and the integer
and float fields of the fit summary, recorded by ``tests/golden/make_back_cols_golden.py`` from the build of the commit
before the rewrite (twice, in two processes: every scene came out the same both times).  The rewrite keeps every
product and every order - per column the blocks in descending order, within a block ``acc`` from 0.0 over m ascending,
``yc -= acc``, the chain's steps j = 31 .. 1, the final ``yc / d`` - so the comparison is for equality.

Scenes: 256 x 256 frames at half widths (3, 7), chosen for block counts and ragged last blocks that
``fit_vectors_parent.json`` does not have (unknowns = 48 nkp + 1 + nbg):

    ko 0 bgo 1   52 unknowns   2 blocks, the last of 20 rows
    ko 1 bgo 2  151            5                  23
    ko 2 bgo 3  299           10                  11
    ko 3 bgo 0  482           16                   2
    ko 3 bgo 2  487           16                   7

a 2 x 2-region scene whose rejections leave later rounds with only some regions live; ko = 5 (1010 unknowns), which
stays with ``k_chol_back``; two jobs through ``SubtractionPool(1, batch=2)`` (``k_chol_back_cols_b``) against their lone
runs; and the 482-unknown scene and the benchmark's 722 unknowns three times in one process: waves that run at their
own pace must not let timing into the bits.
"""
import importlib
import json
import pathlib

import pytest

import hp_scenes as hs
from test_fit_vectors_gram_gpu import explain, record
from test_subtract_gpu import COMMON, scene
from util import pkg, synth

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden' / 'back_cols_parent.json'


def unknowns(ko, bgo):
    return 48 * ((ko + 1) * (ko + 2) // 2) + 1 + (bgo + 1) * (bgo + 2) // 2


def _plain(ko, bgo, ns, seed):
    return (lambda: scene(nx=256, ny=256, seed=seed, nstars=90),
            dict(r=3.0, rss=7.0, nsx=ns, nsy=ns, ko=ko, bgo=bgo, **COMMON), unknowns(ko, bgo))


# name -> (maker, fit settings, unknowns); the stamp grid leaves a region more usable stamps than spatial terms
SCENES = {
    'ko0-bgo1': _plain(0, 1, 3, 200),
    'ko1-bgo2': _plain(1, 2, 3, 201),
    'ko2-bgo3': _plain(2, 3, 4, 202),
    'ko3-bgo0': _plain(3, 0, 5, 203),
    'ko3-bgo2': _plain(3, 2, 5, 204),
    'ko5-bgo0': _plain(5, 0, 6, 205),                                  # 1010 unknowns: k_chol_back
    'rejected-2x2': (lambda: hs.contaminated(nx=256, ny=256, seed=5, nstars=140, ntr=6),
                     dict(hs.BASE, r=3.0, rss=7.0, nsx=3, nsy=3, nrx=2, nry=2, nss=3, ko=2, bgo=1), unknowns(2, 1)),
    # the benchmark's system: 23 blocks, the last of 18 rows
    'ko4-bgo0': (lambda: scene(nx=256, ny=256, seed=206, nstars=90),
                 dict(r=3.0, rss=7.0, nsx=5, nsy=5, ko=4, bgo=0, **COMMON), unknowns(4, 0)),
}
REPEATED = ('ko3-bgo0', 'ko4-bgo0')
POOL = 'pool-batch2'


def run_scene(engine, name):
    make, kw, _ = SCENES[name]
    data = make()
    return data, kw, engine.subtract(*data, **kw)


def pool_jobs():
    import torch
    from test_nightly_gpu import make_jobs
    # ko 2, bgo 1: 292 unknowns, 10 blocks, the last of 4 rows
    jobs = make_jobs(torch, pkg(), synth(), 2, 1024, 1024, 1, {'ko': 2, 'bgo': 1, 'tu': 1e6, 'iu': 1e6}, seed=971)
    for j in jobs:
        j.sci['seeing'] = 4.0
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


@pytest.mark.parametrize('name', sorted(SCENES))
def test_scene_gives_the_recorded_bits(engine, golden, name):
    data, kw, (d, n, info) = run_scene(engine, name)
    got, want = record(d, n, info), golden[name]
    if got != want:
        print('info', {k: (got['info'].get(k), v) for k, v in want['info'].items() if got['info'].get(k) != v})
        explain(data, kw, d, n)
    assert got == want
    assert info['status'] == 0 and info['ncoeff'] == SCENES[name][2]
    if name == 'rejected-2x2':
        assert info['niter'] >= 2 and info['nstamps_used'] < info['nstamps_total']


def test_batched_kernel_gives_the_bits_of_the_single_call(engine, golden):
    """Two jobs as one batch of launches (k_chol_back_cols_b): the digests recorded from one job at a time."""
    assert run_pool(2) == golden[POOL]


@pytest.mark.parametrize('name', REPEATED)
def test_three_runs_in_one_process_give_the_same_bits(engine, golden, name):
    make, kw, _ = SCENES[name]
    data = make()
    for k in range(3):
        d, n, info = engine.subtract(*data, **kw)
        assert record(d, n, info) == golden[name], f'run {k}'
