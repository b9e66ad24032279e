"""Scenes that drive the kernel fit's stamp rejection (helpers, no tests).

``scene()`` of test_subtract_gpu.py has clean stars and constant noise maps: its fits reject a stamp only by accident.
``contaminated()`` puts fake transients on the brightest template stars of the science frame (their stamps fit badly
and are rejected, round after round, substamp after substamp) and replaces the noise maps by varying ones, so that
the merit's denominator ``npix * vbar`` differs from stamp to stamp.

``SCENES`` names every scene the rejection tests use, with the fit settings it is run at and what the oracle
(oracle/hotpants.py) gives for it per region: (rounds, stamps, used).  tests/test_oracle_rejection.py proves on the
CPU, from the oracle's trace, that each scene reaches the branch it is meant to and keeps its margins;
tests/test_subtract_rejection_gpu.py runs the same scenes through the GPU fit.
"""
import numpy as np

from test_subtract_gpu import COMMON, scene

SKY_REF = 150.0          # scene(): template sky; science sky = scale * SKY_REF + bg


def contaminated(nx=384, ny=352, seed=5, nstars=200, ntr=10, amp=0.5, varying=True, faint=1.0, step=None, **kw):
    """``scene(nx, ny, seed, nstars, **kw)`` with ``ntr`` transients of relative amplitude ``amp`` in the science
    frame and (``varying``) noise maps that change over the frame.

    ``faint`` < 1 scales every star by that factor at unchanged sky and pixel noise (the scene is linear in the stars;
    the noise that the scaling takes away is added back from a generator of its own).  ``step=(x0, f)``: the science
    noise map times ``f`` from column ``x0`` on.  Returns (sci, srms, ref, rrms, bpm) like ``scene()``."""
    sci, srms, ref, rrms, bpm = scene(nx=nx, ny=ny, seed=seed, nstars=nstars, **kw)
    sci = sci.astype(np.float64)
    ref = ref.astype(np.float64)
    if faint != 1.0:
        rng = np.random.default_rng(1000003 + seed)
        sky = kw.get('scale', 1.3) * SKY_REF + kw.get('bg', 20.0)
        left = np.sqrt(1.0 - faint * faint)
        ref = SKY_REF + faint * (ref - SKY_REF) + rng.normal(0, 0.5 * left, ref.shape)
        sci = sky + faint * (sci - sky) + rng.normal(0, 3.0 * left, sci.shape)
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    work = ref.copy()
    work[:20] = work[-20:] = -np.inf
    work[:, :20] = work[:, -20:] = -np.inf
    for _ in range(ntr):
        y, x = np.unravel_index(int(np.argmax(work)), work.shape)
        sci += amp * ref[y, x] * np.exp(-((xx - (x + 1.5)) ** 2 + (yy - (y - 1.0)) ** 2) / (2.0 * 1.5 ** 2))
        work[max(y - 25, 0):y + 26, max(x - 25, 0):x + 26] = -np.inf
    if varying:
        srms = 3.0 * (1.0 + 0.5 * np.sin(xx / 37.0) * np.cos(yy / 23.0))
        rrms = 0.5 * (1.0 + 0.4 * np.cos(xx / 51.0))
    if step is not None:
        srms = np.where(xx >= step[0], srms * step[1], srms)
    return (sci.astype(np.float32), np.asarray(srms, np.float32), ref.astype(np.float32),
            np.asarray(rrms, np.float32), bpm)


BASE = dict(r=5.0, rss=12.0, nsx=4, nsy=4, nrx=2, nry=1, ko=1, bgo=1, **COMMON)


def run_oracle(data, **kw):
    """oracle.hotpants.subtract with its trace: (diff, noise, info); info['traces'][region] is the list fit_region
    fills (candidates first, then one record per round)."""
    from oracle import hotpants as ohp
    sci, srms, ref, rrms, bpm = data
    return ohp.subtract(sci, ref, srms, rrms, bpm, trace=True, **kw)


def summary(info):
    """Per region (rounds, stamps, used), None for an unsolved one."""
    return [None if r is None else (r['niter'], r['nstamps_total'], r['nstamps_used']) for r in info['regions']]


def margin(traces, ks):
    """Smallest relative distance, over every round of every region, of a merit from the rejection limit and of a
    merit from a 3-sigma boundary of a clipping pass.  A pass with s == 0 (one value left) has no boundary to miss:
    its limit is that value itself, bit for bit, whatever the order of summation."""
    worst = np.inf
    for tr in traces:
        for rec in (tr or [])[1:]:
            v = np.asarray(rec['merits'])
            worst = min(worst, float(np.min(np.abs(v - rec['limit']) / abs(rec['limit']))) if len(v) > 1 else np.inf)
            for m, s in rec['clips']:
                if s > 0:
                    worst = min(worst, float(np.min(np.abs(np.abs(v - m) - 3.0 * s) / (3.0 * s))))
    return worst


def branches(traces, nss):
    """Which rejection branches a traced fit reaches (the letters of the module docstring of
    test_oracle_rejection.py)."""
    got = set()
    rounds = [len(tr) - 1 for tr in traces if tr]
    if len(rounds) > 1 and max(rounds) >= 5 and min(rounds) < max(rounds):
        got.add('a')
    for ri, tr in enumerate(traces):
        if not tr:
            continue
        cands, recs = tr[0]['cands'], tr[1:]
        if len(recs) == 8 and recs[-1]['rejected']:
            got.add('b')
        seen = {}
        for rec in recs:
            for si, a in zip(rec['live'], rec['active']):
                seen.setdefault(si, set()).add(a)
            for si in rec['rejected']:
                a = rec['active'][rec['live'].index(si)]
                if a + 1 >= len(cands[si]) and rec is not recs[-1]:        # (a solve without the stamp follows)
                    got.add('d_nss' if len(cands[si]) == nss else 'd_short')
        if any({1, 2} <= s for s in seen.values()):
            got.add('c')
        if sum(1 for c in cands if c) > 0 and recs and all(a_gone(recs, cands, si) for si in range(len(cands)) if cands[si]):
            got.add('e')
        for rj, other in enumerate(traces):
            if rj != ri and other:
                for k, rec in enumerate(recs):
                    if not rec['rejected'] and len(other) - 1 > k and other[1 + k]['rejected']:
                        got.add('f')
    return got


def a_gone(recs, cands, si):
    """True when stamp ``si`` ran out of substamps in this fit."""
    for rec in recs:
        if si in rec['rejected'] and rec['active'][rec['live'].index(si)] + 1 >= len(cands[si]):
            return True
    return False


# ---- the committed cases: name -> (maker, scene arguments, fit settings on top of BASE, branches it must reach) -----
# Branch letters (test_oracle_rejection.py): a - a region with >= 5 rounds next to one that converges earlier;
# b - 8 rounds with a rejection in the eighth; c - a stamp on its 2nd and on its 3rd substamp; d_nss / d_short - a
# stamp out of substamps at a == nss / at a (-1, -1) centre before nss; f - a round that rejects nothing in one region
# and something in another.
ONE = dict(nrx=1, nry=1)
WIDE = dict(r=3.0, rss=6.0, nsx=17, nsy=16, ko=1, bgo=0, **ONE)          # 272 cells: the block-wide rejection kernel
CASES = {}


def _case(name, maker, sc, kw, reach=''):
    CASES[name] = dict(maker=maker, sc=sc, kw=kw, reach=set(reach.split()))


for _nss in (1, 3, 8):
    _case(f'tr5-nss{_nss}', 'contaminated', dict(), dict(nss=_nss), 'a b c d_nss f' if _nss == 3 else '')
    _case(f'tr9-nss{_nss}', 'contaminated', dict(seed=9), dict(nss=_nss), 'a b c f' if _nss == 3 else '')
    # (the tenfold step of the science noise map from column 96 on: vbar decides who is rejected - and every branch)
    _case(f'step-nss{_nss}', 'contaminated', dict(step=(96, 10.0)), dict(nss=_nss),
          'a b c d_nss d_short f' if _nss == 3 else '')
for _ks in (0.5, 1.0, 4.0):
    _case(f'ks{_ks}', 'contaminated', dict(), dict(ks=_ks))
for _ft in (5.0, 200.0):
    _case(f'ft{_ft:g}', 'contaminated', dict(faint=0.03), dict(ft=_ft), 'd_short' if _ft == 200.0 else '')
_case('wide', 'contaminated', dict(nx=540, ny=510, seed=13, nstars=500, ntr=20), WIDE, 'b c d_nss d_short')
_case('ko0', 'contaminated', dict(), dict(ko=0))
_case('ko4', 'contaminated', dict(), dict(r=4.0, rss=8.0, nsx=6, nsy=6, ko=4, bgo=0, **ONE))
_case('ko5', 'contaminated', dict(), dict(r=3.0, rss=7.0, nsx=6, nsy=6, ko=5, bgo=0, **ONE))
_case('bgo2', 'contaminated', dict(), dict(bgo=2))
_case('batch-1', 'scene', dict(seed=3), dict(nss=3))                  # (the batch: one configuration, tr5-nss3's)
_case('batch-5', 'contaminated', dict(varying=False), dict(nss=3)) # constant maps: what step-nss3 is held against
_case('basis-4', 'contaminated', dict(), dict(deg=(4,), sigma=(1.2,)))
_case('basis-8-0', 'contaminated', dict(), dict(deg=(8, 0), sigma=(0.8, 2.5)))
_case('basis-3-2-2-1', 'contaminated', dict(), dict(deg=(3, 2, 2, 1), sigma=(0.5, 1.0, 2.0, 4.0)))
_case('basis-0', 'contaminated', dict(), dict(deg=(0,), sigma=(1.0,), ko=0, bgo=0))
_case('basis-limit', 'contaminated', dict(), dict(deg=(6, 4, 3), sigma=(0.7, 1.5, 3.0), bgo=3))   # 53 + 10 + 1 = 64 rows
_case('noise-clean', 'contaminated', dict(ntr=0), dict())
OVER_LIMIT = dict(deg=(6, 4, 3, 0), sigma=(0.7, 1.5, 3.0, 4.0), bgo=3)                # 54 + 10 + 1 = 65 rows: refused


# per region (rounds, stamps, used), from oracle/hotpants.py
EXPECT = {
    'tr5-nss1': [(8, 16, 8), (4, 16, 9)], 'tr5-nss3': [(8, 16, 15), (5, 16, 16)], 'tr5-nss8': [(8, 16, 16), (5, 16, 16)],
    'tr9-nss1': [(2, 16, 15), (5, 16, 10)], 'tr9-nss3': [(2, 16, 16), (8, 16, 16)], 'tr9-nss8': [(2, 16, 16), (8, 16, 16)],
    'ks0.5': [(8, 16, 9), (8, 16, 9)], 'ks1.0': [(8, 16, 11), (8, 16, 13)], 'ks4.0': [(1, 16, 16), (2, 16, 16)],
    'ft5': [(4, 16, 16), (6, 16, 16)], 'ft200': [(4, 15, 15), (8, 12, 10)],
    'wide': [(8, 251, 204)], 'ko0': [(3, 16, 16), (6, 16, 16)], 'ko4': [(8, 36, 34)], 'ko5': [(8, 36, 34)],
    'bgo2': [(8, 16, 15), (5, 16, 16)], 'batch-1': [(1, 16, 16), (1, 14, 14)], 'batch-5': [(5, 16, 16), (4, 16, 16)],
    'basis-4': [(8, 16, 15), (3, 16, 16)], 'basis-8-0': [(8, 16, 15), (5, 16, 16)],
    'basis-3-2-2-1': [(8, 16, 15), (5, 16, 16)], 'basis-0': [(8, 16, 15), (4, 16, 16)],
    'basis-limit': [(8, 16, 15), (5, 16, 16)], 'noise-clean': [(2, 16, 16), (4, 16, 16)],
    'step-nss1': [(6, 16, 9), (4, 16, 9)], 'step-nss3': [(8, 16, 11), (7, 16, 16)], 'step-nss8': [(8, 16, 13), (7, 16, 16)],
}


def case_data(name):
    c = CASES[name]
    return (contaminated if c['maker'] == 'contaminated' else scene)(**c['sc'])


def case_kw(name):
    return dict(BASE, **CASES[name]['kw'])
