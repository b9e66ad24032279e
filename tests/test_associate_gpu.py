"""zm_associate / zm_crossmatch (csrc/associate.hip) against tests/assoc_ref.py on the smallest scenes that can break
them.  Every scene is clear of the band 0.999 r .. 1.001 r (asserted by the restatement), so labels, members, best, count
and idx are compared exactly; ``sep`` alone has a tolerance.

The bound on ``sep``: SEP_K * eps64 radians of chord, converted to arcsec (assoc_ref.SEP_TOL_ARCSEC), eps64 = 2^-52.
Where it comes from: the kernel turns (ra, dec) into a unit vector.  ra * (pi / 180) is rounded once per point: half an
ulp of a value below 2 pi, <= 2 eps64 absolute; for dec, below pi / 2, <= 0.5 eps64 (the error of the constant scales the
whole sky and cancels in a separation).  sin and cos pass that on with slope <= 1 and add their own rounding, <= 1 eps64
on values <= 1 even at 2 ulp.  x = cos(dec) cos(ra) therefore carries <= (0.5 + 1) + (2 + 1) + 0.5 = 5 eps64, y the same,
z <= 1.5 eps64.  The chord vector is the difference of two such points: <= 2 sqrt(5^2 + 5^2 + 1.5^2) = 14.5 eps64 in
length in the worst case, and sep = 2 asin(chord / 2) passes that on unchanged at these radii.  The restatement's
haversine works on coordinate differences and is exact to a small fraction of eps64 here.  Measured with
tests/measure_assoc_tolerance.py on exactly the scenes below: an fp64 numpy evaluation of the chord formula is off by at
most 3.03 eps64 radians from a 50-digit evaluation, the restatement by < 0.01; 4 x 3.03 = 12.1, rounded up to the next
power of two: SEP_K = 16 - which also covers the worst case derived above.  ("Source association".)"""
import importlib

import numpy as np
import pytest

import assoc_ref as ar
from util import pkg

pytestmark = pytest.mark.gpu
R = 2.0
KEYS = ('label', 'offsets', 'members', 'best', 'count')


def src():
    return importlib.import_module('zuds-pipeline_amd.source')


def check_cluster(ra, dec, snr, rb=None, r=R, engine=None):
    got = src().cluster(ra, dec, snr, rb, r, engine=engine)
    want = ar.cluster_ref(ra, dec, snr, rb, r)
    assert got['nsrc'] == want['nsrc']
    for k in KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    assert got['label'].size == np.asarray(ra).size                              # no row left out
    assert got['sumrb'].tobytes() == want['sumrb'].tobytes()                     # fp64, member order: the same bits
    return got, want


@pytest.mark.parametrize('n', [0, 1, 2])
def test_tiny_inputs(engine, n):
    ra, dec = np.array([10.0, 10.0])[:n], np.array([5.0, 5.0 + 1.0 / 3600])[:n]
    got, _ = check_cluster(ra, dec, np.ones(n), np.full(n, 0.25), engine=engine)
    assert got['nsrc'] == (1 if n == 2 else 0) and got['offsets'].size == got['nsrc'] + 1


def test_a_pair_just_inside_and_a_pair_just_outside(engine):
    ra, dec = ar.offset(np.array([30.0, 30.0, 31.0, 31.0]), np.array([-10.0, -10.0, 12.0, 12.0]),
                        np.zeros(4), np.array([0.0, 0.9985 * R, 0.0, 1.0015 * R]))
    got, _ = check_cluster(ra, dec, np.array([3.0, 4.0, 5.0, 6.0]), engine=engine)
    assert list(got['label']) == [0, 0, -1, -1] and list(got['best']) == [1]


def test_exact_duplicates_are_neighbours(engine):
    ra = np.array([77.0, 12.5, 77.0, 12.5, 12.5, 200.0])
    dec = np.array([-33.0, 45.0, -33.0, 45.0, 45.0, 0.0])
    got, _ = check_cluster(ra, dec, np.array([1.0, 9.0, 2.0, 9.0, 3.0, 7.0]), np.arange(6) * 0.125, engine=engine)
    assert list(got['label']) == [0, 1, 0, 1, 1, -1] and list(got['best']) == [2, 1]


@pytest.mark.parametrize('size', [65, 300])
def test_a_cluster_larger_than_a_wave(engine, size):
    rng = np.random.default_rng(size)
    ra, dec = ar.offset(210.0, 33.0, rng.uniform(-0.6, 0.6, size), rng.uniform(-0.6, 0.6, size))
    fra, fdec, fsnr, frb = ar.scene(size, nclusters=5, nnoise=10)
    ra, dec = np.concatenate([fra, ra]), np.concatenate([fdec, dec])
    p = rng.permutation(ra.size)
    ra, dec = ra[p], dec[p]
    got, _ = check_cluster(ra, dec, rng.uniform(5, 50, ra.size), rng.uniform(0, 1, ra.size), engine=engine)
    assert got['count'].max() == size


def test_a_long_chain_needs_many_rounds(engine):
    rng = np.random.default_rng(5)
    ra, dec = ar.offset(151.0, 21.0, 1.5 * np.arange(300), np.zeros(300))
    for order in (np.arange(300), rng.permutation(300)):
        got, _ = check_cluster(ra[order], dec[order], rng.uniform(5, 50, 300), rng.uniform(0, 1, 300), engine=engine)
        assert got['nsrc'] == 1 and got['count'][0] == 300
        assert ar.separation(ra[:1], dec[:1], ra[-1:], dec[-1:])[0, 0] > 400.0
        assert src().assoc_stats(engine)['rounds'] >= 2


@pytest.mark.parametrize('where', ['ra0', 'ra90', 'dec0', 'north', 'south'])
def test_clusters_where_a_vector_component_changes_sign(engine, where):
    rng = np.random.default_rng(sorted(['ra0', 'ra90', 'dec0', 'north', 'south']).index(where))
    if where in ('north', 'south'):
        sign = 1.0 if where == 'north' else -1.0
        ra, dec = ar.polar_cap(sign, rng.uniform(0.0, 0.9, 12), rng.uniform(0, 360, 12))      # one cluster on the pole
        ra2, dec2 = ar.polar_cap(sign, rng.uniform(20.0, 400.0, 30), rng.uniform(0, 360, 30))
        ra, dec = np.concatenate([ra, ra2, [0.0]]), np.concatenate([dec, dec2, [sign * 90.0]])
    else:
        box = dict(ra0=(0.0, 37.0, 0.01), ra90=(90.0, -20.0, 0.01), dec0=(222.0, 0.0, 0.01))[where]
        ra, dec, _, _ = ar.scene(7, nclusters=25, nnoise=25, box=box)
        cra, cdec = ar.offset(box[0], box[1], rng.uniform(-0.6, 0.6, 9), rng.uniform(-0.6, 0.6, 9))   # centred on the line
        ra, dec = np.concatenate([ra, cra]), np.concatenate([dec, cdec])
    k = ar.make_clear(ra, dec, R)
    ra, dec = ra[k], dec[k]
    if where == 'ra0':
        assert (ra > 359.99).any() and (ra < 0.01).any()
    got, _ = check_cluster(ra, dec, rng.uniform(5, 50, ra.size), rng.uniform(0, 1, ra.size), engine=engine)
    assert got['nsrc'] >= 1


def test_forty_isolated_points_in_the_smallest_table(engine):
    rng = np.random.default_rng(40)
    ra, dec = rng.uniform(0, 360, 40), np.degrees(np.arcsin(rng.uniform(-1, 1, 40)))
    got, _ = check_cluster(ra, dec, np.ones(40), engine=engine)
    st = src().assoc_stats(engine)
    assert got['nsrc'] == 0 and (got['label'] == -1).all()
    assert st['capacity'] == 128 and st['probes'] >= 40 and st['probe_max'] >= 1
    # and 32 of them: 64 slots, the minimum
    check_cluster(ra[:32], dec[:32], np.ones(32), engine=engine)
    assert src().assoc_stats(engine)['capacity'] == 64
    check_cluster(ra[:3], dec[:3], np.ones(3), engine=engine)
    assert src().assoc_stats(engine)['capacity'] == 64


def test_rows_that_are_not_finite_take_part_in_nothing(engine):
    ra, dec, snr, rb = ar.scene(9, nclusters=20, nnoise=20)
    n = ra.size
    ra, dec, snr = ra.copy(), dec.copy(), snr.copy()
    clean = ar.cluster_ref(ra, dec, snr, rb, R)
    m0 = clean['members'][clean['offsets'][0]:clean['offsets'][1]]
    ra[m0[0]] = np.nan                        # a member of source 0
    dec[clean['members'][clean['offsets'][1]]] = np.inf
    snr[clean['members'][clean['offsets'][2]]] = -np.inf
    snr[clean['members'][clean['offsets'][3] + 1]] = np.nan
    got, want = check_cluster(ra, dec, snr, rb, engine=engine)
    bad = ~(np.isfinite(ra) & np.isfinite(dec) & np.isfinite(snr))
    assert bad.sum() == 4 and (got['label'][bad] == -1).all() and not np.isin(np.flatnonzero(bad), got['members']).any()
    assert got['label'].size == n
    idx, sep = src().crossmatch(ra, dec, ra[~bad], dec[~bad], 1.0, engine=engine)
    assert (idx[np.isnan(ra) | ~np.isfinite(dec)] == -1).all() and np.isnan(sep[np.isnan(ra) | ~np.isfinite(dec)]).all()


def test_snr_ties_go_to_the_lowest_row(engine):
    ra, dec = ar.offset(15.0, 15.0, np.array([0.0, 0.5, 1.0, 0.2, 0.7]), np.array([0.0, 0.3, -0.2, 0.6, 0.1]))
    for snr, best in (([7.0, 9.0, 9.0, 9.0, 1.0], 1), ([4.0, 4.0, 4.0, 4.0, 4.0], 0), ([1.0, 2.0, 3.0, 8.0, 8.0], 3)):
        got, _ = check_cluster(ra, dec, np.array(snr), engine=engine)
        assert list(got['best']) == [best]


def test_sumrb_is_the_same_bits_on_every_run_and_the_member_order_sum(engine):
    rng = np.random.default_rng(77)
    ra, dec, snr, _ = ar.scene(77, nclusters=150, members=(2, 40), spread=0.6, nnoise=100, box=(10.0, -30.0, 1.0))
    rb = rng.uniform(0, 1, ra.size) * 10.0 ** rng.integers(-8, 8, ra.size)        # sums that depend on the order
    a, want = check_cluster(ra, dec, snr, rb, engine=engine)
    b = src().cluster(ra, dec, snr, rb, R, engine=engine)
    assert a['sumrb'].tobytes() == b['sumrb'].tobytes() == want['sumrb'].tobytes()
    assert a['nsrc'] > 64 and ra.size > 1024
    shuffled = np.array([rb[m[::-1]].sum() for m in np.split(want['members'], want['offsets'][1:-1])])
    assert (shuffled != want['sumrb']).any()                                      # the order does matter for these values
    none = src().cluster(ra, dec, snr, None, R, engine=engine)
    assert not none['sumrb'].any() and np.array_equal(none['label'], a['label'])


def test_host_and_device_entry_points_agree_bit_for_bit(engine):
    import torch
    ra, dec, snr, rb = ar.scene(88, nclusters=300, nnoise=700, box=(180.0, 50.0, 2.0))
    assert ra.size > 1024
    host = src().cluster(ra, dec, snr, rb, R, engine=engine)
    dev = src().cluster_dev(*(torch.from_numpy(v).cuda() for v in (ra, dec, snr, rb)), R, engine=engine)
    torch.cuda.synchronize()
    ns = int(dev['nsrc'].cpu()[0])
    assert ns == host['nsrc'] > 0
    off = dev['offsets'].cpu().numpy()
    assert np.array_equal(off[:ns + 1], host['offsets']) and (off[ns:] == host['members'].size).all()
    assert np.array_equal(dev['label'].cpu().numpy(), host['label'])
    assert np.array_equal(dev['members'].cpu().numpy()[:off[ns]], host['members'])
    assert np.array_equal(dev['best'].cpu().numpy()[:ns], host['best'])
    cnt = dev['count'].cpu().numpy()
    assert np.array_equal(cnt[:ns], host['count']) and not cnt[ns:].any()
    assert dev['sumrb'].cpu().numpy()[:ns].tobytes() == host['sumrb'].tobytes()
    # the cross-match
    cra, cdec = ra[::3], dec[::3]
    hi, hs = src().crossmatch(ra, dec, cra, cdec, 1.0, engine=engine)
    di, ds = src().crossmatch_dev(*(torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (ra, dec, cra, cdec)), 1.0,
                                  engine=engine)
    torch.cuda.synchronize()
    assert np.array_equal(di.cpu().numpy(), hi) and ds.cpu().numpy().tobytes() == hs.tobytes()
    assert (hi[::3] == np.arange(cra.size)).all() and (hs[::3] == 0.0).all()


@pytest.mark.parametrize('name', ['field', 'wrap', 'ra90', 'north', 'south'])
def test_crossmatch_scenes(engine, name):
    ra, dec, cra, cdec, r = ar.xm_scene(name)
    idx, sep = src().crossmatch(ra, dec, cra, cdec, r, engine=engine)
    widx, wsep = ar.crossmatch_ref(ra, dec, cra, cdec, r)
    assert idx.dtype == np.int32 and np.array_equal(idx, widx) and (idx >= 0).sum() >= 10 and (idx < 0).sum() >= 2
    hit = idx >= 0
    assert np.isnan(sep[~hit]).all()
    err = np.abs(sep[hit] - wsep[hit]).max()
    print(f'{name}: largest |sep - restatement| = {err:.3e} arcsec = {err / (ar.EPS64 * ar.ARCSEC_PER_RAD):.2f} eps64 rad '
          f'(bound {ar.SEP_K})')
    assert err <= ar.SEP_TOL_ARCSEC


def test_crossmatch_equidistant_entries_none_in_range_and_an_empty_catalogue(engine):
    # two entries mirrored in the equator and an exact duplicate: the lowest index wins
    cra = np.array([50.0, 50.0, 50.0, 120.0, 120.0])
    cdec = np.array([-1.0 / 3600, 1.0 / 3600, 1.0 / 3600, 10.0, 10.0])
    ra, dec = np.array([50.0, 120.0, 50.0]), np.array([0.0, 10.0, 0.25 / 3600])
    for perm in ([0, 1, 2, 3, 4], [2, 1, 0, 4, 3]):
        idx, sep = src().crossmatch(ra, dec, cra[perm], cdec[perm], 1.5, engine=engine)
        widx, wsep = ar.crossmatch_ref(ra, dec, cra[perm], cdec[perm], 1.5)
        assert np.array_equal(idx, widx) and idx[0] == 0 and idx[1] == 3
        assert np.abs(sep - wsep).max() <= ar.SEP_TOL_ARCSEC and sep[1] == 0.0
    # all rows out of range
    idx, sep = src().crossmatch(ra + 1.0, dec, cra, cdec, 1.5, engine=engine)
    assert (idx == -1).all() and np.isnan(sep).all()
    # m = 0 and n = 0
    idx, sep = src().crossmatch(ra, dec, [], [], 1.5, engine=engine)
    assert idx.shape == (3,) and (idx == -1).all() and np.isnan(sep).all()
    idx, sep = src().crossmatch([], [], cra, cdec, 1.5, engine=engine)
    assert idx.shape == (0,) and sep.shape == (0,)


def test_the_radius_is_checked(engine):
    z = pkg()
    for r in (0.0, 0.1, -1.0, 1e5, np.nan):
        with pytest.raises(z.ZMError, match='radius'):
            src().cluster([1.0], [1.0], [1.0], None, r, engine=engine)
        with pytest.raises(z.ZMError, match='radius'):
            src().crossmatch([1.0], [1.0], [1.0], [1.0], r, engine=engine)
