"""The numpy restatement of the CLEAN pass (tests/clean_ref.py) against itself (no GPU): the properties the operator of
DESIGN.md ("CLEAN") promises, and the condition the scenes of the GPU tests must meet - a smallest relative gap above
``clean_ref.GAP_MIN`` wherever the full call is compared bit for bit."""
import numpy as np
import pytest

import clean_ref as cr
import clean_scenes as cs


def test_kth_largest_equals_a_sort():
    rng = np.random.default_rng(7)
    for n in (1, 2, 5, 9, 40, 300):
        for v in (rng.normal(0, 1, n).astype(np.float32), rng.integers(0, 4, n).astype(np.float32), np.full(n, 2.5, np.float32)):
            for k in {1, 2, 5, 9, n} - set(range(n + 1, 10)):
                assert cr.kth_largest(v, k) == np.sort(v)[::-1][k - 1], (n, k)


def test_fixed_order_sum_is_a_sum_and_exact_on_integers():
    rng = np.random.default_rng(8)
    for n in (1, 63, 64, 255, 256, 257, 1500):
        e = np.sort(rng.choice(4 * n, n, replace=False))
        ints = rng.integers(-1000, 1000, n).astype(np.float64)
        assert cr.fixed_order_sum(e, ints) == ints.sum()
        v = rng.normal(0, 1, n)
        assert abs(cr.fixed_order_sum(e, v) - np.sum(v)) <= 1e-13 * np.abs(v).sum()
        assert cr.fixed_order_sum(e[::-1], v[::-1]) == cr.fixed_order_sum(e, v)       # the walk's order, whatever the input's


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_halo_keeps_the_galaxy_and_the_two_stars(seed):
    r = cs.reference(f'halo{seed}')
    t = r['table']
    assert len(r['pre']['table']) == {1: 6, 2: 16, 3: 15}[seed] and len(t) == 3
    for cx, cy, *_ in cs.HALO_SOURCES:                                        # one row within a pixel of every source
        assert (np.hypot(t['X_IMAGE'] - 1.0 - cx, t['Y_IMAGE'] - 1.0 - cy) < 1.0).sum() == 1
    gal = int(np.argmin(np.hypot(t['X_IMAGE'] - 1.0 - 80.3, t['Y_IMAGE'] - 1.0 - 79.6)))
    assert t['NMERGED'][gal] == len(r['pre']['table']) - 2 and t['NMERGED'].sum() == len(r['pre']['table'])
    assert np.array_equal(np.delete(t['NMERGED'], gal), [1, 1])
    assert np.array_equal(r['segm'] > 0, r['pre']['segm'] > 0)                # pixels change hands, none appears or goes
    assert t['ISOAREA_IMAGE'].sum() == (r['segm'] > 0).sum()
    assert r['gap'] > 0.1


def test_stars_and_equal_pairs_are_not_absorbed():
    for name in ('stars40', 'two_equal', 'shapes5'):
        r = cs.reference(name)
        assert not r['into'].any() and np.array_equal(r['root'], np.arange(1, len(r['root']) + 1))
        assert np.array_equal(r['segm'], r['pre']['segm'])
        for c in r['pre']['table'].dtype.names:
            assert r['table'][c].tobytes() == r['pre']['table'][c].tobytes(), c
        assert (r['table']['NMERGED'] == 1).all()
    assert len(cs.reference('stars40')['table']) == 23
    r = cs.reference('two_equal')
    assert len(r['table']) == 2 and r['F'][0] == r['F'][1]                    # equal to the last bit: NUMBER decides the order


def test_reversed_orders_give_the_same_map():
    img, sigma, kw = cs.scene('halo2')
    fwd = cs.reference('halo2')
    rev = cs.reference('halo2', reverse=True)                                 # reversed member order in every sum
    assert np.array_equal(fwd['segm'], rev['segm']) and np.array_equal(fwd['into'], rev['into'])
    robj = cr.clean(img, sigma, reverse_objects=True, **cs.ref_kw(kw))       # (asserts inside that the decisions agree)
    assert np.array_equal(fwd['segm'], robj['segm'])
    rows, F, T, m = cs.random_table(257, 357)
    into, root, _ = cr.decide(rows, F, T, m)
    i2, r2, _ = cr.decide_permuted(rows, F, T, m, 1.0, np.random.default_rng(3).permutation(257))
    assert np.array_equal(into, i2) and np.array_equal(root, r2) and into.any()


def chain_table():
    """C (3) absorbs B (2), B absorbs A (1), and C alone does not reach A: A lies outside C's zone."""
    rows = np.zeros(3, cr.ROW)
    rows['number'] = [1, 2, 3]
    rows['x_image'], rows['y_image'] = [10.0, 40.0, 100.0], [50.0, 50.0, 50.0]
    a = np.array([0.5, 3.0, 4.0])
    rows['a_image'] = rows['b_image'] = a
    rows['x2'] = rows['y2'] = a * a
    rows['npix'] = [9, 120, 200]
    rows['first'] = [700, 300, 500]
    F = np.array([200.0, 5e5, 5e7])
    T = np.full(3, 6.0, np.float32)
    m = np.array([0.1, 0.05, 3.0], np.float32)
    return rows, F, T, m


def test_chains_resolve_to_the_root():
    rows, F, T, m = chain_table()
    into, root, gap = cr.decide(rows, F, T, m)
    assert into.tolist() == [2, 3, 0] and root.tolist() == [3, 3, 3] and gap > cr.GAP_MIN
    assert not (100.0 - 10.0) ** 2 < (10.0 * (4.0 + 0.5)) ** 2                # C's zone ends short of A
    rows, F, T, m = cs.random_table(1000, 1100)
    into, root, _ = cr.decide(rows, F, T, m)
    chained = (into > 0) & (root != into)
    assert chained.sum() > 5
    assert (into[root - 1] == 0).all()                                        # every root is unabsorbed
    assert (F[into[into > 0] - 1] >= F[into > 0]).all()                       # F grows along a chain


def test_alpha_not_positive_absorbs_nothing():
    rows, F, T, m = chain_table()
    F[2] = 100.0                                                              # amp below T: g < 1, alpha < 0
    F[1] = 50.0
    F[0] = 5.0
    M = cr.model(rows, F, T, 1.0)
    assert not M['ok'].any()
    into, _, _ = cr.decide(rows, F, T, m)
    assert not into.any()


def test_settings():
    rows, F, T, m = chain_table()
    for bad in (0.05, 11.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            cr.decide(rows, F, T, m, bad)


@pytest.mark.parametrize('name,deblend', cs.BITWISE)
def test_scenes_compared_bit_for_bit_have_a_gap(name, deblend):
    r = cs.reference(name, deblend)
    print(f'{name} deblend={deblend}: {len(r["pre"]["table"])} -> {len(r["table"])} objects, gap {r["gap"]:.3g}')
    assert r['gap'] > cr.GAP_MIN


@pytest.mark.parametrize('param', [0.5, 2.0])
@pytest.mark.parametrize('n', cs.TABLE_SIZES)
def test_tables_compared_at_other_exponents_have_a_gap(n, param):
    rows, F, T, m = cs.random_table(n, cs.TABLE_SEED + n)
    into, _, gap = cr.decide(rows, F, T, m, param)
    print(f'n {n} param {param}: {int((into > 0).sum())} absorbed, gap {gap:.3g}')
    assert gap > cr.GAP_MIN


# ---- the scenes at the frame's edges and with bad, flagged and poisoned pixels (clean_scenes.PLANES) --------------------
@pytest.mark.parametrize('nthresh', cs.PLANES_NTHRESH)
@pytest.mark.parametrize('name', cs.PLANES)
def test_scenes_with_planes_are_what_they_claim(name, nthresh):
    """Objects before and after, a gap wherever the GPU test compares bit for bit, and the same map in either order."""
    import deblend_scenes as ds
    import extract_ref as xr
    r, rev = cs.reference(name, nthresh), cs.reference(name, nthresh, reverse=True)
    t = r['table']
    counts = (len(r['pre']['first']['table']), len(r['pre']['table']), len(t))
    print(f'{name} nthresh {nthresh}: {counts[0]} first-pass -> {counts[1]} deblended -> {counts[2]} objects, gap {r["gap"]:.3g}, '
          f'NMERGED {t["NMERGED"].tolist()}')
    assert r['gap'] > cr.GAP_MIN
    assert np.array_equal(r['segm'], rev['segm']) and np.array_equal(r['into'], rev['into'])
    for c in xr.INT_COLUMNS + ['PARENT_NUMBER', 'NMERGED']:
        assert np.array_equal(t[c], rev['table'][c]), c
    if name in cs.SHREDS:
        assert counts == ((2, 3, 2) if nthresh == 32 else (2, 2, 1))
    else:                                                 # stars are not each other's shreds: the deblended objects stay
        assert counts[1:] == (ds.EXPECT[name][4], ds.EXPECT[name][4]) and counts[0] == ds.EXPECT[name][3]
        assert (t['NMERGED'] == 1).all() and np.array_equal(r['segm'], r['pre']['segm'])
    if name in ds.BAD_SCENES or name in ds.POISON_SCENES or name in cs.SHREDS:
        # sensitivity: without the planes (and the poison) the map is another one
        img, sigma, kw = ds.unmasked(name) if name not in cs.SHREDS else cs.scene(name)
        plain = cr.clean(img, sigma, deblend=dict(nthresh=nthresh, mincont=0.005), **cs.ref_kw(kw))
        assert not np.array_equal(plain['segm'], r['segm'])


@pytest.mark.parametrize('name', list(cs.SHREDS))
def test_a_shred_beside_a_hole_is_absorbed(name):
    import scipy.ndimage as ndi
    r = cs.reference(name, 32)
    t, hole = r['table'], r['pre']['first']['bad']
    assert hole.sum() == 9
    ring = ndi.binary_dilation(hole, structure=np.ones((3, 3))) & ~hole
    before, after = set(r['pre']['segm'][ring].tolist()) - {0}, set(r['segm'][ring].tolist()) - {0}
    assert len(before) == 2 and len(after) == 1                               # the star and the shred; then one object
    row = t[after.pop() - 1]
    assert row['NMERGED'] == 2 and row['FLAGS_WEIGHT'] == 1 and (row['FLAGS'] & 2) and t['NMERGED'].tolist() == [2, 1]
    assert t['FLAGS_WEIGHT'].tolist() == [1, 0]
    shred = r['pre']['table'][int(np.flatnonzero(r['into'])[0])]
    assert shred['ISOAREA_IMAGE'] == 6 and r['into'].tolist().count(0) == 2
    if name == 'shred_corner':
        assert (row['XMIN_IMAGE'], row['YMIN_IMAGE']) == (1, 1) and (row['FLAGS'] & 8)
    else:
        assert not (row['FLAGS'] & 8)
