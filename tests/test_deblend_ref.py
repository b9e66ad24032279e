"""The numpy restatement of the deblending (tests/deblend_ref.py) against things that are not ours, and against its own
statement where nothing else exists: scipy.ndimage.label for the components of every level, the mirror symmetry of a
symmetric scene, and the independence of the order in which an object's members are walked."""
import numpy as np
import pytest

import deblend_ref as dr
import deblend_scenes as ds
import extract_ref as xr


def object_levels(name):
    """(L per box pixel, -1 outside) of every first-pass object of a scene."""
    img, sigma, kw = ds.scene(name)
    first = ds.reference(name)['first']
    filt, seg = np.asarray(first['filtered'], np.float32), first['segm']
    thr = np.float32(1.5) * sigma
    out = []
    for k in range(1, seg.max() + 1):
        ys, xs = np.nonzero(seg == k)
        f = filt[ys, xs]
        i = int(np.argmax(f))
        u = dr.thresholds(f[i], thr[ys[i], xs[i]], 32)
        box = np.full((ys.max() - ys.min() + 1, xs.max() - xs.min() + 1), -1, np.int64)
        box[ys - ys.min(), xs - xs.min()] = dr.pixel_levels(f, u)
        out.append((box, u, f[i], thr[ys[i], xs[i]]))
    return out


@pytest.mark.parametrize('name', ['nested', 'noisy_field', 'plateaus'])
def test_level_components_equal_scipy_label_at_every_level(name):
    import scipy.ndimage as ndi                          # (a missing scipy fails the test: the comparison is the point)
    seen = 0
    for box, u, P, T in object_levels(name):
        assert (np.diff(u) >= 0).all() and u[0] == np.float64(T) and u[-1] < np.float64(P) * (1 + 1e-12)
        assert (box >= 0).any() and box.max() <= 31
        for k in range(32):
            for reverse in (False, True):
                ours = dr.level_components(box, k, reverse)
                theirs, n = ndi.label(box >= k, structure=np.ones((3, 3)))
                assert np.array_equal(ours >= 0, theirs > 0)
                # the same partition: every pair (our id, their id) that occurs is one to one
                pairs = np.unique(np.stack([ours[theirs > 0], theirs[theirs > 0]]), axis=1)
                assert pairs.shape[1] == n == len(np.unique(pairs[0])) == len(np.unique(pairs[1]))
                seen += n
    assert seen > 32


def test_two_equal_gaussians_split_into_mirror_images():
    """49 x 49, centres 21 and 27, sigma 1.2: the scene is its own mirror image about column 24; so are the two objects,
    except for the tied bisector column, which the smallest-index rule gives to object 1."""
    img = ds.gaussians(49, 49, [(21, 24, 100.0, 1.2), (27, 24, 100.0, 1.2)]).astype(np.float32)
    assert np.array_equal(img, img[:, ::-1])
    r = dr.deblend(img, np.ones_like(img))
    seg, tab = r['segm'], r['table']
    assert len(r['first']['table']) == 1 and len(tab) == 2 and r['nsplit'] == 1
    assert (tab['FLAGS'] & 2).all() and not (tab['FLAGS'] & 1).any() and (tab['PARENT_NUMBER'] == 1).all()
    one, two = seg == 1, seg == 2
    assert np.array_equal(one[:, :24], two[:, ::-1][:, :24]) and np.array_equal(one[:, 25:], two[:, ::-1][:, 25:])
    column = seg[:, 24]
    assert (column[column > 0] == 1).all() and (column > 0).sum() >= 3
    assert np.array_equal(seg > 0, r['first']['segm'] > 0)                    # every member ends up labelled


@pytest.mark.parametrize('name', ['pair5', 'nested', 'plateaus', 'sigma_step', 'noisy_field', 'edge', 'just_too_small'])
def test_forward_and_reversed_member_order_give_the_same_map(name):
    fwd, rev = ds.reference(name), ds.reference(name, reverse=True)
    assert np.array_equal(fwd['segm'], rev['segm'])
    for c in xr.INT_COLUMNS + ['PARENT_NUMBER']:
        assert np.array_equal(fwd['table'][c], rev['table'][c]), c


def test_the_outcomes_the_scenes_were_chosen_for():
    counts = {name: (len(ds.reference(name)['first']['table']), len(ds.reference(name)['table']))
              for name in ('pair3', 'pair4', 'pair5', 'pair6', 'pair8', 'contrast20', 'contrast60', 'nested', 'plateaus',
                           'sigma_step', 'lone_star', 'edge', 'just_too_small')}
    assert counts == dict(pair3=(1, 1), pair4=(1, 1), pair5=(1, 2), pair6=(1, 2), pair8=(1, 2), contrast20=(1, 1),
                          contrast60=(1, 2), nested=(1, 3), plateaus=(1, 2), sigma_step=(1, 2), lone_star=(1, 1),
                          edge=(1, 2), just_too_small=(2, 3))
    # where nothing splits the restatement is the first pass, bit for bit
    for name in ('pair3', 'contrast20', 'lone_star'):
        r = ds.reference(name)
        assert np.array_equal(r['segm'], r['first']['segm'])
        for c in r['first']['table'].dtype.names:
            assert r['table'][c].tobytes() == r['first']['table'][c].tobytes(), c
    r = ds.reference('noisy_field')
    parts = np.bincount(r['table']['PARENT_NUMBER'])
    assert (len(r['first']['table']), len(r['table']), r['nsplit'], parts.max()) == (15, 20, 3, 4)
    flagged = (r['table']['FLAGS'] & 2) != 0
    assert np.array_equal(flagged, parts[r['table']['PARENT_NUMBER']] > 1)
    # the 9-pixel object of just_too_small stays, the 11-pixel one splits into its two branches
    t = ds.reference('just_too_small')['table']
    assert t['ISOAREA_IMAGE'].tolist() == [9, 6, 5] and t['PARENT_NUMBER'].tolist() == [1, 2, 2]


def test_settings_are_refused():
    img = np.zeros((8, 8), np.float32)
    for kw in (dict(nthresh=24), dict(nthresh=1), dict(nthresh=128), dict(mincont=1.5), dict(mincont=-0.1)):
        with pytest.raises(ValueError):
            dr.deblend(img, np.ones_like(img), **kw)
