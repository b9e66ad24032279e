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


# ---- the census of the scenes added for the tree kernel's indexing: each is what it claims, on the restatement alone --
def largest_first(name):
    """(first-pass table, row of its largest object, first-pass map) of a scene."""
    first = ds.reference(name)['first']
    t = first['table']
    return t, t[int(np.argmax(t['ISOAREA_IMAGE']))], first['segm']


def test_db_cells_is_the_limit_design_md_states():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'DESIGN.md')) as f:
        assert f'`DB_CELLS` = {ds.DB_CELLS} pixels' in f.read()
    assert ds.DB_CELLS == 1024


@pytest.mark.parametrize('name', sorted(ds.EXPECT))
def test_new_scenes_are_what_they_claim(name):
    """Box, pixel count, side of DB_CELLS, objects before and after, and the same map in either member order."""
    r, rev = ds.reference(name), ds.reference(name, reverse=True)
    t1, big, _ = largest_first(name)
    bw, bh = big['XMAX_IMAGE'] - big['XMIN_IMAGE'] + 1, big['YMAX_IMAGE'] - big['YMIN_IMAGE'] + 1
    got = (int(bw), int(bh), int(big['ISOAREA_IMAGE']), len(t1), len(r['table']))
    print(f'{name}: box {bw} x {bh} = {bw * bh} ({"LDS" if bw * bh <= ds.DB_CELLS else "global"} form), {got[2]} pixels, '
          f'{got[3]} -> {got[4]} objects')
    assert got == ds.EXPECT[name]
    if name in ds.BOX_SCENES or name in ds.SINGLE_LINES:
        w, h = (int(v) for v in name[3:].split('x')) if name.startswith('box') else (int(name[4:]), 1)
        assert (bw, bh) == (w, h)
        lds = (w, h) in ds.BOX_SHAPES[True] or name == 'line1024'
        assert (bw * bh <= ds.DB_CELLS) == lds and (lds or (w, h) in ds.BOX_SHAPES[False] or name == 'line1025')
        ny, nx = ds.scene(name)[0].shape
        assert (nx, ny) == (w + 6, h + 5)                                     # the frame is a few pixels larger
    if got[4] > got[3]:
        assert r['nsplit'] >= 1 and (r['table']['FLAGS'] & 2).any()
    else:                                                                     # the single-peak lines: nothing splits
        assert r['nsplit'] == 0 and np.array_equal(r['segm'], r['first']['segm'])
    img = ds.scene(name)[0]
    assert np.abs(img[np.isfinite(img)]).max() <= 1e6
    assert np.array_equal(r['segm'], rev['segm'])
    for c in xr.INT_COLUMNS + ['PARENT_NUMBER']:
        assert np.array_equal(r['table'][c], rev['table'][c]), c


@pytest.mark.parametrize('name', ['box2x512', 'box512x2', 'box3x341', 'box2x513', 'box3x342'])
def test_strips_hang_together_through_one_diagonal_step(name):
    import scipy.ndimage as ndi
    fg = ds.reference(name)['first']['segm'] > 0
    assert ndi.label(fg, structure=np.ones((3, 3)))[1] == 1 and ndi.label(fg)[1] == 2      # 8-connected, not 4-connected
    # ... in the wing: both sub-objects lie on one side of the step each, and the left / upper one reaches across it
    seg = ds.reference(name)['segm']
    four, _ = ndi.label(fg)
    assert len(np.unique(seg[four == 1])) == 1 and len(np.unique(seg[four == 2])) == 2


def test_edge_scenes_reach_the_edges_they_name():
    def edges(name, k):
        seg = ds.reference(name)['first']['segm'] == k
        return bool(seg[:, 0].any()), bool(seg[0].any()), bool(seg[:, -1].any()), bool(seg[-1].any())   # left top right bottom
    assert edges('edge_right', 1) == (False, False, True, False)
    assert edges('edge_bottom', 1) == (False, False, False, True)
    assert sorted(edges('corners', k) for k in (1, 2, 3, 4)) == sorted([(True, True, False, False), (False, True, True, False),
                                                                        (True, False, False, True), (False, False, True, True)])
    for name in ('frame37x29', 'frame31x29', 'frame1x40', 'frame40x1'):
        assert edges(name, 1) == (True, True, True, True) and (ds.reference(name)['first']['segm'] == 1).all()
        assert (ds.reference(name)['table']['FLAGS'] & 8).all()
    assert ds.scene('frame37x29')[0].shape == (29, 37) and 37 % 4 and 37 * 29 > ds.DB_CELLS >= 31 * 29
    assert ds.scene('frame1x40')[0].shape == (40, 1) and ds.scene('frame40x1')[0].shape == (1, 40)
    for name in ('edge_right', 'edge_bottom', 'corners'):
        assert (ds.reference(name)['table']['FLAGS'] & 8).any()


def test_every_nthresh_changes_an_outcome_and_64_fills_the_tables():
    for base, want in ds.NTHRESH_OBJECTS.items():
        got = {n: len(ds.reference(base if n == 32 else f'{base}@{n}')['table']) for n in want}
        print(f'{base}: {len(ds.reference(base)["first"]["table"])} objects before; after, per nthresh: {got}')
        assert got == want
    assert ds.NTHRESH_OBJECTS['deep_saddle'][2] != ds.NTHRESH_OBJECTS['deep_saddle'][32]
    assert max(ds.scene('deep_saddle')[0].shape) <= 64
    for n in ds.NTHRESH:                                  # sensitivity: a kernel that ran 32 levels whatever it is told fails
        differ = [base for base in ds.NTHRESH_OBJECTS
                  if not np.array_equal(ds.reference(f'{base}@{n}')['segm'], ds.reference(base)['segm'])]
        print(f'nthresh {n}: the map differs from that at 32 in {differ}')
        assert differ
    for name in ds.NTHRESH_SCENES:
        n = int(name.split('@')[1])
        occ = ds.occupied_levels(name)
        assert all(o.min() >= 0 and o.max() <= n - 1 for o in occ)
        assert any(o.max() == n - 1 for o in occ)                             # the last entry of u[] / hist[] is used
        print(f'{name}: occupied levels per first-pass object {[len(o) for o in occ]}')
    occ, = ds.occupied_levels('deep_saddle@64')                               # one object, in the LDS form
    _, big, _ = largest_first('deep_saddle@64')
    assert len(occ) >= 40 and occ.max() == 63 and occ.min() == 0
    assert (big['XMAX_IMAGE'] - big['XMIN_IMAGE'] + 1) * (big['YMAX_IMAGE'] - big['YMIN_IMAGE'] + 1) <= ds.DB_CELLS
    assert max(len(o) for o in ds.occupied_levels('noisy_field@64')) >= 60
    assert all(len(o) <= 2 for name in ds.NTHRESH_SCENES if name.endswith('@2') for o in ds.occupied_levels(name))


def bordering(name, where):
    """The final objects that have a pixel 8-adjacent to the pixels ``where`` (a boolean plane)."""
    import scipy.ndimage as ndi
    seg = ds.reference(name)['segm']
    ring = ndi.binary_dilation(where, structure=np.ones((3, 3))) & ~where
    return sorted(set(seg[ring].tolist()) - {0})


@pytest.mark.parametrize('name', sorted(list(ds.BAD_SCENES) + list(ds.POISON_SCENES)))
def test_bad_and_poisoned_scenes_depend_on_their_planes(name):
    """Sensitivity: the map with the bad / flag plane (or the poison) differs from the map of the same image without it, so
    a kernel that ignored the plane would fail; and the holes border the sub-objects they are said to."""
    img, sigma, kw = ds.scene(name)
    r = ds.reference(name)
    pimg, psigma, pkw = ds.unmasked(name)
    plain = dr.deblend(pimg, psigma, use_filter=pkw['filter'], aper_radius=pkw.get('aper_radius', 3.0))
    assert not np.array_equal(r['segm'], plain['segm'])
    badmap = r['first']['bad']
    assert badmap.any() and not plain['first']['bad'].any() and not (r['segm'][badmap] != 0).any()
    kind = name.split('.')[0].split('_')[1]
    t = r['table']
    near = bordering(name, badmap)
    print(f'{name}: {len(r["first"]["table"])} -> {len(t)} objects ({len(plain["first"]["table"])} -> {len(plain["table"])} without '
          f'the plane); objects beside a bad pixel {near}; FLAGS_WEIGHT {t["FLAGS_WEIGHT"].tolist()}')
    assert np.array_equal(np.flatnonzero(t['FLAGS_WEIGHT']) + 1, near)       # the bad-neighbour bit: those and no others
    if kind == 'saddle':
        assert near == [1, 2]                                                 # the hole borders both sub-objects
    elif kind in ('hole1', 'hole9', 'flags'):
        assert near == [1] and len(t) == 2                                    # ... exactly one
        inner = np.zeros_like(badmap)
        inner[1:-1, 1:-1] = True
        assert (r['first']['segm'][np.nonzero(bordering_ring(badmap))] == 1).all()   # a hole: members all around it
    elif kind == 'peak':
        ys, xs = np.nonzero(plain['first']['segm'] == 1)
        f = np.asarray(plain['first']['filtered'])[ys, xs]
        assert badmap[ys[np.argmax(f)], xs[np.argmax(f)]]                      # P and T come from another pixel now
    elif kind in ('diag', 'cut'):
        import scipy.ndimage as ndi
        assert len(plain['first']['table']) == 1 and len(r['first']['table']) == (1 if kind == 'diag' else 2)
        assert ndi.label(r['first']['segm'] > 0)[1] == 2                       # 4-connected: two; across the line by diagonals only
    elif kind == 'edge':
        assert badmap[0].any() and not badmap[1:].any() and (r['first']['segm'][0] == 1).any() and (t['FLAGS'] & 8).any()
    if kind == 'flags':
        assert t['IMAFLAGS_ISO'].tolist() == [0, 0x40000010]                  # the hole's 0x40 reaches no row
        noflag = dr.deblend(img, sigma, kw['bad'], None, use_filter=kw['filter'])
        assert not noflag['table']['IMAFLAGS_ISO'].any() and (np.asarray(kw['flag'])[badmap] == 0x40).all()
    for c in xr.FLOAT_COLUMNS:                                                # finite unless poisoned
        if name in ds.BAD_SCENES:
            assert np.isfinite(t[c]).all(), c


def bordering_ring(where):
    import scipy.ndimage as ndi
    return ndi.binary_dilation(where, structure=np.ones((3, 3))) & ~where


def test_poisoned_apertures_are_not_finite_in_every_way():
    seen = set()
    for name in ds.POISON_SCENES:
        t = ds.reference(name)['table']
        for c in ('FLUX_APER', 'FLUXERR_APER'):
            seen |= {(c, 'nan')} if np.isnan(t[c]).any() else set()
            seen |= {(c, '+inf')} if np.isposinf(t[c]).any() else set()
            seen |= {(c, '-inf')} if np.isneginf(t[c]).any() else set()
        assert (t['FLAGS'] & 16).any()                                        # which is all that says so
        for c in set(xr.FLOAT_COLUMNS) - {'FLUX_APER', 'FLUXERR_APER'}:
            assert np.isfinite(t[c]).all(), c
    assert seen == {('FLUX_APER', 'nan'), ('FLUX_APER', '+inf'), ('FLUX_APER', '-inf'), ('FLUXERR_APER', 'nan')}


def seed_plane(name, k=1):
    """Boolean plane: the pixels of first-pass object ``k`` that are seeds (members of S(root)); the rest of the object is
    handed out by the leftover rounds.  The same steps as ``deblend_ref.deblend_object``."""
    img, sigma, kw = ds.scene(name)
    ex, db = ds.split_kw(kw)
    N = db.get('nthresh', 32)
    first = ds.reference(name)['first']
    filt, seg = np.asarray(first['filtered'], np.float32), first['segm']
    ny, nx = seg.shape
    members = np.flatnonzero(seg.ravel() == k)
    fm = filt.ravel()[members]
    ipk = int(np.argmax(fm))
    u = dr.thresholds(fm[ipk], (np.float32(1.5) * sigma).ravel()[members[ipk]], N)
    y, x = np.divmod(members, nx)
    w, h = x.max() - x.min() + 1, y.max() - y.min() + 1
    box = (y - y.min()) * w + (x - x.min())
    Lbox, fbox = np.full(h * w, -1, np.int64), np.zeros(h * w, np.float32)
    Lbox[box], fbox[box] = dr.pixel_levels(fm, u), fm
    nodes, root = dr.build_tree(Lbox.reshape(h, w), fbox.reshape(h, w), u, fm[ipk], N, db.get('mincont', 0.005),
                                ex.get('detect_minarea', 5))
    inbox = np.zeros(h * w, bool)
    for s in dr.split_sets(nodes)[root]:
        inbox[nodes[s]['pix']] = True
    out = np.zeros(ny * nx, bool)
    out[members] = inbox[box]
    return out.reshape(ny, nx)


@pytest.mark.parametrize('name', ['bad_hole1.f0', 'bad_hole9.f0', 'bad_hole9.f1', 'bad_flags.f1', 'imgnan_hole9.f0', 'box2x512',
                                  'box3x342', 'box1x1025'])
def test_leftover_rounds_reach_what_the_scenes_put_in_their_way(name):
    """The holes in a wing and the diagonal steps of the strips lie among the leftover pixels, not among the seeds: the
    rounds have to walk around the one and across the other."""
    import scipy.ndimage as ndi
    seeds, seg = seed_plane(name), ds.reference(name)['first']['segm']
    left = (seg == 1) & ~seeds
    assert seeds.any() and left.sum() > 100
    if name.startswith('box'):
        four, _ = ndi.label(seg > 0)
        if name[3] in '23':                                                   # the last pixel before the step and the first after
            ends = ndi.binary_dilation(four == 1, structure=np.ones((3, 3))) & (four == 2)
            assert ends.sum() == 1 and not seeds[ends].any()
            assert not seeds[ndi.binary_dilation(ends, structure=np.ones((3, 3))) & (seg > 0)].any()
    else:
        ring = bordering_ring(ds.reference(name)['first']['bad'])
        assert (seg[ring] == 1).all() and not seeds[ring].any()
    print(f'{name}: {int(seeds.sum())} seed pixels, {int(left.sum())} leftover pixels')
