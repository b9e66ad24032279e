"""The scenes of tests/conv_scenes.py do what they are for - shown on the CPU, with the oracle alone.

Every half width 1 .. 20: both regions of ``case(hwk)`` solve with at least four stamps, at least 60 % of the frame
is unfilled, the first region column ends in a block one pixel wide and the frame is no larger than its size rule
allows.

Half widths 1, 5, 11 and 16: a convolution that reads the taps mirrored, transposed or shifted by one column
(``oracle.hotpants.kernel_at`` wrapped; the fit does not go through it) moves at least 50 % of the unfilled pixels of
the difference image and at least 90 % of the unfilled pixels of the noise image by more than ten times the limits of
``test_subtract_gpu.compare``.  On ``test_subtract_gpu.scene`` the same mutations move 6 - 18 % and 0 %.

The size rule of ``case``: the smallest width >= max(2 hw + 200, 260) with (nx // 2) % STEP == 1 and the smallest
height >= max(2 hw + 180, 240) with ny % STEP == STEP - 1, hw = hwk + int(rss).  The search for the residue adds up
to 2 STEP - 1 columns and STEP - 1 rows, and the floor of 260 lies above 2 hw + 230 for half widths 1 - 4, so a flat
"2 hw + 230 on a side" does not follow from the rule (it gives 392 x 311 at half width 19, where 2 hw + 230 is 346).
What is asserted is the rule itself: the residues, that no smaller size at or above the floor has them, and the worst
case of the search.
"""
import numpy as np
import pytest

import conv_scenes as cs
from oracle import hotpants as ohp

HWKS = list(range(1, 21))


@pytest.mark.parametrize('hwk', HWKS)
def test_every_half_width_solves_and_leaves_most_of_the_frame(hwk):
    (sci, srms, ref, rrms, bpm), kw = cs.case(hwk)
    ny, nx = sci.shape
    step = 2 * hwk + 1
    assert int(kw['r']) == hwk and int(kw['rss']) == 2 * hwk + 1
    fx, fy = cs.floor_size(hwk)
    assert (nx // 2) % step == 1 and ny % step == step - 1
    assert not any((w // 2) % step == 1 for w in range(fx, nx))
    assert not any(h % step == step - 1 for h in range(fy, ny))
    assert fx <= nx <= fx + 2 * step - 1 and fy <= ny <= fy + step - 1
    d, n, info = cs.oracle(hwk)
    assert len(info['regions']) == 2
    for reg in info['regions']:
        assert reg is not None
        assert reg['nstamps_used'] >= 4
    assert (d != 1e-30).mean() >= 0.60
    # the template term of the noise plane: a tenth of the science variance or more (scene(): a two-hundredth)
    good = d != 1e-30
    share = (n[good] ** 2 - 9.0) / 9.0
    assert np.median(share) > 0.1
    assert bpm.sum() > 0


@pytest.mark.parametrize('name', list(cs.MUTATIONS))
@pytest.mark.parametrize('hwk', [1, 5, 11, 16])
def test_a_wrong_tap_table_moves_most_pixels_of_both_products(monkeypatch, hwk, name):
    data, kw = cs.case(hwk)
    base = cs.oracle(hwk)
    true_kernel, wrong = ohp.kernel_at, cs.MUTATIONS[name]
    monkeypatch.setattr(ohp, 'kernel_at', lambda *a: wrong(true_kernel(*a)))
    mutant = cs.run(data, kw)
    monkeypatch.undo()
    assert mutant[2]['regions'] == base[2]['regions']          # (the fit never saw the wrong kernel)
    fd, fn = cs.moved(base, mutant, data[0])
    print(f'hwk {hwk} {name}: diff {100 * fd:.1f} %, noise {100 * fn:.1f} % of the unfilled pixels moved')
    assert fd >= 0.50
    assert fn >= 0.90


@pytest.mark.parametrize('layout', cs.LAYOUTS)
@pytest.mark.parametrize('hwk', [2, 8, 12])
def test_ragged_layouts_have_their_residues_and_solve(hwk, layout):
    (sci, *_), kw = cs.ragged(hwk, layout)
    ny, nx = sci.shape
    step = 2 * hwk + 1
    want = {0, 1} if layout == 'thirds' else {0, step - 1}
    assert cs.residues(nx, ny, kw) == (want, want)
    regs = ohp.regions(nx, ny, kw['nrx'], kw['nry'])
    if layout == 'thirds':
        assert nx % 3 != 0 and kw['nrx'] == 3 and kw['nry'] == 2
        assert regs[2][1] - regs[2][0] > regs[0][1] - regs[0][0]          # the last column of regions is the widest
    d, n, info = cs.ragged_oracle(hwk, layout)
    assert all(r is not None and r['nstamps_used'] >= 4 for r in info['regions'])
    assert (d != 1e-30).mean() >= 0.60


def test_nonfinite_template_noise_is_where_it_is_meant_to_be():
    hwk = 6
    (sci, srms, ref, rrms, bpm), kw = cs.nonfinite(hwk)
    clean = cs.case(hwk)[0]
    ny, nx = ref.shape
    ys, xs = np.nonzero(~np.isfinite(rrms))
    assert len(ys) == 12 and np.isnan(rrms).sum() == 6 and np.isposinf(rrms).sum() == 6
    assert np.isfinite(ref[ys, xs]).all() and (bpm[ys, xs] == 0).all()
    assert (np.abs(xs - nx // 2 + 0.5) < hwk).sum() >= 4                      # at the boundary of the two regions
    edge = np.minimum.reduce([xs, nx - 1 - xs, ys, ny - 1 - ys])
    assert (edge <= hwk).sum() >= 4
    d, n, info = cs.nonfinite_oracle(hwk)
    d0, n0, info0 = cs.oracle(hwk)
    assert info['regions'] == info0['regions']                                # the fit is the clean scene's
    assert np.array_equal(d == 1e-30, d0 == 1e-30)                            # such a variance fills nothing
    assert np.array_equal(d, d0) and np.isfinite(n).all()
    assert np.array_equal(clean[0], sci)
    # each of them lowers the noise of the pixels whose taps reach it
    near = ohp.box_any(~np.isfinite(rrms), hwk) & (d != 1e-30)
    assert near.sum() > 8 * (2 * hwk + 1) ** 2 and (n[near] <= n0[near]).all() and (n[near] < n0[near]).mean() > 0.5
    assert np.array_equal(n[~near], n0[~near])
