"""``source.associate`` and its tables with the two library calls replaced by tests/assoc_ref.py (no GPU): the order of
the reference's associate() - join known sources, move them, gate on rb, cluster, name, veto - on a three-image toy
night, the same night given as catalog tables, and the two text tables."""
import importlib

import numpy as np
import pytest

import assoc_ref as ar
from util import pkg


@pytest.fixture
def src(monkeypatch):
    m = importlib.import_module('zuds-pipeline_amd.source')
    calls = []

    def cluster(ra, dec, snr, rb=None, radius_arcsec=2.0, engine=None):
        calls.append(('cluster', len(ra), radius_arcsec))
        return ar.cluster_ref(ra, dec, snr, rb, radius_arcsec)

    def crossmatch(ra, dec, cra, cdec, radius_arcsec, engine=None):
        calls.append(('crossmatch', len(ra), len(cra), radius_arcsec))
        return ar.crossmatch_ref(ra, dec, cra, cdec, radius_arcsec)
    monkeypatch.setattr(m, 'cluster', cluster)
    monkeypatch.setattr(m, 'crossmatch', crossmatch)
    m.calls = calls
    return m


def test_constants_are_the_reference_s():
    z = pkg()
    assert (z.ASSOC_RB_MIN, z.ASSOC_RADIUS_ARCSEC, z.STAR_VETO_ARCSEC) == (0.4, 2.0, 1.5)
    for name in ('associate', 'cluster', 'crossmatch', 'Source', 'detections_from_cat'):
        assert hasattr(z, name)


def test_associate_on_the_toy_night(src):
    z = pkg()
    dets, known, stars = ar.toy_night(z.Detection, src.Source)
    names = []
    out = src.associate(dets, sources=known, stars=stars, name=lambda k: names.append(k) or f'n{k}')
    ar.check_toy_night(dets, out, names)
    # join at 2 arcsec against the one known source, cluster the 9 eligible ones of the other 10 (d2 is gated), veto at 1.5
    assert src.calls == [('crossmatch', 12, 1, 2.0), ('cluster', 9, 2.0), ('crossmatch', 3, 2, 1.5)]


def test_gate_default_names_and_no_rb(src):
    z = pkg()
    dets, _, _ = ar.toy_night(z.Detection, src.Source)
    out = src.associate(dets, rb_min=0.72)                       # no known sources, no stars, a stricter gate
    # S0's two detections: rb 0.9 and 0.6 -> one eligible, alone; A: d1 (0.9), d10 (0.75); C: d3, d8; D: none above 0.72
    assert [s.id for s in out] == ['src0000000', 'src0000001']
    assert out[0].detections == [dets[1], dets[10]] and out[1].detections == [dets[3], dets[8]]
    assert out[0].best_detection is dets[10] and out[1].score == 0.8 + 0.75
    dets, _, _ = ar.toy_night(z.Detection, src.Source)
    for d in dets:
        d.rb = None                                              # no scores at all: every detection is eligible
    out = src.associate(dets)
    assert [len(s.detections) for s in out] == [2, 3, 2, 2, 2] and all(s.score == 0.0 for s in out)
    assert out[2].detections == [dets[2], dets[7]]
    # a detection that has a source already is left alone
    dets, known, stars = ar.toy_night(z.Detection, src.Source)
    dets[1].source = known[0]
    out = src.associate(dets, sources=known, stars=stars)
    assert dets[1].source is known[0] and out[3].detections == [dets[6], dets[10]]        # (C and D, rows 3 and 4, now come first)
    assert src.associate([]) == []


def test_catalog_tables_are_accepted_and_the_tables_round_trip(src, tmp_path):
    z = pkg()
    dets, known, stars = ar.toy_night(z.Detection, src.Source)
    dt = [('X_WORLD', 'f8'), ('Y_WORLD', 'f8'), ('FLUX_APER', 'f4'), ('FLUXERR_APER', 'f4'), ('GOODCUT', 'u1'), ('rb', 'f4')]
    tables = []
    for im in ('img0', 'img1', 'img2'):
        rows = [d for d in dets if d.image == im]
        t = np.zeros(len(rows) + 1, dtype=dt).view(np.recarray)
        for k, d in enumerate(rows):
            t[k + 1] = (d.ra, d.dec, d.flux, d.fluxerr, 1, d.rb)
        t[0] = (rows[0].ra, rows[0].dec, 1e6, 1.0, 0, 0.99)       # a row the filter cut: never a detection
        tables.append(t)
    got = src.detections_from_cat(tables[0], image='x.cat')
    assert [d.row for d in got] == [1, 2, 3, 4, 5] and got[0].image == 'x.cat' and got[0].snr == 30.0
    out = src.associate(tables, sources=known, stars=stars)
    assert [len(s.detections) for s in out] == [3, 3, 2, 2] and out[2].score == -1.0
    assert [(d.image, d.row) for d in out[1].detections] == [(0, 2), (1, 2), (2, 1)]
    assert out[1].score == np.float64(np.float32(0.9)) + np.float64(np.float32(0.5)) + 0.75
    # the two tables
    all_dets = [d for s in out for d in s.detections[1 if s is out[0] else 0:]]
    sp, dp = str(tmp_path / 's.txt'), str(tmp_path / 's.det.txt')
    src.write_source_tables(out, all_dets, sp, dp)
    lines = open(sp).read().splitlines()
    assert lines[0] == '# id ra dec ndet score best_image rejected' and len(lines) == 5
    f = lines[3].split()
    assert f[0] == out[2].id and int(f[3]) == 2 and float(f[4]) == -1.0 and f[5] == '1' and f[6] == '1'
    assert lines[1].split()[6] == '0' and abs(float(lines[2].split()[1]) - out[1].ra) < 1e-8
    rows = [l.split() for l in open(dp).read().splitlines()[1:]]
    assert len(rows) == len(all_dets) and {r[4] for r in rows} == {s.id for s in out}
    back = src.read_sources_table(sp)
    assert [s.id for s in back] == [s.id for s in out] and [s.rejected for s in back] == [False, False, True, False]
    assert all(abs(a.ra - b.ra) < 1e-8 and abs(a.dec - b.dec) < 1e-8 for a, b in zip(back, out))
