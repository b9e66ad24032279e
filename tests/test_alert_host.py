"""``crossmatch.py`` and ``alert.py`` on the host, with no library call: every cross-match function gets its ``idx``, ``sep``
and ``count`` (or ``offsets`` and ``cat_idx``) handed in, and the alert is assembled from hand-made plain objects."""
import importlib
import json
import os
import types

import numpy as np
import pytest

import alert_scenes as sc
from util import pkg

MJD_TO_JD = 2400000.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def xm():
    return importlib.import_module('zuds-pipeline_amd.crossmatch')


def al():
    return importlib.import_module('zuds-pipeline_amd.alert')


def cat(_name, **cols):
    return types.SimpleNamespace(name=_name, index=None, table={k: np.asarray(v) for k, v in cols.items()})


def test_abmag():
    m = xm()
    assert m.abmag(1.0) == 22.5 and m.abmag(100.0) == 17.5 and m.abmag(0.0) == 0 and m.abmag(-3.0) == 0
    assert m.abmag(10.0) == -2.5 * np.log10(10.0) + 22.5
    assert m.abmag(np.array([1.0, 0.0, -1.0, 100.0])).tolist() == [22.5, 0.0, 0.0, 17.5]


def ps1_cat():
    return cat('ps1', ra=np.zeros(5), dec=np.zeros(5), objid=[11, 22, 33, 44, 55], gMeanPSFMag=[1.5, 2.5, 3.5, 4.5, 5.5],
               rMeanPSFMag=[1.25, 2.25, 3.25, 4.25, 5.25], iMeanPSFMag=[1.0, 2.0, 3.0, 4.0, 5.0],
               zMeanPSFMag=[0.5, 0.75, 1.0, 1.25, 1.5], ps_score=[0.125, 0.25, 0.375, 0.5, 0.625])


def test_ps1_slots_are_the_nearest_rows_in_order():
    # three queries: 3 matches (of 4 in range), 2 matches, none
    idx = np.array([[4, 0, 2], [1, 3, -1], [-1, -1, -1]], np.int32)
    sep = np.array([[0.5, 7.25, 20.0], [3.0, 29.5, np.nan], [np.nan] * 3])
    out = xm().ps1(ps1_cat(), [0.0] * 3, [0.0] * 3, idx, sep, np.array([4, 2, 0], np.int32))
    # the first decision: every field of slot i is the i-th nearest row's (the reference takes ids and magnitudes from
    # the unsorted list)
    assert out[0] == {'objectidps1': 55, 'sgscore1': 0.625, 'distpsnr1': 0.5, 'psgmag1': 5.5, 'psrmag1': 5.25, 'psimag1': 5.0,
                      'pszmag1': 1.5,
                      'objectidps2': 11, 'sgscore2': 0.125, 'distpsnr2': 7.25, 'psgmag2': 1.5, 'psrmag2': 1.25, 'psimag2': 1.0,
                      'pszmag2': 0.5,
                      'objectidps3': 33, 'sgscore3': 0.375, 'distpsnr3': 20.0, 'psgmag3': 3.5, 'psrmag3': 3.25, 'psimag3': 3.0,
                      'pszmag3': 1.0}
    assert set(out[1]) == {f'{p}{n}' for p in ('objectidps', 'sgscore', 'distpsnr', 'psgmag', 'psrmag', 'psimag', 'pszmag') for n in (1, 2)}
    assert out[1]['objectidps2'] == 44 and out[1]['distpsnr2'] == 29.5 and out[2] == {}
    assert type(out[0]['objectidps1']) is int and type(out[0]['psgmag1']) is float


def test_legacysurvey_takes_the_three_nearest_ascending():
    cols = {c: np.arange(4) + 0.5 for c in xm().LS_COLUMNS}
    cols.update(OBJID=[101, 102, 103, 104], TYPE=np.array(['PSF', 'REX', 'EXP', 'DEV']), FLUX_G=[1.0, 100.0, 0.0, -2.0], ra=np.zeros(4),
                dec=np.zeros(4))
    idx = np.array([[3, 1, 0], [2, 0, -1], [-1, -1, -1]], np.int32)
    sep = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, np.nan], [np.nan] * 3])
    out = xm().legacysurvey(cat('legacysurvey', **cols), [0.0] * 3, [0.0] * 3, idx, sep, np.array([4, 2, 0], np.int32))
    # the second decision: the nearest three, ascending (the reference's query yields the farthest three)
    assert [out[0][f'lsdistnr{n}'] for n in (1, 2, 3)] == [1.0, 2.0, 3.0]
    assert [out[0][f'lsobjectid{n}'] for n in (1, 2, 3)] == [104, 102, 101] and [out[0][f'lstype{n}'] for n in (1, 2, 3)] == ['DEV', 'REX', 'PSF']
    assert [out[0][f'lsg{n}'] for n in (1, 2, 3)] == [0, 17.5, 22.5] and out[1]['lsg1'] == 0            # abmag(flux <= 0) = 0
    assert out[0]['lsebv1'] == 3.5 and out[0]['lsw4_2'] == xm().abmag(1.5) and out[0]['lszspec3'] == 0.5 and out[0]['lsgaiap1'] == 3.5
    assert len(out[0]) == 3 * 21 and len(out[1]) == 2 * 21 and 'lsdistnr3' not in out[1] and out[2] == {}
    assert type(out[0]['lstype1']) is str and type(out[0]['lsobjectid1']) is int


def test_names_are_unique_sorted_and_joined_with_commas(monkeypatch):
    m = xm()
    names = cat('ztfalerts', ra=np.zeros(5), dec=np.zeros(5), objectId=np.array(['ZTF20b', 'ZTF19a', 'ZTF20b', 'ZTF18c', 'ZTF21z']))
    offsets, cat_idx = np.array([0, 3, 3, 4], np.int64), np.array([0, 1, 2, 4], np.int32)
    got = m.ztfalerts(names, [0.0] * 3, [0.0] * 3, offsets, cat_idx)
    assert [list(v) for v in got] == [['ZTF19a', 'ZTF20b'], [], ['ZTF21z']]
    mq = cat('milliquas', ra=np.zeros(2), dec=np.zeros(2), Name=np.array(['Q b', 'Q a']))
    assert [list(v) for v in m.milliquas(mq, [0.0], [0.0], np.array([0, 2]), np.array([0, 1]))] == [['Q a', 'Q b']]
    tn = cat('tns', ra=np.zeros(1), dec=np.zeros(1), name=np.array(['AT2020x']))
    assert [list(v) for v in m.tns(tn, [0.0], [0.0], np.array([0, 1]), np.array([0]))] == [['AT2020x']]
    # xmatch: the joins, and '' for a table that is not supplied
    monkeypatch.setattr(m, 'ztfalerts', lambda c, ra, dec: got)
    out = m.xmatch([1.0, 2.0, 3.0], [0.0, 0.0, 0.0], {'ztfalerts': names})
    assert out == [{'ztfname': 'ZTF19a,ZTF20b', 'mqid': '', 'tnsid': ''}, {'ztfname': '', 'mqid': '', 'tnsid': ''},
                   {'ztfname': 'ZTF21z', 'mqid': '', 'tnsid': ''}]
    assert m.xmatch([1.0], [2.0]) == [{'ztfname': '', 'mqid': '', 'tnsid': ''}]
    with pytest.raises(ValueError, match='unknown'):
        m.xmatch([1.0], [2.0], {'gaia': names})


def hand_made_source(z):
    """A source with single-epoch detections at 58100.25 and 58090.5 (before), 58120.0 (after), and stack detections on
    coadd A (58080 .. 58095, two detections), coadd B (58050 .. 58099) and coadd C (58110 .. 58130: starts after)."""
    src = z.Source(id='ZUDS20abc', ra=100.0, dec=10.0)
    ref = sc.reference()
    for k, m in enumerate((58100.25, 58120.0, 58090.5)):
        sc.detection(z, sc.single_sub(z, m, id=10 + k, ref=ref), src, id=100 + k)
    a = sc.stack_sub([58095.0, 58080.0, 58090.0], id=20, ref=ref)
    sc.detection(z, a, src, id=200)
    sc.detection(z, sc.stack_sub(None, id=21, ref=ref, coadd=a.target_image), src, id=201)       # a second detection on coadd A
    sc.detection(z, sc.stack_sub([58050.0, 58099.0], id=22, ref=ref), src, id=202)
    sc.detection(z, sc.stack_sub([58110.0, 58130.0], id=23, ref=ref), src, id=203)
    sc.photometry(z, src, [58050.0, 58101.0, 58101.0 + 0.4 / 86400, 58101.0 + 0.6 / 86400, 58125.0])
    return src, ref


def test_a_single_alert_history_dates_and_light_curve_cut():
    z = pkg()
    src, ref = hand_made_source(z)
    sub = sc.single_sub(z, 58101.0, id=31, ref=ref)
    det = sc.detection(z, sub, src, id=999)
    a = z.Alert.from_detection(det)
    assert (a.detection, a.sent) == (det, False) and a.cutoutscience.type == 'new' and a.cutouttemplate.type == 'ref' \
        and a.cutoutdifference.type == 'sub'
    p = a.alert
    assert (p['objectId'], p['candid'], p['schemavsn'], p['publisher']) == ('ZUDS20abc', 999, '0.4', 'ZUDS/NERSC')
    c = p['candidate']
    assert c['alert_type'] == 'single' and c['ztfname'] == c['mqid'] == c['tnsid'] == ''
    assert (c['fid'], c['pid'], c['programpi'], c['programid'], c['pdiffimfilename'], c['candid'], c['isdiffpos'], c['field']) == \
        (2, 31, 'Kulkarni', 2, 'sub.31.fits', 999, 't', 651)
    assert c['rcid'] == (3 - 1) * 4 + (2 - 1) and (c['ra'], c['dec']) == (100.0, 10.0)
    assert (c['aimage'], c['bimage'], c['elong'], c['fwhm'], c['xpos'], c['ypos']) == (1.5, 1.2, 1.25, 3.0, 101.5, 55.25)
    assert c['aimagerat'] == 1.5 / 3.0 and c['bimagerat'] == 1.2 / 3.0 and c['snr'] == 15.0
    assert (c['drb'], c['drbversion']) == (0.875, 'braai_d6_m9')
    assert (c['jdstartref'], c['jdendref'], c['nframesref']) == (58000.25, 58010.5, 3)         # as the reference hands them on
    assert c['jd'] == 58101.0 + MJD_TO_JD and (c['nid'], c['diffmaglim'], c['exptime']) == (101, 20.5, 30.0)
    # history: singles before 58101 (two of the three, and not this detection's own date), ascending
    assert c['ndethist_single'] == 2 and (c['jdstarthist_single'], c['jdendhist_single']) == (58090.5 + MJD_TO_JD, 58100.25 + MJD_TO_JD)
    # stacks: one entry per coadd (A counted once), those that start before 58101 (not C), ordered by their last date
    assert c['ndethist_stack'] == 2 and (c['jdstarthist_stack'], c['jdendhist_stack']) == (58080.0 + MJD_TO_JD, 58099.0 + MJD_TO_JD)
    # the light curve: mjd <= 58101 + 0.5 s
    lc = p['light_curve']
    assert [r['flux'] for r in lc] == [100.0, 101.0, 102.0] and lc[-1]['mjd'] <= 58101.0 + 0.5 / 86400 < 58101.0 + 0.6 / 86400
    assert set(lc[0]) == {'mjd', 'filter', 'zp', 'zpsys', 'flux', 'fluxerr', 'flags', 'lim_mag', 'id'}
    assert lc[0]['filter'] == 'ztfr' and lc[0]['zpsys'] == 'ab' and type(lc[0]['flux']) is float and type(lc[0]['flags']) is int
    d = a.to_dict()
    assert d['cutoutScience'] == b'newnewnew' and d['cutoutTemplate'] == b'refrefref' and d['cutoutDifference'] == b'subsubsub'
    assert 'cutoutScience' not in a.alert and al().validate(d, 'single') == []
    assert json.loads(a.to_json())['candidate'] == json.loads(json.dumps(c))


def test_a_stack_alert():
    z = pkg()
    src, ref = hand_made_source(z)
    sub = sc.stack_sub([58100.0, 58104.0, 58101.0, 58103.0], id=41, ref=ref)
    det = sc.detection(z, sub, src, id=1000)
    a = z.Alert.from_detection(det)
    c = a.alert['candidate']
    assert c['alert_type'] == 'stack' and 'jd' not in c and 'nid' not in c and 'diffmaglim' not in c
    assert (c['jdstartstack'], c['jdendstack'], c['jdmed'], c['nframesstack']) == \
        (58100.0 + MJD_TO_JD, 58104.0 + MJD_TO_JD, 58102.0 + MJD_TO_JD, 4)
    assert c['exptime'] == 30.0 + 31.0 + 32.0 + 33.0 and c['fid'] == 1 and c['programpi'] == 'Kulkarni'
    # history relative to the coadd's last date, 58104: three singles before it? no - 58120 is after
    assert c['ndethist_single'] == 2 and c['ndethist_stack'] == 3            # A, B and this coadd itself (it starts before its own end)
    assert c['jdendhist_stack'] == 58104.0 + MJD_TO_JD
    assert [r['flux'] for r in a.alert['light_curve']] == [100.0, 101.0, 102.0, 103.0]       # mjd <= 58104 + 0.5 s
    assert al().validate(a.to_dict(), 'stack') == []
    # a plain image without input frames makes a single alert (the rule of alert.py:94-96 on plain objects)
    plain = types.SimpleNamespace(id=5, fid=1, field=1, ccdid=1, qid=1, basename='x.fits', mjd=58101.0, target_image=sc.frame(58101.0),
                                  reference_image=ref)
    assert z.Alert.from_detection(sc.detection(z, plain, src, id=1001)).alert['candidate']['alert_type'] == 'single'


def test_the_three_errors():
    z = pkg()
    src, ref = hand_made_source(z)
    sub = sc.single_sub(z, 58101.0, id=31, ref=ref)
    with pytest.raises(ValueError, match=r'not associated with a source \(77\)'):
        z.Alert.from_detection(sc.detection(z, sub, None, id=77))
    with pytest.raises(ValueError, match='not associated with a source'):
        z.make_alerts([sc.detection(z, sub, None, id=78)])
    empty = z.Source(id='nolc', ra=1.0, dec=2.0)
    with pytest.raises(RuntimeError, match='no light curve.*"nolc"'):
        z.Alert.from_detection(sc.detection(z, sub, empty, id=79))
    # strict: a detection without cutouts and without a model name
    det = sc.detection(z, sub, src, id=80, stamps=False)
    det.rb_version = None
    assert len(z.make_alerts([det])) == 1
    with pytest.raises(ValueError) as e:
        z.make_alerts([det], strict=True)
    for name in ('cutoutScience', 'cutoutTemplate', 'cutoutDifference', 'drbversion'):
        assert name in str(e.value)
    assert '80:' in str(e.value)


def test_validate():
    z = pkg()
    v = al().validate
    src, ref = hand_made_source(z)
    single = z.Alert.from_detection(sc.detection(z, sc.single_sub(z, 58101.0, id=31, ref=ref), src, id=1)).to_dict()
    stack = z.Alert.from_detection(sc.detection(z, sc.stack_sub([58100.0, 58104.0], id=41, ref=ref), src, id=2)).to_dict()
    assert v(single, 'single') == [] and v(stack, 'stack') == []
    assert any("'jd'" in p and 'unknown' in p for p in v(single, 'stack'))                  # the other kind's fields
    assert any("'jdmed'" in p and 'missing' in p for p in v(single, 'stack'))
    # cross-match fields of every type fit; a slot that is absent is fine, the same slot as None as well
    full = dict(single, candidate=dict(single['candidate'], objectidps1=123456789012345678, sgscore1=0.5, lstype1='PSF', lsg1=0,
                                       distpsnr2=None, ztfname='ZTF20a,ZTF20b'))
    assert v(full, 'single') == []
    broken = dict(single, candidate={k: w for k, w in single['candidate'].items() if k != 'rcid'})
    assert v(broken, 'single') == ["candidate: required field 'rcid' is missing"]
    broken = dict(single, candidate=dict(single['candidate'], fwhm=None))
    assert v(broken, 'single') == ["candidate: field 'fwhm' is null and may not be"]
    broken = dict(single, candidate=dict(single['candidate'], magpsf=19.5))
    assert v(broken, 'single') == ["candidate: unknown key 'magpsf'"]
    broken = dict(single, candidate=dict(single['candidate'], field='651', objectidps1=1.5, drb=True))
    assert len(v(broken, 'single')) == 3
    broken = dict(single, extra=1, light_curve=single['light_curve'] + [dict(single['light_curve'][0], flags=None, colour='g')])
    got = v(broken, 'single')
    assert "alert: unknown key 'extra'" in got and any('light_curve[3]' in p and "'flags'" in p for p in got) \
        and any('light_curve[3]' in p and "'colour'" in p for p in got) and len(got) == 3
    assert v(dict(single, light_curve=None), 'single') == []                               # the one nullable field of the packet
    with pytest.raises(ValueError):
        v(single, 'both')


def test_the_fixture_holds_field_lists_and_nothing_else():
    with open(os.path.join(ROOT, 'tests', 'golden', 'alert_fields.json')) as f:
        fx = json.load(f)
    assert sorted(fx) == ['schema_single', 'schema_stack']
    for kind in fx.values():
        assert sorted(kind) == ['alert', 'candidate', 'light_curve']
        for fields in kind.values():
            assert all(sorted(x) == ['name', 'nullable', 'type'] for x in fields)
    assert len(fx['schema_single']['candidate']) == 123 and len(fx['schema_stack']['candidate']) == 124
    assert al().alert_fields() == fx
