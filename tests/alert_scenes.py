"""Hand-made pieces the alert tests share: image stubs under the reference's attribute names, a source with a detection
history, small external tables around given positions (cleared by the rules of tests/cone_ref.py), and a complete
candidate record."""
import types

import numpy as np

import assoc_ref as ar
import cone_ref as cr

MJD_TO_JD = 2400000.5


def frame(mjd, exptime=30.0, **header):
    """A science frame: the attributes and header keys an alert reads."""
    hdr = dict(PROGRMPI='Kulkarni', PROGRMID=2)
    hdr.update(header)
    return types.SimpleNamespace(mjd=mjd, exptime=exptime, nid=int(mjd) - 58000, maglimit=20.5, header=hdr)


def reference(mjds=(58000.25, 58010.5, 58005.125)):
    return types.SimpleNamespace(input_images=[frame(m) for m in mjds])


def single_sub(pkg, mjd, id=7, ref=None):
    """A ``SingleEpochSubtraction`` on one frame."""
    sub = pkg.SingleEpochSubtraction.__new__(pkg.SingleEpochSubtraction)
    sub.__dict__.update(id=id, fid=2, field=651, ccdid=3, qid=2, basename=f'sub.{id}.fits', target_image=frame(mjd),
                        reference_image=ref or reference())
    return sub                                            # (its mjd is its target image's: Subtraction.mjd)


def stack_sub(mjds, id=70, ref=None, coadd=None):
    """A multi-epoch subtraction on a science coadd of frames at ``mjds`` (a plain object: anything that is not a
    ``SingleEpochSubtraction`` and has ``target_image.input_images`` makes a stack alert)."""
    coadd = coadd or types.SimpleNamespace(input_images=[frame(m, exptime=30.0 + k) for k, m in enumerate(mjds)])
    return types.SimpleNamespace(id=id, fid=1, field=651, ccdid=3, qid=2, basename=f'sub.stack{id}.fits', target_image=coadd,
                                 reference_image=ref or reference(), mjd=float(np.median([i.mjd for i in coadd.input_images])))


def detection(pkg, image, source=None, id=1234, ra=100.0, dec=10.0, stamps=True):
    d = pkg.Detection(ra=ra, dec=dec, image=image, flux=60.0, fluxerr=4.0, elongation=1.25, flags=0, imaflags_iso=0,
                      a_image=1.5, b_image=1.2, fwhm_image=3.0, x_image=101.5, y_image=55.25)
    d.id, d.rb, d.rb_version, d.source = id, 0.875, 'braai_d6_m9', source
    if stamps:
        d.thumbnails = [pkg.Thumbnail(detection=d, type=t, bytes=t.encode() * 3) for t in ('sub', 'new', 'ref')]
    if source is not None:
        source.detections.append(d)
    return d


def photometry(pkg, source, mjds, flux=100.0):
    source.forced_photometry += [pkg.ForcedPhotometry(flux=flux + k, fluxerr=5.0, flags=0, ra=source.ra, dec=source.dec, zp=26.0,
                                                      obsjd=m + MJD_TO_JD, filtercode='zr', image=k, source=source)
                                 for k, m in enumerate(mjds)]


# ---- external tables ----------------------------------------------------------------------------------------------------
def tables(ra, dec, seed=5):
    """``{name: table}`` of the five tables around the positions (ra, dec): per group of positions up to 5 ps1 and
    legacysurvey rows within 30 arcsec (group g gets g mod 6 of them: 0, 1, 2, 3 and more), name rows within 1.5 arcsec of
    two thirds of the groups - two rows with the SAME name on one, two different names on another - and far rows.  Every
    table is cleared for the queries at 30 and 1.5 arcsec."""
    rng = np.random.default_rng(seed)
    ra, dec = np.asarray(ra, np.float64), np.asarray(dec, np.float64)
    n = ra.size
    # positions within 20 arcsec of an earlier one share that one's rows: rows are placed around the first position of
    # every such group only, group g getting the g-th count
    near = ar.separation(ra, dec, ra, dec) < 20.0
    leader = np.array([int(np.flatnonzero(near[k])[0]) for k in range(n)])
    group = {k: g for g, k in enumerate(sorted(set(leader.tolist())))}

    def around(count_of_group, lo, hi):
        ras, decs = [], []
        for k in range(n):
            c = count_of_group(group[k]) if leader[k] == k else 0
            rho = lo + (hi - lo) * (np.arange(c) + rng.uniform(0.2, 0.8, c)) / max(c, 1)
            th = rng.uniform(0, 2 * np.pi, c)
            a, d = ar.offset(ra[k], dec[k], rho * np.cos(th), rho * np.sin(th))
            ras.append(a)
            decs.append(d)
        ras.append(np.mod(ra[:1] + 0.5, 360.0))           # one far row
        decs.append(dec[:1])
        a, d = np.concatenate(ras), np.concatenate(decs)
        p = rng.permutation(a.size)
        a, d = a[p], d[p]
        keep = cr.clear_catalog(ra, dec, a, d, (cr.R_KNN, cr.R_NAME))
        return a[keep], d[keep]

    out = {}
    a, d = around(lambda g: g % 6, 2.0, 28.0)
    m = a.size
    out['ps1'] = dict(ra=a, dec=d, objid=rng.integers(10 ** 17, 2 * 10 ** 17, m), gMeanPSFMag=rng.uniform(15, 22, m),
                      rMeanPSFMag=rng.uniform(15, 22, m), iMeanPSFMag=rng.uniform(15, 22, m),
                      zMeanPSFMag=rng.uniform(15, 22, m), ps_score=rng.uniform(0, 1, m))
    a, d = around(lambda g: (g + 3) % 6, 1.6, 29.0)
    m = a.size
    ls = dict(ra=a, dec=d, OBJID=rng.integers(1, 10 ** 6, m), TYPE=rng.choice(np.array(['PSF', 'REX', 'EXP', 'DEV']), m),
              EBV=rng.uniform(0, 0.2, m))
    for c in ('FLUX_G', 'FLUX_R', 'FLUX_Z', 'FLUX_W1', 'FLUX_W2', 'FLUX_W3', 'FLUX_W4'):
        ls[c] = np.where(rng.uniform(size=m) < 0.2, -rng.uniform(0, 1, m), rng.uniform(0.1, 100, m))     # some fluxes <= 0
    for c in ('GAIA_PHOT_G_MEAN_MAG', 'PARALLAX', 'z_phot_mean', 'z_phot_median', 'z_phot_std', 'z_phot_l68', 'z_phot_u68',
              'z_phot_l95', 'z_phot_u95', 'z_spec'):
        ls[c] = rng.uniform(0, 2, m)
    out['legacysurvey'] = ls
    for name, col, prefix, shift in (('ztfalerts', 'objectId', 'ZTF20aa', 0), ('milliquas', 'Name', 'MQ J', 1), ('tns', 'name', 'AT2020', 2)):
        a, d = around(lambda g: (g + shift) % 3, 0.05, 1.3)
        m = a.size
        names = np.array([f'{prefix}{k:04d}' for k in rng.permutation(m)])
        if name == 'ztfalerts':
            # rows near one position share a name wherever two of them are near the same position
            sep = ar.separation(ra, dec, a, d)
            for k in range(n):
                rows = np.flatnonzero(sep[k] <= cr.R_NAME)
                if rows.size == 2 and group[int(leader[k])] % 2 == 0:
                    names[rows[1]] = names[rows[0]]
        out[name] = {'ra': a, 'dec': d, col: names}
    return out


def expected_xmatch(tabs, ra, dec):
    """What ``xmatch`` must return for ``tables``: assembled here from cone_ref's indices, independently of crossmatch.py."""
    ra, dec = np.asarray(ra, np.float64), np.asarray(dec, np.float64)
    out = [dict() for _ in range(ra.size)]
    if 'ps1' in tabs:
        t = tabs['ps1']
        idx, sep, _ = cr.knn_ref(ra, dec, t['ra'], t['dec'], cr.R_KNN, 3, what='ps1')
        for i in range(ra.size):
            for s in range(3):
                j = idx[i, s]
                if j < 0:
                    continue
                out[i].update({f'objectidps{s + 1}': int(t['objid'][j]), f'sgscore{s + 1}': float(t['ps_score'][j]),
                               f'distpsnr{s + 1}': float(sep[i, s]), f'psgmag{s + 1}': float(t['gMeanPSFMag'][j]),
                               f'psrmag{s + 1}': float(t['rMeanPSFMag'][j]), f'psimag{s + 1}': float(t['iMeanPSFMag'][j]),
                               f'pszmag{s + 1}': float(t['zMeanPSFMag'][j])})
    if 'legacysurvey' in tabs:
        t = tabs['legacysurvey']
        idx, sep, _ = cr.knn_ref(ra, dec, t['ra'], t['dec'], cr.R_KNN, 3, what='legacysurvey')
        mag = lambda f: 0.0 if f <= 0 else float(-2.5 * np.log10(f) + 22.5)
        for i in range(ra.size):
            for s in range(3):
                j = idx[i, s]
                if j < 0:
                    continue
                n = s + 1
                out[i].update({f'lsdistnr{n}': float(sep[i, s]), f'lsobjectid{n}': int(t['OBJID'][j]), f'lstype{n}': str(t['TYPE'][j]),
                               f'lsebv{n}': float(t['EBV'][j]), f'lsg{n}': mag(t['FLUX_G'][j]), f'lsr{n}': mag(t['FLUX_R'][j]),
                               f'lsz{n}': mag(t['FLUX_Z'][j]), f'lsw1_{n}': mag(t['FLUX_W1'][j]), f'lsw2_{n}': mag(t['FLUX_W2'][j]),
                               f'lsw3_{n}': mag(t['FLUX_W3'][j]), f'lsw4_{n}': mag(t['FLUX_W4'][j]),
                               f'lsgaiag{n}': float(t['GAIA_PHOT_G_MEAN_MAG'][j]), f'lsgaiap{n}': float(t['PARALLAX'][j]),
                               f'lszphotmean{n}': float(t['z_phot_mean'][j]), f'lszphotmed{n}': float(t['z_phot_median'][j]),
                               f'lszphotstd{n}': float(t['z_phot_std'][j]), f'lszphotl68{n}': float(t['z_phot_l68'][j]),
                               f'lszphotu68{n}': float(t['z_phot_u68'][j]), f'lszphotl95{n}': float(t['z_phot_l95'][j]),
                               f'lszphotu95{n}': float(t['z_phot_u95'][j]), f'lszspec{n}': float(t['z_spec'][j])})
    for name, col, field in (('ztfalerts', 'objectId', 'ztfname'), ('milliquas', 'Name', 'mqid'), ('tns', 'name', 'tnsid')):
        for i in range(ra.size):
            out[i][field] = ''
        if name in tabs:
            t = tabs[name]
            off, idx = cr.within_ref(ra, dec, t['ra'], t['dec'], cr.R_NAME, what=name)
            for i in range(ra.size):
                out[i][field] = ','.join(sorted(set(str(v) for v in t[col][idx[off[i]:off[i + 1]]])))
    return out


DIST_FIELDS = tuple(f'{p}{n}' for p in ('distpsnr', 'lsdistnr') for n in (1, 2, 3))


def assert_xmatch_equal(got, want):
    """Identifiers, types and magnitudes exactly; the distance fields within ``SEP_TOL_ARCSEC``."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w), set(g) ^ set(w)
        for k in w:
            if k in DIST_FIELDS:
                assert abs(g[k] - w[k]) <= ar.SEP_TOL_ARCSEC, (k, g[k], w[k])
            else:
                assert g[k] == w[k] and type(g[k]) is type(w[k]), (k, g[k], w[k])
