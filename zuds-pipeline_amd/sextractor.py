"""Check-images and detection catalogs (``zuds/sextractor.py``).

The SExtractor process is replaced by libzudsmi: ``zm_background`` for the mesh background / rms check-images
(``BACKGROUND_RMS``, ``-BACKGROUND``, ``BACKGROUND``; ``zuds/sextractor.py:21-26``) and ``zm_extract`` for the
catalog and the ``SEGMENTATION`` check-image.  A default call produces check-images only (catalog slot ``None``, no
extraction work): that is what the coadd / subtraction path asks for.  ``catalog=True`` (or a ``segm`` request)
runs the extractor with the operator of ``sextractor.conf`` as DESIGN.md ("Source extraction") states it:
filter ``default.conv``, ``DETECT_THRESH`` 1.5, ``DETECT_MINAREA`` 5, no deblending, no cleaning.  ``deblend=True`` (or
``dict(nthresh=, mincont=)``) opts into the multi-threshold deblending of DESIGN.md ("Deblending"); only then may
``sextractor_kws`` carry ``DEBLEND_NTHRESH`` and ``DEBLEND_MINCONT``.  ``clean=True`` (or ``dict(param=)``) opts into the
CLEAN pass of DESIGN.md ("CLEAN"); only then may ``sextractor_kws`` carry ``CLEAN`` (which must say yes) and
``CLEAN_PARAM``.  ``mask='blank' | 'correct'`` (with ``columns='param'``) opts into the masked second pass of DESIGN.md
("MASK_TYPE"); only then may ``sextractor_kws`` carry ``MASK_TYPE`` (``NONE``, ``BLANK`` or ``CORRECT``), which overrides
the keyword.

``sextractor_kws``: ``DETECT_THRESH``, ``DETECT_MINAREA``, ``FILTER``, ``PHOT_APERTURES`` (one diameter),
``SATUR_LEVEL``, ``BACK_SIZE``, ``BACK_FILTERSIZE`` are honoured; keys that would change something this version does
not do (``DEBLEND_*`` without ``deblend=True``, ``CLEAN*`` without ``clean=True``, ``MASK_TYPE`` without ``mask=``, ``FILTER_NAME``, a ``WEIGHT_TYPE`` other than
``MAP_WEIGHT``, an ``ANALYSIS_THRESH`` different from ``DETECT_THRESH``) raise ``ValueError``; bookkeeping keys are ignored.
``columns='param'`` asks for the wide table (``extract.PARAM_COLUMNS``: every column of ``sextractor.param``); only then
may ``sextractor_kws`` carry ``PHOT_AUTOPARAMS`` (two values).
"""
import os

import numpy as np

from .constants import BAD_SUM, BKG_BOX_SIZE, MASK_BORDER

__all__ = ['prepare_sextractor', 'run_sextractor', 'extraction_settings']

checkimage_map = {'rms': 'BACKGROUND_RMS', 'segm': 'SEGMENTATION',
                  'bkgsub': '-BACKGROUND', 'bkg': 'BACKGROUND'}
_SUPPORTED = ['rms', 'bkgsub', 'bkg']         # what 'all' stands for: the check-images of the background run
_EXTRACTION = ['segm']                         # check-images that need the extractor

_HONOURED = ('DETECT_THRESH', 'DETECT_MINAREA', 'FILTER', 'PHOT_APERTURES', 'SATUR_LEVEL', 'BACK_SIZE',
             'BACK_FILTERSIZE', 'ANALYSIS_THRESH', 'WEIGHT_TYPE')
_REFUSED_PREFIXES = ('DEBLEND_', 'CLEAN')
_REFUSED = ('MASK_TYPE', 'FILTER_NAME')
_IGNORED = ('CATALOG_NAME', 'CATALOG_TYPE', 'PARAMETERS_NAME', 'CHECKIMAGE_TYPE', 'CHECKIMAGE_NAME', 'WEIGHT_IMAGE',
            'FLAG_IMAGE', 'FLAG_TYPE', 'VERBOSE_TYPE', 'NTHREADS', 'MEMORY_OBJSTACK', 'MEMORY_PIXSTACK',
            'MEMORY_BUFSIZE', 'STARNNW_NAME', 'WRITE_XML', 'XML_NAME', 'HEADER_SUFFIX', 'MAG_ZEROPOINT', 'GAIN',
            'GAIN_KEY', 'PIXEL_SCALE', 'SEEING_FWHM', 'SATUR_KEY', 'INTERP_TYPE', 'INTERP_MAXXLAG', 'INTERP_MAXYLAG')


def _yes(v):
    if isinstance(v, str):
        return v.strip().upper() in ('Y', 'YES', 'T', 'TRUE', '1')
    return bool(v)


_DEBLEND_KEYS = {'DEBLEND_NTHRESH': 'nthresh', 'DEBLEND_MINCONT': 'mincont'}


def extraction_settings(sextractor_kws=None, header=None, deblend=False, clean=False, mask=None):
    """Keyword arguments of ``Engine.extract`` from ``sextractor_kws`` and the image header (``SATURATE``).
    ``deblend``: False, True or dict(nthresh=, mincont=); only when it is set are ``DEBLEND_NTHRESH`` and
    ``DEBLEND_MINCONT`` accepted (they override the dict), and the result then carries ``deblend``.
    ``clean``: False, True or dict(param=); only when it is set are ``CLEAN`` (which must say yes: the keyword asked for the
    pass) and ``CLEAN_PARAM`` (which overrides the dict) accepted, and the result then carries ``clean``.
    ``mask``: None, 'blank' or 'correct'; only when it is set is ``MASK_TYPE`` accepted (``NONE``, ``BLANK`` or ``CORRECT``:
    it overrides the keyword, ``NONE`` meaning the plain second pass), and the result then carries ``mask`` ('blank',
    'correct', or None after ``NONE``)."""
    from .extract import clean_settings, deblend_settings, mask_setting
    kws = {str(k).upper(): v for k, v in (sextractor_kws or {}).items()}
    db = deblend_settings(deblend)
    if db is not None:
        for k in [k for k in kws if k in _DEBLEND_KEYS]:
            db[_DEBLEND_KEYS[k]] = kws.pop(k)
        db = deblend_settings(db)
    cl = clean_settings(clean)
    if cl is not None:
        if 'CLEAN' in kws and not _yes(kws.pop('CLEAN')):
            raise ValueError('sextractor_kws: CLEAN says no, but clean= asks for the pass')
        if 'CLEAN_PARAM' in kws:
            cl['param'] = kws.pop('CLEAN_PARAM')
        cl = clean_settings(cl)
    asked = mask_setting(mask) is not None
    mk = mask_setting(mask)
    if asked and 'MASK_TYPE' in kws:
        v = kws.pop('MASK_TYPE')
        if not isinstance(v, str) or v.strip().upper() not in ('NONE', 'BLANK', 'CORRECT'):
            raise ValueError(f'sextractor_kws: MASK_TYPE {v!r} must be NONE, BLANK or CORRECT')
        mk = mask_setting(v)
    for k in kws:
        if k in _REFUSED or k.startswith(_REFUSED_PREFIXES):
            raise ValueError(f'sextractor_kws: {k} would change a step this extractor does not have '
                             f'(deblending needs deblend=True, cleaning clean=True, masking mask=; other filters '
                             f'are not in this version)')
        if k not in _HONOURED and k not in _IGNORED:
            raise ValueError(f'sextractor_kws: unknown key {k}')
    thresh = float(kws.get('DETECT_THRESH', 1.5))
    if 'ANALYSIS_THRESH' in kws and float(kws['ANALYSIS_THRESH']) != thresh:
        raise ValueError('sextractor_kws: ANALYSIS_THRESH must equal DETECT_THRESH (measurements are isophotal at the '
                         'detection threshold)')
    if str(kws.get('WEIGHT_TYPE', 'MAP_WEIGHT')).upper() != 'MAP_WEIGHT':
        raise ValueError('sextractor_kws: WEIGHT_TYPE must be MAP_WEIGHT')
    aper = np.atleast_1d(kws.get('PHOT_APERTURES', 6.0)).astype(float)
    if aper.size != 1:
        raise ValueError('sextractor_kws: PHOT_APERTURES takes one diameter')
    satur = kws.get('SATUR_LEVEL', (header or {}).get('SATURATE', 50000.0))
    out = dict(detect_thresh=thresh, detect_minarea=int(kws.get('DETECT_MINAREA', 5)), filter=_yes(kws.get('FILTER', 'Y')),
               satur_level=float(satur), aper_radius=float(aper[0]) / 2.0)
    if db is not None:
        out['deblend'] = db
    if cl is not None:
        out['clean'] = cl
    if asked:
        out['mask'] = mk
    return out


def prepare_sextractor(image, directory=None, checkimage_type=None,
                       catalog_type='FITS_LDAC', use_weightmap=True, sextractor_kws=None):
    """Parameters of one background run: dict(weight, mesh, filtersize, outnames,
    types) (the reference returns a ``sex`` command line, ``zuds/sextractor.py:29-107``)."""
    sextractor_kws = sextractor_kws or {}
    checkimage_types = np.atleast_1d(checkimage_type or []).tolist()
    if 'all' in checkimage_types:
        checkimage_types = list(_SUPPORTED)
    for t in checkimage_types:
        if t not in checkimage_map:
            raise ValueError(f'Invalid CHECKIMAGE_TYPE "{t}". Must be one of '
                             f'{list(checkimage_map)}.')
    if use_weightmap:
        weight = image.weight_image.data
    else:
        # false weight map: masked pixels (and a 10-pixel border of raw science
        # frames) are excluded from the background statistics
        # (zuds/sextractor.py:80-96)
        weight = np.ones(image.mask_image.data.shape, dtype='<f4')
        weight[(image.mask_image.data & BAD_SUM) > 0] = 0
        if image.basename.endswith('sciimg.fits'):
            weight[:MASK_BORDER] = 0
            weight[-MASK_BORDER:] = 0
            weight[:, :MASK_BORDER] = 0
            weight[:, -MASK_BORDER:] = 0
    base = image.local_path if image.ismapped else image.basename
    outnames = [base.replace('.fits', f'.{t}.fits') for t in checkimage_types]
    return dict(weight=weight, mesh=int(sextractor_kws.get('BACK_SIZE', BKG_BOX_SIZE)),
                filtersize=int(sextractor_kws.get('BACK_FILTERSIZE', 3)),
                outnames=outnames, types=checkimage_types)


def measurement_settings(sextractor_kws=None):
    """(``sextractor_kws`` without the keys of the second pass, keyword arguments of that pass) for ``columns='param'``."""
    rest, auto = {}, None
    for k, v in (sextractor_kws or {}).items():
        if str(k).upper() == 'PHOT_AUTOPARAMS':
            auto = v
        else:
            rest[k] = v
    if auto is None:
        return rest, {}
    if isinstance(auto, str):
        auto = auto.split(',')
    auto = np.atleast_1d(auto).astype(float)
    if auto.size != 2 or not (auto > 0).all():
        raise ValueError('sextractor_kws: PHOT_AUTOPARAMS takes two positive values (Kron factor, minimum radius)')
    return rest, dict(kron_fact=float(auto[0]), kron_min_radius=float(auto[1]))


def _extract(image, call, sub, sextractor_kws, columns='isophotal', deblend=False, clean=False, mask=None):
    """(PipelineFITSCatalog, segmentation map) of the background-subtracted plane ``sub``: noise = the image's
    rms_image, bad = weight 0, flags = the mask."""
    from .catalog import PipelineFITSCatalog
    from .engine import get_engine
    if call['catalog_type'] != 'FITS_LDAC':
        raise ValueError(f'catalog_type "{call["catalog_type"]}": only FITS_LDAC catalogs are written')
    if columns == 'param':
        sextractor_kws, second = measurement_settings(sextractor_kws)
        second['columns'] = 'param'
    elif columns == 'isophotal':
        second = {}
    else:
        raise ValueError(f"columns={columns!r}: 'isophotal' or 'param'")
    from .extract import extract_options
    extract_options(columns, deblend, clean, mask)
    settings = extraction_settings(sextractor_kws, image.header, deblend=deblend, clean=clean, mask=mask)
    settings.update(second)
    mask = getattr(image, 'mask_image', None)
    try:
        wcs = image.wcs
    except (ValueError, KeyError, AttributeError):
        wcs = None
    tab, segm = get_engine().extract(sub, image.rms_image.data, bad=call['weight'] == 0,
                                     flag=None if mask is None else mask.data, wcs=wcs, **settings)
    cat = PipelineFITSCatalog()
    base = image.local_path if image.ismapped else image.basename
    cat.basename = os.path.basename(base).replace('.fits', '.cat')
    cat.data = tab
    cat.deblend = settings.get('deblend')
    cat.clean = settings.get('clean')
    cat.mask = settings.get('mask')
    cat.header = dict(image.header or {})
    cat.header_comments = dict(image.header_comments or {})
    if image.ismapped:
        cat.map_to_local_file(base.replace('.fits', '.cat'))
        cat.save()
    return cat, segm


def run_sextractor(image, checkimage_type=None, catalog_type='FITS_LDAC', tmpdir='/tmp',
                   use_weightmap=True, sextractor_kws=None, catalog=False, columns='isophotal', deblend=False,
                   clean=False, mask=None):
    """Produce the requested check-images as FITSImage objects, written next to
    the image when it is mapped (``zuds/sextractor.py:110-150``).  The returned
    list starts with the catalog slot: ``None``, or with ``catalog=True`` (or when ``segm`` is among the
    check-images) the ``PipelineFITSCatalog`` of the image; ``columns='param'``: with the wide table; ``deblend``: with
    multi-threshold deblending, ``clean``: with the CLEAN pass, ``mask='blank' | 'correct'`` (needs ``columns='param'``):
    with the masked second pass (``Engine.extract``)."""
    from .engine import get_engine
    from .image import FITSImage
    call = prepare_sextractor(image, None, checkimage_type=checkimage_type,
                              catalog_type=catalog_type, use_weightmap=use_weightmap,
                              sextractor_kws=sextractor_kws)
    call['catalog_type'] = catalog_type
    extracting = bool(catalog) or any(t in _EXTRACTION for t in call['types'])
    want = {'bkg': 'bkg', 'rms': 'rms', 'bkgsub': 'sub'}
    wanted = [want[t] for t in call['types'] if t in want]
    if extracting and 'sub' not in wanted:
        wanted.append('sub')
    bkg, rms, sub, stats = get_engine().background(
        image.data, call['weight'], mesh=call['mesh'], filtersize=call['filtersize'],
        want=tuple(wanted))
    planes = {'bkg': bkg, 'rms': rms, 'bkgsub': sub}
    result = [None]
    if extracting:
        result[0], planes['segm'] = _extract(image, call, sub, sextractor_kws, columns, deblend, clean, mask)
    for t, name in zip(call['types'], call['outnames']):
        product = FITSImage()
        product.basename = os.path.basename(name)
        product.data = planes[t]
        product.header = dict(image.header)
        product.header_comments = dict(image.header_comments or {})
        for prop in ('field', 'ccdid', 'qid', 'fid'):
            setattr(product, prop, getattr(image, prop, None))
        if image.ismapped:
            product.map_to_local_file(name)
            product.save()
        result.append(product)
    return result
