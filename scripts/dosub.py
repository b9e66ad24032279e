#!/usr/bin/env python
"""Make subtractions: the driver of the reference's ``scripts/dosub.py``
(``do_one``), database-free.

usage: dosub.py images.txt ref.fits [--detect [--stamps] [--param-columns [--mask-type blank|correct]] [--deblend]
                                        [--clean [--clean-param X]]
                                        [--rb-model BASE [--rb-cut X]]] [--maglim] [--psf [--psfref stars.cat]]
images.txt lists science image paths (masks as ``*mskimg.fits``; a ``.weight.fits``
or ``.rms.fits`` sibling is used when present, else the mesh background RMS map).
``ref.fits`` needs ``ref.mask.fits`` and ``ref.weight.fits`` next to it.
With ``--maglim`` every subtraction gets a ``MAGLIM`` card measured on its own rms plane with the ``MAGZP`` and ``APCOR4``
it copied from the science image (``write_maglim``: the median noise in r = 3 px apertures on a lattice, 5 sigma); a
subtraction without a zero point is left without the card, with a warning.
With ``--psf`` the PSF model of every science image is built from its own stars, or with ``--psfref stars.cat`` from the
stars of a FITS_LDAC catalogue (``CalibratedImage.build_psf``; DESIGN.md, "PSF photometry"), and written as
``<sci>.psf.fits`` and - the difference image has the science frame's PSF - copied as ``sub.*.psf.fits``; its cards
(``PSFCOR``, ``PSFCORUN``, ``PSFNSTAR``, ``PSFHALF``, ``PSFFITR``, ``PSFFWHM``, ``ZMPSF``) go into the subtraction's header.
``dophot.py --psf`` reads the model beside each subtraction.  Without ``--psf`` nothing changes.
With ``--detect`` every subtraction also gets its detection catalog (``sub.*.cat``, FITS_LDAC) and its filtered
detections (``PipelineFITSCatalog.from_image`` -> ``Detection.from_catalog``, dosub.py:109-131).
With ``--param-columns`` (needs ``--detect``) the catalog holds every column of ``sextractor.param`` (``MAG_AUTO``,
``XWIN_WORLD``, ... : ``extract.PARAM_COLUMNS``) and the ds9 region file ``sub.*.reg`` is written next to it
once the detections have been filtered (``PipelineRegionFile.from_catalog``: green where ``GOODCUT`` is set, red
elsewhere).
With ``--mask-type blank|correct`` (needs ``--param-columns``) the Kron, windowed and aperture sums of the wide table leave
out the pixels of other objects and the object's own bad pixels, or with ``correct`` take their mirrors about the centre
instead (``MASK_TYPE`` of ``sextractor.conf``; the map is the final one, after ``--deblend`` and ``--clean``): the catalog's
header says ``ZMMASKTY = 'BLANK'`` or ``'CORRECT'``, its table carries ``NREPL_*`` / ``NLOST_*``, and the S/N cut reads the
masked ``FLUX_APER`` / ``FLUXERR_APER``.
With ``--deblend`` (needs ``--detect``) the extraction deblends (``DEBLEND_NTHRESH`` 32, ``DEBLEND_MINCONT`` 0.005): the
catalog's header says ``ZMDEBLND = T`` and its table carries ``PARENT_NUMBER``.
With ``--clean`` (needs ``--detect``) the extraction ends with the CLEAN pass (``CLEAN_PARAM`` 1.0, or ``--clean-param X``):
the catalog's header says ``ZMCLEAN = T`` and ``ZMCLNPAR``, and its table carries ``NMERGED``.
With ``--stamps`` (needs ``--detect``) every detection also gets its three thumbnails - difference, new and reference
image on the reference image's grid (``Thumbnail.from_detections``, dosub.py:133-150) - and ``sub.*.stamps.fits`` is
written next to the catalog: the zero-filled blocks ``[n, 3, 63, 63]`` (sub, new, ref) and a table with ``ra``, ``dec``,
``x0``, ``y0`` and the shape of the stamp trimmed to the grid.
With ``--rb-model BASE`` (needs ``--detect``) the filter ends with the real / bogus network stored as
``BASE.architecture.json`` + ``BASE.weights.npz`` (``realbogus.load_model``): ``rb`` is the score, and rows below
``--rb-cut X`` - or ``RB_CUT`` of the frame's ``FID`` / ``FILTERID`` card - are cut (``filterobjects.py:196-240``).  A frame
without that card and no ``--rb-cut`` is an error.
"""
import os
import sys
import time
import traceback

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zuds_amd as zuds

zuds.init_db()


MAX_DETS = 50


class PredecessorError(Exception):
    pass


def write_stamp_blocks(out, blocks, ra, dec, x0, y0, trimmed):
    """The stamps file: primary array ``blocks`` [n, 3, S, S] (sub, new, ref; zero outside the grid) and one row per
    detection: ``ra``, ``dec``, ``x0``, ``y0`` and ``trimmed`` = (nx, ny) of the stamp trimmed to the grid."""
    import numpy as np
    n, size = len(blocks), blocks.shape[-1]
    tab = np.zeros(n, dtype=[('ra', 'f8'), ('dec', 'f8'), ('x0', 'i4'), ('y0', 'i4'), ('nx_trim', 'i4'), ('ny_trim', 'i4')])
    for k in range(n):
        tab[k] = (ra[k], dec[k], x0[k], y0[k], trimmed[k][0], trimmed[k][1])
    zuds.fits.write_image_table(out, blocks, tab, {'STAMPSZ': size, 'NDET': n},
                                {'STAMPSZ': 'stamp size in pixels', 'NDET': 'detections'})
    return out


def write_stamps(sub, detections, stamps, size=None):
    """``<sub>.stamps.fits``: primary array [n, 3, S, S] (the stamps of each detection, zero outside the grid) and one
    row per detection."""
    import numpy as np
    size = size or zuds.CUTOUT_SIZE
    n = len(detections)
    blocks = np.zeros((n, 3, size, size), np.float32)
    x0, y0, trimmed = [], [], []
    for k, d in enumerate(detections):
        for p, s in enumerate(stamps[3 * k:3 * k + 3]):
            a = np.flipud(s.array)                       # the stamp as stored: trimmed to the grid
            ox, oy = max(s.x0, 0) - s.x0, max(s.y0, 0) - s.y0
            blocks[k, p, oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
        s = stamps[3 * k]
        x0.append(s.x0)
        y0.append(s.y0)
        trimmed.append((s.shape[1], s.shape[0]))
    return write_stamp_blocks(sub.local_path.replace('.fits', '.stamps.fits'), blocks, [d.ra for d in detections],
                              [d.dec for d in detections], x0, y0, trimmed)


def do_one(fn, sciclass, subclass, refname, tmpdir='/tmp', detect=False, stamps=False, param_columns=False, rb_model=None,
           rb_cut=None, deblend=False, clean=False, mask=None, maglim=False, psf=False, psfref=None):
    tstart = time.time()
    sstart = time.time()
    sci = sciclass.from_file(fn)
    maskname = fn.replace('sciimg', 'mskimg') if 'sciimg' in fn else fn.replace('.fits', '.mask.fits')
    sci.mask_image = zuds.MaskImage.from_file(maskname)
    weightname = fn.replace('.fits', '.weight.fits')
    rmsname = fn.replace('.fits', '.rms.fits')
    if os.path.exists(weightname):
        sci._weightimg = zuds.FITSImage.from_file(weightname)
    elif os.path.exists(rmsname):
        sci._rmsimg = zuds.FITSImage.from_file(rmsname)
    else:
        if sciclass == zuds.ScienceImage:
            _ = sci.rms_image       # mesh BACKGROUND_RMS map (dosub.py:42-44)
        else:
            raise RuntimeError(f'Cannot produce a subtraction for {fn},'
                               f' the image has no weightmap or rms map.')
    sstop = time.time()
    print(f'sci: {sstop - sstart:.2f} sec to load  {sci.basename}', flush=True)

    if not os.path.exists(refname):
        raise RuntimeError(f'Ref {refname} does not exist. Skipping...')
    rstart = time.time()
    ref = zuds.ReferenceImage.from_file(refname, load_others=False)
    ref.mask_image = zuds.MaskImage.from_file(refname.replace('.fits', '.mask.fits'))
    ref._weightimg = zuds.FITSImage.from_file(refname.replace('.fits', '.weight.fits'))
    rstop = time.time()
    print(f'ref: {rstop - rstart:.2f} sec to load ref for {sci.basename}', flush=True)

    outname = zuds.sub_name(sci.local_path, ref.local_path)
    if os.path.exists(outname):     # checkpoint by name (dosub.py:85-94)
        raise PredecessorError(f'{os.path.basename(outname)} already has a predecessor')

    substart = time.time()
    sub = subclass.from_images(sci, ref, data_product=False, tmpdir=tmpdir, refined=True)
    substop = time.time()
    print(f'sub: {substop - substart:.2f} sec to make {sub.basename}', flush=True)
    if maglim:
        # MAGLIM from the subtraction's own rms plane and the MAGZP / APCOR4 it copied from the science image; without a
        # zero point the card is skipped with a warning
        zuds.write_maglim(sub)
    if psf:
        # the model of the science image (with -c t -n i the difference image has its PSF), copied beside the subtraction
        pstart = time.time()
        model = sci.build_psf(stars=psfref)['psf']
        model.save(sci.local_path.replace('.fits', '.psf.fits'))
        model.save(sub.local_path.replace('.fits', '.psf.fits'))
        sub.psf_model = model
        if sub.header_comments is None:
            sub.header_comments = {}
        for key, value in model.cards.items():
            sub.header[key] = value
            sub.header_comments[key] = zuds.psf.CARD_COMMENTS.get(key, '')
        if sub.ismapped:
            sub.save()
        print(f'psf: {time.time() - pstart:.2f} sec to model {sci.basename} ({model.cards["PSFNSTAR"]} stars, '
              f'PSFCOR {model.cards["PSFCOR"]:.4f})', flush=True)

    detections = None
    if detect:
        catstart = time.time()
        cat = zuds.PipelineFITSCatalog.from_image(sub, columns='param' if param_columns else 'isophotal',
                                                   deblend=deblend, clean=clean, mask=mask)
        catstop = time.time()
        print(f'cat: {catstop - catstart:.2f} sec to make catalog for {sub.basename}', flush=True)
        dstart = time.time()
        if rb_model is not None:
            zuds.rb_cut_for(getattr(sub, 'fid', None), rb_cut)      # a missing FID card and no --rb-cut: an error, here
        detections = zuds.Detection.from_catalog(cat, filter=True, rb_model=rb_model, rb_cut=rb_cut)
        if param_columns:
            zuds.PipelineRegionFile.from_catalog(cat)     # behind the cuts: green / red by GOODCUT
        if len(detections) > MAX_DETS:
            raise zuds.TooManyDetectionsError(f'Error: {len(detections)} detections (>{MAX_DETS}) '
                                              f'on "{sub.basename}", something wrong with the image probably')
        dstop = time.time()
        print(f'det: {dstop - dstart:.2f} sec to make detections for {sub.basename}', flush=True)

    thumbs = None
    if detect and stamps:
        stampstart = time.time()
        thumbs = zuds.Thumbnail.from_detections(detections, sub) if detections else []
        write_stamps(sub, detections, thumbs)
        stampstop = time.time()
        print(f'stamp: {stampstop - stampstart:.2f} sec to make stamps for {sub.basename}', flush=True)

    cleanstart = time.time()
    sci.unmap()
    cleanstop = time.time()
    tstop = time.time()
    print(f'clean: took {cleanstop - cleanstart} sec to clean up after {sub.basename}"', flush=True)
    print(f'took {tstop - tstart} sec to make "{sub.basename}"', flush=True)
    if detect and stamps:
        return sub, detections, thumbs
    if detect:
        return sub, detections
    return sub


def main(argv):
    detect = '--detect' in argv
    maglim = '--maglim' in argv
    psf = '--psf' in argv
    stamps = '--stamps' in argv
    param_columns = '--param-columns' in argv
    if stamps and not detect:
        print('--stamps needs --detect', file=sys.stderr)
        return 2
    if param_columns and not detect:
        print('--param-columns needs --detect', file=sys.stderr)
        return 2
    deblend = '--deblend' in argv
    if deblend and not detect:
        print('--deblend needs --detect', file=sys.stderr)
        return 2
    clean = '--clean' in argv
    if (clean or '--clean-param' in argv) and not detect:
        print('--clean needs --detect', file=sys.stderr)
        return 2
    if '--clean-param' in argv and not clean:
        print('--clean-param needs --clean', file=sys.stderr)
        return 2
    argv = list(argv)
    rb_model = rb_cut = mask = psfref = None
    for flag in ('--rb-model', '--rb-cut', '--clean-param', '--mask-type', '--psfref'):
        if flag in argv:
            k = argv.index(flag)
            if k + 1 >= len(argv):
                print(f'{flag} needs a value', file=sys.stderr)
                return 2
            value = argv[k + 1]
            del argv[k:k + 2]
            if flag == '--rb-model':
                rb_model = value
            elif flag == '--psfref':
                psfref = value
            elif flag == '--mask-type':
                if value not in ('blank', 'correct'):
                    print(f'--mask-type: {value!r} is neither blank nor correct', file=sys.stderr)
                    return 2
                mask = value
            elif flag == '--clean-param':
                try:
                    clean = zuds.clean_settings(dict(param=float(value)))
                except ValueError as exc:
                    print(f'--clean-param: {exc}', file=sys.stderr)
                    return 2
            else:
                rb_cut = float(value)
    if psfref is not None and not psf:
        print('--psfref needs --psf', file=sys.stderr)
        return 2
    if mask is not None and not param_columns:
        print('--mask-type needs --param-columns', file=sys.stderr)
        return 2
    if (rb_model or rb_cut is not None) and not detect:
        print('--rb-model needs --detect', file=sys.stderr)
        return 2
    if rb_cut is not None and not rb_model:
        print('--rb-cut needs --rb-model', file=sys.stderr)
        return 2
    if rb_model:
        rb_model = zuds.load_model(rb_model)
    args = [a for a in argv if a not in ('--detect', '--stamps', '--param-columns', '--deblend', '--clean', '--maglim', '--psf')]
    infile = args[0]
    refname = args[1]
    subclass = zuds.SingleEpochSubtraction
    sciclass = zuds.ScienceImage
    imgs = zuds.get_my_share_of_work(infile)
    for fn in imgs:
        try:
            do_one(str(fn), sciclass, subclass, refname, detect=detect, stamps=stamps, param_columns=param_columns,
                   rb_model=rb_model, rb_cut=rb_cut, deblend=deblend, clean=clean, mask=mask, maglim=maglim, psf=psf, psfref=psfref)
        except Exception:
            traceback.print_exception(*sys.exc_info())
            continue
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
