"""Image / weight / rms object model (``zuds/image.py``), DB-free.

``weight_image`` and ``rms_image`` keep the reference's lazy semantics; the maps
the reference obtains from SExtractor check-images (``BACKGROUND_RMS``,
``-BACKGROUND``, ``BACKGROUND``; ``zuds/image.py:95-129,206,212-226``) come from
libzudsmi's mesh-background kernels instead.
"""
import os
from pathlib import Path

import numpy as np

from .constants import APER_KEY, BIG_RMS
from .fitsfile import HasWCS

__all__ = ['FITSImage', 'CalibratableImageBase', 'CalibratableImage',
           'CalibratedImage', 'ScienceImage']


class FITSImage(HasWCS):
    """A FITS file whose data member is an image (``zuds/image.py:28-88``)."""

    @property
    def datatype(self):
        return 'float' if 'float' in self.data.dtype.name else 'int'


class CalibratableImageBase(FITSImage):
    __diskmapped_cached_properties__ = ['_path', '_data', '_weightimg', '_bkgimg',
                                        '_filter_kernel', '_rmsimg', '_threshimg',
                                        '_segmimg', '_sourcelist', '_bkgsubimg']

    mask_image = None
    field = ccdid = qid = fid = None

    def _call_source_extractor(self, checkimage_type=None, tmpdir='/tmp',
                               use_weightmap=True, sextractor_kws=None, catalog=False, columns='isophotal',
                               deblend=False, clean=False, mask=None):
        """Produce the requested check-images and, with ``catalog=True``, the detection catalog
        (``zuds/image.py:103-134``)."""
        from . import sextractor
        results = sextractor.run_sextractor(self, checkimage_type=checkimage_type,
                                            tmpdir=tmpdir, use_weightmap=use_weightmap,
                                            sextractor_kws=sextractor_kws, catalog=catalog, columns=columns,
                                            deblend=deblend, clean=clean, mask=mask)
        for result in results:
            if result is None:          # the catalog slot of a call that asked for check-images only
                continue
            if result.basename.endswith('.cat'):
                self.catalog = result
            elif result.basename.endswith('.segm.fits'):
                self._segmimg = result
            elif result.basename.endswith('.rms.fits'):
                self._rmsimg = result
            elif result.basename.endswith('.bkgsub.fits'):
                self._bkgsubimg = result
            elif result.basename.endswith('.bkg.fits'):
                self._bkgimg = result

    def _derived(self, suffix, data):
        im = FITSImage()
        im.basename = self.basename.replace('.fits', suffix)
        im.data = data
        im.header = self.header
        im.header_comments = self.header_comments
        if self.ismapped:
            im.map_to_local_file(os.path.join(os.path.dirname(self.local_path), im.basename))
            im.save()     # guarantees the mapped file exists
        return im

    @property
    def weight_image(self):
        """Inverse-variance map: 1 / rms^2, 0 where the mask is bad or the pixel
        is within 10 % of SATURATE (``zuds/image.py:136-171``)."""
        try:
            return self._weightimg
        except AttributeError:
            from . import objdev
            if objdev.can_derive(self) and (not hasattr(self, '_rmsimg') or
                                            (self._rmsimg.ismapped and '_data' not in self._rmsimg.__dict__)):
                # a frame on disk without maps: derived on the device planes (objdev.derive_maps), same files
                objdev.derive_maps(self, want_weight=True)
                return self._weightimg
            ind = self.mask_image.boolean.data
            wgt = np.empty_like(ind, dtype='<f4')
            wgt[~ind] = 1 / self.rms_image.data[~ind] ** 2
            wgt[ind] = 0.
            if 'SATURATE' in self.header:
                wgt[self.data >= 0.9 * self.header['SATURATE']] = 0.
            self._weightimg = self._derived('.weight.fits', wgt)
        return self._weightimg

    @property
    def rms_image(self):
        """1 / sqrt(weight) with BIG_RMS on bad pixels when a weight map exists,
        else the mesh BACKGROUND_RMS map (``zuds/image.py:173-208``)."""
        try:
            return self._rmsimg
        except AttributeError:
            if hasattr(self, '_weightimg'):
                ind = self.mask_image.boolean.data
                rms = np.empty_like(ind, dtype='<f4')
                with np.errstate(divide='ignore'):
                    rms[~ind] = 1 / np.sqrt(self.weight_image.data[~ind])
                rms[ind] = BIG_RMS
                if 'SATURATE' in self.header:
                    rms[self.data >= 0.9 * self.header['SATURATE']] = BIG_RMS
                self._rmsimg = self._derived('.rms.fits', rms)
                return self._rmsimg
            else:
                from . import objdev
                if objdev.can_derive(self):
                    objdev.derive_maps(self, want_weight=False)
                else:
                    self._call_source_extractor(checkimage_type=['rms'], use_weightmap=False)
        return self._rmsimg

    @property
    def background_image(self):
        try:
            return self._bkgimg
        except AttributeError:
            self._call_source_extractor(checkimage_type=['bkg'])
        return self._bkgimg

    @property
    def background_subtracted_image(self):
        try:
            return self._bkgsubimg
        except AttributeError:
            self._call_source_extractor(checkimage_type=['bkgsub'])
        return self._bkgsubimg

    @classmethod
    def from_file(cls, fname, use_existing_record=True, load_others=True):
        """Also picks up sibling ``.weight/.rms/.bkg/.bkgsub.fits`` files
        (``zuds/image.py:236-262``)."""
        obj = super().from_file(fname, use_existing_record=use_existing_record)
        d = Path(fname).parent
        if load_others:
            for suffix, attr in (('.weight.fits', '_weightimg'), ('.rms.fits', '_rmsimg'),
                                 ('.bkg.fits', '_bkgimg'), ('.thresh.fits', '_threshimg'),
                                 ('.bkgsub.fits', '_bkgsubimg'), ('.segm.fits', '_segmimg')):
                path = d / obj.basename.replace('.fits', suffix)
                if path.exists() and path.name != obj.basename:
                    setattr(obj, attr, FITSImage.from_file(f'{path}'))
        for key, attr in (('FIELD', 'field'), ('FIELDID', 'field'), ('CCDID', 'ccdid'),
                          ('QID', 'qid'), ('FID', 'fid'), ('FILTERID', 'fid')):
            if obj.header and key in obj.header and getattr(obj, attr, None) is None:
                setattr(obj, attr, obj.header[key])
        return obj

    @property
    def mjd(self):
        from .utils import get_time
        return get_time(self, 'mjd')


class CalibratableImage(CalibratableImageBase):
    """``zuds/image.py:265-330`` without the ORM columns."""

    def basic_map(self, quiet=True):
        pass


class CalibratedImage(CalibratableImage):
    """An image with MAGZP / APCOR calibration (``zuds/image.py:333-432``)."""

    @property
    def magzp(self):
        return self.header['MAGZP'] + self.header[APER_KEY]

    @property
    def forced_photometry(self):
        """The ``ForcedPhotometry`` points made on this image so far (the reference's relationship, a plain list)."""
        return self.__dict__.setdefault('_forced_photometry', [])

    @property
    def psf_model(self):
        """The PSF model of this image (``psf.PSFModel``): the one ``build_psf`` made or that was assigned, else the sibling
        ``*.psf.fits`` when there is one, else None."""
        if '_psf_model' not in self.__dict__:
            from .psf import PSFModel
            path = getattr(self, 'local_path', None)
            sibling = None if not path else str(path).replace('.fits', '.psf.fits')
            self.__dict__['_psf_model'] = PSFModel.from_file(sibling) if sibling and os.path.exists(sibling) else None
        return self.__dict__['_psf_model']

    @psf_model.setter
    def psf_model(self, model):
        self.__dict__['_psf_model'] = model

    def build_psf(self, stars=None, psf_kws=None, engine=None):
        """Build the PSF model from the image's own stars, or a catalogue's (``psf.build_psf``; ``psf_kws``: ``-KEY value``
        pairs as ``psf.psf_settings`` takes them; ``PSFREF_NAME`` names the catalogue when ``stars`` is None).  The model
        becomes ``psf_model`` and its cards go into the header; nothing is saved.  Returns the dict of ``psf.build_psf``."""
        from . import psf as _psf
        st = _psf.psf_settings(psf_kws)
        ref = st.pop('psfref')
        res = _psf.build_psf(self, stars=stars if stars is not None else ref, engine=engine, **st)
        self.psf_model = res['psf']
        if self.header_comments is None:
            self.header_comments = {}
        for key, value, comment in res['cards']:
            self.header[key] = value
            self.header_comments[key] = comment
        return res

    def force_photometry(self, sources, assume_background_subtracted=False, use_cutout=False, direct_load=None,
                         method='aperture', fit_sky=None):
        """Force aperture photometry at the locations of ``sources`` (``zuds/image.py:344-377``): one
        ``ForcedPhotometry`` per source, in order.  Assumes that calibration has already been done.  The points are
        returned, not recorded: the caller adds them to ``forced_photometry`` as the reference adds them to its
        session.

        ``method='psf'``: a fit of ``psf_model`` in place of the aperture sum (``psf.psf_photometry``), with ``zp = MAGZP +
        PSFCOR``; ``fit_sky`` defaults to fitting a constant unless ``assume_background_subtracted``.  ``flags`` are then
        those of the fit (``psf.PSF_FLAGS``)."""
        from .photometry import ForcedPhotometry, aperture_photometry
        if method not in ('aperture', 'psf'):
            raise ValueError(f'force_photometry: method {method!r} is neither \'aperture\' nor \'psf\'')
        sources = np.atleast_1d(sources)
        ra = [source.ra for source in sources]
        dec = [source.dec for source in sources]
        if method == 'psf':
            from .psf import psf_photometry
            model = self.psf_model
            if model is None:
                raise RuntimeError(f'"{self.basename}" has no PSF model: build_psf() it, or put its *.psf.fits beside it')
            cor = model.cards.get('PSFCOR', self.header.get('PSFCOR'))
            if cor is None or 'MAGZP' not in self.header:
                raise RuntimeError(f'"{self.basename}" has no MAGZP / PSFCOR: the PSF fluxes would have no zero point')
            x, y = self.wcs.all_world2pix(ra, dec, 0)
            sky = (not assume_background_subtracted) if fit_sky is None else fit_sky
            res = psf_photometry(self, x, y, model, fit_sky=int(bool(sky)))
            jd = self.header.get('OBSJD')
            fc = 'z' + str(self.header['FILTER'])[-1] if 'FILTER' in self.header else None
            return [ForcedPhotometry(flux=float(res['flux'][k]), fluxerr=float(res['fluxerr'][k]), flags=int(res['flags'][k]),
                                     image=self, ra=r, dec=d, source=source, zp=float(self.header['MAGZP']) + float(cor),
                                     obsjd=None if jd is None else float(jd), filtercode=fc)
                    for k, (source, r, d) in enumerate(zip(sources, ra, dec))]
        result = aperture_photometry(self, ra, dec, apply_calibration=True,
                                     assume_background_subtracted=assume_background_subtracted,
                                     use_cutout=use_cutout, direct_load=direct_load)
        photometry = []
        for k, (source, r, d) in enumerate(zip(sources, ra, dec)):
            photometry.append(ForcedPhotometry(
                flux=float(result['flux'][k]), fluxerr=float(result['fluxerr'][k]), flags=int(result['flags'][k]),
                image=self, ra=r, dec=d, source=source, zp=float(result['zp'][k]),
                obsjd=None if result['obsjd'] is None else float(result['obsjd'][k]),
                filtercode=None if result['filtercode'] is None else str(result['filtercode'][k])))
        return photometry

    def unphotometered_sources(self, sources):
        """The ``sources`` that lie inside this image's footprint and have no ``ForcedPhotometry`` on it yet.

        The reference's property (``zuds/image.py:408-432``) asks the database: ``q3c_poly_query`` of every ``Source``
        against the image's polygon, outer-joined to ``forcedphotometry``.  There is no database here, so the candidates
        are handed in; the polygon test is ``footprint_join`` (``zm_footprint_join``: the same spherical quadrilateral,
        on the GPU) and the outer join is a look at ``forced_photometry`` of this image."""
        from .lightcurve import footprint_join
        sources = list(np.atleast_1d(sources))
        if not sources:
            return []
        _, idx = footprint_join([self.wcs], [s.ra for s in sources], [s.dec for s in sources])
        have = {id(p.source) for p in self.forced_photometry}
        return [sources[k] for k in idx.tolist() if id(sources[k]) not in have]


class ScienceImage(CalibratedImage):
    """A single-epoch IPAC science frame (``zuds/image.py:435-567``)."""

    @property
    def obsjd(self):
        from .utils import get_time
        return get_time(self, 'jd')
