"""Detection catalogs (``zuds/catalog.py``), DB-free.

``PipelineFITSCatalog.from_image`` runs the source extractor of libzudsmi (``zm_extract``) where the reference runs
SExtractor; the table holds the columns that are computed (``extract.CATALOG_COLUMNS``) and no others.  On disk a
catalog is a FITS_LDAC file, as the reference asks SExtractor for (``catalog_type='FITS_LDAC'``): the object table is
HDU 2.  ``from_image(..., columns='param')`` asks for the wide table (``extract.PARAM_COLUMNS``: every column of
``sextractor.param``), which ``PipelineRegionFile.from_catalog`` needs.  ``from_image(..., deblend=, clean=)`` pass the
two opt-in steps of the extractor on (``Engine.extract``); the table's header says which ran (``ZMDEBLND``, ``ZMCLEAN`` and
their parameters), and ``from_file`` reads that back into ``cat.deblend`` / ``cat.clean``.  ``from_image(...,
columns='param', mask='blank' | 'correct')`` asks for the masked second pass ("MASK_TYPE"): the wide table's
header then says ``ZMMASKTY = 'BLANK'`` or ``'CORRECT'`` instead of ``'NONE'``, read back into ``cat.mask``.
"""
from pathlib import Path

import numpy as np

from . import fits as _fits
from .constants import BAD_SUM, GROUP_PROPERTIES
from .file import File, UnmappedFileError

__all__ = ['PipelineFITSCatalog', 'PipelineRegionFile']

# what the extraction behind a catalog did not do, stated in its header (a catalog made with deblend= or clean=:
# header_cards; the comments are those of the version that had neither step, kept so that a default catalog's bytes stay)
HEADER_CARDS = [('ZMDEBLND', False, 'multi-threshold deblending (not in this version)'),
                ('ZMCLEAN', False, 'CLEAN pass (not in this version)')]

# ... and of a wide table: the Kron and windowed sums do not mask the pixels of other objects
WIDE_CARDS = [('ZMMASKTY', 'NONE', 'MASK_TYPE of the Kron and windowed sums')]


def wide_cards(mask=None):
    """The cards of a wide table; ``mask``: None, 'blank' or 'correct' (the masked second pass the catalog was made with)."""
    if not mask:
        return list(WIDE_CARDS)
    return [('ZMMASKTY', str(mask).upper(), 'MASK_TYPE of the Kron, windowed and aperture sums')]


def header_cards(deblend=None, clean=None):
    """The cards every catalog's header states the extractor's steps with; ``deblend``: None, or the
    dict(nthresh=, mincont=) the catalog was made with; ``clean``: None, or its dict(param=)."""
    cards = list(HEADER_CARDS)
    if deblend:
        cards[:1] = [('ZMDEBLND', True, 'multi-threshold deblending'), ('ZMDBNTHR', int(deblend['nthresh']), 'DEBLEND_NTHRESH'),
                     ('ZMDBMINC', float(deblend['mincont']), 'DEBLEND_MINCONT')]
    if clean:
        cards[-1:] = [('ZMCLEAN', True, 'CLEAN pass'), ('ZMCLNPAR', float(clean['param']), 'CLEAN_PARAM')]
    return cards


# the two lines every region file starts with (ds9: global properties, then the coordinate system)
REGION_HEAD = ('global color=green dashlist=8 3 width=1 font="helvetica 10 normal" select=1 highlite=1 dash=0 fixed=0 '
               'edit=1 move=1 delete=1 include=1 source=1\nicrs\n')


class PipelineRegionFile(File):
    """The ds9 region file of a catalog, ``<catalog>.reg`` next to it (the product of ``zuds/catalog.py:30-65``): one
    point per row at ``XWIN_WORLD``, ``YWIN_WORLD``; blue for a table that has not been through the cuts, else green
    where ``GOODCUT`` is set and red where it is not."""

    @classmethod
    def from_catalog(cls, catalog):
        tab = catalog.data
        if not {'XWIN_WORLD', 'YWIN_WORLD'} <= set(tab.dtype.names):
            raise ValueError("the catalog has no XWIN_WORLD / YWIN_WORLD: make it with columns='param'")
        reg = cls()
        reg.basename = catalog.basename.replace('.cat', '.reg')
        reg.map_to_local_file(str(Path(catalog.local_path).with_name(reg.basename)))
        for prop in GROUP_PROPERTIES:
            setattr(reg, prop, getattr(catalog, prop, None))
        reg.catalog, catalog.regionfile = catalog, reg
        if 'GOODCUT' in tab.dtype.names:
            colors = np.where(np.asarray(tab['GOODCUT']) != 0, 'green', 'red')
        else:
            colors = np.full(len(tab), 'blue')
        with open(reg.local_path, 'w') as f:
            f.write(REGION_HEAD)
            f.writelines(f'point({ra},{dec}) # color={c}\n' for ra, dec, c in zip(tab['XWIN_WORLD'], tab['YWIN_WORLD'], colors))
        return reg


class PipelineFITSCatalog(File):
    """Python object that maps a catalog stored in a FITS file on disk (``zuds/catalog.py:68-142``)."""

    _DATA_HDU = 2
    _HEADER_HDU = 2
    __diskmapped_cached_properties__ = ['_path', '_data']
    header = None                 # header of the image the catalog was made from (LDAC_IMHEAD)
    header_comments = None
    image = None
    deblend = None                # dict(nthresh=, mincont=) of a catalog made with deblending
    clean = None                  # dict(param=) of a catalog made with the CLEAN pass
    mask = None                   # 'blank' or 'correct' of a wide catalog made with the masked second pass

    @classmethod
    def from_image(cls, image, tmpdir='/tmp', kill_flagged=True, columns='isophotal', deblend=False, clean=False,
                   mask=None):
        from .image import CalibratableImageBase
        if not isinstance(image, CalibratableImageBase):
            raise ValueError('Image is not an instance of CalibratableImage.')
        image._call_source_extractor(tmpdir=tmpdir, catalog=True, columns=columns, deblend=deblend, clean=clean,
                                     mask=mask)
        cat = image.catalog
        for prop in GROUP_PROPERTIES:
            setattr(cat, prop, getattr(image, prop, None))
        cat.basename = image.basename.replace('.fits', '.cat')
        cat.image = image
        if kill_flagged:
            cat.kill_flagged()
        return cat

    @classmethod
    def from_file(cls, f, use_existing_record=True):
        f = Path(f)
        obj = cls()
        obj.basename = f.name
        obj.map_to_local_file(str(f.absolute()))
        obj.load()
        return obj

    @property
    def data(self):
        try:
            return self._data
        except AttributeError:
            self.load()
        return self._data

    @data.setter
    def data(self, d):
        self._data = d

    def load(self):
        self._data, self.table_header, self.header, self.header_comments = _fits.read_ldac(self.local_path)
        if self.table_header.get('ZMDEBLND') is True:
            self.deblend = dict(nthresh=int(self.table_header['ZMDBNTHR']), mincont=float(self.table_header['ZMDBMINC']))
        if self.table_header.get('ZMCLEAN') is True:
            self.clean = dict(param=float(self.table_header['ZMCLNPAR']))
        masked = str(self.table_header.get('ZMMASKTY', 'NONE')).strip().upper()
        self.mask = masked.lower() if masked in ('BLANK', 'CORRECT') else None

    def save(self):
        try:
            f = self.local_path
        except UnmappedFileError:
            f = self.basename
            self.map_to_local_file(f)
        wide = 'FLUX_AUTO' in (self.data.dtype.names or ())
        _fits.write_ldac(f, self.data, self.header or {}, self.header_comments or {},
                         extra=header_cards(self.deblend, self.clean) + (wide_cards(self.mask) if wide else []))

    def kill_flagged(self):
        """Drop the detections with a bad IMAFLAGS_ISO or a bad pixel next to them (``zuds/catalog.py:132-142``); a
        mapped catalog is rewritten."""
        d = self.data
        keep = ((d['IMAFLAGS_ISO'] & BAD_SUM) == 0) & (d['FLAGS_WEIGHT'] == 0)
        self.data = d[keep]
        if self.ismapped:
            self.save()
            self.load()
