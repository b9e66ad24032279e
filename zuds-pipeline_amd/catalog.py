"""Detection catalogs (``zuds/catalog.py``), DB-free.

``PipelineFITSCatalog.from_image`` runs the source extractor of libzudsmi (``zm_extract``) where the reference runs
SExtractor; the table holds the columns that are computed (``extract.CATALOG_COLUMNS``) and no others.  On disk a
catalog is a FITS_LDAC file, as the reference asks SExtractor for (``catalog_type='FITS_LDAC'``): the object table is
HDU 2.
"""
from pathlib import Path

from . import fits as _fits
from .constants import BAD_SUM, GROUP_PROPERTIES
from .file import File, UnmappedFileError

__all__ = ['PipelineFITSCatalog']

# what this version of the extractor does not do, stated in every catalog's header
HEADER_CARDS = [('ZMDEBLND', False, 'multi-threshold deblending (not in this version)'),
                ('ZMCLEAN', False, 'CLEAN pass (not in this version)')]


class PipelineFITSCatalog(File):
    """Python object that maps a catalog stored in a FITS file on disk (``zuds/catalog.py:68-142``)."""

    _DATA_HDU = 2
    _HEADER_HDU = 2
    __diskmapped_cached_properties__ = ['_path', '_data']
    header = None                 # header of the image the catalog was made from (LDAC_IMHEAD)
    header_comments = None
    image = None

    @classmethod
    def from_image(cls, image, tmpdir='/tmp', kill_flagged=True):
        from .image import CalibratableImageBase
        if not isinstance(image, CalibratableImageBase):
            raise ValueError('Image is not an instance of CalibratableImage.')
        image._call_source_extractor(tmpdir=tmpdir, catalog=True)
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

    def save(self):
        try:
            f = self.local_path
        except UnmappedFileError:
            f = self.basename
            self.map_to_local_file(f)
        _fits.write_ldac(f, self.data, self.header or {}, self.header_comments or {}, extra=HEADER_CARDS)

    def kill_flagged(self):
        """Drop the detections with a bad IMAFLAGS_ISO or a bad pixel next to them (``zuds/catalog.py:132-142``); a
        mapped catalog is rewritten."""
        d = self.data
        keep = ((d['IMAFLAGS_ISO'] & BAD_SUM) == 0) & (d['FLAGS_WEIGHT'] == 0)
        self.data = d[keep]
        if self.ismapped:
            self.save()
            self.load()
