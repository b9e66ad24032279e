"""Detections of a filtered catalog (``zuds/detections.py:25-109``), as plain objects."""
from .filterobjects import filter_sexcat

__all__ = ['Detection']


class Detection(object):
    """One candidate: the attributes the reference stores per detection (``zuds/detections.py:88-97``)."""

    def __init__(self, ra=None, dec=None, image=None, flux=None, fluxerr=None, elongation=None, flags=None,
                 imaflags_iso=None, a_image=None, b_image=None, fwhm_image=None, x_image=None, y_image=None):
        self.ra, self.dec, self.image = ra, dec, image
        self.flux, self.fluxerr = flux, fluxerr
        self.elongation, self.flags, self.imaflags_iso = elongation, flags, imaflags_iso
        self.a_image, self.b_image, self.fwhm_image = a_image, b_image, fwhm_image
        self.x_image, self.y_image = x_image, y_image
        self.goodcut = None
        self.rb = None
        self.rb_version = None

    @property
    def snr(self):
        return self.flux / self.fluxerr

    def __repr__(self):
        return f'<Detection x={self.x_image:.2f} y={self.y_image:.2f} snr={self.snr:.1f}>'

    @classmethod
    def from_catalog(cls, cat, filter=True, rb_model=None, rb_cut=None):
        """The detections of ``cat``; with ``filter`` the catalog goes through ``filter_sexcat`` first and only rows
        with ``GOODCUT == 1`` are returned.  ``rb_model``: the real / bogus model the filter scores with; its base name
        is kept as ``rb_version`` beside ``rb`` (``zuds/detections.py:99``)."""
        if filter:
            filter_sexcat(cat, rb_model=rb_model, rb_cut=rb_cut)
        version = rb_model.name if rb_model is not None else getattr(cat, 'rb_version', None)
        names = cat.data.dtype.names
        result = []
        for row in cat.data:
            if filter and row['GOODCUT'] != 1:
                continue
            d = cls(ra=float(row['X_WORLD']), dec=float(row['Y_WORLD']), image=cat.image,
                    flux=float(row['FLUX_APER']), fluxerr=float(row['FLUXERR_APER']),
                    elongation=float(row['ELONGATION']), flags=int(row['FLAGS']),
                    imaflags_iso=int(row['IMAFLAGS_ISO']), a_image=float(row['A_IMAGE']),
                    b_image=float(row['B_IMAGE']), fwhm_image=float(row['FWHM_IMAGE']),
                    x_image=float(row['X_IMAGE']), y_image=float(row['Y_IMAGE']))
            d.rb = float(row['rb']) if 'rb' in names else None
            d.rb_version = version if d.rb is not None and d.rb != -99.0 else None
            if filter:
                d.goodcut = True
            result.append(d)
        return result
