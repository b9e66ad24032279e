"""Dependency-free single-HDU FITS image reader / writer, and the FITS_LDAC catalog layout.

The reference reads and writes its products with ``astropy.io.fits``
(``zuds/fitsfile.py:69-94,146-178``); astropy is not available on the GPU box, and
this path only ever touches primary-HDU images (``_DATA_HDU = _HEADER_HDU = 0``,
``zuds/fitsfile.py:37-38``).  FITS standard 4.0: 2880-byte blocks, 80-character
cards, big-endian data, BITPIX 8 / 16 / 32 / 64 / -32 / -64, BSCALE / BZERO.

Catalogs (``PipelineFITSCatalog``, ``_DATA_HDU = 2``, ``zuds/catalog.py:90-93``) are FITS_LDAC files: an empty
primary HDU, ``LDAC_IMHEAD`` (the image header as one string column) and ``LDAC_OBJECTS`` (a binary table of
fixed-width scalar columns).  ``write_ldac`` / ``read_ldac`` do exactly that and nothing more general.
"""
import numpy as np

BLOCK = 2880
_BITPIX_DTYPE = {8: '>u1', 16: '>i2', 32: '>i4', 64: '>i8', -32: '>f4', -64: '>f8'}
_MANDATORY = ('SIMPLE', 'BITPIX', 'NAXIS', 'EXTEND')


def _parse_value(s):
    """Value field of a card (columns 11-80) -> (python value, comment)."""
    s = s.rstrip()
    t = s.lstrip()
    if t.startswith("'"):
        # quoted string, '' is an escaped quote
        i = 1
        out = []
        while i < len(t):
            if t[i] == "'":
                if i + 1 < len(t) and t[i + 1] == "'":
                    out.append("'")
                    i += 2
                    continue
                break
            out.append(t[i])
            i += 1
        rest = t[i + 1:]
        comment = rest.split('/', 1)[1].strip() if '/' in rest else ''
        return ''.join(out).rstrip(), comment
    if '/' in t:
        v, comment = t.split('/', 1)
        v, comment = v.strip(), comment.strip()
    else:
        v, comment = t.strip(), ''
    if v == 'T':
        return True, comment
    if v == 'F':
        return False, comment
    if v == '':
        return None, comment
    try:
        return int(v), comment
    except ValueError:
        pass
    try:
        return float(v.replace('D', 'E').replace('d', 'e')), comment
    except ValueError:
        return v, comment


def _read_header(read, what, primary=True):
    header, comments = {}, {}
    nblocks = 0
    done = False
    while not done:
        block = read(BLOCK)
        if len(block) < BLOCK:
            raise ValueError(f'{what}: truncated FITS header')
        nblocks += 1
        for i in range(0, BLOCK, 80):
            card = block[i:i + 80].decode('ascii', 'replace')
            key = card[:8].strip()
            if key == 'END':
                done = True
                break
            if not key or key in ('COMMENT', 'HISTORY') or card[8:10] != '= ':
                continue
            val, com = _parse_value(card[10:])
            if val is None:
                continue
            header[key] = val
            comments[key] = com
    if not primary:
        if 'XTENSION' not in header:
            raise ValueError(f'{what}: not a FITS extension (no XTENSION card)')
    elif header.get('SIMPLE') is not True:
        raise ValueError(f'{what}: not a standard FITS file (SIMPLE != T)')
    return header, comments, nblocks * BLOCK


def read_header(path):
    """(header dict, comments dict, data offset in bytes)."""
    with open(path, 'rb') as f:
        return _read_header(f.read, path)


def parse_header(block):
    """(header dict, comments dict) of header bytes as ``header_block`` emits them: what ``read_header``
    returns for a file that starts with them."""
    import io
    h, c, _ = _read_header(io.BytesIO(bytes(block)).read, 'header block')
    return h, c


def read(path, header_only=False):
    """Read the primary HDU: (data or None, header dict, comments dict)."""
    header, comments, off = read_header(path)
    if header_only:
        return None, header, comments
    naxis = int(header.get('NAXIS', 0))
    if naxis == 0:
        return None, header, comments
    shape = tuple(int(header[f'NAXIS{i}']) for i in range(naxis, 0, -1))
    bitpix = int(header['BITPIX'])
    if bitpix not in _BITPIX_DTYPE:
        raise ValueError(f'{path}: unsupported BITPIX {bitpix}')
    dt = np.dtype(_BITPIX_DTYPE[bitpix])
    count = int(np.prod(shape))
    with open(path, 'rb') as f:
        f.seek(off)
        raw = np.fromfile(f, dtype=dt, count=count)
    if raw.size != count:
        raise ValueError(f'{path}: truncated FITS data ({raw.size} of {count} values)')
    data = raw.reshape(shape).astype(dt.newbyteorder('='))
    bscale = header.get('BSCALE', 1)
    bzero = header.get('BZERO', 0)
    if bscale != 1 or bzero != 0:
        if bscale == 1 and float(bzero).is_integer() and bitpix > 0:
            unsigned = {16: (32768, np.uint16), 32: (2147483648, np.uint32)}
            if bitpix in unsigned and int(bzero) == unsigned[bitpix][0]:
                data = (data.astype(np.int64) + int(bzero)).astype(unsigned[bitpix][1])
            else:
                data = data.astype(np.int64) + int(bzero)
        else:
            data = (data * np.float64(bscale) + np.float64(bzero)).astype(np.float32)
    return data, header, comments


def read_raw(path, out=None):
    """The data block of the primary HDU as it lies on disk, undecoded.

    Returns (raw uint8 array of nbytes, header, comments, info) with info =
    dict(bitpix, shape, bscale, bzero, count).  ``out``: optional writable uint8 buffer
    (e.g. pinned memory) of at least nbytes to read into.  Decoding is left to
    ``zm_fits_decode_dev`` on the device (``device.load_fits``)."""
    header, comments, off = read_header(path)
    naxis = int(header.get('NAXIS', 0))
    if naxis == 0:
        raise ValueError(f'{path}: no image data in the primary HDU')
    shape = tuple(int(header[f'NAXIS{i}']) for i in range(naxis, 0, -1))
    bitpix = int(header['BITPIX'])
    if bitpix not in _BITPIX_DTYPE:
        raise ValueError(f'{path}: unsupported BITPIX {bitpix}')
    count = int(np.prod(shape))
    nbytes = count * abs(bitpix) // 8
    if out is None:
        out = np.empty(nbytes, dtype=np.uint8)
    buf = memoryview(out)[:nbytes]
    with open(path, 'rb', buffering=0) as f:
        f.seek(off)
        got = 0
        while got < nbytes:
            k = f.readinto(buf[got:])
            if not k:
                raise ValueError(f'{path}: truncated FITS data ({got} of {nbytes} bytes)')
            got += k
    info = dict(bitpix=bitpix, shape=shape, count=count, nbytes=nbytes,
                bscale=float(header.get('BSCALE', 1)), bzero=float(header.get('BZERO', 0)))
    return out[:nbytes], header, comments, info


def header_block(data_shape, bitpix, header=None, comments=None, extra=()):
    """The padded header bytes ``write`` would emit for an array of this shape / BITPIX."""
    header = dict(header or {})
    comments = comments or {}
    cards = [_card('SIMPLE', True, 'conforms to FITS standard'),
             _card('BITPIX', bitpix, 'array data type'),
             _card('NAXIS', len(data_shape), 'number of array dimensions')]
    for i, n in enumerate(reversed(tuple(data_shape))):
        cards.append(_card(f'NAXIS{i + 1}', int(n)))
    skip = set(_MANDATORY) | {'BSCALE', 'BZERO', 'END'} | {f'NAXIS{i}' for i in range(1, 10)}
    for k, v, c in extra:
        cards.append(_card(k, v, c))
    for k, v in header.items():
        ku = str(k).upper()
        if ku in skip or v is None:
            continue
        if not isinstance(v, (int, float, str, bool, np.integer, np.floating, np.bool_)):
            continue
        cards.append(_card(ku, v, comments.get(k, '') or ''))
    cards.append('END'.ljust(80))
    hdr = ''.join(cards).encode('ascii', 'replace')
    return hdr + b' ' * (-len(hdr) % BLOCK)


def write_raw(path, raw, data_shape, bitpix, header=None, comments=None):
    """Write a primary HDU from an already encoded (big-endian) data block."""
    raw = memoryview(raw)
    with open(path, 'wb') as f:
        f.write(header_block(data_shape, bitpix, header, comments))
        f.write(raw)
        f.write(b'\0' * (-raw.nbytes % BLOCK))


def _fmt_value(v):
    if isinstance(v, (bool, np.bool_)):
        return f"{'T' if v else 'F':>20}"
    if isinstance(v, (int, np.integer)):
        return f'{int(v):>20d}'
    if isinstance(v, (float, np.floating)):
        v = float(v)
        if not np.isfinite(v):
            return f"{repr(str(v)):<20}"
        s = repr(v).upper()
        if 'E' not in s and '.' not in s:
            s += '.0'
        if len(s) > 20:
            s = f'{v:.14E}'
        return f'{s:>20}'
    s = str(v).replace("'", "''")
    return f"'{s:<8}'"


def _card(key, value, comment=''):
    key = str(key).upper()
    if len(key) > 8:
        body = f'HIERARCH {key} = {_fmt_value(value).strip()}'
    else:
        body = f'{key:<8}= {_fmt_value(value)}'
    if comment:
        body += f' / {comment}'
    return body[:80].ljust(80)


def write(path, data, header=None, comments=None):
    """Write a primary-HDU image (overwrites).  ``header`` values that describe
    the array (SIMPLE / BITPIX / NAXIS* / BSCALE / BZERO) are regenerated."""
    with open(path, 'wb') as f:
        f.write(to_bytes(data, header, comments))


def to_bytes(data, header=None, comments=None, cards=()):
    """The bytes ``write`` puts into the file (a thumbnail's FITS file never touches a disk, zuds/thumbnails.py:84-91)."""
    header = dict(header or {})
    comments = comments or {}
    data = np.asarray(data)
    extra = []
    if data.dtype == np.bool_:
        data = data.astype(np.uint8)
    kind = data.dtype
    if kind == np.uint8:
        bitpix = 8
    elif kind == np.int16:
        bitpix = 16
    elif kind == np.uint16:
        bitpix = 16
        data = (data.astype(np.int32) - 32768).astype(np.int16)
        extra = [('BSCALE', 1, ''), ('BZERO', 32768, '')]
    elif kind == np.int32:
        bitpix = 32
    elif kind in (np.int64, np.uint32, np.uint64):
        bitpix = 64
        data = data.astype(np.int64)
    elif kind == np.float32:
        bitpix = -32
    elif kind in (np.float64, np.float16):
        bitpix = -64
        data = data.astype(np.float64)
    elif kind == np.int8:
        bitpix = 16
        data = data.astype(np.int16)
    else:
        raise ValueError(f'cannot write dtype {kind} to FITS')
    hdr = header_block(data.shape, bitpix, header, comments, list(cards) + list(extra))
    raw = np.ascontiguousarray(data).astype(np.dtype(_BITPIX_DTYPE[bitpix])).tobytes()
    return hdr + raw + b'\0' * (-len(raw) % BLOCK)


def _decode(raw, header, what):
    """Physical values of the data block ``raw`` (big-endian array of the header's shape)."""
    bitpix = int(header['BITPIX'])
    dt = np.dtype(_BITPIX_DTYPE[bitpix])
    data = raw.astype(dt.newbyteorder('='))
    bscale = header.get('BSCALE', 1)
    bzero = header.get('BZERO', 0)
    if bscale != 1 or bzero != 0:
        if bscale == 1 and float(bzero).is_integer() and bitpix > 0:
            unsigned = {16: (32768, np.uint16), 32: (2147483648, np.uint32)}
            if bitpix in unsigned and int(bzero) == unsigned[bitpix][0]:
                data = (data.astype(np.int64) + int(bzero)).astype(unsigned[bitpix][1])
            else:
                data = data.astype(np.int64) + int(bzero)
        else:
            data = (data * np.float64(bscale) + np.float64(bzero)).astype(np.float32)
    return data


def from_bytes(buf):
    """``read`` on the bytes of a FITS file held in memory: (data or None, header dict, comments dict)."""
    import io
    buf = bytes(buf)
    header, comments, off = _read_header(io.BytesIO(buf).read, 'FITS bytes')
    naxis = int(header.get('NAXIS', 0))
    if naxis == 0:
        return None, header, comments
    shape = tuple(int(header[f'NAXIS{i}']) for i in range(naxis, 0, -1))
    bitpix = int(header['BITPIX'])
    if bitpix not in _BITPIX_DTYPE:
        raise ValueError(f'FITS bytes: unsupported BITPIX {bitpix}')
    count = int(np.prod(shape))
    dt = np.dtype(_BITPIX_DTYPE[bitpix])
    if len(buf) < off + count * dt.itemsize:
        raise ValueError(f'FITS bytes: truncated data ({len(buf) - off} of {count * dt.itemsize} bytes)')
    raw = np.frombuffer(buf, dtype=dt, count=count, offset=off).reshape(shape)
    return _decode(raw, header, 'FITS bytes'), header, comments


def write_image_table(path, data, table, header=None, comments=None, extname='STAMPS', extra=()):
    """A primary-HDU image followed by ONE binary table of scalar columns (the columns ``write_ldac`` takes): the
    stamps file of scripts/dosub.py --stamps."""
    table = np.asarray(table)
    names = table.dtype.names
    cols, fields = [], []
    for i, name in enumerate(names, 1):
        dt = table.dtype[name]
        code = 'u1' if dt.kind == 'b' else dt.kind + str(dt.itemsize)
        if dt.shape or code not in _TFORM:
            raise ValueError(f'column {name}: dtype {dt} has no FITS binary-table column type here')
        fields.append((name, '>' + code))
        cols += [_card(f'TTYPE{i}', name), _card(f'TFORM{i}', '1' + _TFORM[code])]
    big = np.empty(len(table), dtype=fields)
    for name in names:
        big[name] = table[name]
    head = to_bytes(data, header, comments, cards=[('EXTEND', True, 'a binary table follows')])
    with open(path, 'wb') as f:
        f.write(head)
        f.write(_table_hdu(extname, [_card('TFIELDS', len(names))] + cols, big.dtype.itemsize, len(table),
                           big.tobytes(), extra))


def read_image_table(path):
    """(data, header, table as a native-endian record array, table header) of a file ``write_image_table`` wrote."""
    data, header, _ = read(path)
    _, _, off = read_header(path)
    nbytes = 0 if data is None else int(np.prod(data.shape)) * abs(int(header['BITPIX'])) // 8
    with open(path, 'rb') as f:
        f.seek(off + nbytes + (-nbytes % BLOCK))
        h, _, _ = _read_header(f.read, path, primary=False)
        if h.get('XTENSION') != 'BINTABLE':
            raise ValueError(f'{path}: expected a binary table behind the image')
        fields = []
        for i in range(1, int(h['TFIELDS']) + 1):
            code = str(h[f'TFORM{i}']).strip().lstrip('1')
            if code not in _TFORM_DTYPE:
                raise ValueError(f'{path}: column {h[f"TTYPE{i}"]}: only scalar B I J K E D columns')
            fields.append((str(h[f'TTYPE{i}']).strip(), _TFORM_DTYPE[code]))
        n = int(h['NAXIS1']) * int(h['NAXIS2'])
        body = f.read(n)
        if len(body) != n:
            raise ValueError(f'{path}: truncated table')
    big = np.frombuffer(body, dtype=fields, count=int(h['NAXIS2']))
    native = np.empty(len(big), dtype=[(nm, np.dtype(t).newbyteorder('=')) for nm, t in fields])
    for nm, _ in fields:
        native[nm] = big[nm]
    return data, header, native.view(np.recarray), h


# ---- FITS_LDAC ------------------------------------------------------------------------------------------------
_TFORM = {'u1': 'B', 'i2': 'I', 'i4': 'J', 'i8': 'K', 'f4': 'E', 'f8': 'D'}
_TFORM_DTYPE = {v: '>' + k for k, v in _TFORM.items()}


def _table_hdu(extname, ncols_cards, row_bytes, nrows, body, extra=()):
    cards = [_card('XTENSION', 'BINTABLE', 'binary table extension'), _card('BITPIX', 8), _card('NAXIS', 2),
             _card('NAXIS1', int(row_bytes), 'bytes per row'), _card('NAXIS2', int(nrows), 'rows'),
             _card('PCOUNT', 0), _card('GCOUNT', 1)] + ncols_cards + [_card('EXTNAME', extname)]
    cards += [_card(k, v, c) for k, v, c in extra]
    cards.append('END'.ljust(80))
    hdr = ''.join(cards).encode('ascii', 'replace')
    return hdr + b' ' * (-len(hdr) % BLOCK) + body + b'\0' * (-len(body) % BLOCK)


def write_ldac(path, table, image_header=None, image_comments=None, extra=()):
    """``table``: numpy structured array of scalar columns (uint8, int16 / 32 / 64, float32 / 64; bool is stored as
    uint8).  ``image_header``: the header of the image the catalog was made from (LDAC_IMHEAD).  ``extra``:
    (key, value, comment) cards for the LDAC_OBJECTS header."""
    table = np.asarray(table)
    names = table.dtype.names
    cols, fields = [], []
    for i, name in enumerate(names, 1):
        dt = table.dtype[name]
        if dt.shape:
            raise ValueError(f'column {name}: only scalar columns')
        code = 'u1' if dt.kind == 'b' else dt.kind + str(dt.itemsize)
        if code not in _TFORM:
            raise ValueError(f'column {name}: dtype {dt} has no FITS_LDAC column type here')
        fields.append((name, '>' + code))
        cols += [_card(f'TTYPE{i}', name), _card(f'TFORM{i}', '1' + _TFORM[code])]
    big = np.empty(len(table), dtype=fields)
    for name in names:
        big[name] = table[name]
    objects = _table_hdu('LDAC_OBJECTS', [_card('TFIELDS', len(names))] + cols, big.dtype.itemsize, len(table),
                         big.tobytes(), extra)
    head = header_block((), 8, image_header, image_comments)
    ncards = len(head) // 80
    imhead = _table_hdu('LDAC_IMHEAD', [_card('TFIELDS', 1), _card('TTYPE1', 'Field Header Card'),
                                        _card('TFORM1', f'{len(head)}A'), _card('TDIM1', f'(80, {ncards})')],
                        len(head), 1, head)
    primary = ''.join([_card('SIMPLE', True, 'conforms to FITS standard'), _card('BITPIX', 8), _card('NAXIS', 0),
                       _card('EXTEND', True), 'END'.ljust(80)]).encode('ascii')
    with open(path, 'wb') as f:
        f.write(primary + b' ' * (-len(primary) % BLOCK))
        f.write(imhead)
        f.write(objects)


def read_ldac(path):
    """(table as a native-endian record array, LDAC_OBJECTS header, image header dict, image header comments)."""
    with open(path, 'rb') as f:
        h0, _, _ = _read_header(f.read, path)
        if int(h0.get('NAXIS', 0)) != 0:
            raise ValueError(f'{path}: a FITS_LDAC file has an empty primary HDU')
        found = {}
        for want in ('LDAC_IMHEAD', 'LDAC_OBJECTS'):
            h, _, _ = _read_header(f.read, path, primary=False)
            if h.get('XTENSION') != 'BINTABLE' or h.get('EXTNAME') != want:
                raise ValueError(f'{path}: expected the {want} binary table, found {h.get("EXTNAME")!r}')
            nbytes = int(h['NAXIS1']) * int(h['NAXIS2']) + int(h.get('PCOUNT', 0))
            body = f.read(nbytes)
            if len(body) != nbytes:
                raise ValueError(f'{path}: truncated {want} table')
            f.read(-nbytes % BLOCK)
            found[want] = (h, body)
    ih, ic = parse_header(found['LDAC_IMHEAD'][1])
    h, body = found['LDAC_OBJECTS']
    fields = []
    for i in range(1, int(h['TFIELDS']) + 1):
        form = str(h[f'TFORM{i}']).strip()
        code = form.lstrip('1')
        if code not in _TFORM_DTYPE or form not in (code, '1' + code):
            raise ValueError(f'{path}: column {h[f"TTYPE{i}"]} has TFORM {form}: only scalar B I J K E D columns')
        fields.append((str(h[f'TTYPE{i}']).strip(), _TFORM_DTYPE[code]))
    big = np.frombuffer(body, dtype=fields, count=int(h['NAXIS2']))
    if big.dtype.itemsize != int(h['NAXIS1']):
        raise ValueError(f'{path}: NAXIS1 {h["NAXIS1"]} does not match the columns ({big.dtype.itemsize} bytes)')
    native = np.empty(len(big), dtype=[(n, np.dtype(t).newbyteorder('=')) for n, t in fields])
    for n, _ in fields:
        native[n] = big[n]
    return native.view(np.recarray), h, ih, ic
