"""k_fits_decode / k_fits_encode (csrc/fitsio.hip) against the independent reference tests/fits_ref.py on every
scene of tests/fits_scenes.py and every output kind, bit for bit, and the three call sites that hand files to the
kernel (FITSDeviceIO.load, load_many, FITSRing.prefetch).  The contract is above zm_fits_decode_dev in
include/zudsmi.h."""
import importlib

import numpy as np
import pytest

import fits_ref
import fits_scenes
from util import pkg

pytestmark = pytest.mark.gpu

SCENES = fits_scenes.scenes()
KIND_NO = {'f32': 0, 'i32': 1, 'u8': 2, 'i16': 3}
KIND_NP = {'f32': np.float32, 'i32': np.int32, 'u8': np.uint8, 'i16': np.int16}


@pytest.fixture(scope='module')
def dev(engine):
    """decode(raw bytes, bitpix, bscale, bzero, n, kind) and encode(numpy plane, in_kind) -> numpy, through the C ABI
    on device buffers."""
    import torch
    check = importlib.import_module('zuds-pipeline_amd._lib').check
    engine.set_stream(None)

    class Dev(object):
        def decode(self, raw, bitpix, bscale, bzero, n, kind):
            d_raw = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
            out = torch.from_numpy(np.full(n, 0x5a, np.uint8).repeat(np.dtype(KIND_NP[kind]).itemsize)).cuda()
            torch.cuda.synchronize()
            check(engine.L.zm_fits_decode_dev(engine.ctx, d_raw.data_ptr(), bitpix, bscale, bzero, n, KIND_NO[kind],
                                              out.data_ptr()), 'zm_fits_decode_dev')
            torch.cuda.synchronize()
            return out.cpu().numpy().view(KIND_NP[kind])

        def encode(self, plane, in_kind):
            t = torch.from_numpy(np.ascontiguousarray(plane)).cuda()
            size = {0: 4, 1: 4, 2: 1, 3: 2}[in_kind]
            out = torch.full((plane.size * size,), 0x5a, dtype=torch.uint8, device='cuda')
            torch.cuda.synchronize()
            check(engine.L.zm_fits_encode_dev(engine.ctx, t.data_ptr(), in_kind, plane.size, out.data_ptr()),
                  'zm_fits_encode_dev')
            torch.cuda.synchronize()
            return out.cpu().numpy().tobytes()
    return Dev()


def _f32_bytes(got, any_nan, what):
    """The plane's bits, with the NaNs whose payload the contract leaves open (checked to be NaNs) made canonical."""
    bits = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32).ravel().copy()
    for i in any_nan:
        assert bits[i] & 0x7fffffff > 0x7f800000, (what, i, hex(int(bits[i])))
        bits[i] = fits_ref.NAN_ANY
    return bits


def _differing(got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return f'{bad.size} of {len(want)} pixels differ, first at {bad[:5].tolist()}: ' \
           f'got {[got[i] for i in bad[:5]]} want {[want[i] for i in bad[:5]]}'


def assert_plane(got, ref, kind, what):
    """A decoded plane against the reference, every pixel: bits for float32, values for the integer kinds."""
    assert got.dtype == KIND_NP[kind] and got.size == ref.n, what
    if kind == 'f32':
        want, any_nan = ref.want_f32()
        bits = _f32_bytes(got, any_nan, what)
        want = np.array(want, dtype=np.uint32)
        assert bits.tobytes() == want.tobytes(), (what, _differing(bits.tolist(), want.tolist()))
    else:
        want = ref.want_int(kind)
        assert got.ravel().tolist() == want, (what, _differing(got.ravel().tolist(), want))


@pytest.mark.parametrize('scene', SCENES, ids=repr)
def test_decode_matches_the_reference_on_every_output_kind(dev, scene, tmp_path):
    r = scene.ref
    planes = {}
    for kind in fits_ref.KINDS:
        planes[kind] = dev.decode(scene.raw, r.bitpix, r.bscale, r.bzero, r.n, kind)
        assert_plane(planes[kind], r, kind, f'{scene.name} -> {kind}')
    if not scene.host:
        return
    # the float plane against the host reader too: the same planes from the host route and the device route
    p = str(tmp_path / 'scene.fits')
    with open(p, 'wb') as f:
        f.write(scene.block)
    with np.errstate(all='ignore'):
        host = pkg().fits.read(p)[0].astype(np.float32)
    _, any_nan = r.want_f32()
    got, want = _f32_bytes(planes['f32'], any_nan, scene.name), _f32_bytes(host, any_nan, scene.name)
    assert got.tobytes() == want.tobytes(), (scene.name, _differing(got.tolist(), want.tolist()))


# ---- the call sites ---------------------------------------------------------------------------------------------
CALL_SITE_SCENES = ('scaled16_0.1_-3', f'scaled16_{1 / 3!r}_{2 / 3!r}', 'scaled-32_0.1_-3', 'scaled64_thirds',
                    'convention_bp16', 'edges_bp64', 'edges_bp16', 'cube_bp16')


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('fits_call_sites')
    wanted = []
    for name in CALL_SITE_SCENES:
        s = fits_scenes.by_name(name)
        p = str(d / (name.replace('.', '_') + '.fits'))
        with open(p, 'wb') as f:
            f.write(s.block)
        for kind in ('f32', 'i32', 'u8', 'i16', 'mask'):
            wanted.append((p, kind, s))
    return wanted


def _check_call_site(results, files):
    import torch
    torch.cuda.synchronize()
    assert len(results) == len(files)
    for (t, hdr), (p, kind, s) in zip(results, files):
        r = s.ref
        what = f'{s.name} as {kind}'
        assert tuple(t.shape) == s.shape and hdr['BITPIX'] == r.bitpix, what
        got = t.cpu().numpy()
        if kind == 'mask':
            # unscaled BITPIX 16 comes back as int16; anything else as int32
            kind = 'i16' if (r.bitpix == 16 and not r.scaled) else 'i32'
            if s.name == 'convention_bp16':              # unsigned 16: 0 .. 65535 intact
                assert got.ravel().tolist() == [v + 32768 for v in s.stored], what
                assert min(got.ravel().tolist()) == 0 and max(got.ravel().tolist()) == 65535
        assert_plane(got.reshape(-1), r, kind, what)


def test_load_of_the_device_io_follows_the_contract(engine, files):
    io = importlib.import_module('zuds-pipeline_amd.device').FITSDeviceIO(0, engine=engine)
    try:
        _check_call_site([io.load(p, kind) for p, kind, _ in files], files)
    finally:
        engine.set_stream(None)


def test_load_many_of_the_device_io_follows_the_contract(engine, files):
    io = importlib.import_module('zuds-pipeline_amd.device').FITSDeviceIO(0, engine=engine)
    try:
        _check_call_site(io.load_many([(p, kind) for p, kind, _ in files]), files)
    finally:
        engine.set_stream(None)


def test_ring_prefetch_follows_the_contract(files):
    import torch
    m = importlib.import_module('zuds-pipeline_amd.fitsring')
    ring = m.FITSRing(0, nreaders=4, nwriters=2, pinned_in=8 << 20, pinned_out=1 << 20)
    try:
        stream = torch.cuda.Stream()
        got = ring.prefetch([(p, kind) for p, kind, _ in files]).result(stream)
        stream.synchronize()
        _check_call_site(got, files)
    finally:
        ring.close()


# ---- encode -----------------------------------------------------------------------------------------------------
def _cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


ENCODE_PLANES = {
    # in_kind: (numpy dtype of the plane, values to cycle through, BITPIX of the block, kind that reads it back)
    0: (np.uint32, fits_scenes.F32_SPECIALS + [fits_scenes.f32(v) for v in (1.5, -2.75e-3, 6.02e23, 3.14159)], -32, 'f32'),
    1: (np.int32, [-2 ** 31, 2 ** 31 - 1, -1, 0, 1, 65535, 65536, -32769, 16909060, -16909060], 32, 'i32'),
    2: (np.uint8, [0, 255, 1, 254, 127, 128, 18, 52], 8, 'u8'),
    3: (np.int32, [-32768, 32767, -1, 0, 1, 255, 256, -256, 4660, -4660], 16, 'i16'),
}


@pytest.mark.parametrize('in_kind', sorted(ENCODE_PLANES))
@pytest.mark.parametrize('n', fits_scenes.LENGTHS + (30,))
def test_encode_matches_the_reference_and_decodes_back(dev, in_kind, n):
    dt, values, bitpix, back = ENCODE_PLANES[in_kind]
    values = _cycle(values, n)
    plane = np.array(values, dtype=dt)
    raw = dev.encode(plane.view(np.float32) if in_kind == 0 else plane, in_kind)
    assert raw == fits_ref.encode(values, in_kind), (in_kind, n)
    got = dev.decode(raw, bitpix, 1.0, 0.0, n, back)
    if in_kind == 0:
        assert got.view(np.uint32).tobytes() == plane.tobytes()
    else:
        assert got.tolist() == values
