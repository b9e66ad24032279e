"""The real / bogus score of the candidate filter (``zuds/filterobjects.py:16-26,196-240``): the braai network on the GPU.

The reference builds a Keras model from ``<base>.architecture.json`` (``model.to_json()``) and ``<base>.weights.h5``
(``load_model_helper``) and calls ``predict`` on one 63 x 63 x 3 triplet per surviving row.  Here the architecture is
parsed with ``json``, the weights come from ``<base>.weights.npz`` (the arrays of ``model.get_weights()`` in order;
``tools/braai_to_npz.py`` writes one from the ``.h5`` at a site that has h5py), and the forward pass runs in
``csrc/braai.hip`` on the stamp blocks the thumbnail kernels left in HBM (``zm_rb_score_dev``).  No TensorFlow, Keras or
h5py dependency, and no weights are shipped: the reference ships none either (its ``ml/`` directory is empty).

Supported (everything braai's VGG6 uses; anything else raises ``ValueError``): ``Conv2D`` 3 x 3 / valid / stride 1 /
bias / relu or linear, ``MaxPooling2D`` square with stride = size / valid, ``Flatten``, ``Dense`` relu / sigmoid /
linear, ``Dropout`` (identity at inference: skipped).  DESIGN.md, "Real / bogus score".
"""
import ctypes as C
import json
import os
import re

import numpy as np

from . import _lib
from ._lib import check
from .engine import get_engine

__all__ = ['parse_architecture', 'load_model', 'RBModel', 'Architecture', 'CHANNELS']

CHANNELS = ('new', 'ref', 'sub')          # channel order of make_triplet_for_braai (zuds/filterobjects.py:45)


class Architecture(object):
    """A parsed model: ``in_size``, ``in_channels``, ``layers`` (dicts: kind 'conv' / 'pool' / 'flatten' / 'dense' with
    their sizes, activation and the weight shapes they expect) and ``shapes``, the size chain - the side of the square
    tensor behind the input and every Conv2D / MaxPooling2D, then the length of the vector behind Flatten and every
    Dense (63, 61, 59, 29, 27, 25, 6, 1152, 256, 1 for braai's VGG6)."""

    def __init__(self, in_size, in_channels, layers, shapes, name=None):
        self.in_size, self.in_channels, self.layers, self.shapes, self.name = in_size, in_channels, layers, shapes, name

    @property
    def weight_shapes(self):
        out = []
        for l in self.layers:
            out += l.get('weights', [])
        return out


def _pair(v, what):
    if isinstance(v, int):
        return (v, v)
    v = tuple(int(x) for x in v)
    if len(v) != 2:
        raise ValueError(f'{what}: expected two values, got {v}')
    return v


def _activation(cfg, allowed, what):
    a = cfg.get('activation', 'linear') or 'linear'
    if isinstance(a, dict):                         # newer Keras serialises activations as objects
        a = a.get('config', a.get('class_name'))
    a = str(a).lower()
    if a not in allowed:
        raise ValueError(f'{what}: activation "{a}" is not supported (one of {list(allowed)})')
    return a


def parse_architecture(text):
    """``Architecture`` of the Keras ``model.to_json()`` text (or the dict it decodes to).  Raises ``ValueError`` on
    anything outside the supported family (module docstring)."""
    doc = json.loads(text) if isinstance(text, (str, bytes)) else text
    if not isinstance(doc, dict) or doc.get('class_name') != 'Sequential':
        raise ValueError('only Keras Sequential models are supported')
    cfg = doc.get('config')
    entries = cfg.get('layers') if isinstance(cfg, dict) else cfg
    if not isinstance(entries, list) or not entries:
        raise ValueError('the model has no layers')
    name = cfg.get('name') if isinstance(cfg, dict) else None
    shape = None                                    # (H, W, C) or (features,)
    layers, shapes = [], []
    for k, ent in enumerate(entries):
        kind, c = ent.get('class_name'), ent.get('config', {})
        what = f'layer {k} ({kind})'
        bis = c.get('batch_input_shape', c.get('batch_shape'))
        if bis is not None and shape is None:
            if len(bis) != 4 or bis[1] != bis[2] or bis[1] is None or bis[3] is None:
                raise ValueError(f'{what}: the input must be a square channels-last image, got shape {bis}')
            shape = (int(bis[1]), int(bis[2]), int(bis[3]))
            shapes.append(shape[0])
        if kind == 'InputLayer':
            continue
        if shape is None:
            raise ValueError(f'{what}: no input shape before the first layer')
        if c.get('data_format', 'channels_last') not in (None, 'channels_last'):
            raise ValueError(f'{what}: only channels_last')
        if kind == 'Dropout':
            continue                                # identity at inference
        if kind == 'Conv2D':
            if len(shape) != 3:
                raise ValueError(f'{what}: behind Flatten')
            if _pair(c.get('kernel_size'), what) != (3, 3):
                raise ValueError(f'{what}: only 3 x 3 kernels, got {c.get("kernel_size")}')
            if _pair(c.get('strides', 1), what) != (1, 1):
                raise ValueError(f'{what}: only stride 1, got {c.get("strides")}')
            if _pair(c.get('dilation_rate', 1), what) != (1, 1):
                raise ValueError(f'{what}: no dilation')
            if str(c.get('padding', 'valid')).lower() != 'valid':
                raise ValueError(f'{what}: only "valid" padding, got "{c.get("padding")}"')
            if not c.get('use_bias', True):
                raise ValueError(f'{what}: a layer without bias is not supported')
            if c.get('groups', 1) != 1:
                raise ValueError(f'{what}: no grouped convolutions')
            act = _activation(c, ('relu', 'linear'), what)
            cout = int(c['filters'])
            if not 1 <= cout <= 64 or shape[2] > 64:
                raise ValueError(f'{what}: at most 64 channels (got {shape[2]} -> {cout})')
            if shape[0] < 3:
                raise ValueError(f'{what}: a {shape[0]} x {shape[1]} tensor is smaller than the kernel')
            layers.append(dict(kind='conv', cin=shape[2], cout=cout, activation=act,
                               weights=[(3, 3, shape[2], cout), (cout,)]))
            shape = (shape[0] - 2, shape[1] - 2, cout)
            shapes.append(shape[0])
        elif kind == 'MaxPooling2D':
            if len(shape) != 3:
                raise ValueError(f'{what}: behind Flatten')
            ps = _pair(c.get('pool_size', 2), what)
            st = c.get('strides')
            st = ps if st is None else _pair(st, what)
            if ps[0] != ps[1] or st != ps:
                raise ValueError(f'{what}: only square pools with stride = size, got pool {ps} strides {st}')
            if str(c.get('padding', 'valid')).lower() != 'valid':
                raise ValueError(f'{what}: only "valid" padding, got "{c.get("padding")}"')
            if shape[0] // ps[0] < 1:
                raise ValueError(f'{what}: pool {ps[0]} of a {shape[0]} x {shape[1]} tensor')
            layers.append(dict(kind='pool', pool=ps[0]))
            shape = (shape[0] // ps[0], shape[1] // ps[0], shape[2])      # an odd remainder is dropped
            shapes.append(shape[0])
        elif kind == 'Flatten':
            if len(shape) != 3:
                raise ValueError(f'{what}: of a vector')
            layers.append(dict(kind='flatten'))
            shape = (shape[0] * shape[1] * shape[2],)
            shapes.append(shape[0])
        elif kind == 'Dense':
            if len(shape) != 1:
                raise ValueError(f'{what}: needs a Flatten before it')
            if not c.get('use_bias', True):
                raise ValueError(f'{what}: a layer without bias is not supported')
            act = _activation(c, ('relu', 'sigmoid', 'linear'), what)
            units = int(c['units'])
            layers.append(dict(kind='dense', cin=shape[0], cout=units, activation=act, weights=[(shape[0], units), (units,)]))
            shape = (units,)
            shapes.append(units)
        else:
            raise ValueError(f'{what}: unsupported layer (Conv2D, MaxPooling2D, Flatten, Dense, Dropout)')
    if not layers or layers[0]['kind'] != 'conv':
        raise ValueError('the first layer must be a Conv2D')
    if shape != (1,):
        raise ValueError(f'the model must end in a Dense layer of one unit (it ends with shape {shape})')
    return Architecture(shapes[0], layers[0]['cin'], layers, shapes, name)


def check_weights(arch, weights):
    """The arrays of ``model.get_weights()`` against the shapes ``arch`` expects -> list of float32 arrays."""
    want = arch.weight_shapes
    weights = [np.asarray(w) for w in weights]
    if len(weights) != len(want):
        raise ValueError(f'the architecture takes {len(want)} weight arrays, {len(weights)} given')
    for k, (w, s) in enumerate(zip(weights, want)):
        if tuple(w.shape) != tuple(s):
            raise ValueError(f'weight array {k} has shape {tuple(w.shape)}, the architecture wants {tuple(s)}')
        if not np.isfinite(w).all():
            raise ValueError(f'weight array {k} holds values that are not finite')
    return [np.ascontiguousarray(w, dtype=np.float32) for w in weights]


def pack(arch, weights):
    """(``zm_rb_layer`` array, float32 blob) for ``zm_rb_model_create``: Keras layouts, one array after the other."""
    kinds = {'conv': _lib.RB_CONV2D, 'pool': _lib.RB_MAXPOOL, 'flatten': _lib.RB_FLATTEN, 'dense': _lib.RB_DENSE}
    arr = (_lib.zm_rb_layer * len(arch.layers))()
    off, it = 0, iter(weights)
    for s, l in zip(arr, arch.layers):
        s.type = kinds[l['kind']]
        s.activation = _lib.RB_ACTIVATION[l.get('activation', 'linear')]
        s.cin, s.cout = l.get('cin', 0), l.get('cout', 0)
        s.pool = l.get('pool', 0)
        s.ksize = 3 if l['kind'] == 'conv' else 0
        s.stride = 1 if l['kind'] == 'conv' else l.get('pool', 0)
        s.padding = _lib.RB_VALID
        if 'weights' in l:
            s.w_off = off
            off += next(it).size
            s.b_off = off
            off += next(it).size
    blob = np.concatenate([w.ravel() for w in weights]).astype(np.float32) if weights else np.zeros(0, np.float32)
    return arr, np.ascontiguousarray(blob)


def _old_norm(name):
    m = re.search(r'd6_m(\d+)', name or '')
    return bool(m) and int(m.group(1)) <= 7


def load_model(base):
    """The model stored as ``<base>.architecture.json`` + ``<base>.weights.npz`` (arrays ``arr_0``, ``arr_1``, ... or any
    names that sort in the order of ``model.get_weights()``).  A ``<base>.weights.h5`` is read only where h5py imports.
    Models ``d6_m7`` and older want the TensorFlow normalisation of the triplets (``old_norm``,
    ``zuds/filterobjects.py:13``): ``NotImplementedError``, as ``make_triplet_for_braai(old_norm=True)``."""
    base = os.fspath(base)
    name = os.path.basename(base)
    if _old_norm(name):
        raise NotImplementedError(f'{name}: models d6_m7 and older normalise with tensorflow.keras.utils.normalize '
                                  f'(old_norm), which this package does not depend on')
    with open(base + '.architecture.json') as f:
        arch = parse_architecture(f.read())
    if os.path.exists(base + '.weights.npz'):
        with np.load(base + '.weights.npz', allow_pickle=False) as z:
            def order(k):
                m = re.search(r'(\d+)$', k)
                return (0, int(m.group(1)), k) if m else (1, 0, k)
            weights = [z[k] for k in sorted(z.files, key=order)]
    elif os.path.exists(base + '.weights.h5'):
        try:
            import h5py  # noqa: F401
        except ImportError:
            raise RuntimeError(f'{base}.weights.h5 needs h5py, which is not installed: convert it once with '
                               f'tools/braai_to_npz.py at a site that has h5py and load {base}.weights.npz')
        weights = _weights_from_h5(base + '.weights.h5')
    else:
        raise FileNotFoundError(f'neither {base}.weights.npz nor {base}.weights.h5 exists')
    return RBModel(arch, weights, name=name)


def _weights_from_h5(path):
    """``model.get_weights()`` of a Keras ``save_weights`` file: per layer of ``layer_names`` its ``weight_names``."""
    import h5py
    out = []
    with h5py.File(path, 'r') as f:
        g = f['model_weights'] if 'model_weights' in f else f
        dec = lambda v: v.decode() if isinstance(v, bytes) else str(v)
        for lname in g.attrs['layer_names']:
            lg = g[dec(lname)]
            for wname in lg.attrs['weight_names']:
                out.append(np.asarray(lg[dec(wname)]))
    return out


class RBModel(object):
    """A parsed model and its weights; one device handle per engine (``zm_rb_model_create``), made on first use and
    freed with the engine (``Engine.close``)."""

    def __init__(self, arch, weights, name=None):
        if not isinstance(arch, Architecture):
            arch = parse_architecture(arch)
        self.arch = arch
        self.weights = check_weights(arch, weights)
        self.name = name or arch.name
        if _old_norm(self.name):
            raise NotImplementedError(f'{self.name}: old_norm models are not supported')
        self.in_size, self.in_channels = arch.in_size, arch.in_channels

    def handle(self, engine):
        table = engine.__dict__.setdefault('_rb_handles', {})
        h = table.get(id(self))
        if h is None or h[0] is not self:
            layers, blob = pack(self.arch, self.weights)
            m = C.c_void_p()
            check(engine.L.zm_rb_model_create(engine.ctx, self.in_size, self.in_channels, len(layers), layers,
                                              blob.ctypes.data, blob.size, C.byref(m)), 'zm_rb_model_create')
            h = table[id(self)] = (self, m)
        return h[1]

    def plane_of_channel(self, order):
        order = tuple(order)
        if self.in_channels != len(CHANNELS):
            if len(order) != self.in_channels:
                raise ValueError(f'the model reads {self.in_channels} channels, order names {len(order)} planes')
            return np.arange(self.in_channels, dtype=np.int32)
        try:
            return np.array([order.index(c) for c in CHANNELS], dtype=np.int32)
        except ValueError:
            raise ValueError(f'order must name the planes {CHANNELS}, got {order}')

    def score_dev(self, blocks, norms, order=('sub', 'new', 'ref'), engine=None, stream=None):
        """Scores of stamp blocks that lie in HBM: ``blocks`` [n, P, S, S] float32 and ``norms`` [n, P] float64 torch
        tensors as ``Engine.stamps(..., device_out=True)`` returns them, ``order`` the plane names.  Enqueued on the
        engine's stream (``stream``: the torch stream it is bound to), nothing waited for.  Returns rb [n] float32 on the
        device; NaN where a norm is zero or not finite."""
        import torch
        eng = engine or get_engine()
        if blocks.dim() != 4 or blocks.dtype != torch.float32 or not blocks.is_contiguous() or not blocks.is_cuda:
            raise ValueError('blocks must be a contiguous float32 device tensor [n, planes, S, S]')
        n, P, S, S2 = (int(v) for v in blocks.shape)
        if S != self.in_size or S2 != S:
            raise ValueError(f'the model reads {self.in_size} x {self.in_size} stamps, got {S} x {S2}')
        if tuple(norms.shape) != (n, P) or norms.dtype != torch.float64 or not norms.is_contiguous() or not norms.is_cuda:
            raise ValueError('norms must be a contiguous float64 device tensor [n, planes]')
        poc = self.plane_of_channel(order)
        if len(tuple(order)) != P:
            raise ValueError(f'order names {len(tuple(order))} planes, blocks has {P}')
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(blocks.device):
            rb = torch.empty(n, dtype=torch.float32, device=blocks.device)
            check(eng.L.zm_rb_score_dev(eng.ctx, self.handle(eng), n, blocks.data_ptr(), norms.data_ptr(), P,
                                        poc.ctypes.data, rb.data_ptr()), 'zm_rb_score_dev')
        return rb

    def score_blocks(self, blocks, norms, order=('sub', 'new', 'ref'), engine=None):
        """The host route of ``score_dev``: numpy blocks [n, P, S, S] and norms [n, P] (``zm_rb_score``: copied in, waits).
        Returns rb [n] float32."""
        eng = engine or get_engine()
        blocks = np.ascontiguousarray(blocks, dtype=np.float32)
        norms = np.ascontiguousarray(norms, dtype=np.float64)
        if blocks.ndim != 4 or blocks.shape[2] != self.in_size or blocks.shape[3] != self.in_size:
            raise ValueError(f'blocks must be [n, planes, {self.in_size}, {self.in_size}], got {blocks.shape}')
        n, P = blocks.shape[:2]
        if norms.shape != (n, P) or len(tuple(order)) != P:
            raise ValueError('norms must be [n, planes] and order name every plane')
        poc = self.plane_of_channel(order)
        rb = np.zeros(n, np.float32)
        check(eng.L.zm_rb_score(eng.ctx, self.handle(eng), n, blocks.ctypes.data, norms.ctypes.data, P, poc.ctypes.data,
                                rb.ctypes.data), 'zm_rb_score')
        return rb

    def score_triplets(self, triplets, engine=None):
        """Scores of triplets [n, S, S, 3] that are normalised already (``thumbnails.triplets`` /
        ``make_triplet_for_braai``: channels new, ref, sub).  A channel that holds a value that is not finite (the
        reference's cutout / 0) scores NaN."""
        t = np.asarray(triplets, dtype=np.float64)
        if t.ndim == 3:
            t = t[None]
        if t.ndim != 4 or t.shape[1:] != (self.in_size, self.in_size, self.in_channels):
            raise ValueError(f'triplets must be [n, {self.in_size}, {self.in_size}, {self.in_channels}], got {t.shape}')
        blocks = np.ascontiguousarray(np.moveaxis(t, 3, 1))
        finite = np.isfinite(blocks).all(axis=(2, 3))
        norms = np.where(finite, 1.0, np.nan)
        blocks = np.where(finite[:, :, None, None], blocks, 0.0).astype(np.float32)
        return self.score_blocks(blocks, norms, order=CHANNELS, engine=engine)

