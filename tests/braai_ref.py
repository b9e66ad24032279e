"""float64 numpy forward of the layer family the real / bogus network uses, written from the layer definitions
(Keras: Conv2D 'valid' stride 1, MaxPooling2D stride = size 'valid', Flatten channels-last, Dense), and what the
real / bogus tests share: the two test networks, weights from a seed, stamps, the rescaled last layer, the tolerance.

Tensors are channels-last, [n, H, W, C], as Keras holds them; kernels [kh, kw, cin, cout]; Dense kernels [in, out].
A layer list is [('conv', activation), ('pool', size), ('flatten',), ('dense', activation)] with the weights in one
flat list in ``model.get_weights()`` order (kernel, bias per Conv2D / Dense)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
VGG6_JSON = os.path.join(GOLDEN, 'braai_vgg6.architecture.json')


def activation(x, name):
    if name == 'relu':
        return np.maximum(x, 0.0)
    if name == 'sigmoid':
        return 1.0 / (1.0 + np.exp(-x))
    assert name == 'linear', name
    return x


def conv2d_valid(x, k, b):
    """out[n, i, j, o] = b[o] + sum_{u, v, c} x[n, i + u, j + v, c] k[u, v, c, o] (cross-correlation, as Keras)."""
    n, H, W, C = x.shape
    kh, kw, cin, cout = k.shape
    assert cin == C
    out = np.zeros((n, H - kh + 1, W - kw + 1, cout))
    for u in range(kh):
        for v in range(kw):
            out += x[:, u:u + H - kh + 1, v:v + W - kw + 1, :] @ k[u, v]
    return out + b


def maxpool(x, p):
    """Windows of p x p at stride p; rows / columns beyond the last whole window are dropped."""
    n, H, W, C = x.shape
    oh, ow = H // p, W // p
    return x[:, :oh * p, :ow * p, :].reshape(n, oh, p, ow, p, C).max(axis=(2, 4))


def flatten(x):
    return x.reshape(x.shape[0], -1)          # C order of [H, W, C]: (h, w, c)


def forward(layers, weights, x, upto=None):
    """The network on x [n, H, W, C] (float64).  ``upto``: stop behind that many layers."""
    x = np.asarray(x, dtype=np.float64)
    w = iter(weights)
    for k, l in enumerate(layers):
        if upto is not None and k == upto:
            break
        if l[0] == 'conv':
            x = activation(conv2d_valid(x, np.asarray(next(w), np.float64), np.asarray(next(w), np.float64)), l[1])
        elif l[0] == 'pool':
            x = maxpool(x, l[1])
        elif l[0] == 'flatten':
            x = flatten(x)
        elif l[0] == 'dense':
            x = activation(x @ np.asarray(next(w), np.float64) + np.asarray(next(w), np.float64), l[1])
        else:
            raise ValueError(l)
    return x


# ---- the test networks ---------------------------------------------------------------------------------------------
def keras_json(in_size, in_channels, layers, name='net'):
    """Keras ``model.to_json()`` text of a Sequential model: [('conv', filters, activation), ('pool', size), ('flatten',),
    ('dropout', rate), ('dense', units, activation)]."""
    out = []
    for k, l in enumerate(layers):
        if l[0] == 'conv':
            c = dict(name=f'conv{k}', trainable=True, dtype='float32', filters=l[1], kernel_size=[3, 3], strides=[1, 1],
                     padding='valid', data_format='channels_last', dilation_rate=[1, 1], activation=l[2], use_bias=True)
            out.append(dict(class_name='Conv2D', config=c))
        elif l[0] == 'pool':
            out.append(dict(class_name='MaxPooling2D', config=dict(name=f'pool{k}', trainable=True, dtype='float32',
                                                                   pool_size=[l[1], l[1]], padding='valid',
                                                                   strides=[l[1], l[1]], data_format='channels_last')))
        elif l[0] == 'flatten':
            out.append(dict(class_name='Flatten', config=dict(name='flatten', trainable=True, dtype='float32',
                                                              data_format='channels_last')))
        elif l[0] == 'dropout':
            out.append(dict(class_name='Dropout', config=dict(name=f'drop{k}', trainable=True, dtype='float32', rate=l[1],
                                                              noise_shape=None, seed=None)))
        elif l[0] == 'dense':
            out.append(dict(class_name='Dense', config=dict(name=f'fc{k}', trainable=True, dtype='float32', units=l[1],
                                                            activation=l[2], use_bias=True)))
    out[0]['config']['batch_input_shape'] = [None, in_size, in_size, in_channels]
    return json.dumps(dict(class_name='Sequential', config=dict(name=name, layers=out), keras_version='2.2.4-tf',
                           backend='tensorflow'))


# 9 x 9 x 3 -> conv 5 channels (7 x 7) -> conv 7 channels (5 x 5) -> pool 2 (5 -> 2, the odd row and column dropped) ->
# flatten 28 -> dense 6 -> dense 1
TINY = (9, 3, [('conv', 5, 'relu'), ('conv', 7, 'relu'), ('pool', 2), ('flatten',), ('dense', 6, 'relu'),
               ('dense', 1, 'sigmoid')])
# 11 x 11: the pool sees 7 -> 3; a linear convolution; a Dense wide enough for the thread-per-unit kernel, ragged against
# its block of 256
TINY_WIDE = (11, 3, [('conv', 5, 'relu'), ('conv', 7, 'linear'), ('pool', 2), ('flatten',), ('dense', 70, 'relu'),
                    ('dense', 1, 'sigmoid')])


def ref_layers(spec):
    """The layer list ``forward`` takes, from a spec as ``keras_json`` takes it (Dropout dropped)."""
    out = []
    for l in spec:
        if l[0] == 'conv':
            out.append(('conv', l[2]))
        elif l[0] == 'pool':
            out.append(('pool', l[1]))
        elif l[0] == 'flatten':
            out.append(('flatten',))
        elif l[0] == 'dense':
            out.append(('dense', l[2]))
    return out


def vgg6_spec():
    """(in_size, in_channels, spec) read from the golden architecture file (independent of the product's parser)."""
    doc = json.load(open(VGG6_JSON))
    spec = []
    for ent in doc['config']['layers']:
        c = ent['config']
        kind = ent['class_name']
        if kind == 'Conv2D':
            spec.append(('conv', c['filters'], c['activation']))
        elif kind == 'MaxPooling2D':
            spec.append(('pool', c['pool_size'][0]))
        elif kind == 'Flatten':
            spec.append(('flatten',))
        elif kind == 'Dropout':
            spec.append(('dropout', c['rate']))
        elif kind == 'Dense':
            spec.append(('dense', c['units'], c['activation']))
    shape = doc['config']['layers'][0]['config']['batch_input_shape']
    return shape[1], shape[3], spec


def glorot_weights(in_size, in_channels, spec, seed):
    """Glorot-uniform kernels, small uniform biases, float32, in get_weights() order."""
    rng = np.random.default_rng(seed)
    out, H, C, flat = [], in_size, in_channels, None
    for l in spec:
        if l[0] == 'conv':
            fan_in, fan_out = 9 * C, 9 * l[1]
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            out += [rng.uniform(-lim, lim, (3, 3, C, l[1])).astype(np.float32),
                    rng.uniform(-0.05, 0.05, l[1]).astype(np.float32)]
            C, H = l[1], H - 2
        elif l[0] == 'pool':
            H //= l[1]
        elif l[0] == 'flatten':
            flat = H * H * C
        elif l[0] == 'dense':
            lim = np.sqrt(6.0 / (flat + l[1]))
            out += [rng.uniform(-lim, lim, (flat, l[1])).astype(np.float32),
                    rng.uniform(-0.05, 0.05, l[1]).astype(np.float32)]
            flat = l[1]
    return out


def make_stamps(n, size, seed, planes=3):
    """Gaussian blobs plus noise: blocks [n, planes, size, size] float32 and their float64 L2 norms [n, planes]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:size, :size].astype(np.float64)
    blocks = np.zeros((n, planes, size, size), np.float32)
    for i in range(n):
        for p in range(planes):
            cx, cy = size / 2 + rng.uniform(-0.2, 0.2, 2) * size
            sig = rng.uniform(0.05, 0.2) * size
            amp = rng.uniform(-30.0, 200.0)
            img = amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sig * sig)) + rng.normal(0.0, 5.0, (size, size)) \
                + rng.uniform(-3, 3)
            blocks[i, p] = img.astype(np.float32)
    norms = np.sqrt((blocks.astype(np.float64) ** 2).sum(axis=(2, 3)))
    return blocks, norms


def triplets_of(blocks, norms, plane_of_channel=(0, 1, 2)):
    """[n, S, S, C] float64: channel c = plane plane_of_channel[c] / its norm (make_triplet_for_braai's arithmetic)."""
    poc = list(plane_of_channel)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = blocks[:, poc].astype(np.float64) / norms[:, poc][:, :, None, None]
    return np.ascontiguousarray(np.moveaxis(t, 1, 3))


def rescale_last(layers, weights, x, lo=0.05, hi=0.95):
    """Weights whose last Dense layer is scaled and shifted so that the reference's scores over ``x`` span [lo, hi]
    and beyond: with Glorot weights every logit is 0 +- 1e-3 and every score 0.5.  The logits' range over ``x`` is
    mapped onto 1.2 x [logit(lo), logit(hi)]."""
    assert layers[-1] == ('dense', 'sigmoid')
    feats = forward(layers, weights, x, upto=len(layers) - 1)
    k, b = np.asarray(weights[-2], np.float64), np.asarray(weights[-1], np.float64)
    z = (feats @ k + b).ravel()
    a, c = z.min(), z.max()
    assert c > a
    want = 1.2 * np.log(hi / (1 - hi))
    s = 2 * want / (c - a)
    out = list(weights[:-2]) + [(k * s).astype(np.float32), ((b - (a + c) / 2) * s).astype(np.float32)]
    return out


# ---- the tolerance: fp32 against fp64 torch forward on exactly the given inputs ---------------------------------------
def torch_forward(layers, weights, x, dtype):
    """torch.nn.functional forward on the CPU: conv2d / max_pool2d on [n, C, H, W] (layouts permuted), flatten permuted
    back to (h, w, c)."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(np.asarray(x, np.float64), 3, 1))).to(dtype)
    w = iter(weights)
    act = {'relu': torch.relu, 'sigmoid': torch.sigmoid, 'linear': lambda v: v}
    for l in layers:
        if l[0] == 'conv':
            k, b = torch.from_numpy(np.asarray(next(w))).to(dtype), torch.from_numpy(np.asarray(next(w))).to(dtype)
            t = act[l[1]](F.conv2d(t, k.permute(3, 2, 0, 1).contiguous(), b))
        elif l[0] == 'pool':
            t = F.max_pool2d(t, l[1], stride=l[1])
        elif l[0] == 'flatten':
            t = t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)
        elif l[0] == 'dense':
            k, b = torch.from_numpy(np.asarray(next(w))).to(dtype), torch.from_numpy(np.asarray(next(w))).to(dtype)
            t = act[l[1]](t @ k + b)
    return t.to(torch.float64).numpy()


def measured_spread(layers, weights, x):
    """Largest |rb(float32 torch) - rb(float64 torch)| over the inputs x."""
    import torch
    a = torch_forward(layers, weights, x, torch.float32)
    b = torch_forward(layers, weights, x, torch.float64)
    return float(np.abs(a - b).max())


GPU_FACTOR = 8          # the GPU bound: 8 x the measured spread (two fp32 forwards differ in summation order only; the
                        # longest sum has 1152 terms against torch's blocked order)


_CASES = {}


def case(name, n, seed=77):
    """A test case computed once and shared: dict(spec, layers, json, weights (rescaled), blocks, norms, x, ref, tol)."""
    key = (name, n, seed)
    if key in _CASES:
        return _CASES[key]
    if name == 'vgg6':
        size, ch, spec = vgg6_spec()
        text = open(VGG6_JSON).read()
    else:
        size, ch, spec = {'tiny': TINY, 'tiny_wide': TINY_WIDE}[name]
        text = keras_json(size, ch, spec, name)
    layers = ref_layers(spec)
    blocks, norms = make_stamps(n, size, seed)
    x = triplets_of(blocks, norms)
    weights = rescale_last(layers, glorot_weights(size, ch, spec, seed + 1), x)
    ref = forward(layers, weights, x).ravel()
    tol = GPU_FACTOR * measured_spread(layers, weights, x)
    for a in (blocks, norms, x, ref):
        a.setflags(write=False)
    _CASES[key] = dict(name=name, spec=spec, layers=layers, json=text, weights=weights, blocks=blocks, norms=norms, x=x,
                       ref=ref, tol=tol, size=size)
    return _CASES[key]


def choose_cut(ref, tol, groups=None):
    """A cut for the end-to-end tests: the middle of the widest gap between neighbouring reference scores that leaves
    rows on both sides in every group (``groups``: one label per score; default one group), so that the cut removes and
    keeps something everywhere and no score lies near it.  The distance is asserted: 100 tolerances."""
    ref = np.asarray(ref, dtype=np.float64)
    groups = np.zeros(ref.size, int) if groups is None else np.asarray(groups)
    s = np.sort(ref[np.isfinite(ref)])
    best = None
    for a, b in zip(s[:-1], s[1:]):
        cut = 0.5 * (a + b)
        if all((ref[groups == g] < cut).any() and (ref[groups == g] >= cut).any() for g in np.unique(groups)):
            if best is None or b - a > best[0]:
                best = (b - a, cut)
    assert best is not None, 'no cut splits every group'
    cut = float(best[1])
    assert np.abs(s - cut).min() > 100 * tol, (np.abs(s - cut).min(), tol)       # move the cut, never the tolerance
    return cut


def model_for(x, seed=501):
    """VGG6 with seeded weights whose last layer is rescaled over the triplets ``x``: (json text, weights, layers,
    reference scores, GPU tolerance for exactly these inputs)."""
    size, ch, spec = vgg6_spec()
    layers = ref_layers(spec)
    weights = rescale_last(layers, glorot_weights(size, ch, spec, seed), x)
    ref = forward(layers, weights, x).ravel()
    assert ref.min() < 0.05 and ref.max() > 0.95
    return open(VGG6_JSON).read(), weights, layers, ref, GPU_FACTOR * measured_spread(layers, weights, x)
