"""Capture golden vectors of the reference's Transformer under autograd at
DOWNSAMPLE_LOCATION 'input' and 'inference', for
`emphases_amd.train.TransformerLocationsModel`.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_transformer_locations.py

Follows `generate_transformer.py` point for point: the UNMODIFIED reference
with the stand-ins of `tests/golden/stubs/`, on the CPU with one thread and
without autocast, ARCHITECTURE = 'transformer' with LAYERS = 2 (set as that
script sets it), autograd enabled, from the reference's own initialisation
under `torch.manual_seed(seed)`, a float64 and a float32 run, one utterance at
a time (loss = sum_i (n_i / N) loss_i with n the utterance's words - or, at
'inference', where the loss is a mean over FRAMES, its frames; the backward
calls accumulate).  One utterance at a time also makes the reference pad
every word to the longest word of its utterance, the project's piece layout.

Configs (everything else as `config/defaults.py`):

  input_average     DOWNSAMPLE_LOCATION 'input', DOWNSAMPLE_METHOD 'average'
  input_max         'input', 'max'
  input_center      'input', 'center'
  inference_linear  'inference', 'sum', UPSAMPLE_METHOD 'linear'

The 'input' configs run in `.eval()` (every dropout off: the model under test
draws none).  'inference_linear' must run in `.train()` to take the
frame-rate branch (`model/core.py:119-122`) and the upsampled targets
(`train/core.py:324-336`); AFTER construction this script sets `p` of every
`torch.nn.Dropout` and `dropout` of every `MultiheadAttention` to 0, so that
nothing is dropped there either.

Batch (stored, and asserted below): a one-frame word; a word of 70 frames in
an utterance whose other words are under 20 frames; an utterance of a single
word of 80 frames (no padding, n = k > 64).

tests/golden/transformer_locations.npz: the batch and, per config, the seed,
the loss and the logits (float64; frame rate at 'inference_linear') and
`ref32_error` - the worst over the gradients, the logits and the loss of
max|x32 - x64| / max|x64| for the same run in float32.
tests/golden/transformer_locations_grads_<config>.npz: the gradient of every
parameter from the float64 run, STORED rounded to float32.

'max': a float32 run must choose the same position as float64; the generator
asserts that, in float64, no piece's two largest values over the PADDED axis
lie within 1e-4 (relative) of each other on any channel, and moves to the
next seed otherwise.

The GPU box never runs this script; it only reads the .npz files.
"""
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = '/root/reference'
sys.path[:0] = [os.path.join(HERE, 'stubs'), REFERENCE, ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases  # noqa: E402  (the reference)

torch.set_num_threads(1)
LAYERS = 2
EDGES = ([0, 1, 12, 30, 37], [0, 5, 75, 90, 91, 110], [0, 80])
CONFIGS = {
    'input_average': dict(
        DOWNSAMPLE_LOCATION='input', DOWNSAMPLE_METHOD='average'),
    'input_max': dict(DOWNSAMPLE_LOCATION='input', DOWNSAMPLE_METHOD='max'),
    'input_center': dict(
        DOWNSAMPLE_LOCATION='input', DOWNSAMPLE_METHOD='center'),
    'inference_linear': dict(
        DOWNSAMPLE_LOCATION='inference', DOWNSAMPLE_METHOD='sum',
        UPSAMPLE_METHOD='linear'),
}
TIE_MARGIN = 1e-4


def make_batch():
    """Per utterance: (features [80, T], bounds [2, W], targets [W])."""
    random = np.random.default_rng(20262)
    items = []
    for edges in EDGES:
        edges = np.asarray(edges, dtype=np.int64)
        items.append((
            random.standard_normal((80, int(edges[-1]))).astype(np.float32),
            np.stack([edges[:-1], edges[1:]]),
            random.uniform(0., 1., edges.size - 1).astype(np.float32)))
    lengths = [np.diff(edges) for edges in EDGES]
    assert any(1 in n for n in lengths), 'a one-frame word'
    assert any(n.max() >= 65 and np.sort(n)[-2] < 20
               for n in lengths if n.size > 1), 'a long word among short ones'
    assert any(n.size == 1 and n[0] > 64 for n in lengths), 'a single word'
    return items


def model(seed, dtype, training):
    torch.manual_seed(seed)
    net = emphases.Model()
    net.train(training)
    if training:
        for module in net.modules():
            if isinstance(module, torch.nn.Dropout):
                module.p = 0.
            if isinstance(module, torch.nn.MultiheadAttention):
                module.dropout = 0.
    return net.to(dtype)


def accumulate(net, items, dtype, by_frames, watch=None):
    """Every utterance alone, (n_i / N)-weighted: (loss, logits); the
    gradients are left in `.grad`."""
    net.zero_grad()
    count = (lambda item: item[0].shape[1]) if by_frames else \
        (lambda item: item[1].shape[1])
    whole = sum(count(item) for item in items)
    total, logits = 0., []
    for item in items:
        features, bounds, targets = item
        seen = []
        hook = net.frame_encoder.register_forward_hook(
            lambda module, inputs, output: seen.append(output.detach()))
        frame_lengths = torch.tensor([features.shape[1]])
        word_bounds = torch.from_numpy(bounds)[None]
        word_lengths = torch.tensor([bounds.shape[1]])
        scores = net(torch.from_numpy(features)[None].to(dtype), frame_lengths,
                     word_bounds, word_lengths)
        hook.remove()
        if watch is not None:
            watch(seen[0])
        value = sys.modules['emphases.train.core'].loss(
            scores, torch.from_numpy(targets)[None, None].to(dtype),
            frame_lengths, word_bounds, word_lengths, training=True,
            loss_fn='bce') * (count(item) / whole)
        value.backward()
        total += float(value.detach().double())
        logits.append(scores.detach().double().numpy().reshape(-1))
    return total, np.concatenate(logits)


def gradients(net):
    return {name: parameter.grad.detach().double().numpy().copy()
            for name, parameter in net.named_parameters()}


def no_near_ties(embeddings):
    """`embeddings` [pieces, C, L]: the maximum over the padded axis."""
    if embeddings.shape[2] < 2:
        return
    top = torch.topk(embeddings, 2, dim=2).values
    close = top[..., 0] - top[..., 1] <= TIE_MARGIN * top[..., 0].abs()
    if bool(close.any()):
        raise ArithmeticError('two maxima of a piece within the margin')


def relative(narrow, exact):
    return float(np.abs(narrow - exact).max() / np.abs(exact).max())


def capture(name, settings, items, out):
    emphases.ARCHITECTURE = 'transformer'
    emphases.LAYERS = LAYERS
    for key, value in settings.items():
        setattr(emphases, key, value)
    transformer = sys.modules['emphases.model.layers.transformer'].Transformer
    transformer.__init__.__defaults__ = (LAYERS, emphases.CHANNELS)
    is_max = settings['DOWNSAMPLE_METHOD'] == 'max'
    training = settings['DOWNSAMPLE_LOCATION'] == 'inference'
    for seed in range(100):
        try:
            wide = model(seed, torch.float64, training)
            loss, logits = accumulate(
                wide, items, torch.float64, training,
                no_near_ties if is_max else None)
            break
        except ArithmeticError:
            print(name, 'seed', seed, 'has a near tie; next')
    else:
        raise ArithmeticError(f'{name}: every seed has a near tie')
    assert len(wide.frame_encoder.model.layers) == LAYERS
    assert logits.size == sum(
        item[0].shape[1] if training else item[1].shape[1] for item in items)
    exact = gradients(wide)
    narrow = model(seed, torch.float32, training)
    loss32, logits32 = accumulate(narrow, items, torch.float32, training)
    rounded = gradients(narrow)
    for key, value in exact.items():
        assert np.abs(value).max() > 0, f'{name} {key}: zero gradient'
    error = max([relative(rounded[key], exact[key]) for key in exact] +
                [relative(logits32, logits), abs(loss32 - loss) / abs(loss)])
    out[f'{name}/seed'] = np.int64(seed)
    out[f'{name}/loss'] = np.float64(loss)
    out[f'{name}/logits'] = logits
    out[f'{name}/ref32_error'] = np.float64(error)
    grads = {key: value.astype(np.float32) for key, value in exact.items()}
    path = os.path.join(HERE, f'transformer_locations_grads_{name}.npz')
    np.savez_compressed(path, **grads)
    size = os.path.getsize(path)
    print(name, 'seed', seed, 'loss', loss, 'ref32', error, size, 'bytes')
    assert size < 1 << 20


def main():
    assert emphases.DROPOUT is None and emphases.LOSS == 'bce'
    assert emphases.CHANNELS == 80
    items = make_batch()
    out = {
        'frames': np.array([item[0].shape[1] for item in items]),
        'words': np.array([item[1].shape[1] for item in items]),
        'features': np.concatenate([item[0] for item in items], axis=1),
        'bounds': np.concatenate([item[1] for item in items], axis=1),
        'targets': np.concatenate([item[2] for item in items]),
        'configs': np.array(list(CONFIGS)),
    }
    for name, settings in CONFIGS.items():
        capture(name, settings, items, out)
    path = os.path.join(HERE, 'transformer_locations.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20
    leaked = [
        root for root, dirs, _ in os.walk(REFERENCE) if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
