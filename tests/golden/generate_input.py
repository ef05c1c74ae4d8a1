"""Capture golden vectors of the reference's training step at
DOWNSAMPLE_LOCATION = 'input' (`model/core.py:41-87`, `core.py:552-586`): what
`emphases_amd.train.PieceTrainer` is held to.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_input.py

Imports the UNMODIFIED reference `emphases` with the stand-ins of
`tests/golden/stubs/` (as `generate_grid.py` does) and runs, on the CPU with
one thread and without autocast, its `Model` in train mode, its loss and
autograd with LAYERS = 2 from the reference's own initialisation under
`torch.manual_seed(seed)`, on the stored `ragged` inputs of
tests/golden/train.npz (6 utterances, 1..40 words, word lengths 1..80), one
utterance at a time (loss = sum_i (n_i / N) loss_i; the backward calls
accumulate): every word is padded to the longest word of its own utterance.

Variants (everything else as `config/defaults.py`):

  sum, average, max, center   DOWNSAMPLE_METHOD
  average_mse                 'average', LOSS 'mse'

Per variant (tests/golden/input_<variant>.npz): the seed, the loss (float64),
the gradients from the reference in float64 (`model.double()`), STORED rounded
to float32, `ref32_error` - the worst over tensors of
max|g32 - g64| / max|g64| for the same run in float32 - and, instead of the
weights, the sum and the sum of squares of every initial tensor: the test
rebuilds them from the seed.

'max': a float32 run must choose the same column as float64.  Inside a piece
of a word of n frames padded to L, the columns [n + 3, L - 2) see only zeros
through the three k = 3 layers (the input layer's own 'same' padding is as
zero as the piece's, so the right edge is felt from the second layer on, two
columns deep, not three): they hold one value per channel - asserted - and
carry identical gradients, so they count as ONE candidate.  The generator asserts
that, in float64, no piece's two largest distinct candidates lie within 1e-4
(relative) of each other on any channel whose maximum is positive, and moves
to the next seed otherwise.

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
DEPTH = LAYERS + 1          # k = 3 layers in front of the pooling
DEFAULTS = dict(
    DOWNSAMPLE_METHOD='sum', DOWNSAMPLE_LOCATION='input',
    ACTIVATION_FUNCTION=torch.nn.ReLU, CHANNELS=80, ENCODER_KERNEL_SIZE=3,
    DECODER_KERNEL_SIZE=3)
VARIANTS = {
    'sum': dict(DOWNSAMPLE_METHOD='sum'),
    'average': dict(DOWNSAMPLE_METHOD='average'),
    'max': dict(DOWNSAMPLE_METHOD='max'),
    'center': dict(DOWNSAMPLE_METHOD='center'),
    'average_mse': dict(DOWNSAMPLE_METHOD='average', LOSS='mse'),
}
TIE_MARGIN = 1e-4


def ragged():
    """The stored inputs of generate_train.py's `ragged` case, per utterance:
    (features [80, T], bounds [2, W], targets [W])."""
    with np.load(os.path.join(HERE, 'train.npz')) as data:
        frames, words = data['ragged/frames'], data['ragged/words']
        features, bounds = data['ragged/features'], data['ragged/bounds']
        targets = data['ragged/targets']
    items, f0, w0 = [], 0, 0
    for f, w in zip(frames, words):
        items.append((features[:, f0:f0 + f], bounds[:, w0:w0 + w],
                      targets[w0:w0 + w]))
        f0, w0 = f0 + f, w0 + w
    return items


def model(seed, dtype):
    torch.manual_seed(seed)
    net = emphases.Model()
    net.train()
    return net.to(dtype)


def accumulate(net, items, dtype, loss_fn, watch=None):
    """Every utterance alone, (n_i / N)-weighted: the loss; the gradients are
    left in `.grad`.  `watch(piece_embeddings [W, C, L], bounds)` sees what
    the pooling reads."""
    net.zero_grad()
    total_words = sum(item[1].shape[1] for item in items)
    total = 0.
    for features, bounds, targets in items:
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
            watch(seen[0], bounds)
        value = sys.modules['emphases.train.core'].loss(
            scores, torch.from_numpy(targets)[None, None].to(dtype),
            frame_lengths, word_bounds, word_lengths, training=True,
            loss_fn=loss_fn) * (bounds.shape[1] / total_words)
        value.backward()
        total += float(value.detach().double())
    return total


def gradients(net):
    return {name: parameter.grad.detach().double().numpy().copy()
            for name, parameter in net.named_parameters()}


def no_near_ties(embeddings, bounds):
    padded = embeddings.shape[2]
    for piece, (start, end) in zip(embeddings, bounds.T):
        length = int(end - start)
        flat = list(range(min(length + DEPTH, padded), max(padded - LAYERS, 0)))
        columns = [t for t in range(padded) if t not in flat]
        if len(flat):
            assert bool((piece[:, flat] == piece[:, flat[:1]]).all())
            columns.append(flat[0])
        if len(columns) < 2:
            continue
        top = torch.topk(piece[:, columns], 2, dim=1).values
        close = (top[:, 0] > 0) & \
            (top[:, 0] - top[:, 1] <= TIE_MARGIN * top[:, 0].abs())
        if bool(close.any()):
            raise ArithmeticError('two maxima of a piece within the margin')


def capture(variant, settings, items):
    for name, value in {**DEFAULTS, **settings}.items():
        if name != 'LOSS':
            setattr(emphases, name, value)
    emphases.LAYERS = LAYERS
    loss_fn = settings.get('LOSS', 'bce')
    is_max = settings.get('DOWNSAMPLE_METHOD') == 'max'
    for seed in range(100):
        try:
            wide = model(seed, torch.float64)
            loss = accumulate(wide, items, torch.float64, loss_fn,
                              no_near_ties if is_max else None)
            break
        except ArithmeticError:
            print(variant, 'seed', seed, 'has a near tie; next')
    else:
        raise ArithmeticError(f'{variant}: every seed has a near tie')
    exact = gradients(wide)
    narrow = model(seed, torch.float32)
    accumulate(narrow, items, torch.float32, loss_fn)
    rounded = gradients(narrow)
    for name, value in exact.items():
        assert np.abs(value).max() > 0, f'{variant} {name}: zero gradient'
    error = max(
        np.abs(rounded[name] - exact[name]).max() / np.abs(exact[name]).max()
        for name in exact)
    out = {'seed': np.int64(seed), 'loss': np.float64(loss),
           'ref32_error': np.float64(error)}
    for name, parameter in model(seed, torch.float32).named_parameters():
        value = parameter.detach().double().numpy()
        out[f'init/{name}'] = np.array([value.sum(), (value ** 2).sum()])
    for name, value in exact.items():
        out[f'grad/{name}'] = value.astype(np.float32)
    path = os.path.join(HERE, f'input_{variant}.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(variant, 'seed', seed, 'loss', loss, 'ref32', error, size, 'bytes')
    assert size < 1 << 20


def main():
    assert emphases.DROPOUT is None and emphases.LOSS == 'bce'
    items = ragged()
    for variant, settings in VARIANTS.items():
        capture(variant, settings, items)
    leaked = [
        root for root, dirs, _ in os.walk(REFERENCE) if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
