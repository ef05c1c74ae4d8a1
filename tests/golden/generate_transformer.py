"""Capture golden vectors of the reference's Transformer under autograd, for
`emphases_amd.train.TransformerModel`.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_transformer.py

Imports the UNMODIFIED reference `emphases` with the stand-ins of
`tests/golden/stubs/` (as `generate_grid.py` does) and runs, on the CPU with
one thread and without autocast, its `Model` under ARCHITECTURE =
'transformer' with LAYERS = 2 in `.eval()` (every dropout off: the model under
test draws none) WITH autograd enabled, its loss and its backward, from the
reference's own initialisation under `torch.manual_seed(seed)`, one utterance
at a time (loss = sum_i (n_i / N) loss_i; the backward calls accumulate).

`Transformer.__init__` takes its depth from a default argument that is bound
when the reference is imported (`transformer.py:15`), where its own
configuration files would have set LAYERS already; this script sets the
bound default after the import instead, which builds the same module.

Configs (everything else as `config/defaults.py`):

  intermediate_sum  DOWNSAMPLE_LOCATION 'intermediate', DOWNSAMPLE_METHOD 'sum'
                    (the word decoder is a second Transformer over the words)
  loss_max          'loss', 'max' (no word decoder)

Batch (stored): three utterances of 37, 64 and 130 frames with 3, 5 and 9
words that tile each utterance; unit-normal features, uniform targets.

tests/golden/transformer_train.npz: the batch and, per config, the seed, the
loss and the logits (float64), `ref32_error` - the worst over the gradients,
the logits and the loss of max|x32 - x64| / max|x64| for the same run in
float32 - and the initial state: the reference builds a stack as ONE layer
cloned LAYERS times, so layer 0 of each stack is stored and `clones` says that
the generator found the others equal to it.
tests/golden/transformer_train_grads_<config>.npz: the gradient of every
parameter from the float64 run, STORED rounded to float32 (6e-8 of each
value, far below the tests' bound) so that every file stays below 1 MiB.

'max': a float32 run must choose the same frame as float64; the generator
asserts that, in float64, no word's two largest values lie within 1e-4
(relative) of each other on any channel, and moves to the next seed otherwise.

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
FRAMES, WORDS = (37, 64, 130), (3, 5, 9)
CONFIGS = {
    'intermediate_sum': dict(
        DOWNSAMPLE_LOCATION='intermediate', DOWNSAMPLE_METHOD='sum'),
    'loss_max': dict(DOWNSAMPLE_LOCATION='loss', DOWNSAMPLE_METHOD='max'),
}
TIE_MARGIN = 1e-4


def make_batch():
    """Per utterance: (features [80, T], bounds [2, W], targets [W])."""
    random = np.random.default_rng(20260)
    items = []
    for frames, words in zip(FRAMES, WORDS):
        cuts = np.sort(random.choice(
            np.arange(1, frames), size=words - 1, replace=False))
        edges = np.concatenate([[0], cuts, [frames]]).astype(np.int64)
        items.append((
            random.standard_normal((80, frames)).astype(np.float32),
            np.stack([edges[:-1], edges[1:]]),
            random.uniform(0., 1., words).astype(np.float32)))
    return items


def model(seed, dtype):
    torch.manual_seed(seed)
    net = emphases.Model()
    net.eval()
    return net.to(dtype)


def accumulate(net, items, dtype, watch=None):
    """Every utterance alone, (n_i / N)-weighted: (loss, logits); the
    gradients are left in `.grad`."""
    net.zero_grad()
    total_words = sum(item[1].shape[1] for item in items)
    total, logits = 0., []
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
            watch(seen[0][0], bounds)
        value = sys.modules['emphases.train.core'].loss(
            scores, torch.from_numpy(targets)[None, None].to(dtype),
            frame_lengths, word_bounds, word_lengths, training=True,
            loss_fn='bce') * (bounds.shape[1] / total_words)
        value.backward()
        total += float(value.detach().double())
        logits.append(scores.detach().double().numpy().reshape(-1))
    return total, np.concatenate(logits)


def gradients(net):
    return {name: parameter.grad.detach().double().numpy().copy()
            for name, parameter in net.named_parameters()}


def no_near_ties(embeddings, bounds):
    for start, end in bounds.T:
        if end - start < 2:
            continue
        top = torch.topk(embeddings[:, start:end], 2, dim=1).values
        close = top[:, 0] - top[:, 1] <= TIE_MARGIN * top[:, 0].abs()
        if bool(close.any()):
            raise ArithmeticError('two maxima of a word within the margin')


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
    for seed in range(100):
        try:
            wide = model(seed, torch.float64)
            loss, logits = accumulate(
                wide, items, torch.float64, no_near_ties if is_max else None)
            break
        except ArithmeticError:
            print(name, 'seed', seed, 'has a near tie; next')
    else:
        raise ArithmeticError(f'{name}: every seed has a near tie')
    assert len(wide.frame_encoder.model.layers) == LAYERS
    exact = gradients(wide)
    narrow = model(seed, torch.float32)
    loss32, logits32 = accumulate(narrow, items, torch.float32)
    rounded = gradients(narrow)
    for key, value in exact.items():
        assert np.abs(value).max() > 0, f'{name} {key}: zero gradient'
    error = max([relative(rounded[key], exact[key]) for key in exact] +
                [relative(logits32, logits), abs(loss32 - loss) / abs(loss)])
    out[f'{name}/seed'] = np.int64(seed)
    out[f'{name}/loss'] = np.float64(loss)
    out[f'{name}/logits'] = logits
    out[f'{name}/ref32_error'] = np.float64(error)
    initial = {key: value.detach().numpy().copy() for key, value in
               model(seed, torch.float32).named_parameters()}
    clones = True
    for key, value in initial.items():
        if '.model.layers.' in key:
            prefix, rest = key.split('.model.layers.')
            index, rest = rest.split('.', 1)
            first = initial[f'{prefix}.model.layers.0.{rest}']
            clones = clones and np.array_equal(first, value)
            if index != '0':
                continue
        out[f'{name}/init/{key}'] = value
    out[f'{name}/clones'] = np.bool_(clones)
    assert clones
    grads = {key: value.astype(np.float32) for key, value in exact.items()}
    path = os.path.join(HERE, f'transformer_train_grads_{name}.npz')
    np.savez_compressed(path, **grads)
    size = os.path.getsize(path)
    print(name, 'seed', seed, 'loss', loss, 'ref32', error, size, 'bytes')
    assert size < 1 << 20


def main():
    assert emphases.DROPOUT is None and emphases.LOSS == 'bce'
    assert emphases.CHANNELS == 80
    items = make_batch()
    out = {
        'frames': np.array(FRAMES, dtype=np.int64),
        'words': np.array(WORDS, dtype=np.int64),
        'features': np.concatenate([item[0] for item in items], axis=1),
        'bounds': np.concatenate([item[1] for item in items], axis=1),
        'targets': np.concatenate([item[2] for item in items]),
        'configs': np.array(list(CONFIGS)),
    }
    for name, settings in CONFIGS.items():
        capture(name, settings, items, out)
    path = os.path.join(HERE, 'transformer_train.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20
    leaked = [
        root for root, dirs, _ in os.walk(REFERENCE) if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
