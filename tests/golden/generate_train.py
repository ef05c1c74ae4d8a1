"""Capture golden vectors of the reference's training step.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_train.py

Imports the UNMODIFIED reference `emphases` with the stand-ins of
`tests/golden/stubs/` (as `generate_evaluate.py` does) and runs, on the CPU
with one thread, its `Model` in train mode, `emphases.train.loss`
(`train/core.py:315-353`), autograd and `torch.optim.Adam` - without autocast
and GradScaler - from the reference's own shipped checkpoint.

Cases (inputs are stored, not regenerated):

  ragged    6 utterances of 5, 37, 64, 100, 129, 300 frames and 1, 3, 7, 12,
            2, 40 words that tile each utterance (random interior cuts, at
            least one one-frame word).  Every utterance goes through the
            reference ALONE; the loss is the mean over all words,
            sum_i (n_i / N) loss_i, and the backward calls accumulate.  The
            loss of the reference's padded batch is recorded too
            (`ragged/padded_loss`): it differs, see DESIGN.md.
  uniform   4 utterances x 48 frames x 6 words: ONE padded-batch call of the
            reference (no padding, so the two semantics coincide).
  variants  `ragged` with LOSS = 'mse' and with DOWNSAMPLE_METHOD = 'average':
            the loss and the gradients of output_layer.*, word_decoder.0.*,
            frame_encoder.10.* and input_layer.* (where the changed path
            enters).

Per case: the loss (float64) and the gradient of every parameter from the
reference in float64 (`model.double()`), and `ref32_error`, the worst over
tensors of max|g32 - g64| / max|g64| for the same run in float32.  The float64
gradients are STORED rounded to float32 (6e-8 of each value, a hundredth of
the tests' bound) and spread over `train_grads_<k>.npz`, every file below
1 MiB.

Adam: the losses of steps 0..5 of five updates on `ragged` in float32, in
float64, and in float32 with the utterances accumulated in reverse order;
the loss of a step is added up in the run's own arithmetic (a float32 run
reports a float32 loss).

Initial weights: sum, sum of squares (float64 of the float32 values) and the
first 8 values of every tensor of `emphases.Model()` after
`torch.manual_seed(0)`.

Output (committed): tests/golden/train.npz, tests/golden/train_grads_<k>.npz.
The GPU box never runs this script; it only reads the .npz files.
"""
import glob
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
CHECKPOINT = os.path.join(
    REFERENCE, 'emphases', 'assets', 'checkpoints', 'checkpoint.pt')
RAGGED = ([5, 37, 64, 100, 129, 300], [1, 3, 7, 12, 2, 40])
UNIFORM = ([48] * 4, [6] * 4)
VARIANT_TENSORS = ('output_layer', 'word_decoder.0', 'frame_encoder.10',
                   'input_layer')
FILE_LIMIT = 900 * 1024          # raw bytes per gradient file (< 1 MiB)


def make_case(seed, frames, words):
    """Features, word bounds that tile each utterance, targets."""
    rng = np.random.default_rng(seed)
    items = []
    for count, length in zip(frames, words):
        cuts = np.sort(rng.choice(
            np.arange(1, count), size=length - 1, replace=False))
        edges = np.concatenate([[0], cuts, [count]]).astype(np.int64)
        items.append((
            rng.standard_normal((80, count)).astype(np.float32),
            np.stack([edges[:-1], edges[1:]]),
            rng.uniform(0., 1., length).astype(np.float32)))
    return items


def model(dtype):
    net = emphases.Model()
    state = torch.load(CHECKPOINT, map_location='cpu', weights_only=False)
    net.load_state_dict(state['model'])
    net.train()
    return net.to(dtype)


def single(item, dtype):
    features, bounds, targets = item
    return (torch.from_numpy(features)[None].to(dtype),
            torch.tensor([features.shape[1]]),
            torch.from_numpy(bounds)[None],
            torch.tensor([bounds.shape[1]]),
            torch.from_numpy(targets)[None, None].to(dtype))


def padded(items, dtype):
    """The reference's own collate (`data/collate.py`)."""
    batch = emphases.data.collate([
        (torch.from_numpy(f), torch.from_numpy(t)[None], torch.from_numpy(b),
         None, torch.zeros(1, f.shape[1] * emphases.HOPSIZE), str(i))
        for i, (f, b, t) in enumerate(items)])
    features, frame_lengths, bounds, word_lengths, targets = batch[:5]
    return (features.to(dtype), frame_lengths, bounds, word_lengths,
            targets.to(dtype))


def forward_loss(net, batch, loss_fn):
    features, frame_lengths, bounds, word_lengths, targets = batch
    scores = net(features, frame_lengths, bounds, word_lengths)
    # (`emphases.train` is the function `train`: `from .core import *`)
    return sys.modules['emphases.train.core'].loss(
        scores, targets, frame_lengths, bounds, word_lengths, training=True,
        loss_fn=loss_fn)


def accumulate(net, items, dtype, loss_fn, order=None):
    """Every utterance alone, (n_i / N)-weighted: loss, gradients left in
    `.grad`."""
    net.zero_grad()
    total_words = sum(item[1].shape[1] for item in items)
    total = torch.zeros((), dtype=dtype)
    for index in (order or range(len(items))):
        item = items[index]
        weight = item[1].shape[1] / total_words
        value = forward_loss(net, single(item, dtype), loss_fn) * weight
        value.backward()
        # (in the run's own arithmetic: a float32 run reports a float32 loss)
        total = total + value.detach()
    return float(total)


def gradients(net):
    return {name: parameter.grad.detach().double().numpy().copy()
            for name, parameter in net.named_parameters()}


def measure(run):
    """(loss64, gradients64, ref32_error) of `run(net, dtype) -> loss`."""
    wide = model(torch.float64)
    loss = run(wide, torch.float64)
    exact = gradients(wide)
    narrow = model(torch.float32)
    run(narrow, torch.float32)
    rounded = gradients(narrow)
    for name, value in exact.items():
        assert np.abs(value).max() > 0, f'{name}: zero gradient'
    error = max(
        np.abs(rounded[name] - exact[name]).max() / np.abs(exact[name]).max()
        for name in exact)
    return loss, exact, error


def trajectory(items, dtype, order=None, updates=5):
    net = model(dtype)
    optimizer = torch.optim.Adam(net.parameters())
    losses = []
    for step in range(updates + 1):
        losses.append(accumulate(net, items, dtype, 'bce', order))
        if step < updates:
            optimizer.step()
    return np.array(losses, dtype=np.float64)


def store_inputs(out, case, items):
    out[f'{case}/frames'] = np.array(
        [i[0].shape[1] for i in items], dtype=np.int64)
    out[f'{case}/words'] = np.array(
        [i[1].shape[1] for i in items], dtype=np.int64)
    out[f'{case}/features'] = np.concatenate([i[0] for i in items], axis=1)
    out[f'{case}/bounds'] = np.concatenate([i[1] for i in items], axis=1)
    out[f'{case}/targets'] = np.concatenate([i[2] for i in items])


def main():
    assert emphases.DROPOUT is None and emphases.LOSS == 'bce'
    out, big = {}, {}
    ragged = None
    for seed in range(20261017, 20261117):
        ragged = make_case(seed, *RAGGED)
        if any((b[1] - b[0]).min() == 1 for _, b, _ in ragged[1:]):
            break
    assert any((b[1] - b[0]).min() == 1 for _, b, _ in ragged[1:])
    uniform = make_case(20261018, *UNIFORM)
    store_inputs(out, 'ragged', ragged)
    store_inputs(out, 'uniform', uniform)

    # ---- ragged: every utterance alone
    loss, exact, error = measure(
        lambda net, dtype: accumulate(net, ragged, dtype, 'bce'))
    out['ragged/loss'], out['ragged/ref32_error'] = loss, error
    big.update({f'ragged/{name}': value for name, value in exact.items()})
    with torch.no_grad():
        out['ragged/padded_loss'] = float(forward_loss(
            model(torch.float64), padded(ragged, torch.float64), 'bce'))
    print('ragged', loss, 'padded', out['ragged/padded_loss'], 'ref32', error)

    # ---- uniform: one padded-batch call
    def batch_run(net, dtype):
        net.zero_grad()
        value = forward_loss(net, padded(uniform, dtype), 'bce')
        value.backward()
        return float(value.detach().double())
    loss, exact, error = measure(batch_run)
    out['uniform/loss'], out['uniform/ref32_error'] = loss, error
    big.update({f'uniform/{name}': value for name, value in exact.items()})
    print('uniform', loss, 'ref32', error)

    # ---- variants of ragged
    for variant, loss_fn, method in (
            ('mse', 'mse', 'sum'), ('average', 'bce', 'average')):
        emphases.DOWNSAMPLE_METHOD = method
        loss, exact, error = measure(
            lambda net, dtype: accumulate(net, ragged, dtype, loss_fn))
        emphases.DOWNSAMPLE_METHOD = 'sum'
        out[f'{variant}/loss'], out[f'{variant}/ref32_error'] = loss, error
        for name, value in exact.items():
            if name.rsplit('.', 1)[0] in VARIANT_TENSORS:
                out[f'{variant}/grad/{name}'] = value.astype(np.float32)
        print(variant, loss, 'ref32', error)

    # ---- five Adam updates on ragged
    out['adam/float32'] = trajectory(ragged, torch.float32)
    out['adam/float64'] = trajectory(ragged, torch.float64)
    out['adam/float32_reversed'] = trajectory(
        ragged, torch.float32, order=list(range(len(ragged)))[::-1])
    for name in ('float32', 'float64', 'float32_reversed'):
        print('adam', name, out[f'adam/{name}'])
    assert np.all(np.diff(out['adam/float32']) < 0)

    # ---- initial weights
    torch.manual_seed(0)
    for name, parameter in emphases.Model().named_parameters():
        value = parameter.detach().numpy()
        out[f'init/{name}'] = np.array(
            [value.astype(np.float64).sum(),
             (value.astype(np.float64) ** 2).sum()])
        out[f'init_head/{name}'] = value.ravel()[:8].copy()

    for stale in glob.glob(os.path.join(HERE, 'train_grads_*.npz')):
        os.remove(stale)
    files, current, size = [], {}, 0
    for name, value in big.items():
        value = value.astype(np.float32)
        if current and size + value.nbytes > FILE_LIMIT:
            files.append(current)
            current, size = {}, 0
        current[name] = value
        size += value.nbytes
    files.append(current)
    paths = [(os.path.join(HERE, 'train.npz'), out)] + [
        (os.path.join(HERE, f'train_grads_{k}.npz'), content)
        for k, content in enumerate(files)]
    for path, content in paths:
        np.savez_compressed(path, **content)
        print(path, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < 1 << 20
    leaked = [
        root for root, dirs, _ in os.walk(REFERENCE) if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
