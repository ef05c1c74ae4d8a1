"""Capture golden vectors of the reference's training step for two variants
of its hyperparameter grid that `emphases_amd.train.GridTrainer` trains and no
other golden covers.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_grid_step.py

Shares `generate_grid.py`'s set-up and helpers (the UNMODIFIED reference with
the stand-ins of `tests/golden/stubs/`, on the CPU with one thread and without
autocast, LAYERS = 2 from the reference's own initialisation under
`torch.manual_seed(seed)`, the stored `ragged` inputs of train.npz, one
utterance at a time, loss = sum_i (n_i / N) loss_i) and writes files of the
same format (tests/golden/gridstep_<variant>.npz: seed, loss, ref32_error,
init/<name> = [sum, sum of squares], grad/<name> from the float64 run, stored
as float32, all under the package's internal names):

  center     DOWNSAMPLE_METHOD 'center' at DOWNSAMPLE_LOCATION 'intermediate'
  gelu_p10   torch.nn.GELU with DROPOUT = 0.1: every layer is
             `Sequential(conv, activation, Dropout)`
             (`model/layers/convolution.py:25-33`) and every
             `torch.nn.Dropout` INSTANCE is replaced, as `generate_dropout.py`
             does, by a module that multiplies by a fixed mask and by
             1 / (1 - P) (float32(1 / (1 - P)) in the float32 run).  The mask
             is the package's specification (`emphases_amd/train/dropout.py`):
             `keep_mask(seed, stream_of(config, layer), STEP, channels ld, P)`
             as [channels, ld], cut at each utterance's columns of the packed
             plan; `seed` is the seed of the initialisation, as a trainer has
             one seed for both.  The file also stores `p` and `step`.

The GPU box never runs this script; it only reads the .npz files.
"""
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import generate_grid as grid  # noqa: E402  (paths, stubs, the reference)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases  # noqa: E402  (the reference)
import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import core as api  # noqa: E402
from emphases_amd import train  # noqa: E402
from emphases_amd.train import dropout as spec  # noqa: E402

SEED = 0
STEP = 0
P = 0.1
VARIANTS = {
    'center': (dict(DOWNSAMPLE_METHOD='center'),
               dict(downsample_method='center')),
    'gelu_p10': (dict(ACTIVATION_FUNCTION=torch.nn.GELU),
                 dict(activation='gelu', dropout=P)),
}


class FixedMask(torch.nn.Module):
    """In place of a `torch.nn.Dropout`: x * mask / (1 - p) for the utterance
    `CURRENT[0]`, `masks[u]` a 0/1 array [channels, n_u]."""
    CURRENT = [None]

    def __init__(self, masks, p):
        super().__init__()
        self.masks, self.p = masks, p

    def forward(self, x):
        mask = torch.from_numpy(self.masks[self.CURRENT[0]]).to(x.dtype)
        if x.dtype == torch.float32:
            return x * mask[None] * torch.tensor(spec.scale(self.p))
        return x * mask[None] * (1. / (1. - self.p))


def packed_plan():
    """The packed layout `GridTrainer.prepare` gives the `ragged` batch."""
    frames, words, bounds = train.check_batch(*train_data.collated('ragged'))
    return api._packed_plan(frames, torch.from_numpy(bounds), words)


def layer_masks(config, plan, name, seed):
    """[utterance] -> 0/1 [channels, n_u] of layer `name`."""
    frame_rate = name.startswith('frame_encoder')
    ld = plan.ld_frames if frame_rate else plan.ld_words
    offsets = plan.frame_off if frame_rate else plan.word_off
    counts = plan.frames if frame_rate else plan.words
    whole = spec.keep_mask(
        seed, spec.stream_of(config, name), STEP, config.channels * ld,
        config.dropout).reshape(config.channels, ld)
    return [np.ascontiguousarray(whole[:, int(off):int(off) + int(count)])
            for off, count in zip(offsets, counts)]


def model(seed, dtype, config, plan):
    net = grid.model(seed, dtype)
    if config.dropout is None:
        return net
    replaced = 0
    for prefix in ('frame_encoder', 'word_decoder'):
        stack = getattr(net, prefix)
        assert len(stack) == 3 * config.layers
        for i in range(config.layers):
            assert isinstance(stack[3 * i + 2], torch.nn.Dropout)
            stack[3 * i + 2] = FixedMask(
                layer_masks(config, plan, f'{prefix}.{2 * i}', seed),
                config.dropout)
            replaced += 1
    assert replaced == 2 * config.layers and not any(
        isinstance(module, torch.nn.Dropout) for module in net.modules())
    return net


def accumulate(net, items, dtype):
    """`generate_grid.accumulate` with the utterance announced to the masks."""
    net.zero_grad()
    loss_of = sys.modules['emphases.train.core'].loss
    total_words = sum(item[1].shape[1] for item in items)
    total = 0.
    for index, (features, bounds, targets) in enumerate(items):
        FixedMask.CURRENT[0] = index
        frame_lengths = torch.tensor([features.shape[1]])
        word_bounds = torch.from_numpy(bounds)[None]
        word_lengths = torch.tensor([bounds.shape[1]])
        scores = net(torch.from_numpy(features)[None].to(dtype), frame_lengths,
                     word_bounds, word_lengths)
        value = loss_of(
            scores, torch.from_numpy(targets)[None, None].to(dtype),
            frame_lengths, word_bounds, word_lengths, training=True,
            loss_fn='bce') * (bounds.shape[1] / total_words)
        value.backward()
        total += float(value.detach().double())
    return total


def internal(config, values):
    """The reference's names (`3 i` under DROPOUT) to the package's."""
    saved = train.checkpoint_names(config)
    assert set(saved.values()) == set(values)
    return {name: values[saved[name]] for name in saved}


def capture(variant, settings, fields, items, plan):
    config = emphases_amd.Config(layers=grid.LAYERS, **fields)
    for name, value in {**grid.DEFAULTS, **settings}.items():
        setattr(emphases, name, value)
    emphases.LAYERS = grid.LAYERS
    emphases.DROPOUT = config.dropout
    try:
        wide = model(SEED, torch.float64, config, plan)
        loss = accumulate(wide, items, torch.float64)
        exact = internal(config, grid.gradients(wide))
        narrow = model(SEED, torch.float32, config, plan)
        accumulate(narrow, items, torch.float32)
        rounded = internal(config, grid.gradients(narrow))
        initial = internal(config, {
            name: parameter.detach().double().numpy() for name, parameter in
            grid.model(SEED, torch.float32).named_parameters()})
    finally:
        emphases.DROPOUT = None
        for name, value in grid.DEFAULTS.items():
            setattr(emphases, name, value)
    for name, value in exact.items():
        assert np.abs(value).max() > 0, f'{variant} {name}: zero gradient'
    error = max(
        np.abs(rounded[name] - exact[name]).max() / np.abs(exact[name]).max()
        for name in exact)
    out = {'seed': np.int64(SEED), 'loss': np.float64(loss),
           'ref32_error': np.float64(error)}
    if config.dropout is not None:
        out['p'], out['step'] = np.float64(config.dropout), np.int64(STEP)
    for name, value in initial.items():
        out[f'init/{name}'] = np.array([value.sum(), (value ** 2).sum()])
    for name, value in exact.items():
        out[f'grad/{name}'] = value.astype(np.float32)
    path = os.path.join(HERE, f'gridstep_{variant}.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(variant, 'seed', SEED, 'loss', loss, 'ref32', error, size, 'bytes')
    assert size < 1 << 20


def main():
    assert emphases.DROPOUT is None and emphases.LOSS == 'bce'
    items = grid.ragged()
    plan = packed_plan()
    assert list(plan.frames) == [item[0].shape[1] for item in items]
    for variant, (settings, fields) in VARIANTS.items():
        capture(variant, settings, fields, items, plan)
    leaked = [root for root, dirs, _ in os.walk(grid.REFERENCE)
              if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
