"""Capture golden vectors of the reference's training step under DROPOUT.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_dropout.py

Imports the UNMODIFIED reference `emphases` with the stand-ins of
`tests/golden/stubs/` (through `generate_train.py`, whose helpers it shares),
sets `emphases.DROPOUT = P` before `emphases.Model()` is built - so that
every layer is `Sequential(conv, activation, Dropout)`,
`model/layers/convolution.py:25-33` -, loads the reference's shipped
checkpoint with its `2 i` names mapped to `3 i`, and replaces every
`torch.nn.Dropout` INSTANCE by a module that multiplies by a fixed mask and
by 1 / (1 - P).  The mask is the package's specification
(`emphases_amd/train/dropout.py`, numpy): the mask of layer l for utterance
u is `keep_mask(seed, stream(l), step, 80 ld, P)` as [80, ld], cut at the
utterance's columns of the packed layout (`frame_off`, `word_off`,
`ld_frames`, `ld_words` of the plan: host arithmetic).

Inputs: the `ragged` case stored in train.npz (6 utterances, 635 frames, 65
words).  Every utterance runs ALONE, weighted n_i / N, as `generate_train.py`'s
`accumulate` does.  Per case the loss (float64), the float64 gradients under
the package's internal names (stored as float32) and `ref32_error`: the worst
over tensors of max|g32 - g64| / max|g64| of the same run in float32, its
mask module scaling by float32(1 / (1 - P)).

  p10   P = 0.1, seed 20261018, step 0: every tensor (dropout_grads_<k>.npz)
  p50   P = 0.5, seed 20261018, step 3: the tensors of VARIANT_TENSORS

and `p10/mask_bits`: `np.packbits` of the stream-1 mask of `p10` for the first
utterance [80, 5], which pins the addressing.

Output (committed): tests/golden/dropout.npz, tests/golden/dropout_grads_<k>.npz.
The GPU box never runs this script; it only reads the .npz files.
"""
import glob
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import generate_train as base  # noqa: E402  (paths, stubs, the reference)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases  # noqa: E402  (the reference)
import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import core as api  # noqa: E402
from emphases_amd import train  # noqa: E402
from emphases_amd.train import dropout as spec  # noqa: E402

SEED = 20261018
CASES = {'p10': (0.1, 0), 'p50': (0.5, 3)}       # name -> (P, step)
CHANNELS = 80


class FixedMask(torch.nn.Module):
    """In place of a `torch.nn.Dropout`: x * mask / (1 - p) for the utterance
    `CURRENT[0]`, `masks[u]` a 0/1 array [80, n_u]."""
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
    """The packed layout `Trainer.prepare` gives the `ragged` batch."""
    batch = train_data.collated('ragged')
    frames, words, bounds = train.check_batch(*batch)
    return api._packed_plan(frames, torch.from_numpy(bounds), words)


def layer_masks(config, plan, name, p, step):
    """[utterance] -> 0/1 [80, n_u] of layer `name`."""
    frame_rate = name.startswith('frame_encoder')
    ld = plan.ld_frames if frame_rate else plan.ld_words
    offsets = plan.frame_off if frame_rate else plan.word_off
    counts = plan.frames if frame_rate else plan.words
    whole = spec.keep_mask(
        SEED, spec.stream_of(config, name), step, CHANNELS * ld, p).reshape(
            CHANNELS, ld)
    return [np.ascontiguousarray(whole[:, int(off):int(off) + int(count)])
            for off, count in zip(offsets, counts)]


def model(dtype, config, plan, p, step):
    assert emphases.DROPOUT == p
    net = emphases.Model()
    saved = train.checkpoint_names(config)
    state = torch.load(base.CHECKPOINT, map_location='cpu', weights_only=False)
    net.load_state_dict(
        {saved[name]: value for name, value in state['model'].items()})
    replaced = 0
    for prefix in ('frame_encoder', 'word_decoder'):
        stack = getattr(net, prefix)
        assert len(stack) == 3 * config.layers
        for i in range(config.layers):
            assert isinstance(stack[3 * i + 2], torch.nn.Dropout)
            stack[3 * i + 2] = FixedMask(
                layer_masks(config, plan, f'{prefix}.{2 * i}', p, step), p)
            replaced += 1
    assert replaced == 2 * config.layers and not any(
        isinstance(module, torch.nn.Dropout) for module in net.modules())
    net.train()
    return net.to(dtype)


def accumulate(net, items, dtype):
    """`generate_train.accumulate` with the utterance announced to the masks."""
    net.zero_grad()
    total_words = sum(item[1].shape[1] for item in items)
    total = torch.zeros((), dtype=dtype)
    for index, item in enumerate(items):
        FixedMask.CURRENT[0] = index
        weight = item[1].shape[1] / total_words
        value = base.forward_loss(net, base.single(item, dtype), 'bce') * weight
        value.backward()
        total = total + value.detach()
    return float(total)


def internal(config, gradients):
    """The reference's `3 i` names back to the package's internal ones."""
    saved = train.checkpoint_names(config)
    assert set(saved.values()) == set(gradients)
    return {name: gradients[saved[name]] for name in saved}


def ragged_items():
    data = train_data.golden()
    items, frame, word = [], 0, 0
    for frames, words in zip(data['ragged/frames'], data['ragged/words']):
        items.append((
            data['ragged/features'][:, frame:frame + frames],
            data['ragged/bounds'][:, word:word + words],
            data['ragged/targets'][word:word + words]))
        frame, word = frame + frames, word + words
    return items


def main():
    items = ragged_items()
    plan = packed_plan()
    assert list(plan.frames) == [i[0].shape[1] for i in items]
    out, big = {}, {}
    for case, (p, step) in CASES.items():
        config = emphases_amd.Config(dropout=p)
        emphases.DROPOUT = p
        wide = model(torch.float64, config, plan, p, step)
        loss = accumulate(wide, items, torch.float64)
        exact = internal(config, base.gradients(wide))
        narrow = model(torch.float32, config, plan, p, step)
        accumulate(narrow, items, torch.float32)
        rounded = internal(config, base.gradients(narrow))
        emphases.DROPOUT = None
        for name, value in exact.items():
            assert np.abs(value).max() > 0, f'{case}: {name}: zero gradient'
        error = max(
            np.abs(rounded[name] - exact[name]).max() /
            np.abs(exact[name]).max() for name in exact)
        out[f'{case}/loss'], out[f'{case}/ref32_error'] = loss, error
        out[f'{case}/p'], out[f'{case}/step'] = p, step
        out[f'{case}/seed'] = SEED
        print(case, 'loss', loss, 'ref32', error)
        if case == 'p10':
            big.update({f'{case}/{name}': value for name, value in exact.items()})
            first = layer_masks(config, plan, 'frame_encoder.0', p, step)[0]
            assert first.shape == (CHANNELS, items[0][0].shape[1])
            out['p10/mask_bits'] = np.packbits(first.ravel())
        else:
            for name, value in exact.items():
                if name.rsplit('.', 1)[0] in base.VARIANT_TENSORS:
                    out[f'{case}/grad/{name}'] = value.astype(np.float32)

    for stale in glob.glob(os.path.join(HERE, 'dropout_grads_*.npz')):
        os.remove(stale)
    files, current, size = [], {}, 0
    for name, value in big.items():
        value = value.astype(np.float32)
        if current and size + value.nbytes > base.FILE_LIMIT:
            files.append(current)
            current, size = {}, 0
        current[name] = value
        size += value.nbytes
    files.append(current)
    paths = [(os.path.join(HERE, 'dropout.npz'), out)] + [
        (os.path.join(HERE, f'dropout_grads_{k}.npz'), content)
        for k, content in enumerate(files)]
    for path, content in paths:
        np.savez_compressed(path, **content)
        print(path, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < 1 << 20
    leaked = [root for root, dirs, _ in os.walk(base.REFERENCE)
              if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
