"""The golden vectors of the training step (tests/golden/train.npz and
train_grads_<k>.npz, written by tests/golden/generate_train.py) as the
collated batches the reference's loader yields."""
import functools
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
VARIANTS = {'mse': {'loss': 'mse'}, 'average': {'downsample_method': 'average'}}


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLDEN, 'train.npz')) as archive:
        return {name: archive[name] for name in archive.files}


@functools.lru_cache(maxsize=None)
def gradients(case):
    """{parameter name: the reference's float64 gradient (stored as float32)}
    of a case or a variant."""
    if case in VARIANTS:
        prefix = f'{case}/grad/'
        return {name[len(prefix):]: value.astype(np.float64)
                for name, value in golden().items() if name.startswith(prefix)}
    found = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'train_grads_*.npz'))):
        with np.load(path) as archive:
            for name in archive.files:
                if name.startswith(case + '/'):
                    found[name[len(case) + 1:]] = \
                        archive[name].astype(np.float64)
    return found


def collated(case):
    """(features [B, 80, Tmax], frame_lengths, word_bounds [B, 2, Wmax],
    word_lengths, targets [B, 1, Wmax]) of a case: what `emphases.data.collate`
    makes of its utterances."""
    data = golden()
    case = 'ragged' if case in VARIANTS else case
    frames, words = data[f'{case}/frames'], data[f'{case}/words']
    features = torch.zeros(len(frames), 80, int(frames.max()))
    bounds = torch.zeros(len(frames), 2, int(words.max()), dtype=torch.long)
    targets = torch.zeros(len(frames), 1, int(words.max()))
    frame_first = np.cumsum(frames) - frames
    word_first = np.cumsum(words) - words
    for i, (f0, f, w0, w) in enumerate(
            zip(frame_first, frames, word_first, words)):
        features[i, :, :f] = torch.from_numpy(
            data[f'{case}/features'][:, f0:f0 + f])
        bounds[i, :, :w] = torch.from_numpy(
            data[f'{case}/bounds'][:, w0:w0 + w])
        targets[i, 0, :w] = torch.from_numpy(
            data[f'{case}/targets'][w0:w0 + w])
    return (features, torch.from_numpy(frames), bounds,
            torch.from_numpy(words), targets)
