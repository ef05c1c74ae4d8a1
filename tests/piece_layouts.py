"""Hard layouts of DOWNSAMPLE_LOCATION = 'input': per layout, per utterance
(frames, bounds int64 [2, W]) - what the piece builder, the pooling backward
and `train.PieceTrainer` are tried on."""
import numpy as np
import torch

from emphases_amd import core as api


def _back_to_back(lengths, first=0):
    ends = first + np.cumsum(lengths)
    return np.stack([ends - lengths, ends]).astype(np.int64)


def _short_words(seed, count, low, high):
    return np.random.default_rng(seed).integers(low, high + 1, count)


def layouts():
    many = [_short_words(seed, 120, 1, 9) for seed in (1, 2, 3)]
    beside = np.concatenate(
        [_short_words(4, 20, 1, 12), [300], _short_words(5, 19, 1, 12)])
    return {
        # L = n: no padding at all
        'one_word': [(5, _back_to_back(np.array([5])))],
        # L = 1, and 17 crosses the 16-column alignment of the word axis
        'one_frame_words': [(17, _back_to_back(np.ones(17, dtype=np.int64)))],
        # gaps before, between and after the words
        'gaps': [(40, np.array([[3, 9, 22], [7, 18, 31]], dtype=np.int64)),
                 (12, np.array([[2, 8], [3, 10]], dtype=np.int64))],
        # a piece of exactly one tile and one of a tile and a column
        'tile_edge': [(65, _back_to_back(np.array([64, 1]))),
                      (66, _back_to_back(np.array([1, 65])))],
        # 40 pieces of 300 columns: five tiles each, mostly padding
        'long_word': [(int(beside.sum()), _back_to_back(beside))],
        # 360 pieces: the weight gradient has more than one part
        'many_words': [(int(n.sum()), _back_to_back(n)) for n in many],
    }


ALL_METHODS = ('one_word', 'one_frame_words', 'gaps')
METHODS = ('sum', 'average', 'max', 'center')


def cases():
    """(layout, method): all four methods on the first three layouts, 'sum'
    and 'max' on the rest."""
    return [(name, method) for name in layouts()
            for method in (METHODS if name in ALL_METHODS else
                           ('sum', 'max'))]


def plan_of(layout):
    frames = [f for f, _ in layout]
    words = [b.shape[1] for _, b in layout]
    bounds = torch.zeros(len(layout), 2, max(words), dtype=torch.long)
    for i, (_, b) in enumerate(layout):
        bounds[i, :, :b.shape[1]] = torch.from_numpy(b)
    return api._packed_plan(frames, bounds, words)


def items_of(layout, seed=0, features=80):
    """Per utterance (features [C, T], bounds, targets [W]) float32, seeded."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((features, frames)).astype(np.float32),
             bounds, rng.random(bounds.shape[1]).astype(np.float32))
            for frames, bounds in layout]
