"""`emphases.data.Dataset` (`emphases/data/dataset.py:16-113`) for training on
the GPU: the whole partition is read from the reference-layout cache ONCE,
checked once, and kept on the device as one feature matrix and one target
array, from which `emph_collate` assembles every batch (`data.Loader`).

    <cache_dir>/<name>/mels/<stem>.pt                   [80, T]
                       pitch/<stem>-pitch.pt            [1, T]   config.pitch_feature
                       pitch/<stem>-periodicity.pt      [1, T]   config.periodicity_feature
                       loudness/<stem>.pt               [1, T]   config.loudness_feature
                       scores/<stem>.pt                 [W]
                       alignment/<stem>.TextGrid
    <partition_dir>/<name>.json                         {partition: [stems]}

Every utterance starts on a multiple of 16 columns of the feature matrix (and
of 16 elements of the target array), so its rows move as 16-byte loads.  The
lengths, word bounds and offsets stay on the host as numpy arrays: they are
what the batch plans are made of.

The frame count of an utterance is that of its cached features.  The reference
reads it from the audio header (`dataset.py:26-31`); its preprocessing makes
the two equal, and the audio itself is not needed to train.
"""
import json
import os

import numpy as np
import torch

from .. import alignment as alignment_module
from .. import config as cfg
from .. import runtime

BUCKETS = 2        # emphases/config/defaults.py:224
ALIGN = 16         # columns between the starts of two utterances: a multiple


def _round_up(value, multiple):
    return (value + multiple - 1) // multiple * multiple


def feature_files(config):
    """[(directory, suffix)] of the cached feature files, in the row order of
    the reference's concatenation (`dataset.py:55-83`)."""
    listed = []
    if config.mel_feature:
        listed.append(('mels', ''))
    if config.pitch_feature:
        listed.append(('pitch', '-pitch'))
    if config.periodicity_feature:
        listed.append(('pitch', '-periodicity'))
    if config.loudness_feature:
        listed.append(('loudness', ''))
    return listed


def _load(path):
    return torch.load(path, map_location='cpu', weights_only=True)


class Dataset:
    """`Dataset(name, partition)` of the reference over a device-resident copy.

    Host side (numpy): `stems`, `lengths` (frames), `words`, `frame_first` /
    `word_first` (where an utterance starts in the resident arrays),
    `bounds` (int64 [2, sum(words)], utterance by utterance, silences
    included, clamped to the frame count as a Python slice would) and
    `bound_first`.  Device side: `features` [C, ld_cache], `targets`
    [total_words] (float32).  `upload=False` is for tests of the host side
    alone: the arrays stay on the host (`host_features`, `host_targets`), no
    GPU is needed, and no `Loader` takes the dataset until `upload()`."""

    def __init__(self, name, partition, *, partition_dir,
                 cache_dir='data/cache', config=None, gpu=None, upload=True):
        from .. import core
        self.name, self.partition = name, partition
        self.config = config = config or core.active_config()
        self.cache = os.path.join(os.fspath(cache_dir), name)
        path = os.path.join(os.fspath(partition_dir), f'{name}.json')
        if not os.path.isfile(path):
            raise FileNotFoundError(f'partition file {path} not found')
        with open(path, encoding='utf-8') as file:
            chosen = json.load(file).get(partition) or []
        if not chosen:
            raise ValueError(
                f'dataset {name}: the {partition!r} partition of {path} is '
                'empty')
        self.stems = [str(stem) for stem in chosen]
        self._files = feature_files(config)
        if not self._files:
            raise ValueError('the configuration selects no feature')
        # every file is there before anything is read or uploaded
        for stem in self.stems:
            for file in self.paths(stem):
                if not os.path.isfile(file):
                    raise FileNotFoundError(
                        f'{name}/{stem}: {file} not found')
        self._read()
        self.features = self.targets = self.device = None
        if upload:
            self.upload(gpu)

    def paths(self, stem):
        """Every file of an utterance: features in row order, scores,
        alignment."""
        return [os.path.join(self.cache, directory, f'{stem}{suffix}.pt')
                for directory, suffix in self._files] + [
            os.path.join(self.cache, 'scores', f'{stem}.pt'),
            os.path.join(self.cache, 'alignment', f'{stem}.TextGrid')]

    ###########################################################################
    # Host
    ###########################################################################

    def _rows(self, stem):
        """The feature rows of an utterance, float32 [C, T] (`dataset.py:55-83`)."""
        config, rows = self.config, []
        for directory, suffix in self._files:
            file = os.path.join(self.cache, directory, f'{stem}{suffix}.pt')
            value = torch.as_tensor(_load(file), dtype=torch.float32)
            value = value.reshape(-1, value.shape[-1])
            if suffix == '-pitch':
                value = torch.log2(value)
                if config.normalize:
                    value = (value - cfg.LOGFMIN) / (cfg.LOGFMAX - cfg.LOGFMIN)
            rows.append(value)
        frames = rows[0].shape[-1]
        if any(value.shape[-1] != frames for value in rows):
            raise ValueError(
                f'{self.name}/{stem}: the cached features disagree on the '
                f'frame count ({[int(v.shape[-1]) for v in rows]})')
        rows = rows[0] if len(rows) == 1 else torch.cat(rows)
        if rows.shape[0] != config.num_features or frames < 1:
            raise ValueError(
                f'{self.name}/{stem}: features {tuple(rows.shape)}, wanted '
                f'[{config.num_features}, T >= 1]')
        return rows.numpy()

    def _words(self, stem, frames):
        """(bounds int64 [2, W], targets float32 [W]) of an utterance, checked
        by the rules of `train.check_batch`."""
        label = f'{self.name}/{stem}'
        alignment = alignment_module.Alignment(
            os.path.join(self.cache, 'alignment', f'{stem}.TextGrid'))
        bounds = np.asarray(alignment.word_bounds(
            cfg.SAMPLE_RATE, cfg.HOPSIZE, silences=True),
            dtype=np.int64).reshape(-1, 2).T                # dataset.py:45-50
        bounds = np.clip(bounds, 0, frames)     # xs[..., start:end] clamps
        starts, ends = bounds
        if not bounds.shape[1]:
            raise ValueError(f'{label}: the alignment has no word')
        if np.any(ends <= starts):
            word = int(np.argmax(ends <= starts))
            raise ValueError(
                f'{label}: word {word} is empty inside the {frames} frames '
                f'({int(starts[word])}..{int(ends[word])})')
        if np.any(starts[1:] < ends[:-1]):
            raise ValueError(f'{label}: words overlap or are not in order')
        targets = torch.as_tensor(_load(os.path.join(
            self.cache, 'scores', f'{stem}.pt')), dtype=torch.float32)
        targets = targets.reshape(-1).numpy()
        if targets.size < bounds.shape[1]:
            raise ValueError(
                f'{label}: {targets.size} targets for {bounds.shape[1]} words')
        return np.ascontiguousarray(bounds), targets[:bounds.shape[1]]

    def _read(self):
        rows = [self._rows(stem) for stem in self.stems]
        self.lengths = np.array([r.shape[1] for r in rows], dtype=np.int64)
        words = [self._words(stem, int(frames))
                 for stem, frames in zip(self.stems, self.lengths)]
        self.words = np.array([b.shape[1] for b, _ in words], dtype=np.int64)
        self.bounds = np.concatenate([b for b, _ in words], axis=1)
        self.bound_first = np.cumsum(self.words) - self.words
        padded = _round_up(self.lengths, ALIGN)
        self.frame_first = np.cumsum(padded) - padded
        self.ld_cache = int(padded.sum())
        padded = _round_up(self.words, ALIGN)
        self.word_first = np.cumsum(padded) - padded
        self.total_words = int(padded.sum())
        self.frames = int(self.lengths.sum())               # dataset.py:34
        self.host_features = np.zeros(
            (self.config.num_features, self.ld_cache), dtype=np.float32)
        self.host_targets = np.zeros(self.total_words, dtype=np.float32)
        for first, row in zip(self.frame_first, rows):
            self.host_features[:, first:first + row.shape[1]] = row
        for first, (_, targets) in zip(self.word_first, words):
            self.host_targets[first:first + targets.size] = targets

    def word_bounds(self, index):
        """int64 [2, W] of an utterance (`__getitem__`'s `word_bounds`)."""
        first = self.bound_first[index]
        return self.bounds[:, first:first + self.words[index]]

    ###########################################################################
    # Device
    ###########################################################################

    def upload(self, gpu=None):
        """One copy each of the features and the targets; the host copies are
        dropped."""
        self.device = runtime.require_gpu(gpu)
        with torch.cuda.device(self.device):
            self.features = torch.from_numpy(self.host_features).to(self.device)
            self.targets = torch.from_numpy(self.host_targets).to(self.device)
        self.host_features = self.host_targets = None
        return self

    ###########################################################################
    # `torch.utils.data.Dataset`
    ###########################################################################

    def __len__(self):
        return len(self.stems)

    def buckets(self):
        """`dataset.py:94-113`: the indices in order of length, cut into
        BUCKETS buckets of (index, length) rows; a remainder joins the last."""
        size = max(len(self) // BUCKETS, 1)
        order = np.argsort(self.lengths)
        table = np.stack((order, np.sort(self.lengths))).T
        buckets = [table[i:i + size] for i in range(0, len(self), size)]
        if len(buckets) == BUCKETS + 1:
            rest = buckets.pop()
            buckets[-1] = np.concatenate((buckets[-1], rest), axis=0)
        return buckets
