"""A synthetic reference-layout training cache (`<cache>/<dataset>/{mels,
pitch,loudness,scores,alignment}`, a partition file) of 12 utterances, the
golden vectors of tests/golden/loop.npz (written by
tests/golden/generate_loop.py), and the collated batches the reference's loader
would make of the cache's files on the host."""
import functools
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DATASET = 'synthetic'
FRAMES = [1, 5, 16, 17, 63, 64, 65, 100, 129, 255, 256, 300]
WORDS = [1, 1, 3, 16, 17, 2, 7, 12, 2, 33, 5, 40]     # silences included
STEMS = [f'utt-{index:02d}' for index in range(len(FRAMES))]
VALID = [1, 4, 7, 10]
TRAIN = [index for index in range(len(FRAMES)) if index not in VALID]
MAX_FRAMES = (600, 75000)
EPOCHS = (0, 1, 2)
SEED = 20261018


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(HERE, 'golden', 'loop.npz')) as archive:
        return {name: archive[name] for name in archive.files}


def edges(index):
    """Frame edges [W + 1] that tile utterance `index` into its words, and
    which of the words are silences (gaps of the alignment file)."""
    rng = np.random.default_rng(SEED + index)
    frames, words = FRAMES[index], WORDS[index]
    cuts = np.sort(rng.choice(
        np.arange(1, frames), size=words - 1, replace=False))
    silent = np.zeros(words, dtype=bool)
    if words >= 3:
        silent[1 + int(rng.integers(0, words - 2))] = True
    return np.concatenate([[0], cuts, [frames]]).astype(np.int64), silent


def alignment(index):
    """The utterance's words without its silences (`Alignment` puts a silence
    into every gap); times a quarter frame past the frame edges, so that the
    truncation to frames (`word_bounds`) is safe from rounding."""
    from emphases_amd.alignment import Alignment, Word
    bounds, silent = edges(index)
    return Alignment([
        Word(f'w{j}', (bounds[j] + 0.25) / 100., (bounds[j + 1] + 0.25) / 100.)
        for j in range(WORDS[index]) if not silent[j]])


def build_cache(root):
    """Write the cache under `root` (every feature the reference knows, so any
    configuration finds its files); returns (partition_dir, cache_dir)."""
    partition_dir = os.path.join(root, 'partitions')
    cache = os.path.join(root, 'cache', DATASET)
    for sub in ('mels', 'pitch', 'loudness', 'scores', 'alignment'):
        os.makedirs(os.path.join(cache, sub), exist_ok=True)
    os.makedirs(partition_dir, exist_ok=True)
    one_frame = silences = 0
    for index, stem in enumerate(STEMS):
        rng = np.random.default_rng(SEED + 100 + index)
        frames, words = FRAMES[index], WORDS[index]

        def save(directory, suffix, value):
            torch.save(torch.from_numpy(value.astype(np.float32)),
                       os.path.join(cache, directory, f'{stem}{suffix}.pt'))
        save('mels', '', rng.standard_normal((80, frames)))
        save('pitch', '-pitch', rng.uniform(50., 500., (1, frames)))
        save('pitch', '-periodicity', rng.uniform(0., 1., (1, frames)))
        save('loudness', '', rng.standard_normal((1, frames)))
        save('scores', '', rng.uniform(0., 1., words))
        written = alignment(index)
        written.save(os.path.join(cache, 'alignment', f'{stem}.TextGrid'))
        bounds = np.array(written.word_bounds(16000, 160, silences=True))
        assert bounds.shape == (words, 2) and bounds[-1, 1] == frames
        assert np.array_equal(bounds.T.ravel(), np.concatenate(
            [edges(index)[0][:-1], edges(index)[0][1:]]))
        one_frame += int(np.sum(bounds[:, 1] - bounds[:, 0] == 1))
        silences += sum(str(word) == '<silent>' for word in written)
    assert one_frame and silences
    with open(os.path.join(partition_dir, f'{DATASET}.json'), 'w') as file:
        json.dump({'train': [STEMS[i] for i in TRAIN],
                   'valid': [STEMS[i] for i in VALID],
                   'all': STEMS}, file)
    return partition_dir, os.path.join(root, 'cache')


def item(cache_dir, stem, config):
    """(features [C, T], scores [1, W], word_bounds [2, W]) of an utterance
    as the reference's `Dataset.__getitem__` reads them from the cache."""
    from emphases_amd import config as cfg
    from emphases_amd.alignment import Alignment
    cache = os.path.join(cache_dir, DATASET)
    load = lambda *parts: torch.load(  # noqa: E731
        os.path.join(cache, *parts), map_location='cpu', weights_only=True)
    features = []
    if config.mel_feature:
        features.append(load('mels', f'{stem}.pt'))
    if config.pitch_feature:
        pitch = torch.log2(load('pitch', f'{stem}-pitch.pt'))
        if config.normalize:
            pitch = (pitch - cfg.LOGFMIN) / (cfg.LOGFMAX - cfg.LOGFMIN)
        features.append(pitch)
    if config.periodicity_feature:
        features.append(load('pitch', f'{stem}-periodicity.pt'))
    if config.loudness_feature:
        features.append(load('loudness', f'{stem}.pt'))
    features = features[0] if len(features) == 1 else torch.cat(features)
    bounds = Alignment(os.path.join(
        cache, 'alignment', f'{stem}.TextGrid')).word_bounds(
            16000, 160, silences=True)
    return (features, load('scores', f'{stem}.pt')[None],
            torch.tensor(bounds, dtype=torch.long).T)


def collated(cache_dir, stems, config):
    """(features [B, C, Tmax], frame_lengths, word_bounds [B, 2, Wmax],
    word_lengths, targets [B, 1, Wmax]): what `emphases.data.collate` makes
    of the utterances `stems`, zero padded."""
    items = [item(cache_dir, stem, config) for stem in stems]
    frames = torch.tensor([f.shape[-1] for f, _, _ in items])
    words = torch.tensor([b.shape[-1] for _, _, b in items])
    features = torch.zeros(len(items), config.num_features, int(frames.max()))
    bounds = torch.zeros(len(items), 2, int(words.max()), dtype=torch.long)
    targets = torch.zeros(len(items), 1, int(words.max()))
    for i, (feature, score, bound) in enumerate(items):
        features[i, :, :frames[i]] = feature
        bounds[i, :, :words[i]] = bound
        targets[i, :, :words[i]] = score[:, :words[i]]
    return features, frames, bounds, words, targets
