"""The synthetic dataset of tests/golden/evaluate.npz as a reference-layout
cache (`<cache>/<dataset>/{audio,alignment,scores}`, a partition file), and a
float64 restatement of the per-file rows of `emph_word_metrics_grouped`."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DATASET = 'synthetic'
FIELDS = ('pearson_correlation', 'bce', 'mse')


def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'evaluate.npz')))


def split(flat, counts):
    return np.split(flat, np.cumsum(counts)[:-1], axis=-1)


def build_cache(root, data, decoys=True):
    """Write the cache under `root`; returns (partition_dir, cache_dir)."""
    from emphases_amd import load, synth
    from emphases_amd.alignment import Alignment, Phoneme, Word
    partition_dir = os.path.join(root, 'partitions')
    cache = os.path.join(root, 'cache', DATASET)
    for sub in ('audio', 'alignment', 'scores'):
        os.makedirs(os.path.join(cache, sub), exist_ok=True)
    os.makedirs(partition_dir, exist_ok=True)
    stems = [str(s) for s in data['stems']]
    words = split(data['word_frames'], data['words'])
    labels = split(data['labels'], data['words'])
    counts = split(data['phonemes'], data['words'])
    phones = split(data['phone_frames'], [int(c.sum()) for c in counts])
    targets = split(data['targets'], data['target_lengths'])
    for index, stem in enumerate(stems):
        frames, tail = int(data['frames'][index]), int(data['tails'][index])
        audio = synth.audio(index, frames + 1)[:, :frames * 160 + tail]
        load.save_wav(os.path.join(cache, 'audio', f'{stem}.wav'), audio)
        per_word = split(phones[index], counts[index])
        alignment = Alignment([
            Word(str(label), a / 100., b / 100.,
                 [Phoneme('p', pa / 100., pb / 100.) for pa, pb in p.T])
            for label, (a, b), p in zip(
                labels[index], words[index].T.tolist(), per_word)])
        alignment.save(os.path.join(cache, 'alignment', f'{stem}.TextGrid'))
        torch.save(torch.from_numpy(targets[index].copy()),
                   os.path.join(cache, 'scores', f'{stem}.pt'))
    partition = {'test': stems}
    if decoys:
        partition.update(train=['missing-train'], valid=['missing-valid'])
    with open(os.path.join(partition_dir, f'{DATASET}.json'), 'w') as file:
        json.dump(partition, file)
    return partition_dir, os.path.join(root, 'cache')


def rows(logits, targets, counts, post, bce_form, means=(0., 0.)):
    """float64 [files, 8] of `emph_word_metrics_grouped` restated the way the
    reference reduces a file: per-word values in float32 (torch ops of
    evaluate/metrics.py), BCE / squared error / covariance summed in float32
    (torchutil's Average / PearsonCorrelation stand-ins), the statistics
    sums in float64."""
    out = []
    for x, y in zip(split(np.asarray(logits, np.float32), counts),
                    split(np.asarray(targets, np.float32), counts)):
        x, y = torch.from_numpy(x.copy()), torch.from_numpy(y.copy())
        if post == 1:
            score = torch.sigmoid(x)
        elif post == 2:
            score = torch.clamp(x, 0., 1.)
        else:
            score = x
        if bce_form == 0:
            bce = torch.nn.functional.binary_cross_entropy_with_logits(
                x, y, reduction='none')
        else:
            c = torch.clamp(x, 0., 1.)
            bce = -(y * torch.log(c + 1e-6) + (1 - y) * torch.log(1 - c + 1e-6))
        mse = torch.nn.functional.mse_loss(score, y, reduction='none')
        cov = (score - float(means[0])) * (y - float(means[1]))
        s, t = score.double().numpy(), y.double().numpy()
        out.append([
            x.numel(), float(bce.sum().double()), float(mse.sum().double()),
            float(cov.sum().double()), s.sum(), (s * s).sum(), t.sum(),
            (t * t).sum()])
    return np.array(out, dtype=np.float64).reshape(-1, 8)
