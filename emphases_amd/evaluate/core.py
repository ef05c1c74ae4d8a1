"""Dataset evaluation (`emphases/evaluate/core.py:15-127`, `python -m
emphases.evaluate`): the crowdsourced targets of each dataset's 'test'
partition against the model's logits or a baseline's scores, written as the
reference's `overall.json` and `granular.json`.

The reference runs every file through the model twice at batch 1, once for
the dataset statistics and once for the metrics.  Here each dataset takes ONE
inference pass in ragged batches of `utterances_per_batch` files, and the
compact logits (one float per word) and targets stay on the device.  Two
launches of `emph_word_metrics_grouped` (one group per file) then give

1. with zero means: the count, sum and sum of squares of the scores and
   targets of every file.  Summed over the files in partition order, they are
   the reference's two `Statistics` (mean, (n - 1) standard deviation);
2. with the dataset means: every file's BCE, squared error and covariance
   sums.  Each row is that file's granular metrics (the reference's per-file
   `Metrics` uses the dataset statistics too); the rows summed in file order
   are the dataset's overall metrics.

Every row is a fixed-order reduction over its file's words, so the results do
not depend on `utterances_per_batch`, and the host arithmetic is float64.
Where the reference would divide by zero (a zero standard deviation, a single
word), the values are IEEE inf / nan.
"""
import json
import math
import os

import numpy as np
import torch

from .. import config as cfg
from .. import metrics as metrics_module
from .. import runtime

__all__ = ['datasets', 'statistics', 'results', 'read', 'stems']


###############################################################################
# The cache (`data/dataset.py:15-90`)
###############################################################################


def stems(dataset, partition_dir):
    """The stems of the 'test' partition of `<partition_dir>/<dataset>.json`,
    in file order."""
    path = os.path.join(os.fspath(partition_dir), f'{dataset}.json')
    if not os.path.isfile(path):
        raise FileNotFoundError(f'partition file {path} not found')
    with open(path, encoding='utf-8') as file:
        chosen = json.load(file).get('test') or []
    if not chosen:
        raise ValueError(
            f"dataset {dataset}: the 'test' partition of {path} is empty")
    return [str(stem) for stem in chosen]


def files(dataset, partition_dir, cache_dir):
    """[(stem, audio, alignment, targets)] paths of the 'test' partition,
    every one checked: a missing file raises FileNotFoundError naming it."""
    root = os.path.join(os.fspath(cache_dir), dataset)
    listed = []
    for stem in stems(dataset, partition_dir):
        paths = (os.path.join(root, 'audio', f'{stem}.wav'),
                 os.path.join(root, 'alignment', f'{stem}.TextGrid'),
                 os.path.join(root, 'scores', f'{stem}.pt'))
        for path in paths:
            if not os.path.isfile(path):
                raise FileNotFoundError(f'{dataset}/{stem}: {path} not found')
        listed.append((stem,) + paths)
    return listed


def read(stem, audio_file, alignment_file, targets_file):
    """(audio float32 [1, S'], alignment, targets float32 [W]) of one file
    as the reference's loader hands them over (`data/collate.py`): audio at
    16 kHz (resampled first, `load.audio`), cut to whole hops (the frame count
    of the cached features), words with silences, targets cut to the word
    count.  Fewer targets than words raise ValueError."""
    from .. import alignment as alignment_module
    from .. import load
    audio = load.audio(audio_file)[:1]
    audio = audio[:, :audio.shape[-1] // cfg.HOPSIZE * cfg.HOPSIZE]
    alignment = alignment_module.Alignment(alignment_file)
    words = len(alignment)
    targets = torch.load(targets_file, map_location='cpu', weights_only=True)
    targets = torch.as_tensor(targets, dtype=torch.float32).reshape(-1)
    if targets.numel() < words:
        raise ValueError(
            f'{stem}: {targets.numel()} targets for {words} words '
            f'({targets_file})')
    return audio, alignment, targets[:words].contiguous()


###############################################################################
# Host arithmetic (float64)
###############################################################################


def _total(rows):
    """Sum of the rows in order."""
    total = np.zeros(runtime.METRIC_FIELDS, dtype=np.float64)
    for row in np.asarray(rows, dtype=np.float64):
        total += row
    return total


def _divide(a, b):
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.float64(a) / np.float64(b))


def statistics(rows):
    """((predicted mean, std), (target mean, std)) of the zero-mean rows of
    every file: torchutil's `MeanStd` ((n - 1)-normalised) over every word."""
    total = _total(rows)
    count = total[runtime.METRIC_COUNT]

    def mean_std(sum_field, sumsq_field):
        mean = _divide(total[sum_field], count)
        # (a NaN mean stays NaN: max(nan, 0.) is nan)
        m2 = max(total[sumsq_field] - total[sum_field] * mean, 0.)
        variance = _divide(m2, count - 1)
        return mean, math.sqrt(variance) if variance >= 0 else variance
    return (mean_std(runtime.METRIC_SUM_PREDICTED,
                     runtime.METRIC_SUMSQ_PREDICTED),
            mean_std(runtime.METRIC_SUM_TARGET, runtime.METRIC_SUMSQ_TARGET))


def _values(row, predicted_std, target_std):
    count = row[runtime.METRIC_COUNT]
    return {
        'pearson_correlation': _divide(
            _divide(row[runtime.METRIC_COVARIANCE], count),
            np.float64(predicted_std) * np.float64(target_std)),
        'bce': _divide(row[runtime.METRIC_BCE], count),
        'mse': _divide(row[runtime.METRIC_SQUARED_ERROR], count)}


def results(dataset, names, rows, predicted_std, target_std):
    """(overall metrics of the dataset, {f'{dataset}/{stem}': metrics}) from
    the rows of the second launch (one per file, partition order)."""
    rows = np.asarray(rows, dtype=np.float64)
    granular = {
        f'{dataset}/{stem}': _values(row, predicted_std, target_std)
        for stem, row in zip(names, rows)}
    return _values(_total(rows), predicted_std, target_std), granular


###############################################################################
# Evaluate
###############################################################################


def _scores(method, listed, device, session, pitch_tracker, batch):
    """(compact logits, compact targets, cu_words) of a dataset on the
    device: one inference pass in batches of `batch` files."""
    from .. import baselines
    logits, targets, counts = [], [], []
    for first in range(0, len(listed), batch):
        loaded = [read(*item) for item in listed[first:first + batch]]
        audios = [audio for audio, _, _ in loaded]
        alignments = [alignment for _, alignment, _ in loaded]
        if method == 'neural':
            _, outputs = session.run(
                alignments, audios, cfg.SAMPLE_RATE, None, on_device=True,
                pitch_tracker=pitch_tracker, logits=True)
        else:
            # a baseline's scores are its "logits" (postprocess: identity)
            outputs = baselines.from_alignments_and_audios(
                method, alignments, audios, cfg.SAMPLE_RATE, device.index,
                pitch_tracker)
        for (stem, *_), (_, alignment, target), output in zip(
                listed[first:first + batch], loaded, outputs):
            if output.shape[-1] != len(alignment):
                raise ValueError(
                    f'{stem}: {output.shape[-1]} scores for '
                    f'{len(alignment)} words')
            logits.append(output.reshape(-1).to(device, torch.float32))
            targets.append(target)
            counts.append(len(alignment))
    with torch.cuda.device(device):
        logits = torch.cat(logits)
        targets = torch.cat(targets).pin_memory().to(device)
    return logits, targets, np.concatenate([[0], np.cumsum(counts)])


def datasets(datasets=('libritts',), checkpoint=None, gpu=None, *,
             partition_dir, cache_dir='data/cache', eval_dir='eval',
             name='emphases', config=None, precision='f32',
             pitch_tracker=None, utterances_per_batch=256):
    """Evaluate on the 'test' partition of each dataset
    (`emphases/evaluate/core.py:15-127`) and write
    `<eval_dir>/<name>/overall.json` ({dataset: metrics}) and `granular.json`
    ({f'{dataset}/{stem}': metrics}, partition order); returns the two dicts.

    The cache is the reference's: `<cache_dir>/<dataset>/audio/<stem>.wav`,
    `alignment/<stem>.TextGrid` and `scores/<stem>.pt` (float targets [W]);
    the stems are the 'test' key of `<partition_dir>/<dataset>.json`.  Cached
    features are not read.  Every path is checked before any GPU work.

    `config` (default: the active configuration) supplies `method` and
    `loss`; `checkpoint` and `precision` reach the model as in
    `from_files_to_files`, `pitch_tracker` the pitch-variance baseline (and
    pitch features).  Whole utterances go through the model (`batch_size`
    None, as in both of the reference's passes)."""
    from .. import baselines
    from .. import core
    if isinstance(datasets, str):
        datasets = [datasets]
    datasets = list(datasets)
    config = config or core.active_config()
    method = config.method
    baselines.require(method)
    utterances_per_batch = int(utterances_per_batch)
    if utterances_per_batch < 1:
        raise ValueError('utterances_per_batch must be at least 1')
    listed = {dataset: files(dataset, partition_dir, cache_dir)
              for dataset in datasets}
    if pitch_tracker is None and (
            method == 'pitch-variance' or
            (method == 'neural' and
             (config.pitch_feature or config.periodicity_feature))):
        pitch_tracker = core.penn_tracker(gpu)      # raises without penn

    device = runtime.require_gpu(gpu)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    session = core.get_session(checkpoint, device.index, config,
                               precision=precision) \
        if method == 'neural' else None
    post, bce_form = metrics_module.forms(method, config.loss)

    overall, granular = {}, {}
    for dataset in datasets:
        logits, targets, cu_words = _scores(
            method, listed[dataset], device, session, pitch_tracker,
            utterances_per_batch)
        first = metrics_module.grouped(
            logits, targets, cu_words, post, bce_form).cpu().numpy()
        (predicted_mean, predicted_std), (target_mean, target_std) = \
            statistics(first)
        second = metrics_module.grouped(
            logits, targets, cu_words, post, bce_form, predicted_mean,
            target_mean).cpu().numpy()
        overall[dataset], files_metrics = results(
            dataset, [item[0] for item in listed[dataset]], second,
            predicted_std, target_std)
        granular.update(files_metrics)

    directory = os.path.join(os.fspath(eval_dir), name)
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, 'overall.json'), 'w') as file:
        json.dump(overall, file, indent=4)
    with open(os.path.join(directory, 'granular.json'), 'w') as file:
        json.dump(granular, file, indent=4)
    return overall, granular
