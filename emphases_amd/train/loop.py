"""The training loop (`emphases/train/core.py:13-307`): resume, train,
validate, save - around `Trainer.step` (`EncoderTrainer.step` at
downsample_location 'inference' and 'loss', `PieceTrainer.step` at 'input',
`GridTrainer.step` for the rest of the hyperparameter grid at 'intermediate':
`select_trainer`), fed by the resident loader of `emphases_amd.data`.  That
dispatch covers the convolution model and refuses ARCHITECTURE =
'transformer'; `train(..., trainer=TransformerTrainer)` runs the same loop
around `TransformerTrainer.step`.

Deviations from the reference, besides those of the step (`train/core.py`
here: float32 or `precision='bf16x3'` in place of autocast, every utterance
alone):

* exactly `num_steps` updates.  The reference tests `step >= NUM_STEPS` after
  the update and before counting it (`train/core.py:172-177`), so a run whose
  last epoch does not end on the boundary makes NUM_STEPS + 1;
* validation writes one JSON line per call to `<directory>/scalars.jsonl`
  (the step, 'loss/train' and the three '*/valid' values) in place of
  tensorboard scalars, figures and audio;
* the loss is fetched only when validation runs.  (A step still waits for the
  stream twice, in the loader's two small copies of host tables - the plan's
  metadata and the item table - from pageable memory.)

The checkpoint policy and the file names are the reference's: validation at
`step % log_interval == 0` (after that step's update, counted from 0), a save
to `<step:08d>.pt` when `step >= save_after` and the score beats the best so
far - `best` written before it is raised (`train/core.py:161-170`) - and a
final save after the loop.  A run resumes from the `*.pt` with the largest
step number in `directory`, and restarts that file's epoch from its first
batch, as the reference does.
"""
import functools
import json
import os
import re

import torch

from .. import core as api
from .. import metrics as metrics_module
from ..evaluate import core as evaluate_core
from . import core

# emphases/config/defaults.py:136,139,230,233 and train/core.py:161
NUM_STEPS = 6000
MAX_TRAINING_FRAMES = 75000
LOG_INTERVAL = 100
LOG_STEPS = 32
SAVE_AFTER = 300
RANDOM_SEED = 0


def latest_path(directory):
    """The `<digits>.pt` of `directory` with the largest step number, or None
    (`torchutil.checkpoint.latest_path`)."""
    found = []
    if os.path.isdir(directory):
        for name in os.listdir(directory):
            match = re.fullmatch(r'(\d+)\.pt', name)
            if match:
                found.append((int(match.group(1)), name))
    return os.path.join(directory, max(found)[1]) if found else None


def evaluate(trainer, loader, log_steps=LOG_STEPS):
    """`train/core.py:204-307` without figures, audio and tensorboard: the
    logits of the first `log_steps` batches of `loader` (whose sampler stays
    at the epoch it is at: 0 for validation, as in the reference), then the
    dataset statistics and the metrics in two `metrics.grouped` launches, one
    group per utterance, reduced as dataset evaluation reduces them.  Returns
    {'pearson_correlation', 'bce', 'mse'}."""
    logits, targets, counts, stems = [], [], [], []
    dataset = loader.dataset
    for index, indices in enumerate(loader.sampler):
        batch = loader.batch(indices)
        logits.append(trainer.logits(batch))
        with torch.cuda.device(trainer.device):
            columns = torch.from_numpy(
                batch.plan.word_columns()).to(trainer.device)
            targets.append(batch.targets[columns])
        counts.extend(int(n) for n in batch.plan.words)
        stems.extend(dataset.stems[i] for i in indices)
        if index + 1 == log_steps:
            break
    with torch.cuda.device(trainer.device):
        logits, targets = torch.cat(logits), torch.cat(targets)
    cu_words = [0]
    for count in counts:
        cu_words.append(cu_words[-1] + count)
    post, bce_form = metrics_module.forms('neural', trainer.config.loss)
    first = metrics_module.grouped(
        logits, targets, cu_words, post, bce_form).cpu().numpy()
    (predicted_mean, predicted_std), (target_mean, target_std) = \
        evaluate_core.statistics(first)
    second = metrics_module.grouped(
        logits, targets, cu_words, post, bce_form, predicted_mean,
        target_mean).cpu().numpy()
    overall, _ = evaluate_core.results(
        dataset.name, stems, second, predicted_std, target_std)
    return overall


def train(dataset, directory, gpu=None, *, partition_dir,
          cache_dir='data/cache', config=None, num_steps=NUM_STEPS,
          max_training_frames=MAX_TRAINING_FRAMES, log_interval=LOG_INTERVAL,
          log_steps=LOG_STEPS, save_after=SAVE_AFTER, seed=RANDOM_SEED,
          precision='f32', trainer=None, trainer_arguments=None):
    """Train the model on the 'train' partition of `dataset`, validating on
    its 'valid' partition (`emphases.train`); checkpoints and `scalars.jsonl`
    go to `directory`.  `precision`: 'f32' or 'bf16x3' of the step, for the
    steps and for validation; the files do not record it.
    `trainer`: None - the fused step `select_trainer` names for the
    configuration (the convolution model; the Transformer is refused) - or a
    class with `Trainer`'s interface and a `check(config, precision,
    **trainer_arguments)` that makes its refusals before a GPU is needed:
    `TransformerTrainer`.  `trainer_arguments`: further keyword arguments of
    that class ({'reference_dropout': True}).
    Returns the final checkpoint's path."""
    from .. import data
    config = config or api.active_config()
    # (every refusal before any file is read or any directory is made)
    if trainer is None:
        if trainer_arguments:
            raise ValueError('trainer_arguments go with a trainer= class')
        core.step_class(config, precision)
        build = core.select_trainer
    else:
        trainer_arguments = dict(trainer_arguments or {})
        trainer.check(config, precision, **trainer_arguments)
        build = functools.partial(trainer, **trainer_arguments)
    directory = os.fspath(directory)
    os.makedirs(directory, exist_ok=True)

    def loader(partition, trainer, max_frames):
        resident = data.Dataset(
            dataset, partition, partition_dir=partition_dir,
            cache_dir=cache_dir, config=config, gpu=trainer.device)
        return data.Loader(
            resident, data.Sampler(resident, max_frames, seed), trainer)

    path = latest_path(directory)
    epoch, step, score, best = 0, 0, 0., 0.
    if path is not None:
        state = torch.load(path, map_location='cpu', weights_only=False)
        epoch, step = int(state['epoch']), int(state['step'])
        score, best = float(state['score']), float(state['best'])
        # (the seed keys the dropout masks; the step count, which the
        # optimizer state restores, continues their stream)
        trainer = build(
            config, checkpoint=state, gpu=gpu, seed=seed,
            precision=precision)
    else:
        trainer = build(config, gpu=gpu, seed=seed, precision=precision)
    train_loader = loader('train', trainer, max_training_frames)
    # (the reference's validation sampler is `Sampler(dataset)`: the default
    # frame budget whatever the training one is, `data/sampler.py:15,35`)
    valid_loader = loader('valid', trainer, MAX_TRAINING_FRAMES)

    while step < num_steps:
        train_loader.sampler.set_epoch(epoch)
        for batch in train_loader:
            loss = trainer.step(batch)
            if step % log_interval == 0:
                scalars = {'step': step, 'loss/train': float(loss)}
                scalars.update(
                    (f'{key}/valid', value) for key, value in
                    evaluate(trainer, valid_loader, log_steps).items())
                with open(os.path.join(directory, 'scalars.jsonl'), 'a') as file:
                    file.write(json.dumps(scalars) + '\n')
                score = scalars['pearson_correlation/valid']
            if step >= save_after and score > best:
                trainer.save(
                    os.path.join(directory, f'{step:08d}.pt'), epoch, step,
                    score, best)
                best = score
            step += 1
            if step >= num_steps:
                break
        epoch += 1

    path = os.path.join(directory, f'{step:08d}.pt')
    trainer.save(path, epoch, step, score, best)
    return path
