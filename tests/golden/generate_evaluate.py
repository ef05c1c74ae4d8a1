"""Capture golden vectors of the reference's dataset evaluation.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_evaluate.py

Imports the UNMODIFIED reference `emphases` with the stand-ins of
`tests/golden/stubs/` (as `generate_baselines.py` does) and runs its own
`emphases.evaluate.datasets` (`evaluate/core.py:15-127`) on a synthetic
dataset of 16 utterances:

* `emphases.data.loader` is replaced by a list of batches built by the
  reference's own `emphases.data.collate`, with the features computed by its
  `mels.from_audio` (so the reference itself cuts the audio to whole hops);
* autocast is disabled (`inference_context` keeps eval mode and no_grad, as
  `generate.py`'s O-fp32 path does), the checkpoint is the reference's own,
  `EVAL_DIR` / `CONFIG` point at a temporary directory, `METHOD` selects the
  baselines and `penn.from_audio` is `emphases_amd.synth.pitch_tracks`.

torchutil's `MeanStd` / `Average` / `PearsonCorrelation` are the stand-ins of
`tests/golden/stubs/torchutil/metrics.py` (third-party, absent): the dataset
statistics and the running averages are PARITY UNPINNED, as for `metrics.npz`.

Output (committed; inputs and outputs only, no audio):
  tests/golden/evaluate.npz
  stems          str [U]        partition order
  frames         int64 [U]      whole hops of each utterance
  tails          int64 [U]      samples past the last whole hop: the audio is
                                synth.audio(index, frames + 1) cut to
                                frames * 160 + tail samples
  words          int64 [U]      words per utterance
  word_frames    int64 [2, W]   (start, end) frames of every word (seconds =
                                frames / 100)
  labels         str [W]        '<silent>' every 8th token
  phonemes       int64 [W]      phonemes per word
  phone_frames   int64 [2, P]   (start, end) frames of every phoneme
  target_lengths int64 [U]      targets per file (one longer than its words)
  targets        float32 [T]    multiples of 1/8, back to back
  logits         float32 [W]    the reference's per-word logits (neural)
  {method}_overall   float64 [3]     (pearson_correlation, bce, mse)
  {method}_granular  float64 [U, 3]  per file, partition order
for method in neural, duration_variance, pitch_variance.
The GPU box never runs this script; it only reads the .npz file.
"""
import contextlib
import json
import os
import sys
import tempfile
from pathlib import Path

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = '/root/reference'
sys.path[:0] = [os.path.join(HERE, 'stubs'), REFERENCE, ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases  # noqa: E402  (the reference)
import penn  # noqa: E402  (stand-in)
import pypar  # noqa: E402  (stand-in)

from emphases_amd import synth  # noqa: E402

torch.set_num_threads(1)
CHECKPOINT = os.path.join(
    REFERENCE, 'emphases', 'assets', 'checkpoints', 'checkpoint.pt')
DATASET = 'synthetic'
FIELDS = ('pearson_correlation', 'bce', 'mse')
METHODS = ('neural', 'duration-variance', 'pitch-variance')


class Word(pypar.Word):
    """A word with phonemes: len() is their count (`pypar.Word`)."""

    def __init__(self, word, start, end, phonemes):
        super().__init__(word, start, end)
        self.phonemes = [pypar.Word('p', a, b) for a, b in phonemes]

    def __len__(self):
        return len(self.phonemes)


class Alignment(pypar.Alignment):
    def phonemes(self):
        return [p for word in self._words for p in word.phonemes]


def dataset():
    """The utterances: (stem, frames, tail, word frames [2, W], labels,
    phoneme frames per word, targets)."""
    rng = np.random.default_rng(20261016)
    cases = []
    for index in range(16):
        frames = int(rng.integers(50, 801))
        tail = (0, 1, 159)[index % 3]
        if index == 5:                              # a single word
            bounds = np.array([[0], [frames]], dtype=np.int64)
        else:
            bounds = synth.word_frames(index, frames, 8, 60)
        count = bounds.shape[1]
        labels = synth.word_names(count)
        phones = []
        for (a, b), label in zip(bounds.T.tolist(), labels):
            parts = 1 if label == '<silent>' else int(rng.integers(1, 4))
            parts = max(1, min(parts, b - a))
            edges = [a + (b - a) * k // parts for k in range(parts)] + [b]
            phones.append(list(zip(edges[:-1], edges[1:])))
        length = count + (3 if index == 3 else 0)
        targets = rng.integers(0, 9, length).astype(np.float32) / 8
        targets[0] = 0.
        targets[min(1, length - 1)] = 1. if length > 1 else targets[0]
        cases.append((f'utterance-{index:02d}', frames, tail, bounds, labels,
                       phones, targets))
    return cases


def batches(cases):
    """What the reference's test loader yields: one collated file each."""
    out = []
    for index, (stem, frames, tail, bounds, labels, phones, targets) in \
            enumerate(cases):
        audio = torch.from_numpy(
            synth.audio(index, frames + 1)[:, :frames * 160 + tail].copy())
        alignment = Alignment([
            Word(label, a / 100., b / 100.,
                 [(pa / 100., pb / 100.) for pa, pb in phone])
            for label, (a, b), phone in zip(labels, bounds.T.tolist(), phones)])
        word_bounds = alignment.word_bounds(16000, 160, silences=True)
        word_bounds = torch.cat(
            [torch.tensor(bound)[None] for bound in word_bounds]).T
        features = emphases.data.preprocess.mels.from_audio(audio)
        features = features.reshape(features.shape[-2], features.shape[-1])
        assert features.shape[-1] == frames, (features.shape, frames)
        scores = torch.from_numpy(targets)[None]
        out.append(emphases.data.collate(
            [(features, scores, word_bounds, alignment, audio, stem)]))
    return out


@contextlib.contextmanager
def fp32_context(model):
    model.eval()
    with torch.no_grad():
        yield
    model.train()


def run(method, loaded, directory, recorded):
    emphases.METHOD = method
    emphases.EVAL_DIR = Path(directory)
    emphases.CONFIG = method
    for name in ('model', 'checkpoint', 'device_type'):
        if hasattr(emphases.infer, name):
            delattr(emphases.infer, name)
    recorded.clear()
    emphases.evaluate.datasets([DATASET], CHECKPOINT, None)
    with open(os.path.join(directory, method, 'overall.json')) as file:
        overall = json.load(file)
    with open(os.path.join(directory, method, 'granular.json')) as file:
        granular = json.load(file)
    return overall, granular


def main():
    cases = dataset()
    loaded = batches(cases)
    emphases.data.loader = lambda *args, **kwargs: loaded
    emphases.inference_context = fp32_context
    penn.from_audio = synth.pitch_tracks
    recorded = []
    original = emphases.evaluate.Metrics.update

    def update(self, logits, targets, word_lengths):
        recorded.append(logits.detach()[0, 0].float().numpy().copy())
        return original(self, logits, targets, word_lengths)
    emphases.evaluate.Metrics.update = update

    out = {
        'stems': np.array([c[0] for c in cases]),
        'frames': np.array([c[1] for c in cases], dtype=np.int64),
        'tails': np.array([c[2] for c in cases], dtype=np.int64),
        'words': np.array([c[3].shape[1] for c in cases], dtype=np.int64),
        'word_frames': np.concatenate([c[3] for c in cases], axis=1),
        'labels': np.array([label for c in cases for label in c[4]]),
        'phonemes': np.array([len(p) for c in cases for p in c[5]],
                             dtype=np.int64),
        'phone_frames': np.array(
            [pair for c in cases for p in c[5] for pair in p],
            dtype=np.int64).T.copy(),
        'target_lengths': np.array([len(c[6]) for c in cases],
                                   dtype=np.int64),
        'targets': np.concatenate([c[6] for c in cases]).astype(np.float32)}
    stems = [c[0] for c in cases]
    with tempfile.TemporaryDirectory() as directory:
        for method in METHODS:
            overall, granular = run(method, loaded, directory, recorded)
            assert list(granular) == [f'{DATASET}/{s}' for s in stems]
            key = method.replace('-', '_')
            out[f'{key}_overall'] = np.array(
                [overall[DATASET][f] for f in FIELDS], dtype=np.float64)
            out[f'{key}_granular'] = np.array(
                [[granular[f'{DATASET}/{s}'][f] for f in FIELDS]
                 for s in stems], dtype=np.float64)
            if method == 'neural':
                # file_metrics and dataset_metrics see the same logits
                logits = recorded[0::2]
                assert len(logits) == len(cases)
                out['logits'] = np.concatenate(logits).astype(np.float32)
    assert out['logits'].shape == (int(out['words'].sum()),)
    path = os.path.join(HERE, 'evaluate.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    for method in METHODS:
        print(method, out[f"{method.replace('-', '_')}_overall"])
    leaked = [
        root for root, dirs, _ in os.walk(REFERENCE) if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
