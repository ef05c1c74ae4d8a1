"""Capture golden vectors of the reference's training data path.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_loop.py

Imports the UNMODIFIED reference `emphases` with the stand-ins of
`tests/golden/stubs/` (as `generate_train.py` does) and runs, on the CPU, its
`emphases.data.Dataset` and `emphases.data.sampler.Sampler` over the synthetic
cache of tests/loop_data.py (12 utterances; 8 in 'train', 4 in 'valid', all
of them in 'all').

Third-party stand-ins, for this script only: the cache holds no audio, so
`torchaudio.info` reports frames x HOPSIZE samples and `emphases.load.audio`
silence of that length; `pypar.Alignment(file)` is the stubs' Alignment over
the utterance's words as tests/loop_data.py defines them (`edges`: frame
edges and which words are silences), silences present as words the way pypar
fills gaps - the TextGrid and `emphases_amd.alignment` are not involved.

Recorded, per partition P in train, valid, all:

  P/lengths            Dataset.lengths
  P/buckets/<k>        Dataset.buckets()[k], int64 [n, 2] (index, length)
  P/<max_frames>/<epoch>/batches, .../sizes
                       the Sampler's batches of epochs 0..2 at max_frames 600
                       and 75000, back to back, and the size of each
  all/word_bounds/<i>  `__getitem__(i)[2]` for i = 3 and 11, int64 [2, W]

Output (committed): tests/golden/loop.npz.  The GPU box never runs this
script; it only reads the .npz file.
"""
import os
import sys
import tempfile
import types

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = '/root/reference'
sys.path[:0] = [os.path.join(HERE, 'stubs'), REFERENCE, ROOT,
                os.path.join(ROOT, 'tests')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases  # noqa: E402  (the reference)
import pypar  # noqa: E402  (the stand-in)
import torchaudio  # noqa: E402  (the stand-in)

import loop_data  # noqa: E402


def main():
    from pathlib import Path
    out = {}
    with tempfile.TemporaryDirectory() as root:
        partition_dir, cache_dir = loop_data.build_cache(root)
        emphases.PARTITION_DIR = Path(partition_dir)
        emphases.CACHE_DIR = Path(cache_dir)
        frames = dict(zip(loop_data.STEMS, loop_data.FRAMES))

        def samples(file):
            return frames[Path(file).stem] * emphases.HOPSIZE
        torchaudio.info = lambda file: types.SimpleNamespace(
            num_frames=samples(file))
        emphases.load.audio = lambda file: torch.zeros(1, samples(file))
        stub = pypar.Alignment

        def from_file(file):
            index = loop_data.STEMS.index(Path(file).stem)
            edges, silent = loop_data.edges(index)
            return stub([
                pypar.Word(pypar.SILENCE if silent[j] else f'w{j}',
                           (edges[j] + 0.25) / 100.,
                           (edges[j + 1] + 0.25) / 100.)
                for j in range(loop_data.WORDS[index])])
        pypar.Alignment = from_file

        for partition in ('train', 'valid', 'all'):
            dataset = emphases.data.Dataset(loop_data.DATASET, partition)
            out[f'{partition}/lengths'] = np.array(
                dataset.lengths, dtype=np.int64)
            for k, bucket in enumerate(dataset.buckets()):
                out[f'{partition}/buckets/{k}'] = np.asarray(
                    bucket, dtype=np.int64)
            for max_frames in loop_data.MAX_FRAMES:
                sampler = sys.modules['emphases.data.sampler'].Sampler(
                    dataset, max_frames)
                for epoch in loop_data.EPOCHS:
                    sampler.set_epoch(epoch)
                    batches = [[int(i) for i in batch] for batch in sampler]
                    assert len(batches) == len(sampler)
                    key = f'{partition}/{max_frames}/{epoch}'
                    out[f'{key}/batches'] = np.array(
                        sum(batches, []), dtype=np.int64)
                    out[f'{key}/sizes'] = np.array(
                        [len(batch) for batch in batches], dtype=np.int64)
                    print(key, batches)
            if partition == 'all':
                for index in (3, 11):
                    bounds = dataset[index][2]
                    out[f'all/word_bounds/{index}'] = \
                        bounds.numpy().astype(np.int64)
                    assert bounds.shape == (2, loop_data.WORDS[index])
    path = os.path.join(HERE, 'loop.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    leaked = [
        root for root, dirs, _ in os.walk(REFERENCE) if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
