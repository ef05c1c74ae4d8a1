"""The host side of the training loop (no device): the sampler against the
reference's batches (tests/golden/loop.npz), the dataset's host arrays and
refusals, the C ABI of `emph_collate`, the loop's refusal and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import loop_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import data, runtime, train  # noqa: E402
from emphases_amd.alignment import Alignment, Word  # noqa: E402

FULL = emphases_amd.Config(
    pitch_feature=True, periodicity_feature=True, loudness_feature=True,
    normalize=True)


@pytest.fixture(scope='module')
def cache(tmp_path_factory):
    return loop_data.build_cache(str(tmp_path_factory.mktemp('loop')))


def dataset(cache, partition, config=None, **kwargs):
    partition_dir, cache_dir = cache
    return data.Dataset(
        loop_data.DATASET, partition, partition_dir=partition_dir,
        cache_dir=cache_dir, config=config or emphases_amd.DEFAULT,
        upload=False, **kwargs)


def batches(golden, key):
    flat = golden[f'{key}/batches'].tolist()
    out, cursor = [], 0
    for size in golden[f'{key}/sizes'].tolist():
        out.append(flat[cursor:cursor + size])
        cursor += size
    return out


@pytest.mark.parametrize('partition', ['train', 'valid', 'all'])
def test_sampler_yields_the_reference_batches(cache, partition):
    golden = loop_data.golden()
    resident = dataset(cache, partition)
    assert np.array_equal(resident.lengths, golden[f'{partition}/lengths'])
    buckets = resident.buckets()
    assert len(buckets) == 2
    for k, bucket in enumerate(buckets):
        assert np.array_equal(bucket, golden[f'{partition}/buckets/{k}'])
    before = torch.random.get_rng_state()
    for max_frames in loop_data.MAX_FRAMES:
        sampler = data.Sampler(resident, max_frames)
        for epoch in loop_data.EPOCHS:
            sampler.set_epoch(epoch)
            want = batches(golden, f'{partition}/{max_frames}/{epoch}')
            assert list(sampler) == want
            assert len(sampler) == len(want)
    assert torch.equal(before, torch.random.get_rng_state())
    # another seed is the reference's RANDOM_SEED + epoch shifted
    shifted = data.Sampler(resident, 600, seed=1)
    assert list(shifted) == batches(golden, f'{partition}/600/1')


def test_test_partitions_are_walked_in_order():
    class Held:
        partition = 'test-held-out'

        def __len__(self):
            return 3
    assert list(data.Sampler(Held())) == [[0], [1], [2]]
    assert len(data.Sampler(Held())) == 3


def test_dataset_host_arrays(cache):
    golden = loop_data.golden()
    resident = dataset(cache, 'all', FULL)
    assert resident.features is None and len(resident) == 12
    assert resident.stems == loop_data.STEMS
    assert resident.lengths.tolist() == loop_data.FRAMES
    assert resident.words.tolist() == loop_data.WORDS
    assert resident.frames == sum(loop_data.FRAMES)
    assert resident.host_features.shape == (83, resident.ld_cache)
    assert np.all(resident.frame_first % 16 == 0)
    assert np.all(resident.word_first % 16 == 0)
    for index in (3, 11):
        assert np.array_equal(resident.word_bounds(index),
                              golden[f'all/word_bounds/{index}'])
    _, cache_dir = cache
    covered = np.zeros(resident.ld_cache, dtype=bool)
    for index, stem in enumerate(loop_data.STEMS):
        features, scores, bounds = loop_data.item(cache_dir, stem, FULL)
        assert features.shape == (83, loop_data.FRAMES[index])
        first, count = resident.frame_first[index], resident.lengths[index]
        # mels, log2 pitch normalised, periodicity, loudness: the row order
        assert np.array_equal(
            resident.host_features[:, first:first + count], features.numpy())
        covered[first:first + count] = True
        assert np.array_equal(resident.word_bounds(index), bounds.numpy())
        edges, silent = loop_data.edges(index)
        assert np.array_equal(bounds.numpy(), np.stack([edges[:-1], edges[1:]]))
        first, count = resident.word_first[index], resident.words[index]
        assert np.array_equal(
            resident.host_targets[first:first + count], scores[0].numpy())
    assert not resident.host_features[:, ~covered].any()
    # pitch without normalisation is plain log2
    plain = dataset(cache, 'valid', emphases_amd.Config(pitch_feature=True))
    pitch = torch.load(os.path.join(
        cache_dir, loop_data.DATASET, 'pitch', 'utt-01-pitch.pt'))
    assert np.array_equal(plain.host_features[80, :5], torch.log2(pitch)[0])


def broken_cache(tmp_path):
    """A two-utterance cache to break: returns (cache tuple, cache root)."""
    root = tmp_path / 'cache' / loop_data.DATASET
    for sub in ('mels', 'scores', 'alignment'):
        (root / sub).mkdir(parents=True)
    (tmp_path / 'partitions').mkdir()
    (tmp_path / 'partitions' / f'{loop_data.DATASET}.json').write_text(
        '{"train": ["good", "bad"]}')
    for stem in ('good', 'bad'):
        torch.save(torch.zeros(80, 20), root / 'mels' / f'{stem}.pt')
        torch.save(torch.zeros(2), root / 'scores' / f'{stem}.pt')
        Alignment([Word('a', 0., 0.1), Word('b', 0.1, 0.2)]).save(
            str(root / 'alignment' / f'{stem}.TextGrid'))
    return (str(tmp_path / 'partitions'), str(tmp_path / 'cache')), root


def test_dataset_refuses_what_check_batch_refuses(tmp_path):
    cache, root = broken_cache(tmp_path)
    assert dataset(cache, 'train').words.tolist() == [2, 2]
    # a word past the frames is cut as a slice cuts it ...
    Alignment([Word('a', 0., 0.1), Word('b', 0.1, 0.5)]).save(
        str(root / 'alignment' / 'bad.TextGrid'))
    assert dataset(cache, 'train').word_bounds(1).tolist() == \
        [[0, 10], [10, 20]]
    # ... and refused when nothing of it is left
    Alignment([Word('a', 0., 0.2), Word('b', 0.2, 0.5)]).save(
        str(root / 'alignment' / 'bad.TextGrid'))
    with pytest.raises(ValueError, match=r'bad.*empty'):
        dataset(cache, 'train')
    Alignment([Word('a', 0., 0.15), Word('b', 0.1, 0.2)]).save(
        str(root / 'alignment' / 'bad.TextGrid'))
    with pytest.raises(ValueError, match=r'bad.*overlap'):
        dataset(cache, 'train')
    Alignment([Word('a', 0., 0.1), Word('b', 0.1, 0.2)]).save(
        str(root / 'alignment' / 'bad.TextGrid'))
    torch.save(torch.zeros(1), root / 'scores' / 'bad.pt')
    with pytest.raises(ValueError, match=r'bad.*1 targets for 2 words'):
        dataset(cache, 'train')


@pytest.mark.parametrize('missing', [
    'mels/bad.pt', 'scores/bad.pt', 'alignment/bad.TextGrid',
    'loudness/bad.pt'])
def test_dataset_names_a_missing_file(tmp_path, missing):
    cache, root = broken_cache(tmp_path)
    config = emphases_amd.DEFAULT
    if missing.startswith('loudness'):
        config = emphases_amd.Config(loudness_feature=True)
        (root / 'loudness').mkdir()
        torch.save(torch.zeros(1, 20), root / 'loudness' / 'good.pt')
    else:
        os.remove(root / missing)
    with pytest.raises(FileNotFoundError, match=missing.replace('.', r'\.')):
        dataset(cache, 'train', config)
    with pytest.raises(FileNotFoundError, match='nowhere'):
        data.Dataset(loop_data.DATASET, 'train', partition_dir='nowhere',
                     cache_dir=cache[1], upload=False)


def test_collate_abi_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    assert 'int emph_collate(' in header
    assert 'emph_collate' in runtime.SIGNATURES
    library = runtime.library()
    assert library.emph_abi_version() == runtime.ABI_VERSION >= 35
    # contract violations are reported, not launched
    assert library.emph_collate(
        None, 16, None, 16, None, 1, 80, 160, 160, None, None, None) == -1
    assert b'emph_collate: null' in library.emph_last_error()
    one = 16          # (never dereferenced: the shape is refused first)
    assert library.emph_collate(
        one, 16, one, 16, one, 0, 80, 160, 160, one, one, None) == -1
    assert b'0 items' in library.emph_last_error()
    assert library.emph_collate(
        one, 16, one, 16, one, 1, 80, 161, 160, one, one, None) == -1
    assert b'bad shape' in library.emph_last_error()
    assert library.emph_collate(
        one, 16, one, 16, one, 1, 0, 160, 160, one, one, None) == -1


def test_train_refuses_a_transformer_before_touching_the_cache(tmp_path):
    config = emphases_amd.Config(architecture='transformer')
    with pytest.raises(NotImplementedError, match='architecture'):
        train.train('nothing', tmp_path / 'run', partition_dir='nowhere',
                    cache_dir='nowhere', config=config)
    assert not (tmp_path / 'run').exists()
    assert train.latest_path(str(tmp_path)) is None
    for name in ('00000004.pt', '00000100.pt', '00000020.pt', 'notes.pt'):
        (tmp_path / name).write_bytes(b'')
    assert train.latest_path(str(tmp_path)) == str(tmp_path / '00000100.pt')


def test_cli_help_lists_the_flags():
    out = subprocess.run(
        [sys.executable, '-m', 'emphases_amd.train', '--help'], cwd=ROOT,
        capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    for flag in ('--dataset', '--gpu', '--directory', '--partition_dir',
                 '--cache_dir', '--num_steps', '--max_training_frames',
                 '--log_interval', '--loss', '--downsample_method'):
        assert flag in out.stdout, flag
