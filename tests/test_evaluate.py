"""emphases_amd.evaluate on the host: the dataset reader and its errors, the
float64 host arithmetic against the reference's own evaluation
(tests/golden/evaluate.npz), and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import evaluate_data  # noqa: E402
from emphases_amd import evaluate  # noqa: E402
from emphases_amd.evaluate import core as evaluate_core  # noqa: E402


@pytest.fixture(scope='module')
def data():
    return evaluate_data.golden()


@pytest.fixture
def cache(tmp_path, data):
    return evaluate_data.build_cache(str(tmp_path), data)


def test_exports():
    from emphases_amd import metrics
    assert evaluate.Metrics is metrics.Metrics
    assert evaluate.metrics is metrics
    assert callable(evaluate.datasets)
    import emphases_amd
    assert emphases_amd.evaluate is evaluate


def test_cli_help():
    out = subprocess.run(
        [sys.executable, '-m', 'emphases_amd.evaluate', '--help'],
        cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ('--datasets', '--checkpoint', '--gpu', '--partition_dir',
                 '--cache_dir', '--eval_dir', '--name', '--method',
                 '--precision'):
        assert flag in out.stdout


def test_reader_takes_the_test_partition_only(cache, data):
    partition_dir, cache_dir = cache
    listed = evaluate_core.files(
        evaluate_data.DATASET, partition_dir, cache_dir)
    assert [item[0] for item in listed] == [str(s) for s in data['stems']]
    for stem, audio, alignment, targets in listed:
        assert audio.endswith(os.path.join('audio', f'{stem}.wav'))
        assert alignment.endswith(
            os.path.join('alignment', f'{stem}.TextGrid'))
        assert targets.endswith(os.path.join('scores', f'{stem}.pt'))


@pytest.mark.parametrize('sub,suffix', [
    ('audio', '.wav'), ('alignment', '.TextGrid'), ('scores', '.pt')])
def test_missing_file_raises_before_gpu_work(cache, data, sub, suffix):
    partition_dir, cache_dir = cache
    stem = str(data['stems'][7])
    path = os.path.join(cache_dir, evaluate_data.DATASET, sub, stem + suffix)
    os.remove(path)
    with pytest.raises(FileNotFoundError, match=path.replace('.', r'\.')):
        evaluate.datasets([evaluate_data.DATASET], gpu=0,
                          partition_dir=partition_dir, cache_dir=cache_dir,
                          eval_dir=os.path.join(cache_dir, 'eval'))


def test_missing_partition_and_empty_partition(tmp_path, cache):
    partition_dir, cache_dir = cache
    missing = os.path.join(partition_dir, 'nothing.json')
    with pytest.raises(FileNotFoundError, match='nothing.json'):
        evaluate.datasets(['nothing'], partition_dir=partition_dir,
                          cache_dir=cache_dir, eval_dir=str(tmp_path))
    assert not os.path.exists(missing)
    with open(os.path.join(partition_dir, 'hollow.json'), 'w') as file:
        json.dump({'train': ['a'], 'test': []}, file)
    with pytest.raises(ValueError, match='hollow'):
        evaluate.datasets(['hollow'], partition_dir=partition_dir,
                          cache_dir=cache_dir, eval_dir=str(tmp_path))
    assert not os.path.exists(os.path.join(str(tmp_path), 'emphases'))


def test_prominence_raises(cache, tmp_path):
    import emphases_amd
    partition_dir, cache_dir = cache
    with pytest.raises(NotImplementedError, match='prominence'):
        evaluate.datasets(
            [evaluate_data.DATASET], partition_dir=partition_dir,
            cache_dir=cache_dir, eval_dir=str(tmp_path),
            config=emphases_amd.Config(method='prominence'))


def test_reader_truncates_audio_and_targets(cache, data):
    partition_dir, cache_dir = cache
    listed = evaluate_core.files(
        evaluate_data.DATASET, partition_dir, cache_dir)
    for index, item in enumerate(listed):
        audio, alignment, targets = evaluate_core.read(*item)
        frames = int(data['frames'][index])
        assert audio.shape == (1, frames * 160)
        assert len(alignment) == int(data['words'][index])
        assert targets.dtype == torch.float32
        want = evaluate_data.split(data['targets'], data['target_lengths'])
        np.testing.assert_array_equal(
            targets.numpy(), want[index][:int(data['words'][index])])
    # index 3 has three targets more than words
    assert data['target_lengths'][3] == data['words'][3] + 3
    # fewer targets than words: an error naming the stem
    stem, audio, alignment, targets = listed[2]
    torch.save(torch.zeros(int(data['words'][2]) - 1), targets)
    with pytest.raises(ValueError, match=stem):
        evaluate_core.read(*listed[2])


def _logits(data, method):
    """The neural logits the reference recorded, or the duration-variance
    scores (host arithmetic of the package, pinned by baselines.npz)."""
    if method == 'neural':
        return data['logits']
    from emphases_amd.baselines import duration_variance
    times = data['word_frames'].T / 100.
    return duration_variance.scores(times, data['phonemes'], data['words'])


@pytest.mark.parametrize('method,post', [
    ('neural', 1), ('duration_variance', 0)])
def test_host_arithmetic_matches_reference(data, method, post):
    """Per-file rows restated on the host (float32 per-word values, as the
    reference reduces a file) from the golden's neural logits or the
    duration-variance scores, turned into the JSON dicts: equal to what the
    reference's own evaluation wrote."""
    logits = _logits(data, method)
    words = data['words']
    targets = np.concatenate([
        t[:w] for t, w in zip(
            evaluate_data.split(data['targets'], data['target_lengths']),
            words)])
    first = evaluate_data.rows(logits, targets, words, post, 0)
    (pm, ps), (tm, ts) = evaluate_core.statistics(first)
    second = evaluate_data.rows(logits, targets, words, post, 0,
                                (pm, tm))
    stems = [str(s) for s in data['stems']]
    overall, granular = evaluate_core.results(
        evaluate_data.DATASET, stems, second, ps, ts)
    assert list(granular) == [f'{evaluate_data.DATASET}/{s}' for s in stems]
    np.testing.assert_allclose(
        [overall[f] for f in evaluate_data.FIELDS],
        data[f'{method}_overall'], rtol=1e-9)
    np.testing.assert_allclose(
        [[granular[f'{evaluate_data.DATASET}/{s}'][f]
          for f in evaluate_data.FIELDS] for s in stems],
        data[f'{method}_granular'], rtol=1e-9)


def test_statistics_edge_cases():
    from emphases_amd import runtime
    row = np.zeros((1, runtime.METRIC_FIELDS))
    row[0, runtime.METRIC_COUNT] = 1
    row[0, runtime.METRIC_SUM_PREDICTED] = .5
    row[0, runtime.METRIC_SUMSQ_PREDICTED] = .25
    (pm, ps), (tm, ts) = evaluate_core.statistics(row)
    assert pm == .5 and np.isnan(ps) and tm == 0. and np.isnan(ts)
    overall, granular = evaluate_core.results('d', ['a'], row, 0., 1.)
    assert np.isnan(overall['pearson_correlation'])
    empty = np.zeros((2, runtime.METRIC_FIELDS))
    overall, granular = evaluate_core.results('d', ['a', 'b'], empty, 1., 1.)
    assert all(np.isnan(v) for v in granular['d/a'].values())


def test_cli_pitch_variance_without_penn(cache, tmp_path):
    """Without `penn` (and no tracker to pass on the command line) the
    pitch-variance CLI fails as `python -m emphases_amd` does: penn's
    NotImplementedError, before any GPU work."""
    try:
        import penn  # noqa: F401
    except ImportError:
        pass
    else:
        pytest.skip('penn is installed')
    partition_dir, cache_dir = cache
    out = subprocess.run(
        [sys.executable, '-m', 'emphases_amd.evaluate',
         '--datasets', evaluate_data.DATASET,
         '--partition_dir', partition_dir, '--cache_dir', cache_dir,
         '--eval_dir', str(tmp_path), '--method', 'pitch-variance'],
        cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0
    assert 'NotImplementedError' in out.stderr and 'penn' in out.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), 'emphases'))
