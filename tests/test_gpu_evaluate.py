"""emphases_amd.evaluate on the MI355X: `emph_word_metrics_grouped` against a
float64 oracle and for determinism, `Metrics(method=...)`, and the dataset
evaluation end to end against the reference's own (tests/golden/evaluate.npz)."""
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

pytestmark = pytest.mark.gpu

FORMS = [(1, 0), (2, 1), (0, 0), (0, 1)]   # neural+bce/mse, baseline+bce/mse


def _oracle(x, y, cu, post, bce_form, pm, tm):
    """Per-word terms in float32 as the kernel forms them, sums in float64."""
    x, y = x.astype(np.float32), y.astype(np.float32)
    with np.errstate(over='ignore'):
        if post == 1:
            score = (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(
                np.float32)
        elif post == 2:
            score = np.clip(x, 0, 1).astype(np.float32)
        else:
            score = x
        if bce_form == 0:
            bce = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))
        else:
            c = np.clip(x, 0, 1)
            bce = -(y * np.log(c + np.float32(1e-6)) +
                    (1 - y) * np.log(1 - c + np.float32(1e-6)))
    bce = bce.astype(np.float32)
    error = (score - y).astype(np.float32)
    cov = ((score - np.float32(pm)) * (y - np.float32(tm))).astype(np.float32)
    s, t = score.astype(np.float64), y.astype(np.float64)
    terms = np.stack([np.ones_like(s), bce.astype(np.float64),
                      (error * error).astype(np.float64),
                      cov.astype(np.float64), s, s * s, t, t * t])
    return np.stack([terms[:, a:b].sum(axis=1)
                     for a, b in zip(cu[:-1], cu[1:])])


def _inputs(sizes, seed):
    rng = np.random.default_rng(seed)
    total = int(sum(sizes))
    x = (rng.standard_normal(total) * 3).astype(np.float32)
    x[::7] = rng.uniform(-0.2, 1.2, len(x[::7]))     # around the clamp
    y = (rng.integers(0, 9, total) / 8).astype(np.float32)
    cu = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return x, y, cu


@pytest.mark.parametrize('post,bce_form', FORMS)
def test_grouped_kernel_against_float64_oracle(post, bce_form):
    from emphases_amd import metrics, runtime
    sizes = [0, 1, 63, 64, 65, 0, 2 ** 20 + 3, 7, 0]
    x, y, cu = _inputs(sizes, 7 + post + 3 * bce_form)
    device = torch.device('cuda', 0)
    got = metrics.grouped(
        torch.from_numpy(x).to(device), torch.from_numpy(y).to(device), cu,
        post, bce_form, 0.375, 0.5).cpu().numpy()
    want = _oracle(x, y, cu, post, bce_form, 0.375, 0.5)
    assert got.shape == (len(sizes), runtime.METRIC_FIELDS)
    assert not got[[0, 5, 8]].any()             # empty groups: rows of zeros
    # fields whose per-word terms are exact IEEE float32 arithmetic (no
    # transcendental, no contraction): 1e-9
    exact = [runtime.METRIC_COUNT, runtime.METRIC_SUM_TARGET,
             runtime.METRIC_SUMSQ_TARGET]
    if post != 1:
        exact += [runtime.METRIC_SQUARED_ERROR, runtime.METRIC_COVARIANCE,
                  runtime.METRIC_SUM_PREDICTED, runtime.METRIC_SUMSQ_PREDICTED]
    np.testing.assert_allclose(got[:, exact], want[:, exact], rtol=1e-9,
                               atol=1e-9)
    # the rest: an ulp of expf / log1pf / logf (and fma) per word
    rest = [f for f in range(runtime.METRIC_FIELDS) if f not in exact]
    worst = np.abs(got[:, rest] - want[:, rest]) / np.maximum(
        np.abs(want[:, rest]), 1.)
    print(f'post {post} bce {bce_form}: worst relative {worst.max():.2e}')
    np.testing.assert_allclose(got[:, rest], want[:, rest], rtol=1e-6,
                               atol=1e-6)


def test_grouped_kernel_is_deterministic():
    from emphases_amd import metrics
    device = torch.device('cuda', 0)
    rng = np.random.default_rng(11)
    sizes = rng.integers(0, 3000, 256)
    sizes[100] = 70001
    x, y, cu = _inputs(sizes, 12)
    xd, yd = torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)
    first = metrics.grouped(xd, yd, cu, 1, 0, 0.4, 0.5).cpu().numpy()
    again = metrics.grouped(xd, yd, cu, 1, 0, 0.4, 0.5).cpu().numpy()
    assert first.tobytes() == again.tobytes()
    for group in (0, 100, 255):
        a, b = int(cu[group]), int(cu[group + 1])
        alone = metrics.grouped(xd[a:b], yd[a:b], [0, b - a], 1, 0, 0.4,
                                0.5).cpu().numpy()
        assert alone.tobytes() == first[group:group + 1].tobytes()


def test_grouped_kernel_rejects_bad_arguments():
    from emphases_amd import metrics, runtime
    device = torch.device('cuda', 0)
    x = torch.zeros(4, device=device)
    with pytest.raises(ValueError):
        metrics.grouped(x, x, [0, 5], 0, 0)
    with pytest.raises(ValueError):
        metrics.grouped(x, x, [0, 3, 2, 4], 0, 0)
    with pytest.raises(runtime.LibraryError):
        metrics.grouped(x, x, [0, 4], 0, 2)
    with pytest.raises(runtime.LibraryError):
        metrics.grouped(x, x, [0, 4], 3, 0)


@pytest.mark.parametrize('loss', ['bce', 'mse'])
def test_metrics_method_scores_a_baseline(loss):
    """Metrics(method='duration-variance'): identity postprocess and the
    LOSS's BCE form, as evaluate/metrics.py with METHOD set to a baseline."""
    from emphases_amd import metrics
    rng = np.random.default_rng(5)
    lengths = torch.tensor([5, 1, 9])
    logits = torch.from_numpy(
        rng.uniform(-0.6, 0.8, (3, 1, 9)).astype(np.float32))
    targets = torch.from_numpy(
        (rng.integers(0, 9, (3, 1, 9)) / 8).astype(np.float32))
    mask = torch.arange(9)[None, None] < lengths[:, None, None]
    x = logits[mask].double()
    y = targets[mask].double()
    if loss == 'bce':
        bce = torch.nn.functional.binary_cross_entropy_with_logits(
            x, y, reduction='none')
    else:
        c = torch.clamp(x, 0., 1.)
        bce = -(y * torch.log(c + 1e-6) + (1 - y) * torch.log(1 - c + 1e-6))
    stats = ((0.1, 0.4), (0.5, 0.3))
    want = {
        'pearson_correlation': float(
            ((x - 0.1) * (y - 0.5)).sum() / x.numel() / (0.4 * 0.3)),
        'bce': float(bce.mean()),
        'mse': float(((x - y) ** 2).mean())}
    mine = metrics.Metrics(lambda: stats[0], lambda: stats[1], gpu=0,
                           loss=loss, method='duration-variance')
    mine.update(logits[:2], targets[:2], lengths[:2])
    mine.update(logits[2:], targets[2:], lengths[2:])
    got = mine()
    for key in want:
        assert got[key] == pytest.approx(want[key], rel=1e-5, abs=1e-6), key
    # the default is unchanged: sigmoid postprocess under 'bce'
    neural = metrics.Metrics(lambda: stats[0], lambda: stats[1], gpu=0,
                             loss=loss)
    neural.update(logits, targets, lengths)
    assert neural()['mse'] != pytest.approx(want['mse'], rel=1e-3)


@pytest.fixture(scope='module')
def data():
    return evaluate_data.golden()


@pytest.fixture(scope='module')
def cache(tmp_path_factory, data):
    root = str(tmp_path_factory.mktemp('evaluate'))
    return evaluate_data.build_cache(root, data)


def _run(cache, eval_dir, method, name='emphases', **kwargs):
    import emphases_amd
    from emphases_amd import evaluate, synth
    partition_dir, cache_dir = cache
    return evaluate.datasets(
        [evaluate_data.DATASET], gpu=0, partition_dir=partition_dir,
        cache_dir=cache_dir, eval_dir=eval_dir, name=name,
        config=emphases_amd.Config(method=method),
        pitch_tracker=synth.pitch_tracks, **kwargs)


@pytest.mark.parametrize('method', [
    'neural', 'duration-variance', 'pitch-variance'])
def test_datasets_match_reference(tmp_path, cache, data, method):
    overall, granular = _run(cache, str(tmp_path), method)
    stems = [str(s) for s in data['stems']]
    assert list(granular) == [f'{evaluate_data.DATASET}/{s}' for s in stems]
    assert list(overall) == [evaluate_data.DATASET]
    key = method.replace('-', '_')
    got_overall = [overall[evaluate_data.DATASET][f]
                   for f in evaluate_data.FIELDS]
    got_granular = [[granular[f'{evaluate_data.DATASET}/{s}'][f]
                     for f in evaluate_data.FIELDS] for s in stems]
    print(method, 'worst |overall - reference|',
          np.abs(np.subtract(got_overall, data[f'{key}_overall'])).max(),
          'granular', np.abs(np.subtract(
              got_granular, data[f'{key}_granular'])).max())
    np.testing.assert_allclose(got_overall, data[f'{key}_overall'],
                               rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got_granular, data[f'{key}_granular'],
                               rtol=1e-5, atol=1e-6)
    with open(tmp_path / 'emphases' / 'overall.json') as file:
        assert json.load(file) == overall
    with open(tmp_path / 'emphases' / 'granular.json') as file:
        assert json.load(file) == granular


def _files(directory):
    return [open(os.path.join(directory, name), 'rb').read()
            for name in ('overall.json', 'granular.json')]


@pytest.mark.parametrize('method', ['neural', 'pitch-variance'])
def test_results_do_not_depend_on_batching(tmp_path, cache, method):
    _run(cache, str(tmp_path), method, 'one', utterances_per_batch=1)
    _run(cache, str(tmp_path), method, 'all', utterances_per_batch=256)
    _run(cache, str(tmp_path), method, 'again', utterances_per_batch=256)
    one, every, again = (_files(str(tmp_path / n))
                         for n in ('one', 'all', 'again'))
    assert one == every
    assert every == again


def test_bf16x3_close_to_f32(tmp_path, cache):
    f32, f32_files = _run(cache, str(tmp_path), 'neural', 'f32')
    bf16, bf16_files = _run(cache, str(tmp_path), 'neural', 'bf16',
                            precision='bf16x3')
    assert list(bf16_files) == list(f32_files)
    pairs = [(f32[evaluate_data.DATASET][f], bf16[evaluate_data.DATASET][f])
             for f in evaluate_data.FIELDS]
    pairs += [(f32_files[k][f], bf16_files[k][f])
              for k in f32_files for f in evaluate_data.FIELDS]
    worst = max(abs(a - b) for a, b in pairs)
    print(f'bf16x3 vs f32: worst {worst:.2e}')
    assert worst <= 1e-4


def test_cli_writes_what_the_function_returns(tmp_path, cache):
    partition_dir, cache_dir = cache
    overall, granular = _run(cache, str(tmp_path / 'call'),
                             'duration-variance')
    out = subprocess.run(
        [sys.executable, '-m', 'emphases_amd.evaluate',
         '--datasets', evaluate_data.DATASET, '--gpu', '0',
         '--partition_dir', partition_dir, '--cache_dir', cache_dir,
         '--eval_dir', str(tmp_path / 'cli'), '--name', 'run',
         '--method', 'duration-variance'],
        cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(tmp_path / 'cli' / 'run' / 'overall.json') as file:
        assert json.load(file) == overall
    with open(tmp_path / 'cli' / 'run' / 'granular.json') as file:
        assert json.load(file) == granular
    assert _files(str(tmp_path / 'cli' / 'run')) == \
        _files(str(tmp_path / 'call' / 'emphases'))
