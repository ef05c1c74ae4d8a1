"""Training end to end on the MI355X: `emph_collate` and the resident loader
bitwise against the host-collated path (`Trainer.prepare`), the loop against
hand-driven steps, validation against a float64 restatement, resume and the
CLI - on the synthetic cache of tests/loop_data.py."""
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
import loop_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import data, metrics, synth, train  # noqa: E402
from emphases_amd.evaluate import core as evaluate_core  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = {
    80: emphases_amd.DEFAULT,
    83: emphases_amd.Config(
        pitch_feature=True, periodicity_feature=True, loudness_feature=True,
        normalize=True)}


@pytest.fixture(scope='module')
def cache(tmp_path_factory):
    return loop_data.build_cache(str(tmp_path_factory.mktemp('loop')))


def resident(cache, partition, config=emphases_amd.DEFAULT, upload=True):
    partition_dir, cache_dir = cache
    return data.Dataset(
        loop_data.DATASET, partition, partition_dir=partition_dir,
        cache_dir=cache_dir, config=config, gpu=0, upload=upload)


def host(cache, dataset, indices):
    """The batch `indices` of `dataset` collated on the host from its files."""
    return loop_data.collated(
        cache[1], [dataset.stems[i] for i in indices], dataset.config)


def bits(tensor):
    return tensor.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@pytest.mark.parametrize('features', [80, 83])
def test_collate_is_bitwise_the_host_path(cache, features):
    config = CONFIGS[features]
    dataset = resident(cache, 'all', config)
    assert dataset.features.shape == (features, dataset.ld_cache)
    trainer = train.Trainer(config, gpu=0)
    for indices in ([9, 0, 11, 3, 5], [0]):
        want = trainer.prepare(*host(cache, dataset, indices))
        plan = want.plan
        got_features = torch.full(
            (features, plan.ld_frames), float('nan'), device='cuda:0')
        got_targets = torch.full(
            (plan.ld_words,), float('nan'), device='cuda:0')
        data.collate(dataset, indices, plan, got_features, got_targets)
        assert not torch.isnan(got_features).any()
        assert not torch.isnan(got_targets).any()
        assert same(got_features, want.features)
        assert same(got_targets, want.targets)
    # the loader's own buffers, dirty and reused: three batches, two slots
    loader = data.Loader(dataset, data.Sampler(dataset), trainer)
    loader.batch([10, 11])
    loader.batch([11, 10])
    for slot in loader._slots:
        for buffer in slot:
            buffer.fill_(float('nan'))
    for indices in ([9, 0, 11, 3, 5], [0], [4, 8]):
        got = loader.batch(indices)
        want = trainer.prepare(*host(cache, dataset, indices))
        assert same(got.features, want.features)
        assert same(got.targets, want.targets)
        assert same(got.meta['_buffer'], want.meta['_buffer'])


@pytest.mark.parametrize('shift,ld_pad', [(1, 0), (0, 2), (3, 1)])
def test_collate_moves_unaligned_sources_column_by_column(cache, shift, ld_pad):
    """Resident arrays that are not 16-byte aligned (a source pointer `shift`
    floats past an aligned one, a row length that is no multiple of 4): every
    quad takes the column-by-column path, the result is the same bits."""
    from emphases_amd import runtime
    from emphases_amd.data.collate import item_table
    dataset = resident(cache, 'all')
    trainer = train.Trainer(emphases_amd.DEFAULT, gpu=0)
    indices = [9, 0, 11, 3, 5]
    want = trainer.prepare(*host(cache, dataset, indices))
    plan = want.plan
    ld = dataset.ld_cache + ld_pad
    store = torch.full((80 * ld + shift,), float('nan'), device='cuda:0')
    features = store[shift:].view(80, ld)
    features[:, :dataset.ld_cache] = dataset.features
    words = dataset.targets.numel()
    store_targets = torch.full((words + shift,), float('nan'), device='cuda:0')
    targets = store_targets[shift:]
    targets.copy_(dataset.targets)
    assert (features.data_ptr() % 16 != 0) == (shift != 0)
    table = torch.from_numpy(item_table(dataset, indices, plan)).cuda()
    got_features = torch.full(
        (80, plan.ld_frames), float('nan'), device='cuda:0')
    got_targets = torch.full((plan.ld_words,), float('nan'), device='cuda:0')
    runtime.check(runtime.library().emph_collate(
        features.data_ptr(), ld, targets.data_ptr(), words, table.data_ptr(),
        len(indices), 80, plan.ld_frames, plan.ld_words,
        got_features.data_ptr(), got_targets.data_ptr(), runtime.stream()),
        'emph_collate')
    assert same(got_features, want.features)
    assert same(got_targets, want.targets)


def test_loader_equals_the_host_path(cache):
    dataset = resident(cache, 'train')
    trainer = train.Trainer(gpu=0, config=emphases_amd.DEFAULT)
    sampler = data.Sampler(dataset, 600)
    loader = data.Loader(dataset, sampler, trainer)
    batches = list(sampler)
    assert len(loader) == len(batches) == 3
    count = 0
    for indices, batch in zip(batches, loader):
        loss, gradients = trainer.loss_and_gradients(batch)
        want_loss, want = trainer.loss_and_gradients(
            *host(cache, dataset, indices))
        assert same(loss, want_loss)
        for name in want:
            assert same(gradients[name], want[name]), name
        count += 1
    assert count == 3


def hand_driven(cache, trainer, steps, epoch=0, max_frames=600):
    """`steps` calls of `trainer.step(*host_collated)` over the sampler's
    batches, epoch by epoch from `epoch`."""
    dataset = resident(cache, 'train', upload=False)
    sampler = data.Sampler(dataset, max_frames)
    done = 0
    while done < steps:
        sampler.set_epoch(epoch)
        for indices in sampler:
            trainer.step(*host(cache, dataset, indices))
            done += 1
            if done == steps:
                break
        epoch += 1
    return trainer


def run(cache, directory, **kwargs):
    partition_dir, cache_dir = cache
    return train.train(
        loop_data.DATASET, directory, 0, partition_dir=partition_dir,
        cache_dir=cache_dir, config=emphases_amd.DEFAULT,
        max_training_frames=600, **kwargs)


def load(path):
    return torch.load(path, map_location='cpu', weights_only=False)


def test_loop_equals_hand_driven_steps(cache, tmp_path):
    path = run(cache, tmp_path / 'a', num_steps=8, log_interval=4,
               save_after=2)
    assert path == str(tmp_path / 'a' / '00000008.pt')
    saved = load(path)
    assert saved['step'] == 8
    with open(tmp_path / 'a' / 'scalars.jsonl') as file:
        scalars = [json.loads(line) for line in file]
    assert [line['step'] for line in scalars] == [0, 4]
    for line in scalars:
        assert set(line) == {
            'step', 'loss/train', 'pearson_correlation/valid', 'bce/valid',
            'mse/valid'}
        assert np.isfinite(line['loss/train']) and line['loss/train'] > 0
    want = hand_driven(cache, train.Trainer(emphases_amd.DEFAULT, gpu=0), 8)
    assert want.steps == 8
    state, optimizer = want.state_dict(), want.optimizer_state_dict()
    assert list(saved['model']) == list(state)
    for name, value in state.items():
        assert same(saved['model'][name], value), name
    for index, entry in optimizer['state'].items():
        assert float(saved['optimizer']['state'][index]['step']) == 8.
        for moment in ('exp_avg', 'exp_avg_sq'):
            assert same(saved['optimizer']['state'][index][moment],
                        entry[moment]), (index, moment)
    again = load(run(cache, tmp_path / 'b', num_steps=8, log_interval=4,
                     save_after=2))
    for name, value in saved['model'].items():
        assert same(again['model'][name], value), name


def test_validation_matches_a_float64_restatement(cache):
    trainer = train.Trainer(emphases_amd.DEFAULT, gpu=0)
    dataset = resident(cache, 'valid')
    loader = data.Loader(dataset, data.Sampler(dataset), trainer)
    before = [t.clone() for t in (
        trainer.parameters, trainer.exp_avg, trainer.exp_avg_sq)]
    got = train.evaluate(trainer, loader)
    assert set(got) == {'pearson_correlation', 'bce', 'mse'}
    logits, targets, counts, stems = [], [], [], []
    for indices in loader.sampler:
        batch = loader.batch(indices)
        values = trainer.logits(batch)
        assert values.is_cuda and values.dtype == torch.float32
        assert values.shape == (int(dataset.words[indices].sum()),)
        logits.append(values.cpu().numpy())
        for i in indices:
            first = dataset.word_first[i]
            targets.append(dataset.targets[
                first:first + dataset.words[i]].cpu().numpy())
            counts.append(int(dataset.words[i]))
            stems.append(dataset.stems[i])
    assert sorted(stems) == sorted(dataset.stems)
    for tensor, kept in zip((trainer.parameters, trainer.exp_avg,
                             trainer.exp_avg_sq), before):
        assert same(tensor, kept)
    logits, targets = np.concatenate(logits), np.concatenate(targets)
    post, bce_form = metrics.forms('neural', 'bce')
    first = evaluate_data.rows(logits, targets, counts, post, bce_form)
    (p_mean, p_std), (t_mean, t_std) = evaluate_core.statistics(first)
    second = evaluate_data.rows(
        logits, targets, counts, post, bce_form, (p_mean, t_mean))
    want, _ = evaluate_core.results(
        loop_data.DATASET, stems, second, p_std, t_std)
    for key in want:
        print(key, got[key], want[key])
    for key in want:
        assert got[key] == pytest.approx(want[key], rel=1e-5, abs=1e-6), key
    # log_steps cuts the walk: one batch is two of the four utterances
    assert train.evaluate(trainer, loader, log_steps=1) != got


def test_resume_continues_where_the_file_stops(cache, tmp_path):
    directory = tmp_path / 'run'
    first = run(cache, directory, num_steps=4)
    assert first == str(directory / '00000004.pt')
    stamp = (os.stat(first).st_mtime_ns, open(first, 'rb').read())
    saved = load(first)
    assert saved['step'] == 4
    second = run(cache, directory, num_steps=8)
    assert second == str(directory / '00000008.pt')
    assert stamp == (os.stat(first).st_mtime_ns, open(first, 'rb').read())
    assert sorted(os.listdir(directory)) == [
        '00000004.pt', '00000008.pt', 'scalars.jsonl']
    resumed = load(second)
    assert resumed['step'] == 8 and resumed['epoch'] > saved['epoch']
    # four more hand-driven steps from the file, moments and count restored
    want = hand_driven(
        cache, train.Trainer(emphases_amd.DEFAULT, checkpoint=first, gpu=0),
        4, epoch=saved['epoch'])
    assert want.steps == 8
    for name, value in want.state_dict().items():
        assert same(resumed['model'][name], value), name
    for index, entry in want.optimizer_state_dict()['state'].items():
        assert float(resumed['optimizer']['state'][index]['step']) == 8.
        for moment in ('exp_avg', 'exp_avg_sq'):
            assert same(resumed['optimizer']['state'][index][moment],
                        entry[moment]), (index, moment)
    # nothing is left to do: the run ends where it is
    assert run(cache, directory, num_steps=8) == second


def test_cli_trains_and_writes_a_loadable_checkpoint(cache, tmp_path):
    partition_dir, cache_dir = cache
    out = subprocess.run(
        [sys.executable, '-m', 'emphases_amd.train',
         '--dataset', loop_data.DATASET, '--gpu', '0',
         '--directory', str(tmp_path / 'cli'),
         '--partition_dir', partition_dir, '--cache_dir', cache_dir,
         '--num_steps', '2', '--max_training_frames', '600'],
        cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    path = tmp_path / 'cli' / '00000002.pt'
    assert path.is_file()
    trainer = train.Trainer(checkpoint=str(path), gpu=0)
    assert trainer.steps == 2
    audio = torch.from_numpy(synth.audio(3, 211))
    alignment = emphases_amd.Alignment.from_frames(
        synth.word_frames(3, 211, 3, 40))
    scores = emphases_amd.from_alignment_and_audio(
        alignment, audio, emphases_amd.SAMPLE_RATE, checkpoint=str(path),
        gpu=0)
    assert scores.shape[-1] == len(alignment)
    assert torch.isfinite(scores).all()
