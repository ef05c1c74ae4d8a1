"""`TransformerTrainer` on the MI355X: `emph_adam_step_gathered` bitwise
against `emph_adam_step` tensor by tensor, the trainer's loss and gradients
bitwise against a fresh `TransformerModel` on the back-to-back form of the
same batch, three steps bitwise against that model with `emph_adam_step` per
parameter, the loop with `trainer=TransformerTrainer` (files, resume, the
checkpoint in the inference engine) and validation - all at layers=2."""
import functools
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loop_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import data, runtime, train, weights  # noqa: E402
from emphases_amd import engine as engine_module  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, 'golden', 'transformer_train.npz')
CONFIGS = {
    'intermediate_sum': dict(downsample_location='intermediate',
                             downsample_method='sum'),
    'loss_max': dict(downsample_location='loss', downsample_method='max')}
DEVICE = 'cuda:0'
PARITY = 1e-4                   # the project's tolerance on scores


def config_of(name):
    return emphases_amd.Config(
        architecture='transformer', layers=2, **CONFIGS[name])


def bits(tensor):
    return tensor.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


###############################################################################
# Batches: items (features [C, T], bounds [2, W], targets [W]) on the host
###############################################################################


@functools.lru_cache(maxsize=None)
def golden_items():
    """The three utterances of tests/golden/transformer_train.npz: 37, 64
    and 130 frames."""
    with np.load(GOLDEN) as archive:
        arrays = {name: archive[name] for name in (
            'features', 'frames', 'words', 'bounds', 'targets')}
    items, frame, word = [], 0, 0
    for frames, words in zip(arrays['frames'], arrays['words']):
        items.append((
            torch.from_numpy(arrays['features'][:, frame:frame + frames].copy()),
            torch.from_numpy(arrays['bounds'][:, word:word + words].copy()),
            torch.from_numpy(arrays['targets'][word:word + words].copy())))
        frame, word = frame + int(frames), word + int(words)
    return items


@functools.lru_cache(maxsize=None)
def hard_items():
    """130, 64 and 1 frames with 5, 2 and 1 words: a segment on each side of
    the 128 positions from which 'bf16x3' takes the bf16 pipe, and an
    utterance of one frame."""
    rng = np.random.default_rng(20261021)
    items = []
    for frames, words in ((130, 5), (64, 2), (1, 1)):
        cuts = np.sort(rng.choice(
            np.arange(1, frames), size=words - 1, replace=False))
        edges = np.concatenate([[0], cuts, [frames]]).astype(np.int64)
        items.append((
            torch.from_numpy(
                rng.standard_normal((80, frames)).astype(np.float32)),
            torch.from_numpy(np.stack([edges[:-1], edges[1:]])),
            torch.from_numpy(rng.uniform(0., 1., words).astype(np.float32))))
    return items


def collated(items):
    """`emphases.data.collate`'s first five of `items`, zero padded."""
    frames = torch.tensor([f.shape[1] for f, _, _ in items])
    words = torch.tensor([b.shape[1] for _, b, _ in items])
    features = torch.zeros(len(items), items[0][0].shape[0], int(frames.max()))
    bounds = torch.zeros(len(items), 2, int(words.max()), dtype=torch.long)
    targets = torch.zeros(len(items), 1, int(words.max()))
    for i, (feature, bound, target) in enumerate(items):
        features[i, :, :frames[i]] = feature
        bounds[i, :, :words[i]] = bound
        targets[i, 0, :words[i]] = target
    return features, frames, bounds, words, targets


def back_to_back(items):
    """(`TransformerModel`'s arguments, the targets [sum W]) of `items`."""
    cu = lambda counts: torch.tensor(  # noqa: E731
        np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64)
    return (torch.cat([f for f, _, _ in items], dim=1).to(DEVICE),
            cu([f.shape[1] for f, _, _ in items]),
            torch.cat([b for _, b, _ in items], dim=1),
            cu([b.shape[1] for _, b, _ in items])), \
        torch.cat([t for _, _, t in items]).to(DEVICE)


def model_loss_and_gradients(model, items, steps=0):
    """The comparator: the model in training mode at dropout step `steps`,
    `loss_fn`, `backward()`; (loss, [gradient per parameter])."""
    inputs, targets = back_to_back(items)
    model.train()
    model.steps = steps
    model.zero_grad(set_to_none=True)
    loss = train.loss_fn(model(*inputs), targets, model.config.loss)
    loss.backward()
    return loss.detach(), [p.grad for p in model.parameters()]


###############################################################################
# 5. The kernel, bitwise
###############################################################################


SIZES = (1, 3, 255, 256, 257, 1023, 1025, 19200)
GUARD = 12345.


@pytest.mark.parametrize(
    'filled', [1, runtime.ADAM_TABLE, runtime.ADAM_TABLE + 1])
def test_gathered_adam_is_adam_tensor_by_tensor(filled):
    """`filled` tensors that hold something - a table of one, a full one, and
    one more, which takes a second launch - and, among more than one, an
    empty tensor with a null gradient, which takes no place in a table."""
    library = runtime.library()
    generator = torch.Generator(device=DEVICE).manual_seed(filled)
    # (a single tensor takes the largest size: more than one workgroup)
    sizes = [19200] if filled == 1 else \
        [SIZES[t % len(SIZES)] for t in range(filled)]
    if filled > 1:
        assert set(sizes) == set(SIZES)
        sizes.insert(5, 0)
    tensors = len(sizes)
    launches = -(-filled // runtime.ADAM_TABLE)
    # three guard floats before every tensor and behind the last
    offsets = np.cumsum([3] + [size + 3 for size in sizes[:-1]])
    total = int(offsets[-1]) + sizes[-1] + 3
    inside = torch.zeros(total, dtype=torch.bool, device=DEVICE)
    for offset, size in zip(offsets, sizes):
        inside[int(offset):int(offset) + size] = True
    random = lambda low: torch.rand(  # noqa: E731
        total, device=DEVICE, generator=generator) + low
    flats = [torch.where(inside, values, torch.full_like(values, GUARD))
             for values in (random(-0.5), random(-0.5), random(0.))]
    wants = [flat.clone() for flat in flats]
    starts = flats[0].clone()
    betas, lr, eps = (0.9, 0.999), 1e-3, 1e-8
    host_offsets = np.array(offsets, dtype=np.int64)
    host_counts = np.array(sizes, dtype=np.int64)
    for step in (1, 2, 3):
        # gradients one float into their allocations: 4-byte aligned only
        stores = [torch.randn(size + 1, device=DEVICE, generator=generator)
                  for size in sizes]
        gradients = [store[1:] for store in stores]
        addresses = np.array(
            [g.data_ptr() if g.numel() else 0 for g in gradients],
            dtype=np.uint64)
        assert all(g.data_ptr() % 16 == 4 for g in gradients if g.numel())
        step_size = lr / (1. - betas[0] ** step)
        correction = math.sqrt(1. - betas[1] ** step)
        with runtime.LaunchTimer() as timer:
            runtime.check(library.emph_adam_step_gathered(
                flats[0].data_ptr(), addresses.ctypes.data,
                host_offsets.ctypes.data, host_counts.ctypes.data, tensors,
                flats[1].data_ptr(), flats[2].data_ptr(), *betas, step_size,
                correction, eps, runtime.stream()), 'emph_adam_step_gathered')
        assert timer.launches == launches
        for offset, size, gradient in zip(offsets, sizes, gradients):
            first = 4 * int(offset)
            runtime.check(library.emph_adam_step(
                wants[0].data_ptr() + first, gradient.data_ptr(),
                wants[1].data_ptr() + first, wants[2].data_ptr() + first,
                size, *betas, step_size, correction, eps, runtime.stream()),
                'emph_adam_step')
        for name, got, want in zip(
                ('parameters', 'exp_avg', 'exp_avg_sq'), flats, wants):
            assert same(got, want), (name, step)
            assert bool((got[~inside] == GUARD).all()), (name, step)
    # it did something: three updates of about lr each move a parameter of
    # about 0.25 by thousands of ulps (a few lie where the updates cancel)
    moved = (flats[0][inside] != starts[inside]).float().mean()
    assert float(moved) > 0.99, float(moved)


###############################################################################
# 6. The step's loss and gradients are the model's, bitwise
###############################################################################


CASES = [(name, precision, False, 0) for name in CONFIGS
         for precision in ('f32', 'bf16x3')] + \
        [(name, 'f32', True, steps) for name in CONFIGS for steps in (0, 3)]


def case_id(case):
    name, precision, dropout, steps = case
    return f'{name}-{precision}' + (f'-dropout-step{steps}' if dropout else '')


def assert_same_gradients(trainer, model, items, steps, batch=None):
    trainer.steps = steps
    loss, gradients = trainer.loss_and_gradients(
        *((batch,) if batch is not None else collated(items)))
    want_loss, want = model_loss_and_gradients(model, items, steps)
    names = [name for name, _ in model.named_parameters()]
    assert list(gradients) == names
    assert loss.shape == () and same(loss, want_loss), \
        (float(loss), float(want_loss))
    for name, gradient in zip(names, want):
        assert same(gradients[name], gradient), name
    assert trainer.steps == steps
    return loss


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_loss_and_gradients_are_the_models(case):
    name, precision, dropout, steps = case
    config = config_of(name)
    trainer = train.TransformerTrainer(
        config, gpu=0, seed=3, precision=precision, reference_dropout=dropout)
    model = train.TransformerModel(
        config, seed=3, precision=precision,
        reference_dropout=dropout).to(DEVICE)
    # the state: bitwise the initialisation, flat, the parameters its views
    initial = train.initial_transformer_state(config, 3)
    assert list(trainer.state_dict()) == list(initial)
    for key, value in trainer.state_dict().items():
        assert same(value, torch.from_numpy(initial[key])), key
    first = trainer.parameters.data_ptr()
    for (key, (offset, shape)), parameter in zip(
            trainer.offsets.items(), trainer.model.parameters()):
        assert parameter.data_ptr() == first + 4 * offset, key
        assert tuple(parameter.shape) == tuple(shape), key
    before = trainer.parameters.clone()
    losses = [assert_same_gradients(trainer, model, items, steps)
              for items in (golden_items(), hard_items())]
    assert not same(losses[0], losses[1])
    if dropout:
        # the masks are a function of the step
        other = trainer.loss_and_gradients(*collated(golden_items()))[0]
        assert same(other, losses[0])
        trainer.steps = steps + 1
        moved = trainer.loss_and_gradients(*collated(golden_items()))[0]
        assert not same(moved, losses[0])
    assert same(trainer.parameters, before)
    assert not trainer.exp_avg.any() and not trainer.exp_avg_sq.any()


@pytest.fixture(scope='module')
def cache(tmp_path_factory):
    return loop_data.build_cache(str(tmp_path_factory.mktemp('loop')))


def resident(cache, partition, config):
    partition_dir, cache_dir = cache
    return data.Dataset(
        loop_data.DATASET, partition, partition_dir=partition_dir,
        cache_dir=cache_dir, config=config, gpu=0)


def cache_items(cache, dataset, indices):
    """The utterances `indices` of `dataset` read from the cache's files."""
    items = []
    for index in indices:
        features, scores, bounds = loop_data.item(
            cache[1], dataset.stems[index], dataset.config)
        items.append((features, bounds, scores[0]))
    return items


@pytest.mark.parametrize('precision', ['f32', 'bf16x3'])
def test_a_loader_batch_out_of_dirty_buffers_gives_the_same_bits(
        cache, precision):
    config = config_of('intermediate_sum')
    trainer = train.TransformerTrainer(config, gpu=0, precision=precision)
    model = train.TransformerModel(config, precision=precision).to(DEVICE)
    dataset = resident(cache, 'all', config)
    loader = data.Loader(dataset, data.Sampler(dataset), trainer)
    loader.batch([10, 11])
    loader.batch([11, 10])
    for slot in loader._slots:
        for buffer in slot:
            buffer.fill_(float('nan'))
    # 300, 1, 129 and 64 frames; 40, 1, 2 and 2 words
    indices = [11, 0, 8, 5]
    batch = loader.batch(indices)
    assert_same_gradients(
        trainer, model, cache_items(cache, dataset, indices), 0, batch)
    # and what `prepare` makes of the host-collated batch is that batch
    prepared = trainer.prepare(*loop_data.collated(
        cache[1], [dataset.stems[i] for i in indices], config))
    for key in ('cu_frames', 'cu_words', 'bounds', 'frame_columns',
                'word_columns'):
        assert torch.equal(prepared.meta[key], batch.meta[key]), key
    inputs, targets = trainer._inputs(batch)
    want_inputs, want_targets = trainer._inputs(prepared)
    assert same(inputs[0], want_inputs[0]) and same(targets, want_targets)


###############################################################################
# 7. Three steps, bitwise
###############################################################################


def adam_per_parameter(model, moments, step, lr=1e-3, betas=(0.9, 0.999),
                       eps=1e-8):
    """`emph_adam_step` on a clone of every parameter, copied back with
    `copy_` (which advances the parameter's version)."""
    library = runtime.library()
    for parameter, (exp_avg, exp_avg_sq) in zip(model.parameters(), moments):
        clone = parameter.detach().clone()
        gradient = parameter.grad.contiguous()
        runtime.check(library.emph_adam_step(
            clone.data_ptr(), gradient.data_ptr(), exp_avg.data_ptr(),
            exp_avg_sq.data_ptr(), clone.numel(), *betas,
            lr / (1. - betas[0] ** step), math.sqrt(1. - betas[1] ** step),
            eps, runtime.stream()), 'emph_adam_step')
        with torch.no_grad():
            parameter.copy_(clone)


def flat_of(tensors):
    return torch.cat([tensor.detach().reshape(-1) for tensor in tensors])


@pytest.mark.parametrize('case', [
    ('intermediate_sum', 'f32', False), ('loss_max', 'bf16x3', False),
    ('intermediate_sum', 'f32', True)], ids=lambda case: case_id(case + (0,)))
def test_three_steps_are_the_models_trajectory(case):
    name, precision, dropout = case
    config = config_of(name)
    trainer = train.TransformerTrainer(
        config, gpu=0, precision=precision, reference_dropout=dropout)
    model = train.TransformerModel(
        config, precision=precision, reference_dropout=dropout).to(DEVICE)
    moments = [(torch.zeros_like(p), torch.zeros_like(p))
               for p in model.parameters()]
    batch = trainer.prepare(*collated(golden_items()))
    losses = []
    for step in (1, 2, 3):
        version = trainer.parameters._version
        loss = trainer.step(batch)
        assert trainer.steps == step
        assert trainer.parameters._version == version + 1
        assert all(p._version == version + 1 and p.grad is None
                   for p in trainer.model.parameters())
        want_loss, _ = model_loss_and_gradients(
            model, golden_items(), steps=step - 1)
        adam_per_parameter(model, moments, step)
        assert same(loss, want_loss), (step, float(loss), float(want_loss))
        assert same(trainer.parameters, flat_of(model.parameters())), step
        assert same(trainer.exp_avg, flat_of(m for m, _ in moments)), step
        assert same(trainer.exp_avg_sq, flat_of(v for _, v in moments)), step
        losses.append(loss)
    print('losses', ' '.join(f'{float(loss):.9g}' for loss in losses))
    assert not same(losses[1], losses[0])
    assert float(losses[2]) < float(losses[0])


###############################################################################
# 8. The loop: files, resume, the checkpoint in the inference engine
###############################################################################


def run(cache, directory, config, **kwargs):
    partition_dir, cache_dir = cache
    return train.train(
        loop_data.DATASET, directory, 0, partition_dir=partition_dir,
        cache_dir=cache_dir, config=config, max_training_frames=600,
        log_interval=2, save_after=0, trainer=train.TransformerTrainer,
        **kwargs)


def load(path):
    return torch.load(path, map_location='cpu', weights_only=False)


@pytest.mark.parametrize('dropout', [False, True], ids=['plain', 'dropout'])
def test_loop_writes_the_files_and_resumes_bitwise(cache, tmp_path, dropout):
    config = config_of('intermediate_sum')
    arguments = {'trainer_arguments': {'reference_dropout': True}} \
        if dropout else {}
    # (the eight training utterances are three batches of 600 frames: six
    # steps end the second epoch, three the first)
    whole = run(cache, tmp_path / 'whole', config, num_steps=6, **arguments)
    assert whole == str(tmp_path / 'whole' / '00000006.pt')
    names = sorted(os.listdir(tmp_path / 'whole'))
    assert 'scalars.jsonl' in names and '00000006.pt' in names
    assert all(name == 'scalars.jsonl' or re.fullmatch(r'\d{8}\.pt', name)
               for name in names)
    with open(tmp_path / 'whole' / 'scalars.jsonl') as file:
        scalars = [json.loads(line) for line in file]
    assert [line['step'] for line in scalars] == [0, 2, 4]
    for line in scalars:
        assert set(line) == {
            'step', 'loss/train', 'pearson_correlation/valid', 'bce/valid',
            'mse/valid'}
        assert all(np.isfinite(value) for value in line.values())
    saved = load(whole)
    assert set(saved) == {'epoch', 'step', 'score', 'best', 'model',
                          'optimizer'}
    assert saved['step'] == 6 and saved['epoch'] == 2
    assert list(saved['model']) == list(
        weights.parameter_shapes(config))

    first = run(cache, tmp_path / 'parts', config, num_steps=3, **arguments)
    assert first == str(tmp_path / 'parts' / '00000003.pt')
    assert load(first)['epoch'] == 1
    second = run(cache, tmp_path / 'parts', config, num_steps=6, **arguments)
    resumed = load(second)
    assert resumed['step'] == 6 and resumed['epoch'] == 2
    assert not same(load(first)['model']['output_layer.weight'],
                    resumed['model']['output_layer.weight'])
    for key, value in saved['model'].items():
        assert same(resumed['model'][key], value), key
    assert resumed['optimizer']['param_groups'] == \
        saved['optimizer']['param_groups']
    assert len(saved['optimizer']['state']) == len(saved['model'])
    for index, entry in saved['optimizer']['state'].items():
        other = resumed['optimizer']['state'][index]
        assert float(entry['step']) == float(other['step']) == 6.
        for moment in ('exp_avg', 'exp_avg_sq'):
            assert same(other[moment], entry[moment]), (index, moment)
    if dropout:
        return
    # the final file in the inference engine, on the validation utterances
    trainer = train.TransformerTrainer(config, checkpoint=whole, gpu=0)
    assert trainer.steps == 6
    engine = engine_module.Engine(config, whole, 0)
    dataset = resident(cache, 'valid', config)
    loader = data.Loader(dataset, data.Sampler(dataset), trainer)
    words = 0
    for batch in loader:
        want = torch.sigmoid(trainer.logits(batch))
        with engine.lock:
            scores, _ = engine.forward(
                None, batch.plan, features=batch.features)
            got = scores[batch.meta['word_columns']].clone()
        apart = float((got - want).abs().max())
        print(f'engine against trainer scores: {apart:.3g} over '
              f'{want.numel()} words')
        assert got.shape == want.shape and apart <= PARITY
        words += want.numel()
    assert words == sum(loop_data.WORDS[i] for i in loop_data.VALID)


###############################################################################
# 9. Validation
###############################################################################


class Stored:
    """What `train.evaluate` asks of a trainer, answering with logits made
    beforehand, batch by batch."""

    def __init__(self, trainer, logits):
        self.device, self.config = trainer.device, trainer.config
        self._logits = list(logits)

    def logits(self, batch):
        return self._logits.pop(0)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_validation_is_the_models(cache, name):
    config = config_of(name)
    trainer = train.TransformerTrainer(config, gpu=0, seed=1)
    model = train.TransformerModel(config, seed=1).to(DEVICE).eval()
    dataset = resident(cache, 'valid', config)
    loader = data.Loader(dataset, data.Sampler(dataset), trainer)
    before = trainer.parameters.clone()
    got = train.evaluate(trainer, loader)
    assert set(got) == {'pearson_correlation', 'bce', 'mse'}
    assert all(np.isfinite(value) for value in got.values())
    wanted = []
    for indices in loader.sampler:
        inputs, _ = back_to_back(cache_items(cache, dataset, indices))
        with torch.no_grad():
            wanted.append(model(*inputs))
        logits = trainer.logits(loader.batch(indices))
        assert logits.is_cuda and logits.dtype == torch.float32
        assert same(logits, wanted[-1])
    assert sum(len(w) for w in wanted) == int(dataset.words.sum())
    want = train.evaluate(Stored(trainer, wanted), loader)
    print(got, want)
    assert got == want
    assert same(trainer.parameters, before) and trainer.steps == 0
    assert trainer.model.training is False
