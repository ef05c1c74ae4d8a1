"""`TransformerLocationsModel` and `TransformerLocationsTrainer` on the
MI355X at downsample_location 'input' and 'inference', layers=2: the
trainer's loss and gradients bitwise a fresh model's, three steps bitwise the
model's with `emph_adam_step` per parameter, the loop (resume, the final file
in the inference engine within the project's 1e-4), the same batch behind
garbage in the padded feature columns, and 'intermediate' / 'loss' bitwise
the parent classes."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loop_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import data, runtime, train  # noqa: E402
from emphases_amd import engine as engine_module  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = {
    'input_average': dict(downsample_location='input',
                          downsample_method='average'),
    'input_max': dict(downsample_location='input', downsample_method='max'),
    'input_center': dict(downsample_location='input',
                         downsample_method='center'),
    'inference_linear': dict(downsample_location='inference',
                             downsample_method='sum',
                             upsample_method='linear')}
DEVICE = 'cuda:0'
PARITY = 1e-4                   # the project's tolerance on scores


def config_of(name):
    return emphases_amd.Config(
        architecture='transformer', layers=2, **CONFIGS[name])


def same(a, b):
    return a.shape == b.shape and torch.equal(
        a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def items():
    """Four utterances (features [80, T], bounds [2, W], targets [W]): a
    one-frame word; a word of 70 frames among words under 20 (pieces of 70
    columns with 1 .. 19 real keys: on both sides of the 64-wide tile); a
    single word of 80 frames (no padding, n = k > 64); a one-frame
    utterance."""
    rng = np.random.default_rng(20261022)
    edges = [[0, 1, 12, 30, 37], [0, 5, 75, 90, 91, 110], [0, 80], [0, 1]]
    assert 1 in np.diff(edges[0]) and max(np.diff(edges[1])) == 70
    assert sorted(np.diff(edges[1]))[-2] < 20
    made = []
    for edge in edges:
        edge = np.asarray(edge, dtype=np.int64)
        made.append((
            torch.from_numpy(
                rng.standard_normal((80, int(edge[-1]))).astype(np.float32)),
            torch.from_numpy(np.stack([edge[:-1], edge[1:]])),
            torch.from_numpy(
                rng.uniform(0., 1., edge.size - 1).astype(np.float32))))
    return made


def collated(batch):
    """`emphases.data.collate`'s first five of `batch`, zero padded."""
    frames = torch.tensor([f.shape[1] for f, _, _ in batch])
    words = torch.tensor([b.shape[1] for _, b, _ in batch])
    features = torch.zeros(len(batch), 80, int(frames.max()))
    bounds = torch.zeros(len(batch), 2, int(words.max()), dtype=torch.long)
    targets = torch.zeros(len(batch), 1, int(words.max()))
    for i, (feature, bound, target) in enumerate(batch):
        features[i, :, :frames[i]] = feature
        bounds[i, :, :words[i]] = bound
        targets[i, 0, :words[i]] = target
    return features, frames, bounds, words, targets


def back_to_back(batch, config, training):
    """(the model's arguments, its targets): [sum W], or at 'inference' in
    training the frame targets [sum T] by `emphases_amd.upsample` on the
    collated batch, clamped under 'linear'."""
    cu = lambda counts: torch.tensor(  # noqa: E731
        np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64)
    inputs = (torch.cat([f for f, _, _ in batch], dim=1).to(DEVICE),
              cu([f.shape[1] for f, _, _ in batch]),
              torch.cat([b for _, b, _ in batch], dim=1),
              cu([b.shape[1] for _, b, _ in batch]))
    targets = torch.cat([t for _, _, t in batch]).to(DEVICE)
    if training and config.downsample_location == 'inference':
        _, frames, bounds, words, padded = collated(batch)
        spread = emphases_amd.upsample(
            padded.to(DEVICE), bounds, words, frames, config)
        if config.upsample_method == 'linear':
            spread = spread.clamp(0., 1.)
        targets = torch.cat(
            [spread[i, 0, :int(n)] for i, n in enumerate(frames)])
    return inputs, targets


def model_loss_and_gradients(model, batch):
    inputs, targets = back_to_back(batch, model.config, True)
    model.train()
    model.zero_grad(set_to_none=True)
    logits = model(*inputs)
    assert logits.shape == targets.shape
    loss = train.loss_fn(logits, targets, model.config.loss)
    loss.backward()
    return loss.detach(), [p.grad for p in model.parameters()]


def assert_same_gradients(trainer, model, batch, prepared=None):
    loss, gradients = trainer.loss_and_gradients(
        *((prepared,) if prepared is not None else collated(batch)))
    want_loss, want = model_loss_and_gradients(model, batch)
    names = [name for name, _ in model.named_parameters()]
    assert list(gradients) == names
    assert same(loss, want_loss), (float(loss), float(want_loss))
    assert bool(torch.isfinite(loss))
    for name, gradient in zip(names, want):
        assert gradient is not None and bool(gradient.any()), name
        assert same(gradients[name], gradient), name
    return loss


@pytest.mark.parametrize('name', list(CONFIGS))
def test_loss_and_gradients_are_the_models(name):
    config = config_of(name)
    trainer = train.TransformerLocationsTrainer(config, gpu=0, seed=3)
    model = train.TransformerLocationsModel(config, seed=3).to(DEVICE)
    before = trainer.parameters.clone()
    loss = assert_same_gradients(trainer, model, items())
    other = assert_same_gradients(trainer, model, items()[:2])
    assert not same(loss, other)
    assert same(trainer.parameters, before)
    # eval: word-rate logits at every location, the model's
    prepared = trainer.prepare(*collated(items()))
    inputs, _ = back_to_back(items(), config, False)
    with torch.no_grad():
        want = model.eval()(*inputs)
    got = trainer.logits(prepared)
    assert got.shape == (sum(b.shape[1] for _, b, _ in items()),)
    assert same(got, want)


@pytest.mark.parametrize('name', ['input_max', 'inference_linear'])
def test_garbage_in_the_padded_feature_columns_changes_nothing(name):
    config = config_of(name)
    trainer = train.TransformerLocationsTrainer(config, gpu=0, seed=3)
    prepared = trainer.prepare(*collated(items()))
    loss, gradients = trainer.loss_and_gradients(prepared)
    inside = torch.zeros(prepared.features.shape[1], dtype=torch.bool,
                         device=DEVICE)
    inside[prepared.meta['frame_columns']] = True
    assert int((~inside).sum()) > 0
    prepared.features[:, ~inside] = float('nan')
    again, others = trainer.loss_and_gradients(prepared)
    assert same(loss, again)
    for key, gradient in gradients.items():
        assert same(gradient, others[key]), key


@pytest.mark.parametrize('name', ['input_average', 'inference_linear'])
def test_three_steps_are_the_models_trajectory(name):
    config = config_of(name)
    trainer = train.TransformerLocationsTrainer(config, gpu=0)
    model = train.TransformerLocationsModel(config).to(DEVICE)
    moments = [(torch.zeros_like(p), torch.zeros_like(p))
               for p in model.parameters()]
    library = runtime.library()
    batch = trainer.prepare(*collated(items()))
    flat = lambda tensors: torch.cat(  # noqa: E731
        [t.detach().reshape(-1) for t in tensors])
    losses = []
    for step in (1, 2, 3):
        loss = trainer.step(batch)
        want_loss, _ = model_loss_and_gradients(model, items())
        for parameter, (exp_avg, exp_avg_sq) in zip(
                model.parameters(), moments):
            clone = parameter.detach().clone()
            gradient = parameter.grad.contiguous()
            runtime.check(library.emph_adam_step(
                clone.data_ptr(), gradient.data_ptr(), exp_avg.data_ptr(),
                exp_avg_sq.data_ptr(), clone.numel(), 0.9, 0.999,
                1e-3 / (1. - 0.9 ** step), math.sqrt(1. - 0.999 ** step),
                1e-8, runtime.stream()), 'emph_adam_step')
            with torch.no_grad():
                parameter.copy_(clone)
        assert same(loss, want_loss), (step, float(loss), float(want_loss))
        assert same(trainer.parameters, flat(model.parameters())), step
        assert same(trainer.exp_avg, flat(m for m, _ in moments)), step
        losses.append(float(loss))
    print(name, 'losses', losses)
    assert losses[2] < losses[0]


@pytest.fixture(scope='module')
def cache(tmp_path_factory):
    return loop_data.build_cache(str(tmp_path_factory.mktemp('locations')))


def run(cache, directory, config, **kwargs):
    partition_dir, cache_dir = cache
    return train.train(
        loop_data.DATASET, directory, 0, partition_dir=partition_dir,
        cache_dir=cache_dir, config=config, max_training_frames=600,
        log_interval=2, save_after=0,
        trainer=train.TransformerLocationsTrainer, **kwargs)


def load(path):
    return torch.load(path, map_location='cpu', weights_only=False)


@pytest.mark.parametrize('name', ['input_average', 'inference_linear'])
def test_loop_resumes_bitwise_and_the_engine_scores_the_file(
        cache, tmp_path, name):
    config = config_of(name)
    whole = run(cache, tmp_path / 'whole', config, num_steps=6)
    saved = load(whole)
    assert saved['step'] == 6 and saved['epoch'] == 2
    run(cache, tmp_path / 'parts', config, num_steps=3)
    resumed = load(run(cache, tmp_path / 'parts', config, num_steps=6))
    assert resumed['step'] == 6
    for key, value in saved['model'].items():
        assert same(resumed['model'][key], value), key
    for index, entry in saved['optimizer']['state'].items():
        for moment in ('exp_avg', 'exp_avg_sq'):
            assert same(resumed['optimizer']['state'][index][moment],
                        entry[moment]), (index, moment)
    trainer = train.TransformerLocationsTrainer(
        config, checkpoint=whole, gpu=0)
    assert trainer.steps == 6
    engine = engine_module.Engine(config, whole, 0)
    partition_dir, cache_dir = cache
    dataset = data.Dataset(
        loop_data.DATASET, 'valid', partition_dir=partition_dir,
        cache_dir=cache_dir, config=config, gpu=0)
    loader = data.Loader(dataset, data.Sampler(dataset), trainer)
    words = 0
    for batch in loader:
        want = torch.sigmoid(trainer.logits(batch))
        with engine.lock:
            scores, _ = engine.forward(
                None, batch.plan, features=batch.features)
            got = scores[batch.meta['word_columns']].clone()
        apart = float((got - want).abs().max())
        print(f'{name}: engine against trainer scores: {apart:.3g} over '
              f'{want.numel()} words')
        assert got.shape == want.shape and apart <= PARITY
        words += want.numel()
    assert words == sum(loop_data.WORDS[i] for i in loop_data.VALID)


@pytest.mark.parametrize('location', ['intermediate', 'loss'])
def test_the_parents_locations_are_the_parent_bit_for_bit(location):
    config = emphases_amd.Config(
        architecture='transformer', layers=2, downsample_location=location)
    batch = items()
    new = train.TransformerLocationsModel(config, seed=5).to(DEVICE)
    old = train.TransformerModel(config, seed=5).to(DEVICE)
    for (key, a), (_, b) in zip(new.named_parameters(),
                                old.named_parameters()):
        assert same(a, b), key
    loss, gradients = model_loss_and_gradients(new, batch)
    want_loss, want = model_loss_and_gradients(old, batch)
    assert same(loss, want_loss)
    for a, b in zip(gradients, want):
        assert same(a, b)


###############################################################################
# Against the reference's float64 run (generate_transformer_locations.py)
###############################################################################

GOLDEN = os.path.join(HERE, 'golden')


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLDEN, 'transformer_locations.npz')) as file:
        return {name: file[name] for name in file.files}


@functools.lru_cache(maxsize=None)
def golden_items():
    arrays = golden()
    made, frame, word = [], 0, 0
    for frames, words in zip(arrays['frames'], arrays['words']):
        made.append((
            torch.from_numpy(arrays['features'][:, frame:frame + frames].copy()),
            torch.from_numpy(arrays['bounds'][:, word:word + words].copy()),
            torch.from_numpy(arrays['targets'][word:word + words].copy())))
        frame, word = frame + int(frames), word + int(words)
    return made


@pytest.mark.parametrize('name', list(CONFIGS))
def test_the_model_matches_the_reference(name):
    """Loss, logits and every gradient within 4 x `ref32_error` (the
    reference's own float32 error against its float64 run), each over max
    |want|; the ratios are printed."""
    arrays = golden()
    assert name in arrays['configs']
    reference_error = float(arrays[f'{name}/ref32_error'])
    config = config_of(name)
    model = train.TransformerLocationsModel(
        config, seed=int(arrays[f'{name}/seed'])).to(DEVICE)
    inputs, targets = back_to_back(golden_items(), config, True)
    model.train()
    logits = model(*inputs)
    loss = train.loss_fn(logits, targets, 'bce')
    loss.backward()
    want_loss = float(arrays[f'{name}/loss'])
    loss_error = abs(float(loss.detach()) - want_loss) / abs(want_loss)
    want_logits = arrays[f'{name}/logits']
    assert tuple(logits.shape) == want_logits.shape
    logit_error = np.abs(logits.detach().cpu().numpy().astype(np.float64) -
                         want_logits).max() / np.abs(want_logits).max()
    print(f'{name}: loss {float(loss.detach()):.9g} (reference '
          f'{want_loss:.9g}) error {loss_error / reference_error:.2f}, '
          f'logits {logit_error / reference_error:.2f} (x ref32_error '
          f'{reference_error:.3g})')
    missed = {}
    with np.load(os.path.join(
            GOLDEN, f'transformer_locations_grads_{name}.npz')) as wanted:
        assert set(wanted.files) == {
            key for key, _ in model.named_parameters()}
        for key, parameter in model.named_parameters():
            want = wanted[key].astype(np.float64)
            got = parameter.grad.cpu().numpy().astype(np.float64)
            assert got.shape == want.shape
            error = np.abs(got - want).max() / np.abs(want).max()
            print(f'{name} {key}: error {error / reference_error:.2f} '
                  '(x ref32_error)')
            if not error <= 4. * reference_error:
                missed[key] = error
    assert loss_error <= 4. * reference_error
    assert logit_error <= 4. * reference_error
    assert not missed, (missed, reference_error)


@pytest.mark.parametrize('name', ['input_average', 'input_max',
                                  'input_center'])
def test_eval_logits_at_input_are_the_engines(name):
    """The engine's 'input' path on the same state and batch, at the
    project's 1e-4."""
    config = config_of(name)
    trainer = train.TransformerLocationsTrainer(config, gpu=0, seed=4)
    batch = trainer.prepare(*collated(golden_items()))
    want = trainer.logits(batch)
    engine = engine_module.Engine(config, trainer.state_dict(), 0)
    with engine.lock:
        _, logits = engine.forward(None, batch.plan, features=batch.features)
        got = logits[batch.meta['word_columns']].clone()
    apart = float((got - want).abs().max())
    print(f'{name}: engine against trainer logits: {apart:.3g}')
    assert got.shape == want.shape and apart <= PARITY
