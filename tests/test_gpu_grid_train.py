"""`GridTrainer` on the MI355X: the reference's hyperparameter grid at
downsample_location 'intermediate' against goldens of the unmodified
reference (tests/golden/grid_*.npz of generate_grid.py, gridstep_*.npz of
generate_grid_step.py, train.npz for the default configuration), bit-for-bit
repeatability, the eval forward, checkpoints, and the loop end to end.

A bound is 4 x the golden's own `ref32_error`: the reference's float32 run
against its float64 run, worst tensor, over max |want|.  Each figure is
printed before it is asserted."""
import dataclasses
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
import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import data, train, weights  # noqa: E402
from emphases_amd import engine as engine_module  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDENS = {
    'grid_max': dict(downsample_method='max'),
    'grid_gelu': dict(activation='gelu'),
    'grid_silu': dict(activation='silu'),
    'grid_leaky_relu': dict(activation='leaky_relu'),
    'grid_c64_k5_k1': dict(
        channels=64, encoder_kernel_size=5, decoder_kernel_size=1),
    'grid_c128_k7': dict(channels=128, encoder_kernel_size=7),
    'gridstep_center': dict(downsample_method='center'),
    'gridstep_gelu_p10': dict(activation='gelu', dropout=0.1),
}
GELU_P10 = emphases_amd.Config(layers=2, activation='gelu', dropout=0.1)
MAX = emphases_amd.Config(layers=2, downsample_method='max')
NAN = float('nan')


def bits(tensor):
    return tensor.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ragged():
    return train_data.collated('ragged')


def compare(label, loss, gradients, want_loss, wanted, bound):
    """Print every figure, return the tensors outside the bound."""
    loss_error = abs(float(loss) - want_loss) / abs(want_loss)
    print(f'{label}: loss {float(loss):.9g} (reference {want_loss:.9g}), '
          f'error {loss_error:.3g}, bound {bound:.3g}')
    missed = {} if loss_error <= bound else {'loss': loss_error}
    for name, want in wanted.items():
        got = gradients[name].cpu().numpy().astype(np.float64)
        assert got.shape == want.shape, name
        error = np.abs(got - want).max() / np.abs(want).max()
        print(f'{label}: {name} error {error:.3g} '
              f'({error / bound:.2f} of the bound)')
        if not error <= bound:
            missed[name] = error
    return missed


###############################################################################
# Goldens
###############################################################################


@pytest.mark.parametrize('name', list(GOLDENS))
def test_grid_trainer_matches_the_reference(name):
    with np.load(os.path.join(train_data.GOLDEN, f'{name}.npz')) as file:
        golden = {key: file[key] for key in file.files}
    config = emphases_amd.Config(layers=2, **GOLDENS[name])
    seed = int(golden['seed'])
    for key, value in train.initial_state(config, seed).items():
        wide = value.astype(np.float64)
        assert np.array_equal(
            golden[f'init/{key}'], [wide.sum(), (wide ** 2).sum()]), key
    trainer = train.GridTrainer(config, gpu=0, seed=seed)
    assert type(train.select_trainer(config, gpu=0, seed=seed)) is \
        train.GridTrainer
    if 'step' in golden:
        trainer.steps = int(golden['step'])
        assert float(golden['p']) == config.dropout
    loss, gradients = trainer.loss_and_gradients(*ragged())
    wanted = {key[len('grad/'):]: value.astype(np.float64)
              for key, value in golden.items() if key.startswith('grad/')}
    assert wanted and set(wanted) <= set(gradients)
    if name != 'grid_c128_k7':
        assert set(wanted) == set(gradients)
    bound = 4. * float(golden['ref32_error'])
    missed = compare(name, loss, gradients, float(golden['loss']), wanted,
                     bound)
    assert not missed, (missed, bound)


def test_default_configuration_matches_the_ragged_golden():
    golden = train_data.golden()
    trainer = train.GridTrainer(
        emphases_amd.DEFAULT, checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0)
    loss, gradients = trainer.loss_and_gradients(*ragged())
    wanted = train_data.gradients('ragged')
    assert set(wanted) == set(gradients)
    bound = 4. * float(golden['ragged/ref32_error'])
    missed = compare('default', loss, gradients, float(golden['ragged/loss']),
                     wanted, bound)
    assert not missed, (missed, bound)


###############################################################################
# Repeatability
###############################################################################


@pytest.mark.parametrize('config', [GELU_P10, MAX], ids=['gelu_p10', 'max'])
def test_a_step_is_repeatable_whatever_the_buffers_hold(config):
    trainer = train.GridTrainer(config, gpu=0, seed=3)
    batch = trainer.prepare(*ragged())
    loss, gradients = trainer.loss_and_gradients(batch)
    assert torch.isfinite(loss) and all(
        torch.isfinite(value).all() and value.any()
        for value in gradients.values())
    again_loss, again = trainer.loss_and_gradients(batch)
    assert same(loss, again_loss)
    for name in gradients:
        assert same(gradients[name], again[name]), name
    # finite garbage in every buffer of the step - the pre-activations, the
    # kept outputs and their padding columns, the gradients, the workspace
    buffers = trainer._buffers(batch.plan)
    assert ('pre_frames' in buffers) == ('pre_words' in buffers) == \
        (config.activation == 'gelu')
    generator = torch.Generator(device='cuda:0').manual_seed(5)
    for value in buffers.values():
        if torch.is_tensor(value):
            value.normal_(generator=generator).mul_(1e3)
    trainer.gradients.fill_(NAN)
    trainer.loss.fill_(NAN)
    third_loss, third = trainer.loss_and_gradients(batch)
    assert same(loss, third_loss)
    for name in gradients:
        assert same(gradients[name], third[name]), name
    assert trainer._buffers(batch.plan) is buffers
    if config.dropout:
        trainer.steps = 1
        other_loss, other = trainer.loss_and_gradients(batch)
        assert not same(loss, other_loss)
        assert not same(gradients['input_layer.weight'],
                        other['input_layer.weight'])
        trainer.steps = 0
        back_loss, _ = trainer.loss_and_gradients(batch)
        assert same(loss, back_loss)


###############################################################################
# Eval forward
###############################################################################


@pytest.mark.parametrize('activation', ['gelu', 'silu'])
def test_eval_logits_are_the_training_forward_without_dropout(activation):
    """`logits` runs the activation in the convolution's epilogue, the
    training forward as a pass of its own over the kept pre-activation."""
    config = emphases_amd.Config(
        layers=2, activation=activation, channels=64, encoder_kernel_size=5)
    trainer = train.GridTrainer(config, gpu=0, seed=1)
    assert trainer.dropout == 0.
    batch = trainer.prepare(*ragged())
    logits = trainer.logits(batch)
    columns = torch.from_numpy(batch.plan.word_columns()).cuda()
    training = trainer._forward(batch, training=True)['logits'][columns]
    assert logits.shape == (batch.plan.total_words,)
    assert torch.isfinite(logits).all() and float(logits.std()) > 0
    assert same(logits, training)
    # and under dropout `logits` is the eval model: no mask
    dropped = train.GridTrainer(
        dataclasses.replace(config, dropout=0.5), gpu=0, seed=1)
    assert same(dropped.logits(dropped.prepare(*ragged())), logits)


###############################################################################
# Checkpoint
###############################################################################


def restated_logits(state, config, dtype):
    """The eval model in plain torch on the CPU, one utterance at a time:
    compact logits of the `ragged` batch."""
    conv = torch.nn.functional.conv1d
    activation = {'relu': torch.relu, 'gelu': torch.nn.functional.gelu,
                  'silu': torch.nn.functional.silu,
                  'leaky_relu': torch.nn.functional.leaky_relu}[
                      config.activation]
    p = {name: value.to(dtype) for name, value in state.items()}
    features, frame_lengths, word_bounds, word_lengths, _ = ragged()
    found = []
    for i, (frames, words) in enumerate(zip(frame_lengths, word_lengths)):
        x = conv(features[i:i + 1, :, :int(frames)].to(dtype),
                 p['input_layer.weight'], p['input_layer.bias'],
                 padding='same')
        for layer in range(config.layers):
            name = f'frame_encoder.{2 * layer}'
            x = activation(conv(x, p[f'{name}.weight'], p[f'{name}.bias'],
                                padding='same'))
        pieces = [x[:, :, int(start):int(end)]
                  for start, end in word_bounds[i, :, :int(words)].T]
        reduce = {'sum': lambda piece: piece.sum(dim=2),
                  'average': lambda piece: piece.mean(dim=2),
                  'max': lambda piece: piece.max(dim=2).values,
                  'center': lambda piece: piece[:, :, piece.shape[2] // 2]}[
                      config.downsample_method]
        x = torch.stack([reduce(piece) for piece in pieces], dim=2)
        for layer in range(config.layers):
            name = f'word_decoder.{2 * layer}'
            x = activation(conv(x, p[f'{name}.weight'], p[f'{name}.bias'],
                                padding='same'))
        found.append(conv(x, p['output_layer.weight'], p['output_layer.bias'],
                          padding='same')[0, 0])
    return torch.cat(found).double().numpy()


def test_checkpoint_loads_into_the_engine_and_resumes(tmp_path):
    config = emphases_amd.Config(
        layers=2, activation='gelu', dropout=0.1, channels=64,
        decoder_kernel_size=1, downsample_method='average')
    batch = ragged()
    trainer = train.GridTrainer(config, gpu=0, seed=7)
    prepared = trainer.prepare(*batch)
    for _ in range(2):
        trainer.step(prepared)
    path = tmp_path / '00000002.pt'
    trainer.save(path)
    saved = torch.load(path, map_location='cpu', weights_only=False)
    assert saved['step'] == 2
    assert 'frame_encoder.3.weight' in saved['model']
    assert list(saved['model']) == list(train.checkpoint_names(config).values())

    # ---- into the engine
    state = weights.load(str(path), config)
    internal = {name: torch.from_numpy(np.asarray(value))
                for name, value in state.items()}
    exact = restated_logits(internal, config, torch.float64)
    narrow = restated_logits(internal, config, torch.float32)
    scale = np.abs(exact).max()
    bound = 4. * float(np.abs(narrow - exact).max() / scale)
    logits = trainer.logits(prepared).cpu().double().numpy()
    features, frame_lengths, word_bounds, word_lengths, _ = batch
    model = emphases_amd.Model(checkpoint=str(path), gpu=0, config=config)
    assert isinstance(model.engine, engine_module.Engine)
    padded = model(features.cuda(), frame_lengths, word_bounds, word_lengths)
    from_engine = torch.cat([
        padded[i, 0, :int(n)] for i, n in enumerate(word_lengths)]
    ).cpu().double().numpy()
    errors = {
        'trainer against float64': np.abs(logits - exact).max() / scale,
        'engine against float64': np.abs(from_engine - exact).max() / scale,
        'trainer against engine': np.abs(logits - from_engine).max() / scale}
    for what, error in errors.items():
        print(f'checkpoint: {what} {error:.3g}, bound {bound:.3g}')
    assert errors['trainer against float64'] <= bound
    assert errors['trainer against engine'] <= bound

    # ---- resumed: parameters, both moments and the masks continue
    resumed = train.GridTrainer(config, checkpoint=str(path), gpu=0, seed=7)
    assert resumed.steps == 2
    assert same(resumed.parameters, trainer.parameters)
    loss = trainer.step(prepared)
    assert same(resumed.step(resumed.prepare(*batch)), loss)
    for name in ('parameters', 'exp_avg', 'exp_avg_sq'):
        assert same(getattr(resumed, name), getattr(trainer, name)), name
    # (another seed is another mask: the comparison above would see it)
    other = train.GridTrainer(config, checkpoint=str(path), gpu=0, seed=8)
    assert not same(other.step(other.prepare(*batch)), loss)


###############################################################################
# Loop
###############################################################################

LOOP = emphases_amd.Config(
    layers=2, activation='gelu', channels=64, decoder_kernel_size=1,
    downsample_method='max')


@pytest.fixture(scope='module')
def cache(tmp_path_factory):
    return loop_data.build_cache(str(tmp_path_factory.mktemp('grid_loop')))


def hand_driven(cache, trainer, steps, epoch=0, max_frames=600):
    """`steps` calls of `trainer.step(*host_collated)` over the sampler's
    batches, epoch by epoch from `epoch`."""
    partition_dir, cache_dir = cache
    dataset = data.Dataset(
        loop_data.DATASET, 'train', partition_dir=partition_dir,
        cache_dir=cache_dir, config=trainer.config, gpu=0, upload=False)
    sampler = data.Sampler(dataset, max_frames)
    done = 0
    while done < steps:
        sampler.set_epoch(epoch)
        for indices in sampler:
            trainer.step(*loop_data.collated(
                cache_dir, [dataset.stems[i] for i in indices],
                dataset.config))
            done += 1
            if done == steps:
                break
        epoch += 1
    return trainer


def run(cache, directory, **kwargs):
    partition_dir, cache_dir = cache
    return train.train(
        loop_data.DATASET, directory, 0, partition_dir=partition_dir,
        cache_dir=cache_dir, config=LOOP, max_training_frames=600, **kwargs)


def load(path):
    return torch.load(path, map_location='cpu', weights_only=False)


def assert_same_run(saved, want, steps):
    for name, value in want.state_dict().items():
        assert same(saved['model'][name], value), name
    for index, entry in want.optimizer_state_dict()['state'].items():
        assert float(saved['optimizer']['state'][index]['step']) == steps
        for moment in ('exp_avg', 'exp_avg_sq'):
            assert same(saved['optimizer']['state'][index][moment],
                        entry[moment]), (index, moment)


def test_loop_equals_hand_driven_grid_steps_and_resumes(cache, tmp_path):
    directory = tmp_path / 'run'
    path = run(cache, directory, num_steps=4, log_interval=4)
    assert path == str(directory / '00000004.pt')
    saved = load(path)
    assert saved['step'] == 4
    want = hand_driven(cache, train.GridTrainer(LOOP, gpu=0), 4)
    assert want.steps == 4
    assert list(saved['model']) == list(want.state_dict())
    assert_same_run(saved, want, 4)
    # resumed: two more steps from the file
    second = run(cache, directory, num_steps=6, log_interval=4)
    assert second == str(directory / '00000006.pt')
    resumed = load(second)
    more = hand_driven(
        cache, train.GridTrainer(LOOP, checkpoint=path, gpu=0), 2,
        epoch=saved['epoch'])
    assert more.steps == 6
    assert_same_run(resumed, more, 6)


def test_cli_trains_a_configuration_file_with_import_torch(cache, tmp_path):
    partition_dir, cache_dir = cache
    experiment = tmp_path / 'gelu-small.py'
    experiment.write_text(
        "import torch\n\nMODULE = 'emphases'\n\nCONFIG = 'gelu-small'\n\n"
        'ACTIVATION_FUNCTION = torch.nn.GELU\nLAYERS = 2\n')
    out = subprocess.run(
        [sys.executable, '-m', 'emphases_amd.train',
         '--config', str(experiment),
         '--dataset', loop_data.DATASET, '--gpu', '0',
         '--directory', str(tmp_path / 'cli'),
         '--partition_dir', partition_dir, '--cache_dir', cache_dir,
         '--num_steps', '2', '--max_training_frames', '600'],
        cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    path = tmp_path / 'cli' / '00000002.pt'
    assert path.is_file()
    config = emphases_amd.Config(layers=2, activation='gelu')
    trainer = train.GridTrainer(config, checkpoint=str(path), gpu=0)
    assert trainer.steps == 2
    assert torch.isfinite(trainer.parameters).all()
