"""The fused step of the reference's hyperparameter grid without a GPU: the
ABI, `check_grid_supported` and its refusals, the dispatcher, the state and the
packs of a configuration with other shapes than the default, `--config` files
with `import torch`, and the new flags."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import emphases_amd  # noqa: E402
from emphases_amd import runtime, train, weights  # noqa: E402
from emphases_amd.train import __main__ as cli  # noqa: E402
from emphases_amd.train import core as train_core  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
SYMBOLS = ('emph_output_layer_backward_any', 'emph_activation_dropout',
           'emph_activation_dropout_gradient')
# the eleven experiment files of the reference that only this step trains
# (config/hparam-search/*.py, config/downsample/{max,center}-intermediate.py)
ELEVEN = {
    'gelu': dict(activation='gelu'),
    'silu': dict(activation='silu'),
    'leaky-relu': dict(activation='leaky_relu'),
    'encoder-kernel-5': dict(encoder_kernel_size=5),
    'encoder-kernel-7': dict(encoder_kernel_size=7),
    'decoder-kernel-1': dict(decoder_kernel_size=1),
    'decoder-kernel-5': dict(decoder_kernel_size=5),
    'convolution-6-64': dict(layers=6, channels=64),
    'convolution-6-128': dict(layers=6, channels=128),
    'max-intermediate': dict(downsample_method='max'),
    'center-intermediate': dict(downsample_method='center'),
}


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    version = int(re.search(r'#define EMPH_ABI_VERSION (\d+)', header).group(1))
    assert version == runtime.ABI_VERSION == 45
    stripped = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    library = runtime.library()
    assert library.emph_abi_version() == 45
    for name in SYMBOLS:
        assert re.search(rf'\bint {name}\s*\(', stripped), name
        assert name in runtime.SIGNATURES
        function = getattr(library, name)
        assert function.argtypes == runtime.SIGNATURES[name][1]
    assert 'grid.hip' in open(os.path.join(
        ROOT, 'emphases_amd', 'csrc', 'Makefile')).read()
    assert 'asm' not in open(os.path.join(
        ROOT, 'emphases_amd', 'csrc', 'grid.hip')).read()


def test_contract_violations_are_refused_and_never_launched():
    """Checked before the launch, so host memory (never read) will do."""
    library = runtime.library()
    buffer = np.zeros(64, dtype=np.float32)
    pointer = buffer.ctypes.data
    assert pointer % 16 == 0
    EINVAL, ERANGE = -1, -2
    segment = np.zeros(16, dtype=np.int32).ctypes.data

    def head(kernel_size=3, channels=4, columns=16):
        return library.emph_output_layer_backward_any(
            pointer, pointer, 16, pointer, segment, channels, kernel_size,
            columns, pointer, pointer, pointer, 16, None)
    for kernel_size in (0, 2, 4, 6, 9, -3):
        assert head(kernel_size=kernel_size) == ERANGE
    assert head(channels=0) == EINVAL and head(channels=1025) == EINVAL
    assert head(columns=17) == EINVAL and head(columns=0) == EINVAL

    for entry in (library.emph_activation_dropout,
                  library.emph_activation_dropout_gradient):
        def call(a=pointer, b=pointer, count=64, activation=2, p=0.1):
            return entry(a, b, count, activation, p, 1, 1, 0, None)
        assert call(count=0) == 0
        for bad in (dict(count=62), dict(count=-4), dict(a=pointer + 4),
                    dict(b=pointer + 8), dict(p=1.), dict(p=-0.1),
                    dict(p=float('nan')), dict(activation=5),
                    dict(activation=-1), dict(a=None), dict(b=None)):
            assert call(**bad) == EINVAL, bad
    assert not buffer.any()


###############################################################################
# check_grid_supported
###############################################################################


@pytest.mark.parametrize('experiment', list(ELEVEN))
def test_check_grid_supported_passes_for_the_eleven(experiment):
    config = emphases_amd.Config(**ELEVEN[experiment])
    with pytest.raises(NotImplementedError):
        train.check_supported(config)
    train.check_grid_supported(config)
    for more in ({'dropout': 0.1}, {'loss': 'mse'}, {'dropout': 0.,
                 'loss': 'mse', 'layers': 2}, {'loudness_feature': True}):
        train.check_grid_supported(dataclasses.replace(config, **more))


def test_check_grid_supported_passes_for_combinations():
    train.check_grid_supported(emphases_amd.DEFAULT)
    for overrides in (
            dict(activation='silu', channels=16, encoder_kernel_size=7,
                 decoder_kernel_size=5, downsample_method='max', layers=0),
            dict(activation='leaky_relu', channels=112, layers=16,
                 encoder_kernel_size=1, downsample_method='average')):
        train.check_grid_supported(emphases_amd.Config(**overrides))


@pytest.mark.parametrize('field,value', [
    ('architecture', 'transformer'), ('method', 'pitch-variance'),
    ('downsample_location', 'input'), ('downsample_location', 'inference'),
    ('downsample_location', 'loss'), ('channels', 72), ('channels', 144),
    ('layers', 17), ('mel_feature', False)])
def test_check_grid_supported_names_the_field(field, value):
    config = dataclasses.replace(emphases_amd.DEFAULT, **{field: value})
    with pytest.raises(NotImplementedError, match=field):
        train.check_grid_supported(config)
    with pytest.raises(NotImplementedError, match=field):
        train.GridTrainer(config=config)


def test_grid_trainer_refuses_bf16x3_before_a_gpu_is_needed():
    with pytest.raises(NotImplementedError, match='precision'):
        train.GridTrainer(precision='bf16x3')
    with pytest.raises(NotImplementedError, match='precision'):
        train.GridTrainer(
            emphases_amd.Config(activation='gelu'), precision='bf16x3')
    with pytest.raises(ValueError, match='precision'):
        train.GridTrainer(precision='f64')


###############################################################################
# Dispatch
###############################################################################


def test_select_trainer_dispatches_before_a_gpu_is_needed(monkeypatch):
    built = []
    for name in ('Trainer', 'EncoderTrainer', 'PieceTrainer', 'GridTrainer'):
        monkeypatch.setattr(
            train_core, name,
            lambda config, _name=name, **arguments: built.append(
                (_name, config, arguments)) or _name)
    wanted = {'intermediate': 'Trainer', 'inference': 'EncoderTrainer',
              'loss': 'EncoderTrainer', 'input': 'PieceTrainer'}
    for location, name in wanted.items():
        config = emphases_amd.Config(downsample_location=location)
        assert train.select_trainer(config, precision='bf16x3', seed=3) == name
        assert built[-1] == (name, config, {'precision': 'bf16x3', 'seed': 3})
    # what `Trainer` covers keeps `Trainer`
    for overrides in ({'dropout': 0.1}, {'downsample_method': 'average'},
                      {'loss': 'mse', 'layers': 2}):
        assert train.select_trainer(
            emphases_amd.Config(**overrides)) == 'Trainer'
    for experiment, overrides in ELEVEN.items():
        config = emphases_amd.Config(**overrides)
        assert train.select_trainer(config, seed=5) == 'GridTrainer', \
            experiment
        assert built[-1] == ('GridTrainer', config, {'seed': 5})
        assert train.select_trainer(
            dataclasses.replace(config, dropout=0.1, loss='mse'),
            precision='f32') == 'GridTrainer'
    count = len(built)
    # the specialised step's refusal where the grid step refuses too
    with pytest.raises(NotImplementedError, match='architecture'):
        train.select_trainer(emphases_amd.Config(architecture='transformer'))
    with pytest.raises(NotImplementedError, match='activation'):
        train.select_trainer(emphases_amd.Config(
            downsample_location='input', activation='gelu'))
    with pytest.raises(NotImplementedError, match='dropout'):
        train.select_trainer(emphases_amd.Config(
            downsample_location='input', downsample_method='max',
            dropout=0.1))
    with pytest.raises(NotImplementedError, match='activation'):
        train.select_trainer(emphases_amd.Config(
            downsample_location='loss', activation='silu'))
    with pytest.raises(NotImplementedError, match='channels'):
        train.select_trainer(emphases_amd.Config(channels=72))
    with pytest.raises(NotImplementedError, match='precision'):
        train.select_trainer(
            emphases_amd.Config(activation='gelu'), precision='bf16x3')
    with pytest.raises(NotImplementedError, match='precision'):
        train.select_trainer(emphases_amd.DEFAULT, precision='bf16x6')
    with pytest.raises(ValueError, match='precision'):
        train.select_trainer(
            emphases_amd.Config(activation='gelu'), precision='f64')
    assert len(built) == count
    # the narrower dispatchers keep their refusals
    with pytest.raises(NotImplementedError, match='downsample_method'):
        train.make_trainer(emphases_amd.Config(downsample_method='max'))
    with pytest.raises(NotImplementedError, match='downsample_method'):
        train.trainer_for(emphases_amd.Config(downsample_method='max'))
    with pytest.raises(NotImplementedError, match='activation'):
        train.trainer_for(emphases_amd.Config(activation='gelu'))
    assert len(built) == count


def test_train_refuses_before_any_file_is_read():
    def run(config, **arguments):
        return train.train('none', 'none', partition_dir='none',
                           config=config, **arguments)
    with pytest.raises(NotImplementedError, match='architecture'):
        run(emphases_amd.Config(architecture='transformer'))
    with pytest.raises(NotImplementedError, match='precision'):
        run(emphases_amd.Config(activation='gelu'), precision='bf16x3')
    with pytest.raises(NotImplementedError, match='activation'):
        run(emphases_amd.Config(downsample_location='input',
                                activation='gelu'))
    with pytest.raises(NotImplementedError, match='channels'):
        run(emphases_amd.Config(channels=72))
    assert not os.path.exists('none')


###############################################################################
# State and packs of other shapes
###############################################################################


def test_state_and_packs_of_c64_k5_k1():
    config = emphases_amd.Config(
        layers=2, channels=64, encoder_kernel_size=5, decoder_kernel_size=1)
    with np.load(os.path.join(GOLDEN, 'grid_c64_k5_k1.npz')) as file:
        golden = {name: file[name] for name in file.files}
    state = train.initial_state(config, seed=int(golden['seed']))
    shapes = weights.parameter_shapes(config)
    assert list(state) == list(shapes)
    assert shapes['input_layer.weight'] == (64, 80, 5)
    assert shapes['word_decoder.2.weight'] == (64, 64, 1)
    assert shapes['output_layer.weight'] == (1, 64, 1)
    for name, value in state.items():
        assert value.shape == tuple(shapes[name]) and value.dtype == np.float32
        wide = value.astype(np.float64)
        assert np.array_equal(
            np.array([wide.sum(), (wide ** 2).sum()]), golden[f'init/{name}']), \
            name

    offsets, count = train.parameter_offsets(config)
    assert list(offsets) == list(shapes)
    tables = train.gather_tables(config)
    index = tables['index']
    assert index.dtype == np.int32 and -1 <= index.min() and index.max() < count
    flat = np.arange(1, count + 1, dtype=np.float32)
    taken = np.where(index < 0, np.float32(0), flat[np.maximum(index, 0)])
    assert set(tables['forward']) == set(train.layer_names(config))
    assert set(tables['backward']) == \
        set(train.layer_names(config)) - {'input_layer'}
    for name in train.layer_names(config):
        first, shape = offsets[f'{name}.weight']
        weight = flat[first:first + int(np.prod(shape))].reshape(shape)
        start, size = tables['forward'][name]
        want = runtime.conv_pack(weight)
        assert size == want.size
        assert np.array_equal(taken[start:start + size], want)
        if name == 'input_layer':
            continue
        start, size = tables['backward'][name]
        flipped = np.ascontiguousarray(weight.transpose(1, 0, 2)[:, :, ::-1])
        assert np.array_equal(
            taken[start:start + size], runtime.conv_pack(flipped))


def test_checkpoint_names_of_a_grid_configuration():
    config = emphases_amd.Config(layers=2, activation='gelu', dropout=0.1)
    names = train.checkpoint_names(config)
    assert names['frame_encoder.2.weight'] == 'frame_encoder.3.weight'
    assert names['word_decoder.2.bias'] == 'word_decoder.3.bias'
    assert names['output_layer.weight'] == 'output_layer.weight'


###############################################################################
# --config and the flags
###############################################################################

FLAGS = ['--directory', 'run', '--partition_dir', 'parts']


def test_config_file_with_import_torch_is_read(tmp_path):
    path = tmp_path / 'swish.py'
    path.write_text(
        'import torch\n\nMODULE = "emphases"\n\n# the experiment\n'
        "CONFIG = 'swish'\n\nACTIVATION_FUNCTION = torch.nn.SiLU\n")
    assert cli.read_config(path) == ({'activation': 'silu'}, {})
    overrides, _ = cli.settings(FLAGS + ['--config', str(path)])
    assert overrides == {'activation': 'silu'}
    train.check_grid_supported(emphases_amd.Config(**overrides))


@pytest.mark.parametrize('text', [
    'import torch as t\nACTIVATION_FUNCTION = t.nn.SiLU\n',
    'import torch, os\nLAYERS = 2\n',
    'import os\nLAYERS = 2\n',
    'import torch.nn\nLAYERS = 2\n',
    'from torch import nn\nLAYERS = 2\n',
    'import torch\ntorch.manual_seed(0)\nLAYERS = 2\n',
    "import torch\nLAYERS = 2\nopen('written', 'w')\n",
    'import torch\nBUCKETS = 1\n'])
def test_config_file_accepts_no_other_statement(tmp_path, text, monkeypatch):
    monkeypatch.chdir(tmp_path)
    path = tmp_path / 'experiment.py'
    path.write_text(text)
    with pytest.raises(ValueError):
        cli.read_config(path)
    assert not (tmp_path / 'written').exists()


def test_new_flags_reach_the_settings(tmp_path):
    overrides, _ = cli.settings(FLAGS + [
        '--activation', 'gelu', '--channels', '64', '--layers', '2',
        '--encoder_kernel_size', '5', '--decoder_kernel_size', '1',
        '--downsample_method', 'max'])
    assert overrides == {
        'activation': 'gelu', 'channels': 64, 'layers': 2,
        'encoder_kernel_size': 5, 'decoder_kernel_size': 1,
        'downsample_method': 'max'}
    train.check_grid_supported(emphases_amd.Config(**overrides))
    # explicit flags override the file
    path = tmp_path / 'gelu.py'
    path.write_text('import torch\nACTIVATION_FUNCTION = torch.nn.GELU\n'
                    'CHANNELS = 128\n')
    overrides, _ = cli.settings(FLAGS + [
        '--config', str(path), '--activation', 'leaky_relu'])
    assert overrides == {'activation': 'leaky_relu', 'channels': 128}
    assert cli.settings(FLAGS)[0] == {}
    with pytest.raises(SystemExit):
        cli.settings(FLAGS + ['--activation', 'tanh'])


def test_downsample_method_help_names_no_location(capsys):
    with pytest.raises(SystemExit):
        cli.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert "'max' or 'center'" in text
    assert 'inference or loss only' not in text
