"""The decoder-less training step without a GPU: `Config.upsample_method`,
`check_encoder_supported`, `make_trainer`'s dispatch, the CLI flags, the C ABI
of the frame-rate head, and the formula of `upsample` itself as a float64
numpy restatement against the reference's recorded output
(tests/golden/upsample.npz, written by tests/golden/generate_locations.py)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import emphases_amd  # noqa: E402
from emphases_amd import runtime, train, weights  # noqa: E402
from emphases_amd.train import __main__ as cli  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
ENTRIES = ('emph_upsample', 'emph_frame_head', 'emph_frame_loss_grad',
           'emph_frame_head_parts', 'emph_frame_head_backward')


def upsample_float64(x, starts, ends, frames, method):
    """`emphases_amd.upsample` of one utterance, restated: x [C, W] ->
    [C, frames] in float64."""
    x = np.asarray(x, dtype=np.float64)
    starts = np.asarray(starts, dtype=np.float64)
    ends = np.asarray(ends, dtype=np.float64)
    words = x.shape[1]
    centres = starts + (ends - starts) / 2.
    times = np.arange(frames) + 0.5
    if words == 1:
        return np.repeat(x[:, :1], frames, axis=1)
    index = (centres[None, :] <= times[:, None]).sum(axis=1) - 1
    if method == 'nearest':
        return x[:, np.clip(index, 0, words - 1)]
    j = np.clip(index, 0, words - 2)
    slope = (x[:, j + 1] - x[:, j]) / (centres[j + 1] - centres[j])
    return x[:, j] + slope * (times - centres[j])


def upsample_cases():
    """[(frames, starts, ends, {method: (x [C, W], y [C, T])})] and
    {method: ref32_error} of upsample.npz."""
    with np.load(os.path.join(GOLDEN, 'upsample.npz')) as file:
        data = {name: file[name] for name in file.files}
    cases, frame, word = [], 0, 0
    for frames, words in zip(data['frames'], data['words']):
        cases.append((
            int(frames), data['bounds'][0, word:word + words],
            data['bounds'][1, word:word + words],
            {method: (data[f'{method}/x'][:, word:word + words],
                      data[f'{method}/y'][:, frame:frame + frames])
             for method in ('linear', 'nearest')}))
        frame, word = frame + frames, word + words
    return cases, {method: float(data[f'{method}/ref32_error'])
                   for method in ('linear', 'nearest')}


def test_upsample_method_is_validated_and_defaults_to_linear():
    assert emphases_amd.DEFAULT.upsample_method == 'linear'
    assert emphases_amd.Config() == emphases_amd.DEFAULT
    assert emphases_amd.Config(upsample_method='nearest').upsample_method == \
        'nearest'
    with pytest.raises(ValueError, match='Interpolation method cubic is not'):
        emphases_amd.Config(upsample_method='cubic')
    assert emphases_amd.upsample is emphases_amd.core.upsample


def test_restated_formula_matches_the_reference():
    cases, _ = upsample_cases()
    assert [(frames, len(starts)) for frames, starts, _, _ in cases] == [
        (1, 1), (7, 2), (64, 5), (65, 9), (200, 40)]
    equal_centres = 0
    for frames, starts, ends, methods in cases:
        centres = starts + (ends - starts) / 2.
        equal_centres += np.isin(np.arange(frames) + 0.5, centres).sum()
        for method, (x, y) in methods.items():
            assert x.shape[0] == (1 if method == 'linear' else 3)
            got = upsample_float64(x, starts, ends, frames, method)
            assert got.shape == y.shape
            if len(starts) == 1:
                # the reference's one-word branch writes `x[0]`, CHANNEL 0,
                # to every channel (`core.py:494-495`); as under 'linear',
                # the package gives every channel its own value
                assert np.array_equal(y, np.repeat(y[:1], len(y), axis=0))
                assert np.array_equal(got[0], y[0])
                assert np.array_equal(got, np.repeat(x, frames, axis=1))
                continue
            assert np.abs(got - y).max() <= 1e-12, (frames, method)
    assert equal_centres > 0
    # 'linear' leaves [0, 1] where it extrapolates: the loss's clamp matters
    with np.load(os.path.join(GOLDEN, 'locations_sum_inference.npz')) as file:
        assert 0 < int(file['clamped_frames']) < 635


GRID = [dict(downsample_location=location, downsample_method=method,
             loss=loss, upsample_method=upsample)
        for location in ('inference', 'loss')
        for method in emphases_amd.config.DOWNSAMPLE_METHODS
        for loss in ('bce', 'mse') for upsample in ('linear', 'nearest')]


def test_supported_grid_passes():
    for overrides in GRID:
        for layers in (0, 2, 16):
            train.check_encoder_supported(
                emphases_amd.Config(layers=layers, dropout=0.1, **overrides))
    train.check_encoder_supported(emphases_amd.Config(
        downsample_location='loss', pitch_feature=True, loudness_feature=True))


@pytest.mark.parametrize('field,overrides', [
    ('method', dict(method='prominence')),
    ('architecture', dict(architecture='transformer')),
    ('downsample_location', dict(downsample_location='intermediate')),
    ('downsample_location', dict(downsample_location='input')),
    ('activation', dict(activation='gelu')),
    ('channels', dict(channels=64)),
    ('encoder_kernel_size', dict(encoder_kernel_size=5)),
    ('decoder_kernel_size', dict(decoder_kernel_size=1)),
    ('layers', dict(layers=17)),
    ('mel_feature', dict(mel_feature=False, pitch_feature=True)),
])
def test_refusals_name_the_field(field, overrides):
    config = emphases_amd.Config(
        **{'downsample_location': 'inference', **overrides})
    with pytest.raises(NotImplementedError, match=field):
        train.check_encoder_supported(config)
    with pytest.raises(NotImplementedError, match=field):
        train.EncoderTrainer(config=config)
    if overrides.get('downsample_location') != 'intermediate':
        with pytest.raises(NotImplementedError, match=field):
            train.make_trainer(config)


def test_make_trainer_dispatches_before_a_gpu_is_needed(monkeypatch):
    class NoGpu(Exception):
        pass

    def fail(device=None):
        raise NoGpu(device)
    monkeypatch.setattr(runtime, 'require_gpu', fail)
    seen = []
    for cls in (train.Trainer, train.EncoderTrainer):
        original = cls.__init__

        def recording(self, *args, _original=original, _cls=cls, **kwargs):
            seen.append(_cls)
            _original(self, *args, **kwargs)
        monkeypatch.setattr(cls, '__init__', recording)
    for location, cls in (('intermediate', train.Trainer),
                          ('inference', train.EncoderTrainer),
                          ('loss', train.EncoderTrainer)):
        with pytest.raises(NoGpu):
            train.make_trainer(emphases_amd.Config(
                layers=1, downsample_location=location))
        assert seen[-1] is cls
    # refusals come first: nothing is constructed
    count = len(seen)
    with pytest.raises(NotImplementedError, match='architecture'):
        train.make_trainer(emphases_amd.Config(architecture='transformer'))
    with pytest.raises(NotImplementedError, match='architecture'):
        train.make_trainer(emphases_amd.Config(
            architecture='transformer', downsample_location='loss'))
    with pytest.raises(NotImplementedError, match='downsample_location'):
        train.make_trainer(emphases_amd.Config(downsample_location='input'))
    with pytest.raises(NotImplementedError, match='downsample_method'):
        train.make_trainer(emphases_amd.Config(downsample_method='max'))
    assert len(seen) == count


def test_decoderless_state_has_the_reference_layout():
    config = emphases_amd.Config(layers=2, downsample_location='inference')
    assert train.layer_names(config) == [
        'input_layer', 'frame_encoder.0', 'frame_encoder.2']
    state = train.initial_state(config, seed=4)
    assert list(state) == list(weights.parameter_shapes(config))
    assert not any(name.startswith('word_decoder') for name in state)
    # the encoder's tensors are those of the model with a decoder: the
    # reference builds input layer and frame encoder first (model/core.py:16-30)
    full = train.initial_state(emphases_amd.Config(layers=2), seed=4)
    for name in ('input_layer.weight', 'frame_encoder.2.bias'):
        assert np.array_equal(state[name], full[name])
    assert not np.array_equal(
        state['output_layer.weight'], full['output_layer.weight'])
    tables = train.gather_tables(config)
    assert set(tables['forward']) == set(train.layer_names(config))
    names = train.checkpoint_names(emphases_amd.Config(
        layers=2, downsample_location='loss', dropout=0.1))
    assert names['frame_encoder.2.weight'] == 'frame_encoder.3.weight'


def test_cli_flags_reach_train(monkeypatch):
    arguments = cli.parse_args([
        '--directory', 'run', '--partition_dir', 'parts',
        '--downsample_location', 'inference', '--upsample_method', 'nearest',
        '--downsample_method', 'max'])
    assert arguments.downsample_location == 'inference'
    assert arguments.upsample_method == 'nearest'
    assert arguments.downsample_method == 'max'
    defaults = cli.parse_args(['--directory', 'run', '--partition_dir', 'p'])
    assert defaults.downsample_location is None
    assert defaults.upsample_method is None and defaults.precision == 'f32'
    with pytest.raises(SystemExit):
        cli.parse_args(['--directory', 'run', '--partition_dir', 'p',
                        '--downsample_location', 'input'])
    calls = []
    monkeypatch.setattr(
        emphases_amd.train, 'train',
        lambda *args, **kwargs: calls.append(
            (args, kwargs, emphases_amd.active_config())))
    before = emphases_amd.active_config()
    try:
        cli.main(['--directory', 'run', '--partition_dir', 'parts',
                  '--downsample_location', 'loss', '--downsample_method',
                  'center', '--upsample_method', 'nearest'])
    finally:
        emphases_amd.configure(before)
    (args, kwargs, config), = calls
    assert args[0] == 'libritts' and str(args[1]) == 'run'
    assert config.downsample_location == 'loss'
    assert config.downsample_method == 'center'
    assert config.upsample_method == 'nearest'
    train.check_encoder_supported(config)


def test_frame_head_abi_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    version = int(re.search(r'#define EMPH_ABI_VERSION (\d+)', header).group(1))
    assert version == runtime.ABI_VERSION >= 40
    for name in ENTRIES:
        assert re.search(rf'\b{name}\(', header), name
        assert name in runtime.SIGNATURES
    assert runtime.UPSAMPLE_METHODS == {'linear': 0, 'nearest': 1}
    library = runtime.library()
    assert library.emph_abi_version() == runtime.ABI_VERSION
    one = 16          # (never dereferenced: the arguments are refused first)
    # null pointers
    assert library.emph_upsample(
        None, 16, one, one, 16, 1, one, one, 1, 0, None) == -1
    assert b'emph_upsample: null' in library.emph_last_error()
    assert library.emph_frame_head(
        one, 16, None, one, 80, 3, one, 1, one, None) == -1
    assert b'emph_frame_head: null' in library.emph_last_error()
    assert library.emph_frame_loss_grad(
        one, one, one, 16, one, one, 1, 5, 0, 0, None, one, one, None) == -1
    assert b'emph_frame_loss_grad: null' in library.emph_last_error()
    assert library.emph_frame_head_backward(
        one, one, 16, one, 80, 3, one, 1, one, one, one, None, 16, None) == -1
    assert b'emph_frame_head_backward: null' in library.emph_last_error()
    # bad shapes and switches
    assert library.emph_upsample(
        one, 16, one, one, 16, 1, one, one, 1, 2, None) == -1
    assert b'method 2' in library.emph_last_error()
    assert library.emph_upsample(
        one, 16, one, one, 16, 0, one, one, 1, 0, None) == -1
    assert library.emph_frame_head(
        one, 16, one, one, 80, 5, one, 1, one, None) == -2
    assert b'kernel_size 5' in library.emph_last_error()
    assert library.emph_frame_head(
        one, 16, one, one, 0, 3, one, 1, one, None) == -2
    assert library.emph_frame_loss_grad(
        one, one, one, 16, one, one, 1, 5, 2, 0, one, one, one, None) == -1
    assert b'form 2' in library.emph_last_error()
    assert library.emph_frame_loss_grad(
        one, one, one, 16, one, one, 1, 65, 0, 0, one, one, one, None) == -1
    assert b'bad shape' in library.emph_last_error()
    assert library.emph_frame_loss_grad(
        one, one, one, 16, one, one, 0, 5, 0, 0, one, one, one, None) == -1
    assert library.emph_frame_head_backward(
        one, one, 16, one, 81, 3, one, 1, one, one, one, one, 16, None) == -2
    assert b'channels 81' in library.emph_last_error()
    assert library.emph_frame_head_backward(
        one, one, 16, one, 80, 3, one, 0, one, one, one, one, 16, None) == -1
    # nothing to do launches nothing
    assert library.emph_upsample(
        None, 16, None, None, 16, 1, None, None, 0, 0, None) == 0
    assert library.emph_frame_head(
        None, 16, None, None, 80, 3, None, 0, None, None) == 0
    # the parts depend on the tile count alone, and cover every tile once
    assert library.emph_frame_head_parts(0) == 0
    for tiles in (1, 2, 1023, 1024, 1025, 1200, 2048, 2049, 5000, 20000):
        parts = library.emph_frame_head_parts(tiles)
        per = -(-tiles // parts)
        assert 1 <= parts <= 1024 and (parts - 1) * per < tiles <= parts * per
    assert library.emph_frame_head_parts(1200) == 600
    assert library.emph_frame_head_parts(5000) == 1000


def test_ragged_has_the_shapes_the_gpu_tests_rely_on():
    """The GPU tests run on `ragged`: a one-word utterance, a two-word one, 64
    frames (one tile) and 129 (two tiles and a frame)."""
    import train_data
    data = train_data.golden()
    assert list(data['ragged/frames']) == [5, 37, 64, 100, 129, 300]
    assert list(data['ragged/words']) == [1, 3, 7, 12, 2, 40]
    assert torch.from_numpy(data['ragged/targets']).dtype == torch.float32
