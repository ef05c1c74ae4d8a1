"""`Config.dropout` and the dropout masks of the training step, host side (no
device): the Philox known answers, the mask specification
(`emphases_amd/train/dropout.py`) against the stored bits, the configuration,
the checkpoint names, the CLI flag and the C ABI of the two entry points."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import dropout_data  # noqa: E402
import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import core as api  # noqa: E402
from emphases_amd import runtime, train, weights  # noqa: E402
from emphases_amd.train import __main__ as cli  # noqa: E402
from emphases_amd.train import dropout  # noqa: E402

SYMBOLS = ('emph_dropout', 'emph_activation_dropout_backward')
EINVAL = -1                      # include/emphases_hip.h


@pytest.mark.parametrize('counter,key,want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(counter, key, want):
    """The Random123 known answers of Philox-4x32-10."""
    words = dropout.philox4x32_10(counter, key)
    assert all(word.dtype == np.uint32 for word in words)
    assert ' '.join(f'{int(word):08x}' for word in words) == want


def test_philox_is_vectorised():
    counters = np.array([[0, 0xffffffff, 0x243f6a88], [0, 0xffffffff, 0x85a308d3],
                         [0, 0xffffffff, 0x13198a2e], [0, 0xffffffff, 0x03707344]],
                        dtype=np.uint32)
    keys = np.array([[0, 0xffffffff, 0xa4093822], [0, 0xffffffff, 0x299f31d0]],
                    dtype=np.uint32)
    words = np.stack(dropout.philox4x32_10(counters, keys))
    assert words.shape == (4, 3)
    assert [f'{word:08x}' for word in words[:, 2]] == \
        'd16cfe09 94fdcceb 5001e420 24126ea1'.split()
    assert f'{words[0, 0]:08x}' == '6627e8d5'


def test_config_validation():
    for value in (None, 0.0, 0.05):
        assert emphases_amd.Config(dropout=value).dropout == value
    for value in (-0.1, 1.0, 'a'):
        with pytest.raises(ValueError, match='dropout'):
            emphases_amd.Config(dropout=value)


def test_defaults_are_unchanged():
    assert emphases_amd.DEFAULT.dropout is None
    assert emphases_amd.Config() == emphases_amd.DEFAULT
    assert emphases_amd.DEFAULT == emphases_amd.Config(
        mel_feature=True, pitch_feature=False, periodicity_feature=False,
        loudness_feature=False, normalize=False, architecture='convolution',
        activation='relu', channels=80, layers=6, encoder_kernel_size=3,
        decoder_kernel_size=3, downsample_location='intermediate',
        downsample_method='sum', loss='bce', heads=2, layer_norm_eps=1e-5,
        method='neural', dropout=None)
    # the field changes neither the layout nor what the step supports
    for value in (None, 0.0, 0.1):
        config = emphases_amd.Config(dropout=value)
        train.check_supported(config)
        assert weights.parameter_shapes(config) == weights.parameter_shapes()
        assert train.layer_names(config) == train.layer_names(
            emphases_amd.DEFAULT)


def test_threshold_and_scale():
    """min(round(p 2^32), 2^32 - 1) and float32(1 / (1 - p)) of the float32
    probability (the C ABI carries a float): 0.05f 2^32 = 13421773 x 16 and
    0.1f 2^32 = 13421773 x 32 exactly."""
    assert dropout.threshold(0.05) == 214748368 == 13421773 * 16
    assert dropout.threshold(0.1) == 429496736 == 13421773 * 32
    assert dropout.threshold(0.5) == 1 << 31
    assert dropout.threshold(0.) == 0
    assert dropout.threshold(np.nextafter(np.float32(1), np.float32(0))) == \
        (1 << 32) - 256
    for p, want in ((0.05, 1. / 0.95), (0.1, 1. / 0.9), (0.5, 2.), (0., 1.)):
        scale = dropout.scale(p)
        assert scale.dtype == np.float32
        assert scale == np.float32(1. / (1. - float(np.float32(p))))
        assert abs(float(scale) - want) <= 2. ** -24 * want * 1.01
    assert dropout.scale(0.5) == 2 and dropout.scale(0.) == 1


def test_streams_follow_layer_names():
    config = emphases_amd.Config(layers=3, dropout=0.1)
    names = train.layer_names(config)
    assert names[0] == 'input_layer'
    for position, name in enumerate(names[1:], 1):
        assert dropout.stream_of(config, name) == position


def test_stored_mask_bits_are_reproduced():
    """The stream-1 mask of `p10` for the first utterance of `ragged`, cut
    from the packed layout: pins quad addressing, word order and threshold."""
    p, seed, step = dropout_data.settings('p10')
    batch = train_data.collated('ragged')
    frames, words, bounds = train.check_batch(*batch)
    plan = api._packed_plan(frames, torch.from_numpy(bounds), words)
    whole = dropout.keep_mask(seed, 1, step, 80 * plan.ld_frames, p)
    assert whole.dtype == bool and whole.shape == (80 * plan.ld_frames,)
    first = whole.reshape(80, plan.ld_frames)[
        :, plan.frame_off[0]:plan.frame_off[0] + frames[0]]
    want = dropout_data.golden()['p10/mask_bits']
    assert np.array_equal(np.packbits(first.ravel()), want)
    assert 0 < np.unpackbits(want).sum() < 80 * frames[0]


def test_mask_addressing():
    """A window of the mask is the mask of the window; stream, step and seed
    each change it; p = 0 keeps everything."""
    whole = dropout.keep_mask(7, 2, 5, 4096, 0.5)
    assert np.array_equal(
        dropout.keep_mask(7, 2, 5, 100, 0.5, origin=1000), whole[1000:1100])
    high = dropout.keep_mask(7, 2, 5, 64, 0.5, origin=(1 << 34) - 8)
    assert np.array_equal(
        dropout.keep_mask(7, 2, 5, 32, 0.5, origin=1 << 34), high[8:40])
    assert not np.array_equal(high, whole[:64])
    for other in (dropout.keep_mask(8, 2, 5, 4096, 0.5),
                  dropout.keep_mask(7, 3, 5, 4096, 0.5),
                  dropout.keep_mask(7, 2, 6, 4096, 0.5),
                  dropout.keep_mask(7 + (1 << 32), 2, 5, 4096, 0.5)):
        assert 0.4 < np.mean(other != whole) < 0.6
    assert dropout.keep_mask(7, 2, 5, 4096, 0.).all()
    # nested in p: what p = 0.1 drops, p = 0.5 drops too
    assert not (dropout.keep_mask(7, 2, 5, 4096, 0.5) &
                ~dropout.keep_mask(7, 2, 5, 4096, 0.1)).any()


@pytest.mark.parametrize('p', [0.05, 0.1, 0.5])
def test_kept_share(p):
    """A condition on the specification: the kept share of 80 x 1024 elements
    is within 5 standard deviations of 1 - p (0.21, 0.00 and 1.04 here)."""
    count = 80 * 1024
    kept = dropout.keep_mask(20261018, 3, 7, count, p).mean()
    deviation = abs(kept - (1. - p)) / np.sqrt(p * (1. - p) / count)
    print(f'p {p}: kept {kept:.6f}, {deviation:.2f} standard deviations')
    assert deviation <= 5.


@pytest.mark.parametrize('value,stride', [(0.1, 3), (0.0, 3), (None, 2)])
def test_checkpoint_names(tmp_path, value, stride):
    """Layer i of a stack is module 3 i under `dropout is not None`, as the
    reference builds `Sequential(conv, activation, Dropout)`; `weights.load`
    reads the file back under the internal names."""
    config = emphases_amd.Config(layers=3, dropout=value)
    names = train.checkpoint_names(config)
    assert list(names) == list(weights.parameter_shapes(config))
    assert [saved for saved in names.values() if 'encoder' in saved] == [
        f'frame_encoder.{stride * i}.{kind}' for i in range(3)
        for kind in ('weight', 'bias')]
    assert [saved for saved in names.values() if 'decoder' in saved] == [
        f'word_decoder.{stride * i}.{kind}' for i in range(3)
        for kind in ('weight', 'bias')]
    assert names['input_layer.weight'] == 'input_layer.weight'
    assert names['output_layer.bias'] == 'output_layer.bias'
    state = train.initial_state(config, seed=3)
    saved = {names[name]: torch.from_numpy(array)
             for name, array in state.items()}
    # the reference's stack under this configuration loads it strictly
    layers = []
    for _ in range(3):
        layers += [torch.nn.Conv1d(80, 80, 3, padding='same'), torch.nn.ReLU()]
        if value is not None:
            layers.append(torch.nn.Dropout(value))
    for prefix in ('frame_encoder.', 'word_decoder.'):
        torch.nn.Sequential(*layers).load_state_dict(
            {name[len(prefix):]: tensor for name, tensor in saved.items()
             if name.startswith(prefix)}, strict=True)
    path = tmp_path / '00000000.pt'
    train.write_checkpoint(path, saved, train.adam_state_dict(
        config, 0, None, None))
    for source in (str(path), saved):
        loaded = weights.load(source, config)
        assert list(loaded) == list(state)
        for name, array in state.items():
            assert np.array_equal(loaded[name], array), name
    # and under any other setting of the field: inference ignores it
    other = weights.load(str(path), emphases_amd.Config(layers=3))
    assert all(np.array_equal(other[name], state[name]) for name in state)


def test_cli_flag_reaches_train(monkeypatch, tmp_path):
    arguments = ['--directory', str(tmp_path), '--partition_dir', 'p']
    assert cli.parse_args(arguments).dropout is None
    assert cli.parse_args(arguments + ['--dropout', '0.05']).dropout == 0.05
    seen = {}
    monkeypatch.setattr(api, '_ACTIVE', [emphases_amd.DEFAULT])

    def fake(dataset, directory, config=None, **kwargs):
        seen.update(kwargs, config=config or api.active_config())
    monkeypatch.setattr(emphases_amd.train, 'train', fake)
    cli.main(arguments + ['--dropout', '0.05', '--loss', 'mse'])
    assert seen['config'].dropout == 0.05 and seen['config'].loss == 'mse'
    assert 'dropout' not in seen and seen['precision'] == 'f32'
    cli.main(arguments + ['--dropout', '0'])
    assert seen['config'].dropout == 0.0
    monkeypatch.setattr(api, '_ACTIVE', [emphases_amd.DEFAULT])
    cli.main(arguments)
    assert seen['config'].dropout is None
    with pytest.raises(ValueError, match='dropout'):
        cli.main(arguments + ['--dropout', '1'])


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    version = int(re.search(r'#define EMPH_ABI_VERSION (\d+)', header).group(1))
    assert version == runtime.ABI_VERSION >= 37
    stripped = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    library = runtime.library()
    assert library.emph_abi_version() == runtime.ABI_VERSION
    for name in SYMBOLS:
        assert re.search(rf'\bint {name}\s*\(', stripped), name
        assert name in runtime.SIGNATURES
        function = getattr(library, name)
        assert function.argtypes == runtime.SIGNATURES[name][1]
    assert 'dropout.hip' in open(os.path.join(
        ROOT, 'emphases_amd', 'csrc', 'Makefile')).read()
    source = open(os.path.join(
        ROOT, 'emphases_amd', 'csrc', 'dropout.hip')).read()
    for constant in ('0xD2511F53', '0xCD9E8D57', '0x9E3779B9', '0xBB67AE85'):
        assert constant in source
    assert 'asm' not in source


def test_contract_violations_are_refused_and_never_launched():
    """Checked before the launch, so host memory (never read) will do."""
    library = runtime.library()
    buffer = np.zeros(64, dtype=np.float32)
    pointer = buffer.ctypes.data
    assert pointer % 16 == 0

    def forward(x=pointer, count=64, origin=0, p=0.1):
        return library.emph_dropout(x, count, origin, p, 1, 1, 0, None)

    def backward(y=pointer, gradient=pointer, count=64, activation=1, p=0.1):
        return library.emph_activation_dropout_backward(
            y, gradient, count, activation, p, None)

    for bad in ({'x': None}, {'count': 62}, {'origin': 2}, {'p': 1.}, {'p': -.1},
                {'p': float('nan')}, {'x': pointer + 4}, {'count': -4},
                {'origin': -4}):
        assert forward(**bad) == EINVAL, bad
        assert b'emph_dropout' in library.emph_last_error()
    for bad in ({'y': None}, {'gradient': None}, {'count': 62}, {'p': 1.},
                {'p': -.1}, {'y': pointer + 4}, {'gradient': pointer + 8},
                {'activation': 2}, {'activation': 0}):
        assert backward(**bad) == EINVAL, bad
        assert b'emph_activation_dropout_backward' in library.emph_last_error()
    # nothing to do is not an error, and launches nothing either
    assert forward(count=0) == 0 and backward(count=0) == 0
    assert not buffer.any()
