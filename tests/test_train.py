"""The host side of `emphases_amd.train` (no device): initial weights against
the reference's, the gather tables of the weight packs, the refusals, batch
validation, the saved file and the C ABI of the training kernels."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import runtime, train, weights  # noqa: E402

TRAIN_SYMBOLS = (
    'emph_take', 'emph_loss_grad', 'emph_output_layer_backward',
    'emph_activation_backward', 'emph_segment_broadcast',
    'emph_conv_weight_grad_parts', 'emph_conv_weight_grad', 'emph_adam_step')


def test_initial_weights_are_the_reference_model_bitwise():
    """`emphases.Model()` after torch.manual_seed(0): sums, sums of squares
    and the leading values of every tensor (tests/golden/train.npz)."""
    golden = train_data.golden()
    before = torch.random.get_rng_state()
    state = train.initial_state(emphases_amd.DEFAULT, seed=0)
    assert torch.equal(before, torch.random.get_rng_state())
    assert list(state) == list(weights.parameter_shapes())
    for name, value in state.items():
        assert value.dtype == np.float32
        wide = value.astype(np.float64)
        assert np.array_equal(
            np.array([wide.sum(), (wide ** 2).sum()]), golden[f'init/{name}'])
        assert np.array_equal(value.ravel()[:8], golden[f'init_head/{name}'])
    other = train.initial_state(emphases_amd.DEFAULT, seed=1)
    assert not np.array_equal(
        other['input_layer.weight'], state['input_layer.weight'])


@pytest.mark.parametrize('features', [80, 83])
def test_gather_tables_are_the_packs_of_the_flat_buffer(features):
    """Taking the flat parameter buffer through the table equals
    `emph_conv_pack` of every layer's weight, and of
    W'[ci][co][j] = W[co][ci][2 - j] for the data gradient."""
    config = emphases_amd.Config(
        layers=2, pitch_feature=features > 80, periodicity_feature=features > 81,
        loudness_feature=features > 82)
    assert config.num_features == features
    offsets, count = train.parameter_offsets(config)
    tables = train.gather_tables(config)
    index = tables['index']
    assert index.dtype == np.int32 and index.max() < count
    # (80 -> 80 packs have no padding; 83 input rows are padded to 88)
    assert index.min() == (0 if features == 80 else -1)
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
        assert size == want.size and start % 64 == 0
        assert np.array_equal(taken[start:start + size], want)
        # a permutation with padding: every weight exactly once
        inside = index[start:start + size]
        assert np.array_equal(
            np.sort(inside[inside >= 0]),
            np.arange(first, first + weight.size))
        if name == 'input_layer':
            continue
        start, size = tables['backward'][name]
        flipped = np.ascontiguousarray(weight.transpose(1, 0, 2)[:, :, ::-1])
        assert np.array_equal(
            taken[start:start + size], runtime.conv_pack(flipped))


@pytest.mark.parametrize('field,value', [
    ('architecture', 'transformer'), ('downsample_location', 'input'),
    ('downsample_location', 'inference'), ('downsample_location', 'loss'),
    ('downsample_method', 'max'), ('downsample_method', 'center'),
    ('activation', 'gelu'), ('activation', 'silu'),
    ('activation', 'leaky_relu'), ('channels', 64),
    ('encoder_kernel_size', 5), ('decoder_kernel_size', 1), ('layers', 17),
    ('mel_feature', False), ('method', 'pitch-variance')])
def test_unsupported_configurations_are_refused_by_name(field, value):
    config = dataclasses.replace(emphases_amd.DEFAULT, **{field: value})
    with pytest.raises(NotImplementedError, match=field):
        train.Trainer(config=config)
    with pytest.raises(NotImplementedError, match=field):
        train.check_supported(config)


def test_supported_configurations_pass():
    for overrides in ({}, {'loss': 'mse'}, {'downsample_method': 'average'},
                      {'layers': 16}, {'layers': 1, 'loudness_feature': True}):
        train.check_supported(emphases_amd.Config(**overrides))


def test_malformed_batches_raise_value_error():
    batch = train_data.collated('ragged')
    frames, words, bounds = train.check_batch(*batch)
    assert frames == [5, 37, 64, 100, 129, 300]
    assert words == [1, 3, 7, 12, 2, 40] and bounds.shape == (6, 2, 40)
    features, frame_lengths, word_bounds, word_lengths, targets = batch

    def broken(**changes):
        arguments = dict(
            features=features, frame_lengths=frame_lengths,
            word_bounds=word_bounds, word_lengths=word_lengths,
            targets=targets)
        arguments.update(changes)
        with pytest.raises(ValueError):
            train.check_batch(**arguments)
    empty = word_bounds.clone()
    empty[2, 1, 3] = empty[2, 0, 3]                      # end == start
    broken(word_bounds=empty)
    backwards = word_bounds.clone()
    backwards[3, :, 5] = backwards[3, :, 5].flip(0)      # end < start
    broken(word_bounds=backwards)
    late = word_bounds.clone()
    late[1, 1, 2] += 1                                   # past its 37 frames
    broken(word_bounds=late)
    shorter = frame_lengths.clone()
    shorter[5] = 299
    broken(frame_lengths=shorter)
    broken(targets=targets[:, :, :39])                   # fewer than 40 words
    overlapping = word_bounds.clone()
    overlapping[5, 0, 7] -= 1
    broken(word_bounds=overlapping)
    broken(features=features[:, :79])
    broken(frame_lengths=frame_lengths[:5])
    broken(word_lengths=torch.zeros_like(word_lengths))


def test_saved_file_is_a_reference_checkpoint(tmp_path):
    config = emphases_amd.DEFAULT
    state = train.initial_state(config, seed=3)
    model = {name: torch.from_numpy(value) for name, value in state.items()}
    _, count = train.parameter_offsets(config)
    generator = torch.Generator().manual_seed(5)
    exp_avg = torch.randn(count, generator=generator)
    exp_avg_sq = torch.rand(count, generator=generator)
    optimizer = train.adam_state_dict(
        config, 7, exp_avg, exp_avg_sq, lr=2e-3, betas=(0.8, 0.99), eps=1e-7)
    path = tmp_path / '00000007.pt'
    train.write_checkpoint(path, model, optimizer, epoch=2, step=7,
                           score=0.5, best=0.25)
    saved = torch.load(path, map_location='cpu', weights_only=False)
    assert set(saved) == {'epoch', 'step', 'score', 'best', 'model', 'optimizer'}
    assert (saved['epoch'], saved['step']) == (2, 7)
    assert (saved['score'], saved['best']) == (0.5, 0.25)
    # the reference's modules in Model.parameters() order take both halves
    modules = [torch.nn.Parameter(torch.zeros(shape))
               for shape in weights.parameter_shapes(config).values()]
    adam = torch.optim.Adam(modules)
    adam.load_state_dict(saved['optimizer'])
    group = adam.param_groups[0]
    assert (group['lr'], group['betas'], group['eps']) == (2e-3, (0.8, 0.99), 1e-7)
    cursor = 0
    for module in modules:
        entry = adam.state[module]
        size = module.numel()
        assert float(entry['step']) == 7.
        assert torch.equal(entry['exp_avg'].ravel(), exp_avg[cursor:cursor + size])
        assert torch.equal(
            entry['exp_avg_sq'].ravel(), exp_avg_sq[cursor:cursor + size])
        cursor += size
    assert cursor == count
    # inference reads the file as checkpoint=
    loaded = weights.load(str(path), config)
    for name, value in state.items():
        assert np.array_equal(loaded[name], value)
    # no state before the first step, as torch.optim.Adam
    fresh = train.adam_state_dict(config, 0, exp_avg, exp_avg_sq)
    assert fresh['state'] == {}
    torch.optim.Adam(modules).load_state_dict(fresh)


def test_training_abi_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    version = int(re.search(r'#define EMPH_ABI_VERSION (\d+)', header).group(1))
    assert version == runtime.ABI_VERSION >= 34
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(emph_\w+)\s*\(', header))
    library = runtime.library()
    assert library.emph_abi_version() == runtime.ABI_VERSION
    for name in TRAIN_SYMBOLS:
        assert name in declared and name in runtime.SIGNATURES
        assert getattr(library, name) is not None
    # slabs: one per workgroup, never more than the tiles, never none
    parts = library.emph_conv_weight_grad_parts
    assert [parts(n) for n in (0, 1, 2, 64, 256)] == [0, 1, 2, 64, 256]
    assert parts(257) == 129 and parts(1172) == 235
    # contract violations are reported, not launched
    assert library.emph_conv_weight_grad(
        None, 0, None, 0, 80, 80, 3, None, 1, 64, None, None, None, None) == -1
    assert b'null' in library.emph_last_error()
    assert library.emph_take(None, None, None, 4, None) == -1
    assert library.emph_adam_step(
        None, None, None, None, 4, 0.9, 0.999, 1e-3, 1., 1e-8, None) == -1
