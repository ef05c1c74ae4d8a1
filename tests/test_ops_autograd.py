"""The differentiable operator seams without a GPU: the new C ABI, the layout
of `train.TorchModel` against `weights.parameter_shapes`, its initial values,
its refusals, and the index tables of the device-side weight packs."""
import os
import re

import numpy as np
import pytest
import torch

import emphases_amd
from emphases_amd import ops, runtime, train, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('emph_conv_weight_grad_any_workspace', 'emph_conv_weight_grad_any',
               'emph_segment_reduce_backward', 'emph_activation_gradient')
GRID = dict(channels=64, encoder_kernel_size=5, decoder_kernel_size=1,
            activation='gelu', downsample_location='loss',
            downsample_method='max')


def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    version = int(re.search(r'#define EMPH_ABI_VERSION (\d+)', header).group(1))
    assert version == runtime.ABI_VERSION >= 38
    library = runtime.library()
    for name in NEW_SYMBOLS:
        assert f'{name}(' in header
        assert name in runtime.SIGNATURES
        assert getattr(library, name).argtypes == runtime.SIGNATURES[name][1]
    makefile = open(os.path.join(
        ROOT, 'emphases_amd', 'csrc', 'Makefile')).read()
    assert 'conv_grad_any.hip' in makefile and 'autograd.hip' in makefile


def test_weight_grad_workspace_and_range():
    """Host arithmetic only: nothing is launched."""
    library = runtime.library()
    parts = library.emph_conv_weight_grad_parts(300)
    assert library.emph_conv_weight_grad_any_workspace(128, 128, 7, 300) == \
        parts * (128 * 128 * 7 + 128)
    assert library.emph_conv_weight_grad_any_workspace(3, 7, 5, 1) == 3 * 7 * 5 + 7
    for c_in, c_out, k in ((0, 80, 3), (129, 80, 3), (80, 0, 3), (80, 129, 3),
                           (80, 80, 2), (80, 80, 9), (80, 80, 0)):
        assert library.emph_conv_weight_grad_any_workspace(c_in, c_out, k, 4) == 0
        # (the shape is checked before any pointer is looked at)
        assert library.emph_conv_weight_grad_any(
            None, 64, None, 64, c_in, c_out, k, None, 1, 64, None, None, None,
            None) == -2


@pytest.mark.parametrize('overrides', [{}, GRID, {'dropout': 0.1}],
                         ids=['default', 'grid', 'dropout'])
def test_parameters_follow_the_reference_layout(overrides):
    config = emphases_amd.Config(**overrides)
    model = train.TorchModel(config)
    named = [(name, tuple(parameter.shape))
             for name, parameter in model.named_parameters()]
    wanted = [(train.checkpoint_names(config)[name], tuple(shape))
              for name, shape in weights.parameter_shapes(config).items()]
    assert named == wanted
    assert list(model.state_dict()) == [name for name, _ in wanted]
    # ... and the state dict is what weights.load reads
    loaded = weights.load(model.state_dict(), config)
    assert list(loaded) == list(weights.parameter_shapes(config))
    if overrides == GRID:
        assert named[0] == ('input_layer.weight', (64, 80, 5))
        assert named[-2] == ('output_layer.weight', (1, 64, 1))
        assert not any(name.startswith('word_decoder') for name, _ in named)
    if 'dropout' in overrides:
        assert 'frame_encoder.3.weight' in dict(named)
        assert isinstance(getattr(model.frame_encoder, '2'), torch.nn.Dropout)


def test_initial_values_are_the_trainers():
    before = torch.random.get_rng_state()
    model = train.TorchModel(emphases_amd.DEFAULT, seed=3)
    assert torch.equal(before, torch.random.get_rng_state())
    wanted = train.initial_state(emphases_amd.DEFAULT, seed=3)
    state = model.state_dict()
    assert list(state) == list(wanted)
    for name, value in wanted.items():
        assert np.array_equal(state[name].numpy(), value), name
    other = train.TorchModel(emphases_amd.DEFAULT, seed=4).state_dict()
    assert not torch.equal(other['input_layer.weight'],
                           state['input_layer.weight'])


@pytest.mark.parametrize('overrides, field', [
    ({'downsample_location': 'inference'}, 'downsample_location'),
    ({'downsample_location': 'input'}, 'downsample_location'),
    ({'architecture': 'transformer'}, 'architecture'),
    ({'channels': 72}, 'channels'),
    ({'channels': 144}, 'channels'),
])
def test_unsupported_configurations_are_refused_by_name(overrides, field):
    with pytest.raises(NotImplementedError, match=field):
        train.TorchModel(emphases_amd.Config(**overrides))


def test_loss_fn_is_the_masked_mean():
    logits = torch.tensor([0.5, -1.25, 3.])
    targets = torch.tensor([1., 0., 0.25])
    bce = (torch.clamp(logits, min=0) - logits * targets +
           torch.log1p(torch.exp(-logits.abs()))).mean()
    assert torch.allclose(train.loss_fn(logits, targets, 'bce'), bce)
    assert torch.allclose(train.loss_fn(logits, targets, 'mse'),
                          ((logits - targets) ** 2).mean())
    with pytest.raises(ValueError):
        train.loss_fn(logits, targets, 'l1')


@pytest.mark.parametrize('shape', [(80, 64, 5), (1, 80, 3)])
def test_pack_index_tables_agree_with_the_host_pack(shape):
    """Taking a weight through the tables gives `runtime.conv_pack` of the
    weight, and of its flipped transpose."""
    generator = torch.Generator().manual_seed(sum(shape))
    weight = torch.randn(shape, generator=generator).numpy()
    forward, flipped = ops.pack_index_tables(shape)
    assert forward.dtype == flipped.dtype == np.int32

    def take(table):
        return np.where(table < 0, np.float32(0),
                        weight.ravel()[np.maximum(table, 0)])
    assert np.array_equal(take(forward), runtime.conv_pack(weight))
    turned = np.ascontiguousarray(weight.transpose(1, 0, 2)[:, :, ::-1])
    assert turned.shape == (shape[1], shape[0], shape[2])
    assert np.array_equal(take(flipped), runtime.conv_pack(turned))


def test_backward_bounds_check():
    plan = ops._frame_plan(
        np.array([40, 30]), np.array([2, 2]),
        np.array([[0, 10, 5, 20], [10, 20, 20, 30]]))
    ops.check_backward_bounds(plan)
    for bad in ([[0, 8, 5, 20], [10, 20, 20, 30]],      # overlap
                [[10, 0, 5, 20], [20, 10, 20, 30]],     # out of order
                [[0, 10, 5, 20], [10, 20, 5, 30]]):     # empty word
        with pytest.raises(ValueError):
            ops.check_backward_bounds(ops._frame_plan(
                np.array([40, 30]), np.array([2, 2]), np.array(bad)))


def test_weight_caches_never_answer_for_another_tensor():
    """The device-pack and first-version caches key on an address; an entry
    must die with the storage it was made from (the allocator reuses the
    address of a dropped weight)."""
    import gc
    cache = ops._ByStorage(2)
    first = torch.zeros(4, 3, 3)
    key = cache.key(first, first._version, False)
    assert cache.get(first, key) is None
    assert cache.put(first, key, 'first') == 'first'
    assert cache.get(first, key) == 'first'
    assert cache.get(first.detach(), key) == 'first'      # the same storage
    # another live tensor asking under the same key: a miss, the entry goes
    other = torch.zeros(4, 3, 3)
    assert cache.get(other, key) is None
    assert cache.get(first, key) is None
    # a dead storage
    cache.put(first, key, 'first')
    del first
    gc.collect()
    assert cache.get(other, key) is None and not cache.entries
    # the version and the direction are part of the key; the LRU holds `size`
    keys = [cache.key(other, other._version, flipped) for flipped in (False, True)]
    assert keys[0] != keys[1]
    other.add_(1)
    keys.append(cache.key(other, other._version, False))
    assert keys[2] != keys[0]
    for index, entry in enumerate(keys):
        cache.put(other, entry, index)
    assert cache.get(other, keys[0]) is None
    assert cache.get(other, keys[1]) == 1 and cache.get(other, keys[2]) == 2


def test_an_entry_of_several_tensors_answers_for_those_tensors_alone():
    """The host packs of a convolution and the one-layer engine are made from
    several tensors: a hit needs every one of their storages alive and the
    asking tensors' own, and a strided view has a key of its own."""
    import gc
    cache = ops._ByStorage(4)
    weight, bias = torch.zeros(4, 4, 3), torch.zeros(4)

    def key(*pair):
        return cache.key(pair, tuple(tensor._version for tensor in pair), 0)
    entry = key(weight, bias)
    assert cache.get((weight, bias), entry) is None
    assert cache.put((weight, bias), entry, 'pack') == 'pack'
    assert cache.get((weight, bias), entry) == 'pack'
    assert cache.get((weight.detach(), bias), entry) == 'pack'
    assert cache.get((weight, bias.detach()), entry) == 'pack'
    assert cache.get([weight.detach(), bias.detach()], entry) == 'pack'
    # either tensor replaced by another of the same shape: a miss, and the
    # entry goes
    for pair in ((torch.zeros(4, 4, 3), bias), (weight, torch.zeros(4))):
        assert cache.get(pair, entry) is None
        assert cache.get((weight, bias), entry) is None and not cache.entries
        cache.put((weight, bias), entry, 'pack')
    # either storage dead (a stand-in asks: the key is all that is left)
    other_weight, other_bias = torch.zeros(4, 4, 3), torch.zeros(4)
    del weight
    gc.collect()
    assert cache.get((other_weight, bias), entry) is None and not cache.entries
    cache.put((other_weight, bias), entry, 'pack')
    del bias
    gc.collect()
    assert cache.get((other_weight, other_bias), entry) is None
    assert not cache.entries
    # a transposed view shares address, version and shape with its base
    square = torch.zeros(4, 4, 3)
    turned = square.transpose(0, 1)
    assert (turned.data_ptr(), turned._version, turned.shape) == \
        (square.data_ptr(), square._version, square.shape)
    assert cache.key(square) != cache.key(turned)
    assert key(square, other_bias) != key(turned, other_bias)


def test_weight_changes_follows_the_version_of_one_storage():
    import gc
    weight = torch.zeros(8, 4, 3)
    assert not ops._weight_changes(weight)
    assert not ops._weight_changes(weight.detach())
    weight.add_(1)
    assert ops._weight_changes(weight)
    # a new tensor under a stale entry's key starts over
    key = ops._ByStorage.key(weight)
    stale = ops._first_versions.entries[key]
    fresh = torch.zeros(8, 4, 3)
    fresh.add_(1)
    ops._first_versions.entries[ops._ByStorage.key(fresh)] = stale
    del weight
    gc.collect()
    assert not ops._weight_changes(fresh)
    fresh.add_(1)
    assert ops._weight_changes(fresh)
