"""`encoder_layer` under autograd and `train.TransformerModel` without a GPU:
the new C ABI and its argument checks, the model's parameter layout against
`weights.parameter_shapes`, its initial values against the reference's
recorded initialisation (tests/golden/transformer_train.npz), its refusals."""
import os
import re

import numpy as np
import pytest
import torch

import emphases_amd
from emphases_amd import runtime, train, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'transformer_train.npz')
NEW_SYMBOLS = ('emph_attention_backward_workspace', 'emph_attention_backward',
               'emph_add_layernorm_backward_parts',
               'emph_add_layernorm_backward')
CONFIGS = {
    'intermediate_sum': dict(downsample_location='intermediate',
                             downsample_method='sum'),
    'loss_max': dict(downsample_location='loss', downsample_method='max'),
}


def config_of(name, **more):
    return emphases_amd.Config(
        architecture='transformer', layers=2, **CONFIGS[name], **more)


def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    version = int(re.search(r'#define EMPH_ABI_VERSION (\d+)', header).group(1))
    assert version == runtime.ABI_VERSION >= 41
    library = runtime.library()
    assert library.emph_abi_version() == runtime.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert f'{name}(' in header
        assert name in runtime.SIGNATURES
        assert getattr(library, name).argtypes == runtime.SIGNATURES[name][1]
    makefile = open(os.path.join(
        ROOT, 'emphases_amd', 'csrc', 'Makefile')).read()
    assert 'transformer_grad.hip' in makefile


def test_attention_backward_argument_checks():
    """Return codes of calls that launch nothing (no GPU here)."""
    library = runtime.library()
    assert library.emph_attention_backward_workspace(1024, 2) == 2 * 2 * 1024
    assert library.emph_attention_backward_workspace(0, 2) == 0
    # the shape is checked before any pointer is looked at: head dimension
    # 32, 64, 80, and 40 in four heads
    for channels, heads in ((64, 2), (128, 2), (80, 1), (160, 4), (80, 0),
                            (80, 3)):
        assert library.emph_attention_backward(
            None, None, None, None, None, 64, channels, heads, None, 1, 64,
            None, None) == -2
    # the right shape: null pointers, another tile width
    assert library.emph_attention_backward(
        None, None, None, None, None, 64, 80, 2, None, 1, 64, None, None) == -1
    assert b'null pointer' in library.emph_last_error()
    assert library.emph_attention_backward(
        None, None, None, None, None, 64, 80, 2, None, 1, 32, None, None) == -1
    # no tile: nothing to do
    assert library.emph_attention_backward(
        None, None, None, None, None, 64, 80, 2, None, 0, 64, None, None) == 0


def test_add_layernorm_backward_argument_checks():
    library = runtime.library()
    assert library.emph_add_layernorm_backward_parts(0) == 0
    assert library.emph_add_layernorm_backward_parts(1) == 1
    assert library.emph_add_layernorm_backward_parts(512) == 512
    # runs of 3 tiles: 1172 tiles in 391 slabs
    assert library.emph_add_layernorm_backward_parts(1172) == 391
    for channels in (0, 129, -1):
        assert library.emph_add_layernorm_backward(
            None, None, None, None, 64, channels, 1e-5, None, 1, 64, None, None,
            None, None) == -2
    assert library.emph_add_layernorm_backward(
        None, None, None, None, 64, 80, 1e-5, None, 1, 64, None, None, None,
        None) == -1
    assert b'null pointer' in library.emph_last_error()
    assert library.emph_add_layernorm_backward(
        None, None, None, None, 64, 80, 1e-5, None, 1, 16, None, None, None,
        None) == -1


@pytest.mark.parametrize('name', list(CONFIGS))
def test_parameters_follow_the_reference_layout(name):
    config = config_of(name)
    model = train.TransformerModel(config)
    named = [(key, tuple(parameter.shape))
             for key, parameter in model.named_parameters()]
    wanted = [(key, tuple(shape))
              for key, shape in weights.parameter_shapes(config).items()]
    assert named == wanted
    assert list(model.state_dict()) == [key for key, _ in wanted]
    loaded = weights.load(model.state_dict(), config)
    for key, parameter in model.named_parameters():
        assert np.array_equal(loaded[key], parameter.detach().numpy())


@pytest.mark.parametrize('name', list(CONFIGS))
def test_initial_state_is_the_reference_initialisation(name):
    """Bitwise: the fixture keeps layer 0 of each stack (the reference clones
    one layer, `clones`)."""
    config = config_of(name)
    before = torch.get_rng_state()
    with np.load(GOLDEN) as golden:
        seed = int(golden[f'{name}/seed'])
        assert bool(golden[f'{name}/clones'])
        state = train.initial_transformer_state(config, seed)
        assert list(state) == list(weights.parameter_shapes(config))
        for key, value in state.items():
            stored = re.sub(r'\.model\.layers\.\d+\.', '.model.layers.0.', key)
            want = golden[f'{name}/init/{stored}']
            assert value.dtype == np.float32 and value.shape == want.shape
            assert np.array_equal(value.view(np.uint32), want.view(np.uint32)), key
    assert torch.equal(before, torch.get_rng_state())
    model = train.TransformerModel(config, seed=seed)
    for key, parameter in model.named_parameters():
        assert np.array_equal(parameter.detach().numpy(), state[key]), key
    other = train.initial_transformer_state(config, seed + 1)
    assert not np.array_equal(other['input_layer.weight'],
                              state['input_layer.weight'])


@pytest.mark.parametrize('overrides, field', [
    ({'downsample_location': 'inference'}, 'downsample_location'),
    ({'downsample_location': 'input'}, 'downsample_location'),
    ({'method': 'pitch-variance'}, 'method'),
    ({'architecture': 'convolution'}, 'architecture'),
    ({'channels': 64}, 'channels'),
    ({'heads': 4}, 'heads'),
    ({'dropout': 0.1}, 'dropout'),
])
def test_refusals_name_their_field(overrides, field):
    settings = dict(architecture='transformer', layers=2)
    settings.update(overrides)
    config = emphases_amd.Config(**settings)
    with pytest.raises(NotImplementedError, match=field):
        train.TransformerModel(config)
    with pytest.raises(NotImplementedError, match=field):
        train.initial_transformer_state(config)


def test_torch_model_still_refuses_the_transformer():
    with pytest.raises(NotImplementedError, match='architecture'):
        train.TorchModel(emphases_amd.Config(architecture='transformer'))


def test_every_method_is_accepted():
    for method in ('sum', 'average', 'max', 'center'):
        for location in ('intermediate', 'loss'):
            train.check_transformer_supported(emphases_amd.Config(
                architecture='transformer', downsample_location=location,
                downsample_method=method))


def test_a_segment_past_the_positional_table_raises():
    from emphases_amd.train import transformer_model
    cu = np.array([0, 10, 10 + emphases_amd.config.MAX_POSITIONS + 1],
                  dtype=np.int64)
    with pytest.raises(ValueError, match='positional encoding'):
        transformer_model._positions(cu.tobytes())
    index = transformer_model._positions(
        np.array([0, 3, 5], dtype=np.int64).tobytes())
    assert index.tolist() == [0, 1, 2, 0, 1]
