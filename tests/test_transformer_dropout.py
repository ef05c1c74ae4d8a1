"""The reference's dropout of the Transformer, checked without a device: the
specification (`train/dropout.py`: streams, the attention mask), the C ABI of
the two new entry points, the constructor of `TransformerModel`, and the
float64 restatement of `transformer_dropout_data` anchored against the
reference's recorded runs without masks (transformer_train*.npz) and with
them (transformer_dropout*.npz)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import transformer_dropout_data as data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import runtime, train  # noqa: E402
from emphases_amd.train import dropout as spec  # noqa: E402
from emphases_amd.train import transformer_model  # noqa: E402

ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')
CONFIGS = {
    'intermediate_sum': dict(downsample_location='intermediate',
                             downsample_method='sum'),
    'loss_max': dict(downsample_location='loss', downsample_method='max'),
}
NEW_SYMBOLS = ('emph_attention_dropout', 'emph_attention_dropout_backward',
               'emph_attention_dropout_backward_workspace')


def test_the_constants_are_the_references():
    assert spec.TRANSFORMER_LAYER_DROPOUT == 0.1
    assert spec.TRANSFORMER_POSITION_DROPOUT == 0.1


def test_transformer_streams_are_distinct():
    config = emphases_amd.Config(architecture='transformer', layers=6)
    ids = []
    for stack in ('frame_encoder', 'word_decoder'):
        ids.append(spec.transformer_stream(config, stack))
        for layer in range(6):
            sites = [spec.transformer_stream(config, stack, layer, site)
                     for site in ('attention', 'residual1', 'hidden',
                                  'residual2')]
            # what `encoder_layer_dropout` assumes of its stream_base
            assert sites == list(range(sites[0], sites[0] + 4))
            ids += sites
    assert len(ids) == 2 * (1 + 4 * 6) == len(set(ids))
    assert all(0 <= i < 1 << 32 for i in ids)
    # a pure function
    assert spec.transformer_stream(config, 'word_decoder', 5, 'hidden') == \
        spec.transformer_stream(config, 'word_decoder', 5, 'hidden')


def test_attention_mask_is_philox_on_the_specified_counters():
    seed, stream, step, p, ld = (0x0123456789ABCDEF, 7, 11, 0.1, 1088)
    head, column, keys = 1, 345, 23
    got = spec.attention_keep_mask(seed, stream, step, p, ld, head, column,
                                   keys)
    assert got.dtype == np.bool_ and got.shape == (keys,)
    for k in range(keys):
        words = spec.philox4x32_10(
            (k // 4, head * ld + column, stream, step),
            (seed & 0xFFFFFFFF, seed >> 32))
        assert bool(got[k]) == (int(words[k % 4]) >= spec.threshold(p)), k
    # a shorter row is a prefix: keys need not be a multiple of the quad
    for fewer in (1, 2, 3, 4, 5, 22):
        assert np.array_equal(spec.attention_keep_mask(
            seed, stream, step, p, ld, head, column, fewer), got[:fewer])
    assert spec.attention_keep_mask(
        seed, stream, step, p, ld, head, column, 0).shape == (0,)
    # the whole segment at once is the same function
    whole = spec.attention_segment_mask(seed, stream, step, p, ld, 2, 340, 23)
    assert whole.shape == (2, 23, 23)
    assert np.array_equal(whole[head, column - 340], got)


def test_attention_mask_differs_between_heads_columns_streams_and_steps():
    base = dict(seed=5, stream=3, step=2, p=0.5, ld=1024, head=0,
                query_column=17, keys=256)
    first = spec.attention_keep_mask(**base)
    for change in (dict(head=1), dict(query_column=18), dict(stream=4),
                   dict(step=3), dict(seed=6)):
        other = spec.attention_keep_mask(**{**base, **change})
        differing = int((other != first).sum())
        print(change, differing, 'of 256 differ')
        # independent fair bits differ in 128 +- 8 of 256
        assert 80 <= differing <= 176, (change, differing)
    # p = 0 keeps everything, whatever the words
    assert spec.attention_keep_mask(**{**base, 'p': 0.}).all()


def test_attention_mask_keeps_nine_in_ten():
    count = 1000
    kept = spec.attention_segment_mask(9, 1, 0, 0.1, 1024, 1, 0, count)
    assert kept.size == 10 ** 6
    fraction = float(kept.mean())
    sigma = (0.1 * 0.9 / kept.size) ** 0.5
    print(f'kept {fraction:.6f}, {(fraction - 0.9) / sigma:+.2f} sigma')
    assert abs(fraction - 0.9) <= 4. * sigma


def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(emph_\w+)\s*\(', header))
    library = runtime.library()
    for name in NEW_SYMBOLS:
        assert name in declared and name in runtime.SIGNATURES
        assert getattr(library, name) is not None
    assert len(runtime.SIGNATURES['emph_attention_dropout'][1]) == 14
    assert len(runtime.SIGNATURES['emph_attention_dropout_backward'][1]) == 17
    assert runtime.ABI_VERSION == 45 == library.emph_abi_version()


def test_the_constructor_needs_no_device_and_still_refuses_config_dropout():
    config = emphases_amd.Config(architecture='transformer', layers=2)
    model = train.TransformerModel(config, seed=3, reference_dropout=True)
    assert model.reference_dropout is True and model.steps == 0
    assert isinstance(model.steps, int)
    plain = train.TransformerModel(config, seed=3)
    assert plain.reference_dropout is False
    # `steps` is no parameter and no buffer: checkpoints keep their names
    assert list(model.state_dict()) == list(plain.state_dict())
    assert 'steps' not in dict(model.named_buffers())
    with pytest.raises(NotImplementedError, match='dropout'):
        train.TransformerModel(
            emphases_amd.Config(architecture='transformer', dropout=0.1),
            reference_dropout=True)
    assert 'reference_dropout' in transformer_model.__doc__


###############################################################################
# The restatement against the reference's recorded runs
###############################################################################


def load(name):
    with np.load(os.path.join(GOLDEN, name)) as file:
        return {key: file[key] for key in file.files}


def restated(name, golden, dropout):
    batch = load('transformer_train.npz')
    config = emphases_amd.Config(
        architecture='transformer', layers=2, **CONFIGS[name])
    seed = int(golden[f'{name}/seed'])
    state = transformer_model.initial_transformer_state(config, seed)
    import torch
    return data.model(
        state, config, batch['features'], batch['frames'], batch['bounds'],
        batch['words'], batch['targets'], torch.float64,
        (seed, int(golden[f'{name}/step'])) if dropout else None)


def compare(name, found, golden, grads):
    """The stored gradients are float64 rounded to float32 (6e-8 of a value):
    2e-7 of max |want| leaves room for that and nothing else; the loss and the
    logits are stored in float64."""
    loss, logits, gradients = found
    want = float(golden[f'{name}/loss'])
    print(f'{name}: loss {loss:.15g} (reference {want:.15g})')
    assert abs(loss - want) <= 1e-11 * abs(want)
    wanted = golden[f'{name}/logits']
    assert np.abs(logits - wanted).max() <= 1e-11 * np.abs(wanted).max()
    assert set(grads) == set(gradients)
    for key, stored in grads.items():
        error = np.abs(gradients[key] - stored.astype(np.float64)).max() / \
            np.abs(stored).max()
        print(f'{name} {key}: {error:.3g}')
        assert error <= 2e-7, (key, error)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_the_restatement_without_masks_reproduces_the_reference(name):
    golden = load('transformer_train.npz')
    golden[f'{name}/step'] = 0
    compare(name, restated(name, golden, False), golden,
            load(f'transformer_train_grads_{name}.npz'))


@pytest.mark.parametrize('name', list(CONFIGS))
def test_the_restatement_with_masks_reproduces_the_reference(name):
    golden = load('transformer_dropout.npz')
    assert float(golden[f'{name}/keep_all_error']) <= 1e-12
    assert int(golden[f'{name}/step']) == 3
    plain = load('transformer_train.npz')
    # the masks bite: not the run without dropout
    if int(golden[f'{name}/seed']) == int(plain[f'{name}/seed']):
        assert abs(float(golden[f'{name}/loss']) -
                   float(plain[f'{name}/loss'])) > 1e-3
    compare(name, restated(name, golden, True), golden,
            load(f'transformer_dropout_grads_{name}.npz'))
