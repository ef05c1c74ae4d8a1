"""`precision='bf16x3'` of Transformer training, checked without a device: the
float64 restatement of tests/attention_split_emulation.py anchored against the
reference's recorded runs (transformer_train*.npz), its attention against
torch autograd, the condition that the piece arithmetic flips no ReLU of the
cases the GPU tests use, the refusals of `encoder_layer_split` and of
`TransformerModel(precision=)`, and the C ABI of the new entry points."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import attention_split_emulation as emulation  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import ops, runtime, train  # noqa: E402
from emphases_amd.train import transformer_model  # noqa: E402

ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')
NEW_SYMBOLS = ('emph_attention_backward_split',
               'emph_attention_backward_split_workspace',
               'emph_attention_backward_split_bytes')


def golden():
    with np.load(os.path.join(GOLDEN, 'transformer_train.npz')) as data:
        return {name: data[name] for name in data.files}


@pytest.mark.parametrize('name', list(emulation.GOLDEN_CONFIGS))
def test_the_restatement_reproduces_the_reference(name):
    """split=False against the reference's float64 gradients, which the
    golden files hold as float32: within 2^-23 of max |want| per tensor,
    twice the storage rounding."""
    data = golden()
    loss, logits, grads, _ = emulation.golden_results(GOLDEN, name)[False]
    assert abs(loss - float(data[f'{name}/loss'])) <= 1e-12
    assert np.abs(logits - data[f'{name}/logits']).max() <= 1e-12
    worst = 0.
    with np.load(os.path.join(
            GOLDEN, f'transformer_train_grads_{name}.npz')) as wanted:
        assert set(wanted.files) == set(grads)
        for key in wanted.files:
            want = wanted[key].astype(np.float64)
            error = np.abs(grads[key] - want).max() / np.abs(want).max()
            worst = max(worst, error)
            assert error <= 2. ** -23, (key, error)
    print(f'{name}: worst tensor {worst:.3g} of max |want|')


@pytest.mark.parametrize('name', list(emulation.GOLDEN_CONFIGS))
def test_the_emulation_flips_no_relu_on_the_golden_batch(name):
    results = emulation.golden_results(GOLDEN, name)
    flips, margin = emulation.relu_flips(results[False][3], results[True][3])
    worst = max(
        np.abs(results[True][2][key] - value).max() / np.abs(value).max()
        for key, value in results[False][2].items())
    print(f'{name}: {flips} flips, smallest |pre-activation| {margin:.3g} of '
          f'the largest; worst gradient {worst:.3g} from float64')
    assert flips == 0
    # the piece arithmetic is in use (a long segment exists) and at fp32 grade
    assert 0. < worst < 1e-5


def test_the_emulation_flips_no_relu_on_the_layer_case():
    case, exact, emulated, seed = emulation.layer_case()
    print(f'layer case: seed {seed}')
    _, exact_record = emulation.layer_results(
        case, emulation.LAYER_SEGMENTS, False)
    _, record = emulation.layer_results(case, emulation.LAYER_SEGMENTS, True)
    assert emulation.relu_flips(exact_record, record)[0] == 0
    # short segments are exact: the emulation changes the long ones alone
    first = sum(n for n in emulation.LAYER_SEGMENTS[:3])
    assert emulation.LAYER_SEGMENTS[:3] == (1, 17, 64)
    assert torch.equal(exact[0][:, :first], emulated[0][:, :first])
    assert not torch.equal(exact[0][:, first:], emulated[0][:, first:])


def test_unsplit_attention_is_torch_autograd():
    generator = torch.Generator().manual_seed(4)
    q, k, v, dout = (torch.randn(200, 40, generator=generator,
                                 dtype=torch.float64) for _ in range(4))
    ours = [t.clone().requires_grad_(True) for t in (q, k, v)]
    emulation.attention(*ours, split=False).backward(dout)
    theirs = [t.clone().requires_grad_(True) for t in (q, k, v)]
    (torch.softmax(theirs[0] @ theirs[1].t() / 40. ** 0.5, dim=1) @
     theirs[2]).backward(dout)
    for one, other in zip(ours, theirs):
        error = float((one.grad - other.grad).abs().max() /
                      other.grad.abs().max())
        assert error <= 1e-12, error
    # ... and below 128 positions `split=True` is that too
    short = [t[:127].clone().requires_grad_(True) for t in (q, k, v)]
    exact = [t[:127].clone().requires_grad_(True) for t in (q, k, v)]
    emulation.attention(*short, split=True).backward(dout[:127])
    emulation.attention(*exact, split=False).backward(dout[:127])
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(short, exact))


def test_three_pieces_add_up_exactly_and_six_products_are_fp32_grade():
    generator = torch.Generator().manual_seed(5)
    a = torch.randn(64, 40, generator=generator).double()
    b = torch.randn(64, 40, generator=generator).double()
    assert torch.equal(sum(emulation.pieces3(a)), a)
    exact = a @ b.t()
    six = emulation.product6(lambda x, y: x @ y.t(), a, b, True)
    three = emulation.product(lambda x, y: x @ y.t(), a, b, True)
    scale = float(exact.abs().max())
    six_error = float((six - exact).abs().max()) / scale
    three_error = float((three - exact).abs().max()) / scale
    print(f'six products {six_error:.3g}, three {three_error:.3g}')
    assert six_error < 2. ** -22 < three_error < 2. ** -14


###############################################################################
# Refusals, before a GPU is needed
###############################################################################


def layer_arguments(channels=80):
    x = torch.zeros(channels, 10)
    return [x] + [torch.zeros(1)] * 12 + [torch.tensor([0, 10])]


def test_encoder_layer_split_refuses_by_name():
    split = torch.ops.emphases_amd.encoder_layer_split
    assert 'encoder_layer_split' in ops.__all__
    with pytest.raises(ValueError, match="precision='f32'"):
        split(*layer_arguments(), 2, 'f32')
    for precision in ('bf16x3_fast', 'bf16x6'):
        with pytest.raises(NotImplementedError, match='precision'):
            split(*layer_arguments(), 2, precision)
    with pytest.raises(ValueError, match='precision'):
        split(*layer_arguments(), 2, 'fp16')
    with pytest.raises(NotImplementedError, match='80 channels'):
        split(*layer_arguments(64), 2, 'bf16x3')
    with pytest.raises(NotImplementedError, match='heads'):
        split(*layer_arguments(), 4, 'bf16x3')
    # a host tensor: no CPU implementation
    with pytest.raises(runtime.LibraryError, match='no CPU'):
        split(*layer_arguments(), 2, 'bf16x3')


def test_the_constructor_takes_precision_and_needs_no_device():
    config = emphases_amd.Config(architecture='transformer', layers=2)
    plain = train.TransformerModel(config, seed=3, precision='f32')
    assert plain.precision == 'f32'
    assert train.TransformerModel(config, seed=3).precision == 'f32'
    model = train.TransformerModel(config, seed=3, precision='bf16x3')
    assert model.precision == 'bf16x3'
    assert all(stack.precision == 'bf16x3'
               for stack in (model.frame_encoder, model.word_decoder))
    # checkpoints do not record the precision
    assert list(model.state_dict()) == list(plain.state_dict())
    for one, other in zip(model.state_dict().values(),
                          plain.state_dict().values()):
        assert torch.equal(one, other)
    plain.load_state_dict(model.state_dict())
    with pytest.raises(NotImplementedError, match='reference_dropout'):
        train.TransformerModel(config, precision='bf16x3',
                               reference_dropout=True)
    for precision in ('bf16x3_fast', 'bf16x6'):
        with pytest.raises(NotImplementedError, match='precision'):
            train.TransformerModel(config, precision=precision)
    for precision in ('fp16', None, 3):
        with pytest.raises(ValueError, match='precision'):
            train.TransformerModel(config, precision=precision)
    assert "precision='bf16x3'" in transformer_model.__doc__


def test_the_loop_still_refuses_the_architecture():
    config = emphases_amd.Config(architecture='transformer', layers=2)
    with pytest.raises((NotImplementedError, ValueError)):
        train.make_trainer(config, precision='bf16x3')


###############################################################################
# The C ABI
###############################################################################


def test_the_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(emph_\w+)\s*\(', header))
    library = runtime.library()
    for name in NEW_SYMBOLS:
        assert name in declared and name in runtime.SIGNATURES
        assert getattr(library, name) is not None
    # (the stream is the last argument)
    assert len(runtime.SIGNATURES['emph_attention_backward_split'][1]) == 14
    assert runtime.ABI_VERSION == 45 == library.emph_abi_version()


def test_the_sizes_are_host_arithmetic():
    library = runtime.library()
    assert library.emph_attention_backward_split_workspace(1024, 2) == 4096
    assert library.emph_attention_backward_split_workspace(0, 2) == 0
    # 92 928 bytes per 64 positions and head (include/emphases_hip.h)
    assert library.emph_attention_backward_split_bytes(1024, 3, 80, 2) == \
        (1024 // 64 + 3 + 1) * 2 * 92928
    for channels, heads in ((64, 2), (128, 2), (80, 1), (160, 4)):
        assert library.emph_attention_backward_split_bytes(
            1024, 3, channels, heads) == -1
