"""`torch.ops.emphases_amd.encoder_layer_padded` on the MI355X: the encoder
layer behind `src_key_padding_mask`, against
`torch.nn.TransformerEncoderLayer` in float64 on the CPU, `opcheck`, the plain
layer's bits at `key_counts == T`, and the host check of `key_counts`.

The bound is the project's (the convention of `test_gpu_ops_transformer`,
restated here): error <= 4 x the error of the same torch computation in
float32, both over max |want|, per tensor.  Each figure is printed before it
is asserted.
"""
import functools

import numpy as np
import pytest
import torch

from emphases_amd import ops

pytestmark = pytest.mark.gpu

CHANNELS, HEADS = 80, 2
# (positions, real positions) of every piece
PIECES = [(1, 1), (17, 5), (64, 64), (130, 70)]
LENGTHS = [n for n, _ in PIECES]
KEYS = [k for _, k in PIECES]
LAYER_NAMES = ('self_attn.in_proj_weight', 'self_attn.in_proj_bias',
               'self_attn.out_proj.weight', 'self_attn.out_proj.bias',
               'norm1.weight', 'norm1.bias', 'linear1.weight', 'linear1.bias',
               'linear2.weight', 'linear2.bias', 'norm2.weight', 'norm2.bias')


def device():
    return torch.device('cuda', 0)


def check(name, got, want, narrow):
    """error <= 4 x the float32 CPU error, both over max |want|."""
    want = want.double()
    scale = float(want.abs().max())
    allowed = 4. * float((narrow.double() - want).abs().max()) / scale
    error = float((got.detach().cpu().double() - want).abs().max()) / scale
    print(f'{name}: error {error:.3g}, bound {allowed:.3g}, ratio '
          f'{error / allowed if allowed else float("inf"):.2f}')
    assert error <= allowed, (name, error, allowed)


def layer_cu(lengths=LENGTHS):
    return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]))


@functools.lru_cache(maxsize=None)
def layer_case():
    """x, upstream [C, sum T] and the twelve parameters (the op's order) of a
    seeded `TransformerEncoderLayer`, on the CPU in float32.  The padded
    positions hold values like any other: they are queries, and the cotangent
    covers their rows."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(13)
        module = torch.nn.TransformerEncoderLayer(
            CHANNELS, HEADS, dim_feedforward=CHANNELS, dropout=0.)
        values = dict(module.named_parameters())
        parameters = []
        for name in LAYER_NAMES:
            value = values[name].detach().clone()
            if 'norm' in name or name.endswith('bias'):
                # (torch starts them at 1 and 0)
                value = value + 0.1 * torch.randn(value.shape)
            parameters.append(value)
        x = torch.randn(CHANNELS, sum(LENGTHS))
        upstream = torch.randn(CHANNELS, sum(LENGTHS))
    return x, upstream, tuple(parameters)


def layer_torch(dtype):
    """(out, dx, twelve gradients) of the torch layer with
    `src_key_padding_mask`, a piece at a time."""
    x, upstream, parameters = layer_case()
    module = torch.nn.TransformerEncoderLayer(
        CHANNELS, HEADS, dim_feedforward=CHANNELS, dropout=0.).to(dtype)
    with torch.no_grad():
        for name, value in zip(LAYER_NAMES, parameters):
            module.get_parameter(name).copy_(value.to(dtype))
    module.train()
    leaf = x.detach().clone().to(dtype).requires_grad_(True)
    outs, first = [], 0
    for count, keys in PIECES:
        mask = (torch.arange(count) >= keys)[None]
        outs.append(module(leaf[:, first:first + count].t()[:, None],
                           src_key_padding_mask=mask)[:, 0].t())
        first += count
    out = torch.cat(outs, dim=1)
    out.backward(upstream.to(dtype))
    return [out.detach().double(), leaf.grad.double()] + \
        [module.get_parameter(name).grad.double() for name in LAYER_NAMES]


@functools.lru_cache(maxsize=None)
def layer_want():
    return layer_torch(torch.float64), layer_torch(torch.float32)


def layer_leaves(requires_grad=True):
    x, upstream, parameters = layer_case()
    return [t.to(device()).requires_grad_(requires_grad)
            for t in (x,) + parameters], upstream.to(device())


def test_gradients_against_torch_with_a_padding_mask():
    exact, narrow = layer_want()
    leaves, upstream = layer_leaves()
    out = torch.ops.emphases_amd.encoder_layer_padded(
        *leaves, layer_cu(), torch.tensor(KEYS), HEADS)
    assert out.requires_grad and out.shape == leaves[0].shape
    out.backward(upstream)
    got = [out.detach()] + [leaf.grad for leaf in leaves]
    names = ('out', 'dx') + tuple('d ' + name for name in LAYER_NAMES)
    for name, value, want, rounded, leaf in zip(
            names, got, exact, narrow, [leaves[0]] + leaves):
        assert value.shape == leaf.shape and value.dtype == leaf.dtype
        check(f'encoder_layer_padded {name}', value, want, rounded)


def test_opcheck():
    leaves, _ = layer_leaves()
    cu = torch.tensor([0, 3, 70])
    leaves[0] = leaves[0][:, :70].detach().clone().requires_grad_(True)
    torch.library.opcheck(
        torch.ops.emphases_amd.encoder_layer_padded.default,
        (*leaves, cu, torch.tensor([2, 40]), HEADS),
        test_utils=('test_schema', 'test_autograd_registration',
                    'test_faketensor'))


def test_full_key_counts_are_the_plain_layer_after_an_update():
    results = []
    for name in ('encoder_layer', 'encoder_layer_padded'):
        leaves, upstream = layer_leaves()
        # (the ops tell a weight in training by its version since they first
        # saw it)
        assert not any([ops._weight_changes(leaf) for leaf in leaves[1:]])
        with torch.no_grad():
            leaves[7].add_(0)                  # what an optimizer step does
        assert ops._weight_changes(leaves[7])
        more = (torch.tensor(LENGTHS),) if name.endswith('padded') else ()
        out = getattr(torch.ops.emphases_amd, name)(
            *leaves, layer_cu(), *more, HEADS)
        out.backward(upstream)
        results.append([out.detach()] + [leaf.grad for leaf in leaves])
    for plain, padded in zip(*results):
        assert torch.equal(plain, padded)


@pytest.mark.parametrize('keys', [
    [1, 5, 64, 131], [0, 5, 64, 70], [1, 5, 64], [1, -1, 64, 70]])
def test_bad_key_counts_raise(keys):
    leaves, _ = layer_leaves(requires_grad=False)
    with pytest.raises(ValueError, match='key_counts'):
        torch.ops.emphases_amd.encoder_layer_padded(
            *leaves, layer_cu(), torch.tensor(keys), HEADS)
