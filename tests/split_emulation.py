"""What precision='bf16x3' of the training step computes, with exact
accumulation: the convolution model in float64 (pure torch on the CPU, no
reference, no GPU) whose Conv1d(80, 80, 3) layers on the frame axis multiply
as the HIP kernels do -

    hi = bf16(a)    lo = bf16(a - hi)        a: the float32 rounding of an operand,
                                             both rounded to nearest, a - hi in float32
    a . b  ->  hi_a hi_b + hi_a lo_b + lo_a hi_b

in the forward pass, in the data gradient and in the weight gradient (a custom
`autograd.Function`); everything else - word-rate layers, output layer, word
sums, loss, the bias gradient, the accumulation itself - is exact float64.
The distance of its gradients from plain float64 is what the three-product
arithmetic costs; the tests add what float32 accumulation costs (measured on
the reference) and the project's factor 4.

Every utterance is trained alone with weight n_i / N and the bce loss, as
tests/golden/generate_train.py runs the reference.
"""
import collections
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKPOINT = os.path.join(ROOT, 'emphases_amd', 'assets', 'checkpoint.npz')
LAYERS = 6
F = torch.nn.functional


def pieces(value):
    """(hi, lo) of a float64 tensor, as float64."""
    rounded = value.detach().to(torch.float32)
    high = rounded.to(torch.bfloat16).to(torch.float32)
    low = (rounded - high).to(torch.bfloat16).to(torch.float32)
    return high.double(), low.double()


def product(function, a, b, split):
    """function(a, b), bilinear, as three products of pieces (or exactly)."""
    if not split:
        return function(a.detach(), b.detach())
    (a_high, a_low), (b_high, b_low) = pieces(a), pieces(b)
    return function(a_high, b_high) + function(a_high, b_low) + \
        function(a_low, b_high)


def forward_product(x, weight, split=True):
    """Conv1d(., ., 3, 'same') without bias of x [1, C, T]."""
    return product(lambda a, b: F.conv1d(a, b, padding=1), x, weight, split)


def data_gradient(dy, weight, split=True):
    return product(
        lambda a, b: F.conv_transpose1d(a, b, padding=1), dy, weight, split)


def weight_gradient(dy, x, split=True):
    """dW[co][ci][j] = sum_t dy[co][t] x[ci][t + j - 1] of dy, x [1, C, T]."""
    shape = (dy.shape[1], x.shape[1], 3)
    return product(
        lambda a, b: torch.nn.grad.conv1d_weight(b, shape, a, padding=1),
        dy, x, split)


class SplitConv(torch.autograd.Function):
    """Conv1d(80, 80, 3, 'same') of a layer in scope."""

    @staticmethod
    def forward(ctx, x, weight, bias, split):
        ctx.save_for_backward(x, weight)
        ctx.split = split
        return forward_product(x, weight, split) + bias[None, :, None]

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        return (data_gradient(dy, weight, ctx.split),
                weight_gradient(dy, x, ctx.split), dy.sum(dim=(0, 2)), None)


def load_state(path=CHECKPOINT):
    """The shipped convolution model as float64 leaf tensors."""
    with np.load(path) as archive:
        return collections.OrderedDict(
            (name, torch.from_numpy(archive[name].astype(np.float64))
             .requires_grad_()) for name in archive.files)


def in_scope(name, state):
    """The Conv1d(80, 80, 3) layers on the frame axis."""
    return (name == 'input_layer' or name.startswith('frame_encoder.')) and \
        tuple(state[f'{name}.weight'].shape) == (80, 80, 3)


def logits(state, features, bounds, split=True):
    """The model's word logits [W] of one utterance: features [80, T]
    (numpy), bounds [2, W]."""
    def conv(name, x, relu):
        weight, bias = state[f'{name}.weight'], state[f'{name}.bias']
        if in_scope(name, state):
            y = SplitConv.apply(x, weight, bias, split)
        else:
            y = F.conv1d(x, weight, bias, padding=1)
        return torch.relu(y) if relu else y
    x = torch.from_numpy(np.asarray(features, dtype=np.float64))[None]
    x = conv('input_layer', x, False)
    for i in range(LAYERS):
        x = conv(f'frame_encoder.{2 * i}', x, True)
    x = torch.stack(
        [x[0, :, int(s):int(e)].sum(dim=1) for s, e in np.asarray(bounds).T],
        dim=1)[None]
    for i in range(LAYERS):
        x = conv(f'word_decoder.{2 * i}', x, True)
    return conv('output_layer', x, False)[0, 0]


def loss_and_gradients(state, items, split=True):
    """(loss, {name: gradient}) as float64 numpy: every utterance of `items`
    ((features, bounds, targets)) alone, weighted n_i / N, bce."""
    for parameter in state.values():
        parameter.grad = None
    total_words = sum(len(item[2]) for item in items)
    total = 0.
    for features, bounds, targets in items:
        target = torch.from_numpy(np.asarray(targets, dtype=np.float64))
        value = F.binary_cross_entropy_with_logits(
            logits(state, features, bounds, split), target) * \
            (len(targets) / total_words)
        value.backward()
        total += float(value.detach())
    return total, {name: parameter.grad.numpy().copy()
                   for name, parameter in state.items()}


def adam_losses(items, updates=5, split=True):
    """The losses of steps 0 .. updates of `updates` Adam steps
    (`torch.optim.Adam` defaults, float64 state) from the shipped model."""
    state = load_state()
    optimizer = torch.optim.Adam(list(state.values()))
    losses = []
    for step in range(updates + 1):
        losses.append(loss_and_gradients(state, items, split)[0])
        if step < updates:
            optimizer.step()
    return np.array(losses, dtype=np.float64)


def items_of(golden, case):
    """The utterances of a case of tests/golden/train.npz."""
    frames, words = golden[f'{case}/frames'], golden[f'{case}/words']
    frame_first, word_first = np.cumsum(frames) - frames, np.cumsum(words) - words
    return [(golden[f'{case}/features'][:, f0:f0 + f],
             golden[f'{case}/bounds'][:, w0:w0 + w],
             golden[f'{case}/targets'][w0:w0 + w])
            for f0, f, w0, w in zip(frame_first, frames, word_first, words)]
