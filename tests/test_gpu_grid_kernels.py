"""The three kernels of csrc/grid.hip on the MI355X, alone:
`emph_output_layer_backward_any` on the `HARD` layout of
tests/word_rate_data.py against torch CPU autograd in float64,
`emph_activation_dropout` and `emph_activation_dropout_gradient` against the
mask specification of emphases_amd/train/dropout.py and float64 torch, and
each against the existing entry point whose bits it promises.

A bound is 4 x the error of the same computation in float32 on the CPU
against float64, both over max |want| (the project's standing allowance).
Every output buffer starts as NaN; each figure is printed before it is
asserted.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import word_rate_data  # noqa: E402

from emphases_amd import runtime  # noqa: E402
from emphases_amd.train import dropout as spec  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float('nan')
EINVAL, ERANGE = -1, -2
ACTIVATIONS = ('relu', 'gelu', 'silu', 'leaky_relu')
PROBABILITIES = (0., 0.1, 0.5)
SEED, STREAM, STEP = (1 << 40) + 12345, 3, 7
ROWS, COLUMNS = 80, 128
TORCH_ACTIVATIONS = {
    'relu': torch.nn.functional.relu, 'gelu': torch.nn.functional.gelu,
    'silu': torch.nn.functional.silu,
    'leaky_relu': torch.nn.functional.leaky_relu}


def nan(*shape):
    return torch.full(shape, NAN).cuda()


def bits(tensor):
    return tensor.contiguous().view(torch.int32)


def same(a, b):
    """Bit for bit, NaN included."""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def report(label, got, want, narrow):
    """Print error and bound of a tensor, return whether it is inside."""
    got, want, narrow = got.double(), want.double(), narrow.double()
    scale = want.abs().max()
    allowed = 4. * float((narrow - want).abs().max() / scale)
    error = float((got - want).abs().max() / scale)
    ratio = error / allowed if allowed else float('inf') if error else 0.
    print(f'{label}: error {error:.3g}, bound {allowed:.3g}, '
          f'ratio {ratio:.2f}')
    return error <= allowed


###############################################################################
# emph_output_layer_backward_any
###############################################################################


@functools.lru_cache(maxsize=None)
def hard():
    plan = word_rate_data.plan_of(word_rate_data.HARD)
    segment = torch.from_numpy(plan.word_segment).cuda()
    return plan, segment, torch.from_numpy(plan.word_segment >= 0)


def run_head(entry, dlogit, x, weight, channels, kernel_size, ld):
    plan, segment, _ = hard()
    lib = runtime.library()
    dlogit, x, weight = dlogit.cuda(), x.cuda(), weight.cuda()
    results = []
    for _ in range(2):
        # (a row and a tap more than the kernel owns)
        dweight, dbias = nan(channels * kernel_size + 1), nan(2)
        dx = nan(channels + 1, ld)
        runtime.check(getattr(lib, entry)(
            dlogit.data_ptr(), x.data_ptr(), ld, weight.data_ptr(),
            segment.data_ptr(), channels, kernel_size, plan.ld_words,
            dweight.data_ptr(), dbias.data_ptr(), dx.data_ptr(), ld,
            runtime.stream()), entry)
        results.append((dweight.cpu(), dbias.cpu(), dx.cpu()))
    for first, second in zip(*results):
        assert same(first, second)
    return results[0]


def head_case(channels, kernel_size):
    plan, _, valid = hard()
    columns = plan.ld_words
    ld = columns + 16              # ldx = ld_dx > columns: a swapped stride shows
    generator = torch.Generator().manual_seed(100 * channels + kernel_size)
    x = torch.randn(channels, ld, generator=generator)
    x[:, :columns][:, ~valid] = NAN
    x[:, columns:] = NAN
    # dbias is ONE sum of the 354 valid dlogit.  The float32 error of a single
    # sum is a random draw that can land next to 0, and 4 x such a draw bounds
    # nothing; so dlogit is drawn from the multiples of 2^-10 in [-4, 4), whose
    # partial sums are exact in float32 in any order (354 x 4 x 2^10 < 2^24):
    # the float32 reference has error 0 and dbias must be exact.  dweight and
    # dx multiply by x and weight and round as ever.
    dlogit = torch.randint(
        -4096, 4096, (columns,), generator=generator).float() / 1024.
    dlogit[~valid] = 0.            # what emph_loss_grad guarantees
    weight = torch.randn(1, channels, kernel_size, generator=generator) / 15.
    return x, dlogit, weight, ld


@pytest.mark.parametrize('kernel_size', [1, 3, 5, 7])
@pytest.mark.parametrize('channels', [16, 80, 128])
def test_output_layer_backward_any(channels, kernel_size):
    plan, _, valid = hard()
    columns = plan.ld_words
    assert min(w for w in plan.words if w) < 7 < max(plan.words)
    x, dlogit, weight, ld = head_case(channels, kernel_size)
    dweight, dbias, dx = run_head(
        'emph_output_layer_backward_any', dlogit, x, weight, channels,
        kernel_size, ld)

    def autograd(dtype):
        w = weight.to(dtype).requires_grad_()
        b = torch.zeros(1, dtype=dtype, requires_grad=True)
        gradient = torch.zeros(channels, columns, dtype=dtype)
        for off, count in zip(plan.word_off, plan.words):
            if not count:
                continue
            piece = x[None, :, off:off + count].to(dtype).requires_grad_()
            out = torch.nn.functional.conv1d(piece, w, b, padding='same')
            out.backward(dlogit[None, None, off:off + count].to(dtype))
            gradient[:, off:off + count] = piece.grad[0]
        return w.grad.double(), b.grad.double(), gradient.double()
    exact, rounded = autograd(torch.float64), autograd(torch.float32)
    taps = channels * kernel_size
    got = (dweight[:taps].view(1, channels, kernel_size), dbias[:1],
           dx[:channels, :columns][:, valid])
    label = f'head backward c{channels} k{kernel_size}'
    inside = [
        report(f'{label} {name}', value,
               want[..., valid] if name == 'dx' else want,
               narrow[..., valid] if name == 'dx' else narrow)
        for name, value, want, narrow in zip(
            ('dweight', 'dbias', 'dx'), got, exact, rounded)]
    assert all(inside), inside
    # 0 on padding columns, nothing written past what the kernel owns
    assert not dx[:channels, :columns][:, ~valid].any()
    assert torch.isnan(dx[:channels, columns:]).all()
    assert torch.isnan(dx[channels]).all()
    assert torch.isnan(dweight[taps:]).all() and torch.isnan(dbias[1]).all()


def test_output_layer_backward_any_at_3_is_the_existing_entry():
    x, dlogit, weight, ld = head_case(80, 3)
    new = run_head('emph_output_layer_backward_any', dlogit, x, weight, 80, 3,
                   ld)
    old = run_head('emph_output_layer_backward', dlogit, x, weight, 80, 3, ld)
    for name, first, second in zip(('dweight', 'dbias', 'dx'), new, old):
        assert same(first, second), name


def test_output_layer_backward_any_refusals_write_nothing():
    plan, segment, _ = hard()
    lib = runtime.library()
    ld = plan.ld_words
    dlogit, x, weight = nan(ld), nan(16, ld), nan(16 * 9)
    dweight, dbias, dx = nan(16 * 9), nan(1), nan(16, ld)

    def call(channels=16, kernel_size=3, columns=ld):
        return lib.emph_output_layer_backward_any(
            dlogit.data_ptr(), x.data_ptr(), ld, weight.data_ptr(),
            segment.data_ptr(), channels, kernel_size, columns,
            dweight.data_ptr(), dbias.data_ptr(), dx.data_ptr(), ld,
            runtime.stream())
    assert call(kernel_size=2) == ERANGE and call(kernel_size=9) == ERANGE
    assert call(channels=0) == EINVAL and call(channels=1025) == EINVAL
    assert call(columns=ld + 1) == EINVAL
    torch.cuda.synchronize()
    for buffer in (dweight, dbias, dx):
        assert torch.isnan(buffer).all()


###############################################################################
# emph_activation_dropout and emph_activation_dropout_gradient
###############################################################################


@functools.lru_cache(maxsize=None)
def values():
    """z [80, 128] with the planted values, and the upstream gradient."""
    generator = torch.Generator().manual_seed(11)
    z = torch.randn(ROWS, COLUMNS, generator=generator) * 2.
    planted = torch.tensor([0., 1e-6, -1e-6, 10., -10., -100., NAN, -0.])
    z.view(-1)[torch.arange(len(planted)) * 397 + 5] = planted
    g = torch.randn(ROWS, COLUMNS, generator=generator)
    return z, g, torch.isnan(z)


def kept_mask(p):
    return torch.from_numpy(spec.keep_mask(
        SEED, STREAM, STEP, ROWS * COLUMNS, p)).view(ROWS, COLUMNS)


def forward(z, y, activation, p, seed=SEED, stream=STREAM, step=STEP):
    return runtime.library().emph_activation_dropout(
        z.data_ptr(), y.data_ptr(), z.numel(), runtime.ACTIVATIONS[activation],
        p, seed, stream, step, runtime.stream())


def backward(source, gradient, activation, p, count=None):
    return runtime.library().emph_activation_dropout_gradient(
        source.data_ptr(), gradient.data_ptr(),
        gradient.numel() if count is None else count,
        runtime.ACTIVATIONS[activation], p, SEED, STREAM, STEP,
        runtime.stream())


def scale_of(p, dtype):
    return float(spec.scale(p)) if dtype == torch.float32 else \
        1. / (1. - spec.probability(p))


@pytest.mark.parametrize('p', PROBABILITIES)
@pytest.mark.parametrize('activation', ACTIVATIONS)
def test_activation_dropout(activation, p):
    z, _, is_nan = values()
    kept = kept_mask(p)
    if p == 0.:
        assert kept.all()
    else:
        assert abs(float((~kept).float().mean()) - p) < 0.02
    device_z = z.cuda()
    y = nan(ROWS, COLUMNS)
    runtime.check(forward(device_z, y, activation, p),
                  'emph_activation_dropout')
    again = nan(ROWS, COLUMNS)
    runtime.check(forward(device_z, again, activation, p),
                  'emph_activation_dropout')
    in_place = device_z.clone()
    runtime.check(forward(in_place, in_place, activation, p),
                  'emph_activation_dropout')
    assert same(y, again) and same(y, in_place)
    assert same(device_z, z.cuda())
    y = y.cpu()
    # the dropped set is the specification's, +0 there, the NaN included
    assert torch.equal(bits(y[~kept]), torch.zeros(
        int((~kept).sum()), dtype=torch.int32))

    def reference(dtype):
        return TORCH_ACTIVATIONS[activation](z.to(dtype)) * scale_of(p, dtype)
    compare = kept & ~is_nan
    inside = report(f'activation_dropout {activation} p={p}', y[compare],
                    reference(torch.float64)[compare],
                    reference(torch.float32)[compare])
    assert inside
    if bool((kept & is_nan).any()) and activation != 'relu':
        assert torch.isnan(y[kept & is_nan]).all()
    # another stream, step or seed: another mask
    if p > 0.:
        for change in (dict(stream=STREAM + 1), dict(step=STEP + 1),
                       dict(seed=SEED + (1 << 32))):
            other = nan(ROWS, COLUMNS)
            runtime.check(forward(device_z, other, activation, p, **change),
                          'emph_activation_dropout')
            assert not torch.equal(other.cpu() == 0, y == 0), change


def test_activation_dropout_none_is_a_copy_or_emph_dropout():
    z, _, _ = values()
    device_z = z.cuda()
    y = nan(ROWS, COLUMNS)
    runtime.check(forward(device_z, y, None, 0.), 'emph_activation_dropout')
    assert same(y, device_z)
    for p in (0.1, 0.5):
        runtime.check(forward(device_z, y, None, p), 'emph_activation_dropout')
        want = device_z.clone()
        runtime.check(runtime.library().emph_dropout(
            want.data_ptr(), want.numel(), 0, p, SEED, STREAM, STEP,
            runtime.stream()), 'emph_dropout')
        assert same(y, want)


@pytest.mark.parametrize('activation', ACTIVATIONS)
def test_activation_dropout_at_p0_is_the_epilogue_of_conv1d(activation):
    """The same pre-activation through `emph_conv1d`'s fused epilogue and
    through `emph_conv1d` without activation + `emph_activation_dropout`."""
    layout = word_rate_data.utterances(
        np.array([200, 77]), np.array([1, 1]),
        np.array([[0, 0], [200, 77]], dtype=np.int64))
    plan = word_rate_data.plan_of(layout)
    host, offsets = plan.pack_metadata([(runtime.AXIS_FRAMES, 64)])
    meta = torch.from_numpy(host).cuda()
    start, size = offsets[('tiles', runtime.AXIS_FRAMES, 64)]
    tiles = meta[start:start + size]
    ld = plan.ld_frames
    generator = torch.Generator().manual_seed(3)
    x = (torch.randn(80, ld, generator=generator) * 3.).cuda()
    weight = torch.randn(80, 80, 3, generator=generator) / 5.
    bias = torch.randn(80, generator=generator).cuda()
    pack = torch.from_numpy(runtime.conv_pack(weight.numpy())).cuda()
    lib = runtime.library()

    def conv(act):
        y = torch.zeros(80, ld).cuda()
        runtime.check(lib.emph_conv1d(
            x.data_ptr(), ld, y.data_ptr(), ld, pack.data_ptr(),
            bias.data_ptr(), 80, 80, 3, runtime.ACTIVATIONS[act],
            tiles.data_ptr(), tiles.numel() // runtime.TILE_FIELDS, 64, 0,
            runtime.stream()), 'emph_conv1d')
        return y
    fused, pre = conv(activation), conv(None)
    two = nan(80, ld)
    runtime.check(forward(pre, two, activation, 0.), 'emph_activation_dropout')
    inside = torch.zeros(ld, dtype=torch.bool)
    for off, count in zip(plan.frame_off, plan.frames):
        inside[off:off + count] = True
    assert float(pre[:, inside.cuda()].abs().max()) > 10.
    assert float(pre[:, inside.cuda()].min()) < -10.
    assert same(fused[:, inside.cuda()], two[:, inside.cuda()])


@pytest.mark.parametrize('p', PROBABILITIES)
@pytest.mark.parametrize('activation', ACTIVATIONS)
def test_activation_dropout_gradient(activation, p):
    z, g, is_nan = values()
    kept = kept_mask(p)
    device_z = z.cuda()
    y = nan(ROWS, COLUMNS)
    runtime.check(forward(device_z, y, activation, p),
                  'emph_activation_dropout')
    # what emph_activation_gradient reads
    source = y if activation in ('relu', 'leaky_relu') else device_z
    got = g.cuda()
    runtime.check(backward(source, got, activation, p),
                  'emph_activation_dropout_gradient')
    again = g.cuda()
    runtime.check(backward(source, again, activation, p),
                  'emph_activation_dropout_gradient')
    assert same(got, again)
    got = got.cpu()
    assert not got[~kept].any()

    def reference(dtype):
        wide = z.detach().clone().to(dtype).requires_grad_()
        TORCH_ACTIVATIONS[activation](wide).backward(
            g.to(dtype) * scale_of(p, dtype))
        return wide.grad
    compare = kept & ~is_nan
    inside = report(f'activation_dropout_gradient {activation} p={p}',
                    got[compare], reference(torch.float64)[compare],
                    reference(torch.float32)[compare])
    assert inside

    if p == 0.:
        want = g.cuda()
        runtime.check(runtime.library().emph_activation_gradient(
            source.data_ptr(), want.data_ptr(), want.numel(),
            runtime.ACTIVATIONS[activation], runtime.stream()),
            'emph_activation_gradient')
        assert same(got.cuda(), want)


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_relu_gradient_is_activation_dropout_backward(p):
    """Fed the output that `emph_dropout` leaves behind a ReLU."""
    z, g, _ = values()
    lib = runtime.library()
    y = torch.relu(z).cuda()
    runtime.check(lib.emph_dropout(
        y.data_ptr(), y.numel(), 0, p, SEED, STREAM, STEP, runtime.stream()),
        'emph_dropout')
    fused = nan(ROWS, COLUMNS)
    runtime.check(forward(z.cuda(), fused, 'relu', p),
                  'emph_activation_dropout')
    finite = ~torch.isnan(z) & (z != 0)       # (the sign of relu(-0) is free)
    assert same(y.cpu()[finite], fused.cpu()[finite])
    got, want = g.cuda(), g.cuda()
    runtime.check(backward(y, got, 'relu', p),
                  'emph_activation_dropout_gradient')
    runtime.check(lib.emph_activation_dropout_backward(
        y.data_ptr(), want.data_ptr(), want.numel(),
        runtime.ACTIVATIONS['relu'], p, runtime.stream()),
        'emph_activation_dropout_backward')
    assert same(got, want)
    assert int((got != 0).sum()) > 0


def test_elementwise_refusals_write_nothing():
    a, b = nan(ROWS * COLUMNS + 4), nan(ROWS * COLUMNS + 4)
    count = ROWS * COLUMNS

    def calls(**changes):
        arguments = dict(a=a, b=b, count=count, p=0.1)
        arguments.update(changes)
        lib = runtime.library()
        return [entry(
            arguments['a'].data_ptr(), arguments['b'].data_ptr(),
            arguments['count'], runtime.ACTIVATIONS['gelu'], arguments['p'],
            SEED, STREAM, STEP, runtime.stream())
            for entry in (lib.emph_activation_dropout,
                          lib.emph_activation_dropout_gradient)]
    assert calls(a=a[1:]) == [EINVAL, EINVAL]
    assert calls(b=b[2:]) == [EINVAL, EINVAL]
    assert calls(count=count - 2) == [EINVAL, EINVAL]
    assert calls(p=1.) == [EINVAL, EINVAL]
    assert calls(count=0) == [0, 0]
    torch.cuda.synchronize()
    assert torch.isnan(a).all() and torch.isnan(b).all()
