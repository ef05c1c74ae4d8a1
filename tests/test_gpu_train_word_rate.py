"""The word-rate end of the training step on the MI355X, alone and on hard
layouts: `emph_loss_grad`, `emph_output_layer_backward` and
`emph_segment_broadcast` against torch CPU autograd in float64 on the `HARD`
layout of tests/word_rate_data.py (more than 512 packed word columns, segments
that abut, an utterance without words, a one-frame utterance, frames no word
covers), the whole step against the float64 restatement, and one trainer's
buffers under two layouts with the same leading dimensions.

Every output buffer starts as NaN and every kernel runs twice.  A bound is
4 x the error of the same computation in float32 on the CPU against float64,
both over max |want| (the project's standing allowance); the oracle is torch,
never the library.  Each figure is printed before it is asserted.
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

from emphases_amd import runtime, train, weights  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float('nan')
EINVAL, ERANGE = -1, -2
FRAMES = runtime.AXIS_FRAMES
# tests/test_gpu_ops_autograd.py, `REDUCE_*`: a one-frame word, a word across
# the 64-frame edge, a 130-frame word; no word; a one-frame word, then frames
# 0..4, 6..9, 30..59, 140..149 uncovered
REDUCE = word_rate_data.utterances(
    np.array([200, 40, 150]), np.array([3, 0, 5]),
    np.array([[0, 3, 70, 5, 10, 60, 68, 100],
              [1, 70, 200, 6, 30, 68, 100, 140]], dtype=np.int64))
LAYOUTS = {'hard': word_rate_data.HARD, 'reduce': REDUCE}


def nan(*shape):
    return torch.full(shape, NAN).cuda()


def bits(tensor):
    return tensor.contiguous().view(torch.int32)


def same(a, b):
    """Bit for bit, NaN included."""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def tables(name):
    """(plan, {name: device table}) of a layout with the 64-wide frame tiles,
    and `valid` / `inside`: the word / frame columns of an utterance."""
    plan = word_rate_data.plan_of(LAYOUTS[name])
    host, offsets = plan.pack_metadata([(FRAMES, 64)])
    meta = torch.from_numpy(host).cuda()
    found = {key: meta[start:start + size]
             for key, (start, size) in offsets.items()}
    found['tiles'] = found[('tiles', FRAMES, 64)]
    found['n_tiles'] = found['tiles'].numel() // runtime.TILE_FIELDS
    found['valid'] = torch.from_numpy(plan.word_segment >= 0)
    inside = torch.zeros(plan.ld_frames, dtype=torch.bool)
    for off, count in zip(plan.frame_off, plan.frames):
        inside[off:off + count] = True
    found['inside'] = inside
    return plan, found


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
# emph_loss_grad
###############################################################################


@pytest.mark.parametrize('loss', ['bce', 'mse'])
def test_loss_grad_alone(loss):
    plan, meta = tables('hard')
    ld, valid = plan.ld_words, meta['valid']
    columns = torch.from_numpy(plan.word_columns())
    assert int(valid.sum()) == plan.total_words == 354 == len(columns)
    generator = torch.Generator().manual_seed(5)
    logits = torch.randn(ld, generator=generator) * 2.
    targets = torch.rand(ld, generator=generator)
    # planted on both sides of column 256: saturated logits against either
    # target, exact 0 and 1 against ordinary logits
    spots = columns[[0, 15, 16, 47, 48, 200, 201, 280, 300, 340, 352, 353]]
    assert spots.min() < 256 < spots.max() and ld > 512
    logits[spots[:9]] = torch.tensor(
        [0., 30., -30., 100., -100., 100., -100., 30., -30.])
    targets[spots[:9]] = torch.tensor(
        [0.25, 0., 1., 0., 1., 1., 0., 0.75, 0.5])
    targets[spots[9:]] = torch.tensor([0., 1., 0.])
    logits[~valid] = NAN
    targets[~valid] = NAN

    def autograd(dtype):
        z = logits[valid].to(dtype).requires_grad_()
        function = torch.nn.functional.binary_cross_entropy_with_logits \
            if loss == 'bce' else torch.nn.functional.mse_loss
        value = function(z, targets[valid].to(dtype))
        value.backward()
        return value.detach().double(), z.grad.double()
    (want_loss, want), (_, narrow) = \
        autograd(torch.float64), autograd(torch.float32)
    lib = runtime.library()
    logits_device, targets_device = logits.cuda(), targets.cuda()
    results = []
    for _ in range(2):
        out, dlogit = nan(1), nan(ld)
        runtime.check(lib.emph_loss_grad(
            logits_device.data_ptr(), targets_device.data_ptr(),
            meta['word_segment'].data_ptr(), ld, plan.total_words,
            runtime.BCE_FORMS[loss], out.data_ptr(), dlogit.data_ptr(),
            runtime.stream()), 'emph_loss_grad')
        results.append((out.cpu(), dlogit.cpu()))
    assert same(results[0][0], results[1][0])
    assert same(results[0][1], results[1][1])
    out, dlogit = results[0]
    loss_error = abs(float(out) - float(want_loss)) / float(want_loss)
    print(f'loss_grad {loss}: loss {float(out):.9g} (float64 '
          f'{float(want_loss):.9g}), error {loss_error:.3g}')
    inside = report(f'loss_grad {loss} dlogit', dlogit[valid], want, narrow)
    assert loss_error <= 1e-6
    assert inside
    # exactly 0 on padding, as the header states
    assert torch.equal(dlogit[~valid], torch.zeros(int((~valid).sum())))


###############################################################################
# emph_output_layer_backward
###############################################################################


def run_output_backward(plan, meta, dlogit, x, weight, channels, ld):
    lib = runtime.library()
    dlogit, x, weight = dlogit.cuda(), x.cuda(), weight.cuda()
    results = []
    for _ in range(2):
        # (a row more than the kernel owns, and the 80 x 3 of the widest model)
        dweight, dbias, dx = nan(80 * 3), nan(2), nan(channels + 1, ld)
        runtime.check(lib.emph_output_layer_backward(
            dlogit.data_ptr(), x.data_ptr(), ld, weight.data_ptr(),
            meta['word_segment'].data_ptr(), channels, 3, plan.ld_words,
            dweight.data_ptr(), dbias.data_ptr(), dx.data_ptr(), ld,
            runtime.stream()), 'emph_output_layer_backward')
        results.append((dweight.cpu(), dbias.cpu(), dx.cpu()))
    for first, second in zip(*results):
        assert same(first, second)
    return results[0]


@pytest.mark.parametrize('channels', [80, 7])
def test_output_layer_backward_alone(channels):
    plan, meta = tables('hard')
    columns, valid = plan.ld_words, meta['valid']
    ld = columns + 16              # ldx = ld_dx > columns: a swapped stride shows
    generator = torch.Generator().manual_seed(channels)
    x = torch.randn(channels, ld, generator=generator)
    dlogit = torch.randn(columns, generator=generator)
    dlogit[~valid] = 0.            # what emph_loss_grad guarantees
    weight = torch.randn(1, channels, 3, generator=generator) / 15.
    dweight, dbias, dx = run_output_backward(
        plan, meta, dlogit, x, weight, channels, ld)

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
    taps = channels * 3
    got = (dweight[:taps].view(1, channels, 3), dbias[:1],
           dx[:channels, :columns][:, valid])
    inside = [
        report(f'output backward {channels} {name}', value,
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
    # what lies in the padding columns of x reaches nothing
    noisy = x.clone()
    noisy[:, :columns][:, ~valid] = NAN
    noisy[:, columns:] = NAN
    again = run_output_backward(plan, meta, dlogit, noisy, weight, channels, ld)
    for name, first, second in zip(
            ('dweight', 'dbias', 'dx'), (dweight, dbias, dx), again):
        assert same(first, second), name


###############################################################################
# emph_segment_broadcast
###############################################################################


def run_broadcast(plan, meta, dword, channels, mode):
    """(status, dx on the CPU) of two launches over a NaN-filled dx."""
    lib = runtime.library()
    dword = dword.cuda()
    results = []
    for _ in range(2):
        dx = nan(channels, plan.ld_frames)
        status = lib.emph_segment_broadcast(
            dword.data_ptr(), plan.ld_words, meta['bounds'].data_ptr(),
            dx.data_ptr(), plan.ld_frames, channels, meta['table'].data_ptr(),
            meta['tiles'].data_ptr(), meta['n_tiles'],
            runtime.REDUCTIONS[mode], runtime.stream())
        results.append((status, dx.cpu()))
    assert results[0][0] == results[1][0]
    assert same(results[0][1], results[1][1])
    return results[0]


@pytest.mark.parametrize('mode', ['sum', 'average'])
@pytest.mark.parametrize('channels', [80, 7])
@pytest.mark.parametrize('name', list(LAYOUTS))
def test_segment_broadcast_alone(name, channels, mode):
    plan, meta = tables(name)
    valid, inside = meta['valid'], meta['inside']
    generator = torch.Generator().manual_seed(channels)
    dword = torch.randn(channels, plan.ld_words, generator=generator)
    dword[:, ~valid] = NAN
    status, dx = run_broadcast(plan, meta, dword, channels, mode)
    assert status == 0, runtime.library().emph_last_error()

    def autograd(dtype):
        gradient = torch.zeros(channels, plan.ld_frames, dtype=dtype)
        for utterance, off, first in zip(
                LAYOUTS[name], plan.frame_off, plan.word_off):
            count = utterance.bounds.shape[1]
            if not count:
                continue
            x = torch.zeros(channels, utterance.frames, dtype=dtype,
                            requires_grad=True)
            pieces = [x[:, start:end] for start, end in utterance.bounds.T]
            torch.stack([
                piece.sum(dim=1) if mode == 'sum' else piece.mean(dim=1)
                for piece in pieces], dim=1).backward(
                    dword[:, first:first + count].to(dtype))
            gradient[:, off:off + utterance.frames] = x.grad
        return gradient
    exact, narrow = autograd(torch.float64), autograd(torch.float32)
    # columns between the utterances are left alone, the rest is finite
    assert torch.isnan(dx[:, ~inside]).all()
    assert torch.isfinite(dx[:, inside]).all()
    # frames no word covers, and the utterance without words: exactly 0
    covered = torch.zeros(plan.ld_frames, dtype=torch.bool)
    for utterance, off in zip(LAYOUTS[name], plan.frame_off):
        for start, end in utterance.bounds.T:
            covered[off + start:off + end] = True
    uncovered = inside & ~covered
    assert int(uncovered.sum()) == {'hard': 9 + 71, 'reduce': 2 + 40 + 49}[name]
    assert not dx[:, uncovered].any()
    if mode == 'sum':
        assert same(dx[:, inside], narrow[:, inside])
    else:
        assert report(f'broadcast {name} average {channels}', dx[:, inside],
                      exact[:, inside], narrow[:, inside])


@pytest.mark.parametrize('mode', ['max', 'center'])
def test_segment_broadcast_refuses_max_and_center(mode):
    plan, meta = tables('hard')
    dword = torch.randn(7, plan.ld_words)
    status, dx = run_broadcast(plan, meta, dword, 7, mode)
    assert status == EINVAL
    assert torch.isnan(dx).all()


###############################################################################
# Calls that launch nothing
###############################################################################


def test_refused_calls_return_their_codes_and_write_nothing():
    plan, meta = tables('hard')
    lib = runtime.library()
    ld, segment = plan.ld_words, meta['word_segment']
    source = torch.randn(80, ld).cuda()
    weight = torch.randn(1, 80, 3).cuda()
    out, dlogit = nan(1), nan(ld)
    for form, count, want in ((2, plan.total_words, EINVAL), (0, 0, EINVAL),
                              (0, ld + 1, EINVAL), (-1, 1, EINVAL)):
        assert lib.emph_loss_grad(
            source.data_ptr(), source[1].data_ptr(), segment.data_ptr(), ld,
            count, form, out.data_ptr(), dlogit.data_ptr(),
            runtime.stream()) == want, (form, count)
        assert lib.emph_last_error()
    dweight, dbias, dx = nan(80 * 3), nan(1), nan(80, ld)
    for channels, kernel_size, want in ((80, 5, ERANGE), (0, 3, EINVAL)):
        assert lib.emph_output_layer_backward(
            source[0].data_ptr(), source.data_ptr(), ld, weight.data_ptr(),
            segment.data_ptr(), channels, kernel_size, ld, dweight.data_ptr(),
            dbias.data_ptr(), dx.data_ptr(), ld,
            runtime.stream()) == want, (channels, kernel_size)
    torch.cuda.synchronize()
    for buffer in (out, dlogit, dweight, dbias, dx):
        assert torch.isnan(buffer).all()


###############################################################################
# The whole step
###############################################################################

# name -> (class, downsample_location)
TRAINERS = {
    'Trainer': (train.Trainer, 'intermediate'),
    'EncoderTrainer-loss': (train.EncoderTrainer, 'loss'),
    'EncoderTrainer-inference': (train.EncoderTrainer, 'inference'),
}


def make(kind, method='sum', loss='bce', precision='f32'):
    cls, location = TRAINERS[kind]
    return cls(word_rate_data.step_config(location, method, loss), gpu=0,
               seed=word_rate_data.SEED, precision=precision)


@pytest.mark.parametrize('kind,method,loss', [
    ('Trainer', 'sum', 'bce'), ('Trainer', 'average', 'mse'),
    ('EncoderTrainer-loss', 'sum', 'bce')])
def test_the_step_on_the_hard_layout_matches_the_restatement(
        kind, method, loss):
    state, want_loss, wanted, ref32 = word_rate_data.step_reference(
        TRAINERS[kind][1], method, loss)
    model = make(kind, method, loss)
    for name, value in model.state_dict().items():
        assert np.array_equal(value.numpy(), state[name]), name
    bound = 4. * ref32
    got_loss, gradients = model.loss_and_gradients(
        *word_rate_data.collate(word_rate_data.HARD, word_rate_data.SEED))
    label = f'step {kind} {method} {loss}'
    loss_error = abs(float(got_loss) - want_loss) / abs(want_loss)
    print(f'{label}: loss {float(got_loss):.9g} (float64 {want_loss:.9g}), '
          f'error {loss_error:.3g}, bound {bound:.3g}, ratio '
          f'{loss_error / bound:.2f}')
    assert set(gradients) == set(wanted) == \
        set(weights.parameter_shapes(model.config))
    worst = {}
    for name, want in wanted.items():
        got = gradients[name].cpu().double()
        assert got.shape == want.shape
        worst[name] = float((got - want).abs().max() / want.abs().max())
        print(f'{label} {name}: error {worst[name]:.3g}, bound {bound:.3g}, '
              f'ratio {worst[name] / bound:.2f}')
    assert loss_error <= bound
    missed = {name: error for name, error in worst.items()
              if not error <= bound}
    assert not missed, (missed, bound)


@pytest.mark.parametrize('precision', ['f32', 'bf16x3'])
@pytest.mark.parametrize('kind', list(TRAINERS))
def test_a_new_layout_in_reused_buffers_changes_nothing(kind, precision):
    """One trainer runs HARD, then REVERSED in the same buffers, which hold
    HARD's values in REVERSED's padding columns; a fresh trainer runs REVERSED
    alone.  (At 'inference' every utterance needs a word: HARD is refused
    there, and the pair with one word in utterance 2 takes its place.)"""
    first, second = word_rate_data.HARD, word_rate_data.REVERSED
    if kind == 'EncoderTrainer-inference':
        with pytest.raises(ValueError, match='an utterance has none'):
            make(kind).loss_and_gradients(
                *word_rate_data.collate(first, word_rate_data.SEED))
        first, second = \
            word_rate_data.HARD_WORDED, word_rate_data.REVERSED_WORDED
    plans = [word_rate_data.plan_of(layout) for layout in (first, second)]
    assert plans[0].ld_frames == plans[1].ld_frames
    assert plans[0].ld_words == plans[1].ld_words
    assert not np.array_equal(plans[0].word_off, plans[1].word_off)
    used, fresh = make(kind, precision=precision), \
        make(kind, precision=precision)
    used.loss_and_gradients(*word_rate_data.collate(first, word_rate_data.SEED))
    buffers = dict(used._workspace)
    # ... and now hold the first layout's values between the second's utterances
    outside = torch.ones(plans[1].ld_frames, dtype=torch.bool)
    for off, count in zip(plans[1].frame_off, plans[1].frames):
        outside[off:off + count] = False
    (kept,) = buffers.values()
    assert kept['frames'][:, :, outside.cuda()].any()
    batch = word_rate_data.collate(second, word_rate_data.SEED)
    got_loss, got = used.loss_and_gradients(*batch)
    # the cached buffers really were reused
    assert len(used._workspace) == 1 and all(
        used._workspace[key] is value for key, value in buffers.items())
    want_loss, want = fresh.loss_and_gradients(*batch)
    assert float(want_loss) > 0. and np.isfinite(float(want_loss))
    assert torch.equal(got_loss, want_loss), (got_loss, want_loss)
    for name in want:
        assert torch.isfinite(want[name]).all() and want[name].any(), name
        assert torch.equal(got[name], want[name]), name
    assert torch.equal(used.step(*batch), fresh.step(*batch))
    assert used.steps == fresh.steps == 1
    for name in ('parameters', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(used, name), getattr(fresh, name)), name
    assert not torch.equal(fresh.exp_avg, torch.zeros_like(fresh.exp_avg))
