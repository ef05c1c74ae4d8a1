"""`emphases_amd.train` on the MI355X: gradients and losses against the
unmodified reference in float64 (tests/golden/train.npz, written by
tests/golden/generate_train.py), determinism, the weight-gradient and Adam
kernels alone against float64 oracles, five Adam steps, and the checkpoint
round trip.

Every bound is 4 x the error of the same computation in float32 on the CPU
(the project's standing allowance, `test_gpu_frontend`): the reference's own
for the goldens (`ref32_error`), torch's for the kernels alone (computed
here).  Each figure is printed before it is asserted.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import core as api  # noqa: E402
from emphases_amd import engine as engine_module  # noqa: E402
from emphases_amd import runtime, session, synth, train, weights  # noqa: E402

pytestmark = pytest.mark.gpu

_TRAINERS = {}


def trainer(case='ragged'):
    """One trainer per configuration, on the shipped checkpoint; the tests
    that update parameters build their own."""
    overrides = tuple(sorted(train_data.VARIANTS.get(case, {}).items()))
    if overrides not in _TRAINERS:
        _TRAINERS[overrides] = train.Trainer(
            config=emphases_amd.Config(**dict(overrides)),
            checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0)
    return _TRAINERS[overrides]


@pytest.mark.parametrize('case', ['ragged', 'uniform', 'mse', 'average'])
def test_gradients_match_the_reference(case):
    golden = train_data.golden()
    bound = 4. * float(golden[f'{case}/ref32_error'])
    loss, gradients = trainer(case).loss_and_gradients(
        *train_data.collated(case))
    assert loss.is_cuda and loss.dim() == 0
    want_loss = float(golden[f'{case}/loss'])
    loss_error = abs(float(loss) - want_loss) / abs(want_loss)
    print(f'{case}: loss {float(loss):.9g} (reference {want_loss:.9g}), '
          f'error {loss_error:.3g}, bound {bound:.3g}')
    wanted = train_data.gradients(case)
    assert wanted and set(wanted) <= set(gradients)
    if case in ('ragged', 'uniform'):
        assert set(wanted) == set(gradients)
    worst = {}
    for name, want in wanted.items():
        got = gradients[name].cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        worst[name] = np.abs(got - want).max() / np.abs(want).max()
        print(f'{case}: {name} error {worst[name]:.3g} '
              f'({worst[name] / bound:.2f} of the bound)')
    assert loss_error <= bound
    missed = {name: error for name, error in worst.items() if not error <= bound}
    assert not missed, (missed, bound)


def test_same_batch_twice_is_bitwise_the_same():
    batch = train_data.collated('ragged')
    first_loss, first = trainer().loss_and_gradients(*batch)
    second_loss, second = trainer().loss_and_gradients(*batch)
    assert torch.equal(first_loss, second_loss)
    for name in first:
        assert torch.equal(first[name], second[name]), name


@pytest.mark.parametrize('c_in', [80, 83])
def test_conv_weight_grad_alone(c_in):
    """4 096 positions in 5 uneven segments against conv1d autograd in float64
    on the CPU; what surrounds the segments is noise, not zeros."""
    frames = [1000, 37, 2047, 12, 1000]
    assert sum(frames) == 4096
    bounds = torch.zeros(len(frames), 2, 1, dtype=torch.long)
    bounds[:, 1, 0] = torch.tensor(frames)
    plan = api._packed_plan(frames, bounds, [1] * len(frames))
    tiles = torch.from_numpy(plan.tiles(runtime.AXIS_FRAMES, 64)).cuda()
    n_tiles = tiles.shape[0]
    lib = runtime.library()
    parts = int(lib.emph_conv_weight_grad_parts(n_tiles))
    assert parts >= 3
    generator = torch.Generator().manual_seed(c_in)
    ld = plan.ld_frames
    dy = torch.randn(80, ld, generator=generator)
    x = torch.randn(c_in, ld, generator=generator)
    slabs = torch.full((parts * (80 * 3 * c_in + 80),), float('nan')).cuda()
    dweight = torch.full((80, c_in, 3), float('nan')).cuda()
    dbias = torch.full((80,), float('nan')).cuda()
    dy_device, x_device = dy.cuda(), x.cuda()
    for launch in range(2):
        runtime.check(lib.emph_conv_weight_grad(
            dy_device.data_ptr(), ld, x_device.data_ptr(), ld, c_in, 80, 3,
            tiles.data_ptr(), n_tiles, 64, slabs.data_ptr(),
            dweight.data_ptr(), dbias.data_ptr(), runtime.stream()),
            'emph_conv_weight_grad')
        if launch == 0:
            first = (dweight.clone(), dbias.clone())
    assert torch.equal(first[0], dweight) and torch.equal(first[1], dbias)

    def autograd(dtype):
        weight = torch.zeros(80, c_in, 3, dtype=dtype, requires_grad=True)
        bias = torch.zeros(80, dtype=dtype, requires_grad=True)
        for off, count in zip(plan.frame_off, frames):
            out = torch.nn.functional.conv1d(
                x[None, :, off:off + count].to(dtype), weight, bias,
                padding='same')
            out.backward(dy[None, :, off:off + count].to(dtype))
        return weight.grad.double(), bias.grad.double()
    exact = autograd(torch.float64)
    rounded = autograd(torch.float32)
    for name, got, want, narrow in zip(
            ('weight', 'bias'), (dweight, dbias), exact, rounded):
        scale = want.abs().max()
        allowed = 4. * float((narrow - want).abs().max() / scale)
        error = float((got.cpu().double() - want).abs().max() / scale)
        print(f'c_in {c_in} d{name}: error {error:.3g}, bound {allowed:.3g}')
        assert error <= allowed, (name, error, allowed)


def test_adam_step_alone():
    """Three consecutive updates of 4 096 elements, gradients that are zero or
    log-uniform in 1e-12..1e-1, against Adam in float64."""
    count, lr, betas, eps = 4096, 1e-3, (0.9, 0.999), 1e-8
    generator = torch.Generator().manual_seed(11)
    start = torch.randn(count, generator=generator)
    steps = []
    for _ in range(3):
        magnitude = 10. ** (torch.rand(count, generator=generator) * 11. - 12.)
        sign = torch.where(torch.rand(count, generator=generator) < 0.5, -1., 1.)
        gradient = (magnitude * sign).float()
        gradient[torch.rand(count, generator=generator) < 0.1] = 0.
        steps.append(gradient)
    steps[1][:64] = 0.                       # zero after non-zero ...
    steps[0][64:128] = 0.                    # ... and zero from the start
    steps[1][64:128] = 0.
    steps[2][64:128] = 0.

    def run_torch(dtype):
        parameter = torch.nn.Parameter(start.to(dtype).clone())
        optimizer = torch.optim.Adam([parameter], lr=lr, betas=betas, eps=eps)
        for gradient in steps:
            parameter.grad = gradient.to(dtype).clone()
            optimizer.step()
        state = optimizer.state[parameter]
        return (parameter.detach().double(), state['exp_avg'].double(),
                state['exp_avg_sq'].double())
    exact = run_torch(torch.float64)
    rounded = run_torch(torch.float32)
    lib = runtime.library()
    parameter = start.clone().cuda()
    exp_avg, exp_avg_sq = torch.zeros(count).cuda(), torch.zeros(count).cuda()
    for index, gradient in enumerate(steps, 1):
        gradient = gradient.cuda()
        runtime.check(lib.emph_adam_step(
            parameter.data_ptr(), gradient.data_ptr(), exp_avg.data_ptr(),
            exp_avg_sq.data_ptr(), count, betas[0], betas[1],
            lr / (1. - betas[0] ** index), (1. - betas[1] ** index) ** 0.5,
            eps, runtime.stream()), 'emph_adam_step')
    assert torch.equal(parameter[64:128].cpu(), start[64:128])
    for name, got, want, narrow in zip(
            ('parameter', 'exp_avg', 'exp_avg_sq'),
            (parameter, exp_avg, exp_avg_sq), exact, rounded):
        scale = want.abs().max()
        allowed = 4. * float((narrow - want).abs().max() / scale)
        error = float((got.cpu().double() - want).abs().max() / scale)
        print(f'adam {name}: error {error:.3g}, bound {allowed:.3g}')
        assert error <= allowed, (name, error, allowed)


def test_five_steps_follow_the_reference():
    """Five Adam steps from the shipped checkpoint on `ragged` against the three
    recorded reference trajectories (float32, float64, float32 with the
    utterances in reverse order).  Step 0 is held to the gradient test's
    bound, every later step to 4 x the spread of the three at that step.  At
    step 3 they agree to 4e-09, a fifteenth of a float32 ulp of the loss, so
    that bound asks for a correctly rounded loss: `emph_loss_grad` sums in
    double and rounds once."""
    golden = train_data.golden()
    runs = np.stack([golden[f'adam/{name}'] for name in (
        'float32', 'float64', 'float32_reversed')])
    batch = train_data.collated('ragged')
    model = train.Trainer(checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0)
    prepared = model.prepare(*batch)
    losses = [model.step(prepared) for _ in range(5)]
    losses.append(model.loss_and_gradients(prepared)[0])
    losses = np.array([float(loss) for loss in losses], dtype=np.float64)
    spread = runs.max(axis=0) - runs.min(axis=0)
    for step, loss in enumerate(losses):
        print(f'step {step}: loss {loss:.9g}, reference {runs[1, step]:.9g}, '
              f'off by {np.abs(runs[:, step] - loss).max():.3g}, '
              f'spread of the references {spread[step]:.3g}')
    assert model.steps == 5
    first = 4. * float(golden['ragged/ref32_error'])
    assert abs(losses[0] - runs[1, 0]) / runs[1, 0] <= first
    assert np.all(np.diff(losses) < 0), losses
    for step in range(1, 6):
        assert np.abs(runs[:, step] - losses[step]).max() <= \
            4. * spread[step], (step, losses[step], runs[:, step])


def test_checkpoint_round_trip(tmp_path):
    batch = train_data.collated('ragged')
    model = train.Trainer(checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0)
    for _ in range(2):
        model.step(*batch)
    path = tmp_path / '00000002.pt'
    model.save(path, epoch=1)
    saved = torch.load(path, map_location='cpu', weights_only=False)
    assert set(saved) == {'epoch', 'step', 'score', 'best', 'model', 'optimizer'}
    assert saved['step'] == 2 and saved['epoch'] == 1
    # inference from the file = inference from the trainer's state
    audio = torch.from_numpy(synth.audio(3, 211))
    alignment = emphases_amd.Alignment.from_frames(
        synth.word_frames(3, 211, 3, 40))
    from_file = emphases_amd.from_alignment_and_audio(
        alignment, audio, emphases_amd.SAMPLE_RATE, checkpoint=str(path), gpu=0)
    direct = session.Session(engine_module.Engine(
        emphases_amd.DEFAULT, model.state_dict(), 0)).run(
            [alignment], [audio], on_device=True)[0]
    assert from_file.shape == direct.shape and from_file.shape[1] > 1
    assert torch.equal(from_file, direct)
    shipped = emphases_amd.from_alignment_and_audio(
        alignment, audio, emphases_amd.SAMPLE_RATE, gpu=0)
    assert not torch.equal(from_file, shipped)
    # a trainer resumed from the file continues as the saved one does
    resumed = train.Trainer(checkpoint=str(path), gpu=0)
    assert resumed.steps == 2
    assert torch.equal(resumed.parameters, model.parameters)
    assert torch.equal(resumed.exp_avg, model.exp_avg)
    assert torch.equal(resumed.exp_avg_sq, model.exp_avg_sq)
    assert torch.equal(resumed.step(*batch), model.step(*batch))
    assert torch.equal(resumed.step(*batch), model.step(*batch))
    torch.optim.Adam([
        torch.nn.Parameter(torch.zeros(shape))
        for shape in weights.parameter_shapes().values()]).load_state_dict(
            model.optimizer_state_dict())
