"""`emphases_amd.upsample`, the frame-rate head and `EncoderTrainer` on the
MI355X: `upsample` against the reference's recorded output
(tests/golden/upsample.npz), the head kernels and the frame-rate loss alone
against torch in float64, the step's loss and gradients against the unmodified
reference in float64 (tests/golden/locations_<variant>.npz, written by
tests/golden/generate_locations.py, and two grid_<variant>.npz), eval-mode
logits, repeatability, Adam steps, the checkpoint round trip, 'bf16x3' and the
loop.

Every bound is 4 x the error of the same computation in float32 on the CPU
(the project's standing allowance): the reference's own for the goldens
(`ref32_error`), torch's for the kernels alone (computed here).  Each figure
is printed before it is asserted.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loop_data  # noqa: E402
import train_data  # noqa: E402
from test_encoder_train import upsample_cases, upsample_float64  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import core as api  # noqa: E402
from emphases_amd import engine as engine_module  # noqa: E402
from emphases_amd import data, runtime, train, weights  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = runtime.AXIS_FRAMES
FORMS = {'bce': 0, 'mse': 1}
# variant -> (fixture, configuration besides layers=2)
VARIANTS = {
    'sum_inference': ('locations_sum_inference', dict(
        downsample_location='inference')),
    'sum_inference_nearest_mse': ('locations_sum_inference_nearest_mse', dict(
        downsample_location='inference', upsample_method='nearest',
        loss='mse')),
    'sum_loss': ('locations_sum_loss', dict(downsample_location='loss')),
    'max_loss': ('locations_max_loss', dict(
        downsample_location='loss', downsample_method='max')),
    'sum_inference_dropout10': ('locations_sum_inference_dropout10', dict(
        downsample_location='inference', dropout=0.1)),
    'center_loss': ('grid_center_loss', dict(
        downsample_location='loss', downsample_method='center')),
    'average_loss_mse': ('grid_average_loss_mse', dict(
        downsample_location='loss', downsample_method='average', loss='mse')),
}


def fixture(name):
    with np.load(os.path.join(train_data.GOLDEN, f'{name}.npz')) as file:
        return {key: file[key] for key in file.files}


def bits(tensor):
    return tensor.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def layout(frames, words=None, bounds=None):
    """(plan, {name: device table}) of a packed layout with the 64-wide frame
    tile table; without words every utterance is one word."""
    if bounds is None:
        words = [1] * len(frames)
        bounds = torch.zeros(len(frames), 2, 1, dtype=torch.long)
        bounds[:, 1, 0] = torch.tensor(frames)
    plan = api._packed_plan(frames, bounds, words)
    host, offsets = plan.pack_metadata([(FRAMES, 64)])
    meta = torch.from_numpy(host).cuda()
    tables = {name: meta[start:start + size]
              for name, (start, size) in offsets.items()}
    tables['tiles'] = tables[('tiles', FRAMES, 64)]
    tables['n_tiles'] = tables['tiles'].numel() // runtime.TILE_FIELDS
    return plan, tables


def inside(plan):
    """bool [ld_frames]: the columns inside an utterance."""
    mask = torch.zeros(plan.ld_frames, dtype=torch.bool)
    for off, count in zip(plan.frame_off, plan.frames):
        mask[off:off + count] = True
    return mask


###############################################################################
# upsample
###############################################################################


@pytest.mark.parametrize('method', ['linear', 'nearest'])
def test_upsample_matches_the_reference(method):
    cases, errors = upsample_cases()
    channels = 1 if method == 'linear' else 3
    frames = [case[0] for case in cases]
    words = [len(case[1]) for case in cases]
    xs = torch.zeros(len(cases), channels, max(words))
    bounds = torch.zeros(len(cases), 2, max(words), dtype=torch.long)
    for i, (_, starts, ends, methods) in enumerate(cases):
        xs[i, :, :words[i]] = torch.from_numpy(methods[method][0])
        bounds[i, 0, :words[i]] = torch.from_numpy(starts)
        bounds[i, 1, :words[i]] = torch.from_numpy(ends)
    config = emphases_amd.Config(upsample_method=method)
    got = emphases_amd.upsample(
        xs.cuda(), bounds, torch.tensor(words), torch.tensor(frames), config)
    assert got.is_cuda and got.shape == (len(cases), channels, max(frames))
    on_host = emphases_amd.upsample(xs, bounds, words, frames, config)
    assert not on_host.is_cuda and torch.equal(on_host, got.cpu())
    bound = 4. * errors[method]
    for i, (count, starts, ends, methods) in enumerate(cases):
        x, want = methods[method]
        value = got[i, :, :count].cpu().numpy()
        assert not got[i, :, count:].any()
        if words[i] == 1:
            # every channel its own word (the reference: channel 0's)
            assert np.array_equal(value[0].astype(np.float64), want[0])
            assert np.array_equal(value, np.repeat(x, count, axis=1))
            continue
        if method == 'nearest':
            # a selection of float32 inputs
            assert np.array_equal(value.astype(np.float64), want), count
            continue
        error = np.abs(value - want).max() / np.abs(want).max()
        print(f'upsample linear ({count}, {words[i]}): error {error:.3g}, '
              f'bound {bound:.3g}')
        assert error <= bound, (count, error, bound)
        restated = upsample_float64(x, starts, ends, count, method)
        assert np.abs(restated - want).max() <= 1e-12


def test_upsample_refuses_unsorted_and_empty_words():
    xs = torch.rand(1, 1, 3)
    good = torch.tensor([[[0, 4, 8], [4, 8, 12]]])

    def call(bounds, words=(3,), frames=(12,)):
        return emphases_amd.upsample(xs, bounds, list(words), list(frames))
    assert call(good).shape == (1, 1, 12)
    unsorted = good[:, :, [1, 0, 2]]
    empty = good.clone()
    empty[0, 1, 1] = empty[0, 0, 1]
    overlap = good.clone()
    overlap[0, 1, 0] = 5
    for bad in (unsorted, empty, overlap):
        with pytest.raises(ValueError):
            call(bad)
    with pytest.raises(ValueError):
        call(good, words=(0,))
    with pytest.raises(ValueError):
        call(good, frames=(0,))


###############################################################################
# The head kernels alone
###############################################################################


def run_head(plan, tables, h, dlogit, weight, bias):
    """emph_frame_head and emph_frame_head_backward on device copies; every
    output starts as NaN.  Returns (logits, dx, dweight, dbias)."""
    lib = runtime.library()
    ld = plan.ld_frames
    h, dlogit = h.cuda(), dlogit.cuda()
    weight, bias = weight.cuda(), bias.cuda()
    nan = lambda *shape: torch.full(shape, float('nan')).cuda()  # noqa: E731
    logits, dx = nan(ld), nan(80, ld)
    dweight, dbias = nan(1, 80, 3), nan(1)
    parts = int(lib.emph_frame_head_parts(tables['n_tiles']))
    workspace = nan(parts * 241)
    runtime.check(lib.emph_frame_head(
        h.data_ptr(), ld, weight.data_ptr(), bias.data_ptr(), 80, 3,
        tables['tiles'].data_ptr(), tables['n_tiles'], logits.data_ptr(),
        runtime.stream()), 'emph_frame_head')
    runtime.check(lib.emph_frame_head_backward(
        dlogit.data_ptr(), h.data_ptr(), ld, weight.data_ptr(), 80, 3,
        tables['tiles'].data_ptr(), tables['n_tiles'], workspace.data_ptr(),
        dweight.data_ptr(), dbias.data_ptr(), dx.data_ptr(), ld,
        runtime.stream()), 'emph_frame_head_backward')
    return logits.cpu(), dx.cpu(), dweight.cpu(), dbias.cpu()


@pytest.mark.parametrize('frames', [
    [5, 37, 64, 100, 129, 300], [1, 2], [64 * 1024 + 1, 3]])
def test_head_kernels_alone(frames):
    """Random h, dlogit and weights against conv1d + autograd in float64 on
    the CPU, one utterance at a time; then again with NaN in every column
    outside the utterances.  (The third layout has more tiles than parts: a
    workgroup of the backward owns two.)"""
    plan, tables = layout(frames)
    if len(frames) == 2 and frames[0] > 64:
        assert runtime.library().emph_frame_head_parts(tables['n_tiles']) < \
            tables['n_tiles']
    ld = plan.ld_frames
    generator = torch.Generator().manual_seed(sum(frames))
    h = torch.randn(80, ld, generator=generator)
    dlogit = torch.randn(ld, generator=generator)
    weight = torch.randn(1, 80, 3, generator=generator) / 15.
    bias = torch.randn(1, generator=generator)
    got = run_head(plan, tables, h, dlogit, weight, bias)
    valid = inside(plan)

    def autograd(dtype):
        w = weight.to(dtype).requires_grad_()
        b = bias.to(dtype).requires_grad_()
        logits = torch.zeros(ld, dtype=dtype)
        dx = torch.zeros(80, ld, dtype=dtype)
        for off, count in zip(plan.frame_off, plan.frames):
            x = h[None, :, off:off + count].to(dtype).requires_grad_()
            out = torch.nn.functional.conv1d(x, w, b, padding='same')
            out.backward(dlogit[None, None, off:off + count].to(dtype))
            logits[off:off + count] = out.detach()[0, 0]
            dx[:, off:off + count] = x.grad[0]
        return (logits.double(), dx.double(), w.grad.double(),
                b.grad.double())
    exact, rounded = autograd(torch.float64), autograd(torch.float32)
    for name, value, want, narrow in zip(
            ('logits', 'dx', 'dweight', 'dbias'), got, exact, rounded):
        value = value.double()
        if name in ('logits', 'dx'):
            assert torch.isnan(value[..., ~valid]).all(), name  # left alone
            value = value[..., valid]
            want, narrow = want[..., valid], narrow[..., valid]
        scale = want.abs().max()
        allowed = 4. * float((narrow - want).abs().max() / scale)
        error = float((value - want).abs().max() / scale)
        print(f'head {frames[:2]}.. {name}: error {error:.3g}, '
              f'bound {allowed:.3g}')
        assert error <= allowed, (name, error, allowed)
    # what lies between the utterances reaches nothing
    noisy_h, noisy_dlogit = h.clone(), dlogit.clone()
    noisy_h[:, ~valid] = float('nan')
    noisy_dlogit[~valid] = float('nan')
    again = run_head(plan, tables, noisy_h, noisy_dlogit, weight, bias)
    for name, first, second in zip(
            ('logits', 'dx', 'dweight', 'dbias'), got, again):
        assert same(first, second), name


###############################################################################
# The frame-rate loss
###############################################################################


@pytest.mark.parametrize('loss', ['bce', 'mse'])
@pytest.mark.parametrize('method', ['linear', 'nearest'])
def test_frame_loss_grad_alone(loss, method):
    features, frame_lengths, word_bounds, word_lengths, targets = \
        train_data.collated('ragged')
    frames = [int(n) for n in frame_lengths]
    words = [int(n) for n in word_lengths]
    plan, tables = layout(frames, words, word_bounds)
    ld_f, ld_w = plan.ld_frames, plan.ld_words
    generator = torch.Generator().manual_seed(7)
    logits = torch.randn(ld_f, generator=generator) * 2.
    valid = inside(plan)
    logits[~valid] = float('nan')
    packed = torch.full((ld_w,), float('nan'))
    spread, clamped = [], 0
    for i, (off, count) in enumerate(zip(plan.word_off, words)):
        packed[off:off + count] = targets[i, 0, :count]
        value = upsample_float64(
            targets[i, :, :count].numpy(), word_bounds[i, 0, :count].numpy(),
            word_bounds[i, 1, :count].numpy(), frames[i], method)[0]
        if method == 'linear':
            clamped += int(((value < 0) | (value > 1)).sum())
            value = np.clip(value, 0., 1.)
        spread.append(torch.from_numpy(value))
    assert (clamped > 0) == (method == 'linear')
    spread = torch.cat(spread)

    def autograd(dtype):
        z = logits[valid].to(dtype).requires_grad_()
        function = torch.nn.functional.binary_cross_entropy_with_logits \
            if loss == 'bce' else torch.nn.functional.mse_loss
        value = function(z, spread.to(dtype))
        value.backward()
        return value.detach().double(), z.grad.double()
    (want_loss, want), (_, narrow) = \
        autograd(torch.float64), autograd(torch.float32)
    lib = runtime.library()
    logits_device, packed = logits.cuda(), packed.cuda()
    results = []
    for _ in range(2):
        out = torch.full((1,), float('nan')).cuda()
        dlogit = torch.full((ld_f,), float('nan')).cuda()
        workspace = torch.full(
            (tables['n_tiles'],), float('nan'), dtype=torch.float64).cuda()
        runtime.check(lib.emph_frame_loss_grad(
            logits_device.data_ptr(), packed.data_ptr(),
            tables['bounds'].data_ptr(), ld_w, tables['table'].data_ptr(),
            tables['tiles'].data_ptr(), tables['n_tiles'], plan.total_frames,
            FORMS[loss], runtime.UPSAMPLE_METHODS[method],
            workspace.data_ptr(), out.data_ptr(), dlogit.data_ptr(),
            runtime.stream()), 'emph_frame_loss_grad')
        results.append((out.cpu(), dlogit.cpu()))
    assert same(results[0][0], results[1][0])
    assert same(results[0][1], results[1][1])
    out, dlogit = results[0]
    assert torch.isnan(dlogit[~valid]).all()
    loss_error = abs(float(out) - float(want_loss)) / float(want_loss)
    scale = want.abs().max()
    allowed = 4. * float((narrow - want).abs().max() / scale)
    error = float((dlogit[valid].double() - want).abs().max() / scale)
    print(f'frame loss {loss} {method}: loss {float(out):.9g} (float64 '
          f'{float(want_loss):.9g}), error {loss_error:.3g}; dlogit error '
          f'{error:.3g}, bound {allowed:.3g}; {clamped} targets clamped')
    assert loss_error <= 1e-6
    assert error <= allowed, (error, allowed)


###############################################################################
# The step against the reference
###############################################################################


def reference_trainer(variant, precision='f32'):
    name, overrides = VARIANTS[variant]
    golden = fixture(name)
    config = emphases_amd.Config(layers=2, **overrides)
    seed = int(golden['seed'])
    state = train.initial_state(config, seed)
    for key, value in state.items():
        value = value.astype(np.float64)
        assert np.array_equal(
            golden[f'init/{key}'], [value.sum(), (value ** 2).sum()]), key
    return golden, train.EncoderTrainer(
        config, gpu=0, seed=seed, precision=precision)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_gradients_match_the_reference(variant):
    golden, model = reference_trainer(variant)
    assert model.steps == 0
    bound = 4. * float(golden['ref32_error'])
    loss, gradients = model.loss_and_gradients(*train_data.collated('ragged'))
    assert loss.is_cuda and loss.dim() == 0
    want_loss = float(golden['loss'])
    loss_error = abs(float(loss) - want_loss) / abs(want_loss)
    print(f'{variant}: loss {float(loss):.9g} (reference {want_loss:.9g}), '
          f'error {loss_error:.3g}, bound {bound:.3g}')
    wanted = {name[len('grad/'):]: value.astype(np.float64)
              for name, value in golden.items() if name.startswith('grad/')}
    assert set(wanted) == set(gradients) == \
        set(weights.parameter_shapes(model.config))
    worst = {}
    for name, want in wanted.items():
        got = gradients[name].cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        worst[name] = np.abs(got - want).max() / np.abs(want).max()
        print(f'{variant}: {name} error {worst[name]:.3g} '
              f'({worst[name] / bound:.2f} of the bound)')
    assert loss_error <= bound
    missed = {name: error for name, error in worst.items() if not error <= bound}
    assert not missed, (missed, bound)


@pytest.mark.parametrize('method', ['sum', 'average', 'max', 'center'])
def test_eval_logits_match_the_reference(method):
    golden = fixture('locations_sum_inference')
    model = train.EncoderTrainer(
        emphases_amd.Config(layers=2, downsample_location='inference',
                            downsample_method=method),
        gpu=0, seed=int(golden['seed']))
    batch = model.prepare(*train_data.collated('ragged'))
    got = model.logits(batch)
    assert got.is_cuda and got.shape == (65,)
    want = golden[f'eval/{method}']
    bound = 4. * float(golden['ref32_error'])
    error = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
    print(f'eval logits {method}: error {error:.3g}, bound {bound:.3g}')
    assert error <= bound
    # the location changes nothing in eval mode
    other = train.EncoderTrainer(
        emphases_amd.Config(layers=2, downsample_location='loss',
                            downsample_method=method),
        gpu=0, seed=int(golden['seed']))
    assert same(other.logits(batch), got)


@pytest.mark.parametrize('overrides', [
    dict(downsample_location='inference'),
    dict(downsample_location='loss', downsample_method='max')])
def test_same_batch_twice_is_bitwise_the_same(overrides):
    model = train.EncoderTrainer(
        emphases_amd.Config(layers=2, **overrides), gpu=0, seed=1)
    batch = train_data.collated('ragged')
    first_loss, first = model.loss_and_gradients(*batch)
    second_loss, second = model.loss_and_gradients(*batch)
    assert same(first_loss, second_loss)
    for name in first:
        assert same(first[name], second[name]), name


@pytest.mark.parametrize('location', ['inference', 'loss'])
def test_five_adam_steps_lower_the_loss(location):
    model = train.EncoderTrainer(
        emphases_amd.Config(downsample_location=location),
        checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0)
    prepared = model.prepare(*train_data.collated('ragged'))
    losses = [float(model.step(prepared)) for _ in range(5)]
    losses.append(float(model.loss_and_gradients(prepared)[0]))
    print(f'{location}: losses {losses}')
    assert model.steps == 5 and np.all(np.isfinite(losses))
    assert np.all(np.diff(losses) < 0), losses


def test_an_utterance_without_words_is_refused_at_inference():
    features, frame_lengths, word_bounds, word_lengths, targets = \
        train_data.collated('ragged')
    word_lengths = word_lengths.clone()
    word_lengths[1] = 0
    model = train.EncoderTrainer(
        emphases_amd.Config(layers=1, downsample_location='inference'), gpu=0)
    with pytest.raises(ValueError, match='an utterance has none'):
        model.step(features, frame_lengths, word_bounds, word_lengths, targets)


def test_checkpoint_round_trip(tmp_path):
    config = emphases_amd.Config(
        downsample_location='inference', downsample_method='average',
        dropout=0.1)
    batch = train_data.collated('ragged')
    model = train.EncoderTrainer(config, gpu=0, seed=5)
    for _ in range(2):
        model.step(*batch)
    path = tmp_path / '00000002.pt'
    model.save(path, epoch=1)
    saved = torch.load(path, map_location='cpu', weights_only=False)
    assert set(saved) == {'epoch', 'step', 'score', 'best', 'model', 'optimizer'}
    assert saved['step'] == 2 and saved['epoch'] == 1
    # the reference's names: no word decoder, `3 i` under dropout
    assert list(saved['model']) == list(train.checkpoint_names(config).values())
    assert 'frame_encoder.15.weight' in saved['model']
    assert not any(name.startswith('word_decoder') for name in saved['model'])
    resumed = train.EncoderTrainer(config, checkpoint=str(path), gpu=0, seed=5)
    assert resumed.steps == 2
    assert same(resumed.parameters, model.parameters)
    assert same(resumed.exp_avg, model.exp_avg)
    assert same(resumed.exp_avg_sq, model.exp_avg_sq)
    assert same(resumed.step(*batch), model.step(*batch))
    assert same(resumed.parameters, model.parameters)
    # the inference engine loads the file under the same config: the file and
    # the trainer's state give the same bits (`test_checkpoint_round_trip` of
    # test_gpu_train.py), and what it computes is what the trainer's eval
    # mode computes, each a float32 evaluation of the same function
    model.save(path)
    features, frame_lengths, word_bounds, word_lengths, _ = batch
    arguments = (features.cuda(), frame_lengths, word_bounds, word_lengths)
    engine = emphases_amd.Model(checkpoint=str(path), gpu=0, config=config)
    from_file = engine(*arguments)
    engine.engine = engine_module.Engine(config, model.state_dict(), 0)
    assert same(from_file, engine(*arguments))
    compact = torch.cat([
        from_file[i, 0, :int(n)] for i, n in enumerate(word_lengths)])
    logits = model.logits(model.prepare(*batch))
    bound = 4. * float(fixture('locations_sum_inference')['ref32_error'])
    scores = api.postprocess(compact, config).cpu().double()
    want = api.postprocess(logits, config).cpu().double()
    error = float((scores - want).abs().max() / want.abs().max())
    print(f'engine against trainer scores: error {error:.3g}, bound {bound:.3g}')
    assert error <= bound


###############################################################################
# bf16x3
###############################################################################


def precision_gap(cls, config):
    """Worst over tensors of max|g_bf16x3 - g_f32| / max|g_f32| on `ragged`
    from the shipped checkpoint, and the two losses."""
    batch = train_data.collated('ragged')
    results = {}
    for precision in ('f32', 'bf16x3'):
        model = cls(config, checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0,
                    precision=precision)
        results[precision] = model.loss_and_gradients(*batch)
    ratios = {}
    for name, exact in results['f32'][1].items():
        split = results['bf16x3'][1][name]
        ratios[name] = float((split - exact).abs().max() / exact.abs().max())
    return ratios, [float(results[p][0]) for p in ('f32', 'bf16x3')]


def test_bf16x3_at_inference_is_as_close_as_the_existing_trainer():
    """The yardstick is `Trainer`: its own gap between the two precisions on
    the same batch; the factor of two allows for the different head shaping
    the gradient's spectrum."""
    yardstick, _ = precision_gap(train.Trainer, emphases_amd.DEFAULT)
    ratios, losses = precision_gap(
        train.EncoderTrainer,
        emphases_amd.Config(downsample_location='inference'))
    allowed = 2. * max(yardstick.values())
    for name, ratio in ratios.items():
        print(f'bf16x3 at inference: {name} {ratio:.3g} '
              f'({ratio / allowed:.2f} of the bound)')
    print(f'bf16x3: Trainer worst {max(yardstick.values()):.3g}, '
          f'EncoderTrainer worst {max(ratios.values()):.3g}, bound '
          f'{allowed:.3g}; losses {losses}')
    assert max(ratios.values()) > 0.
    assert max(ratios.values()) <= allowed
    # the frame-rate head itself is float32 at either precision
    assert abs(losses[1] - losses[0]) / losses[0] <= allowed


###############################################################################
# The loop
###############################################################################


@pytest.fixture(scope='module')
def cache(tmp_path_factory):
    return loop_data.build_cache(str(tmp_path_factory.mktemp('locations')))


def test_loop_at_inference_equals_hand_driven_steps(cache, tmp_path):
    partition_dir, cache_dir = cache
    config = emphases_amd.Config(layers=2, downsample_location='inference')
    path = train.train(
        loop_data.DATASET, tmp_path / 'run', 0, partition_dir=partition_dir,
        cache_dir=cache_dir, config=config, max_training_frames=600,
        num_steps=4, log_interval=2, save_after=1)
    assert path == str(tmp_path / 'run' / '00000004.pt')
    saved = torch.load(path, map_location='cpu', weights_only=False)
    assert saved['step'] == 4
    with open(tmp_path / 'run' / 'scalars.jsonl') as file:
        assert len(file.readlines()) == 2
    model = train.make_trainer(config, gpu=0)
    assert isinstance(model, train.EncoderTrainer)
    dataset = data.Dataset(
        loop_data.DATASET, 'train', partition_dir=partition_dir,
        cache_dir=cache_dir, config=config, gpu=0, upload=False)
    sampler = data.Sampler(dataset, 600)
    epoch = 0
    while model.steps < 4:
        sampler.set_epoch(epoch)
        for indices in sampler:
            model.step(*loop_data.collated(
                cache_dir, [dataset.stems[i] for i in indices], config))
            if model.steps == 4:
                break
        epoch += 1
    state, optimizer = model.state_dict(), model.optimizer_state_dict()
    assert list(saved['model']) == list(state)
    for name, value in state.items():
        assert same(saved['model'][name], value), name
    for index, entry in optimizer['state'].items():
        for moment in ('exp_avg', 'exp_avg_sq'):
            assert same(saved['optimizer']['state'][index][moment],
                        entry[moment]), (index, moment)
    # and the run resumes through the same dispatch
    again = train.train(
        loop_data.DATASET, tmp_path / 'run', 0, partition_dir=partition_dir,
        cache_dir=cache_dir, config=config, max_training_frames=600,
        num_steps=5, log_interval=100, save_after=100)
    assert again == str(tmp_path / 'run' / '00000005.pt')
