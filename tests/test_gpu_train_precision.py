"""`precision='bf16x3'` of the training step on the MI355X: the device pack
bitwise against the host's, the single-layer split launch and the split
weight gradient alone against float64, then the trainer - gradients, loss,
five Adam steps against the reference's goldens, determinism, the checkpoint
round trip between precisions and the loop.

The bound of every comparison is 4 x (emulated_error + ref32_error): what the
three-product arithmetic costs with exact accumulation (measured on the CPU by
tests/split_emulation.py - recorded in tests/golden/train_split.npz for the
goldens, computed here for the kernels alone), what float32 accumulation costs
the float32 computation it is compared with, and the project's factor 4.  Each
figure is printed before it is asserted.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loop_data  # noqa: E402
import split_emulation  # noqa: E402
import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import core as api  # noqa: E402
from emphases_amd import runtime, synth, train, weights  # noqa: E402

pytestmark = pytest.mark.gpu

RAGGED_FRAMES = [5, 37, 64, 100, 129, 300]
_TRAINERS = {}


def trainer(precision='bf16x3'):
    """One trainer per precision on the shipped checkpoint; the tests that
    update parameters build their own."""
    if precision not in _TRAINERS:
        _TRAINERS[precision] = train.Trainer(
            config=emphases_amd.DEFAULT, checkpoint=weights.DEFAULT_CHECKPOINT,
            gpu=0, precision=precision)
    return _TRAINERS[precision]


def split_golden():
    with np.load(os.path.join(HERE, 'golden', 'train_split.npz')) as archive:
        return {name: archive[name] for name in archive.files}


def bound_of(case):
    return 4. * (float(split_golden()[f'{case}/emulated_error']) +
                 float(train_data.golden()[f'{case}/ref32_error']))


def frame_plan(frames):
    bounds = torch.zeros(len(frames), 2, 1, dtype=torch.long)
    bounds[:, 1, 0] = torch.tensor(frames)
    return api._packed_plan(frames, bounds, [1] * len(frames))


def special_weights(seed):
    """[80, 80, 3] float32: normals at 1e-3, 1 and 1e3, zeros and -0, values
    exact in bf16, values whose low piece is a rounding tie, subnormals."""
    rng = np.random.default_rng(seed)
    count = 80 * 80 * 3
    value = rng.standard_normal(count).astype(np.float32)
    kind = rng.integers(0, 8, count)
    value[kind == 0] *= np.float32(1e-3)
    value[kind == 1] *= np.float32(1e3)
    value[kind == 3] = np.float32(0.)
    value[kind == 4] = np.float32(-0.)
    exact = (value.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    value[kind == 5] = exact[kind == 5]
    # hi = +-2^e, the rest 2^(e - 10) (1 + k 2^-7 + 2^-8): nine significant
    # bits, the last one set - halfway between two bf16 values
    k = rng.integers(0, 128, count).astype(np.float64)
    tie = (1. + 2. ** -10 * (1. + k * 2. ** -7 + 2. ** -8)) * \
        2. ** rng.integers(-6, 7, count) * rng.choice([-1., 1.], count)
    assert np.array_equal(tie.astype(np.float32).astype(np.float64), tie)
    value[kind == 6] = tie.astype(np.float32)[kind == 6]
    subnormal = (rng.integers(1, 1 << 23, count).astype(np.uint32) |
                 (rng.integers(0, 2, count).astype(np.uint32) << 31))
    value[kind == 7] = subnormal.view(np.float32)[kind == 7]
    for wanted in range(8):
        assert (kind == wanted).sum() > 1000
    assert np.signbit(value[kind == 4]).all()
    return value.reshape(80, 80, 3)


def test_device_packs_are_bitwise_the_host_packs():
    config = emphases_amd.DEFAULT
    offsets, count = train.parameter_offsets(config)
    tables = train.split_pack_tables(config)
    assert len(tables['forward']) == 7 and len(tables['backward']) == 6
    flat = np.zeros(count, dtype=np.float32)
    layers = {}
    for seed, name in enumerate(train.split_layer_names(config)):
        layers[name] = special_weights(seed)
        first, _ = offsets[f'{name}.weight']
        flat[first:first + layers[name].size] = layers[name].ravel()
    lib = runtime.library()
    size = int(lib.emph_conv_split_pack_size())
    packs = torch.full((13, size), 0xa5, dtype=torch.uint8, device='cuda:0')
    index = torch.from_numpy(tables['index']).cuda()
    parameters = torch.from_numpy(flat).cuda()
    runtime.check(lib.emph_conv_split_pack_device(
        parameters.data_ptr(), index.data_ptr(), packs.data_ptr(), 13,
        runtime.stream()), 'emph_conv_split_pack_device')
    got = packs.cpu()
    for direction in ('forward', 'backward'):
        for name, number in tables[direction].items():
            weight = layers[name]
            if direction == 'backward':
                weight = np.ascontiguousarray(
                    weight.transpose(1, 0, 2)[:, :, ::-1])
            want = torch.from_numpy(runtime.conv_split_pack(weight))
            differ = int((got[number] != want).sum())
            print(f'{direction} {name}: pack {number}, {differ} bytes differ')
            assert torch.equal(got[number], want), (direction, name)


def conv_errors(got, want, emulated, narrow, what):
    scale = float(want.abs().max())
    error = float((got - want).abs().max()) / scale
    emulated_error = float((emulated - want).abs().max()) / scale
    narrow_error = float((narrow - want).abs().max()) / scale
    allowed = 4. * (emulated_error + narrow_error)
    print(f'{what}: error {error:.3g}, emulation {emulated_error:.3g}, '
          f'float32 {narrow_error:.3g}, bound {allowed:.3g}')
    return error, allowed


def test_single_layer_split_launch():
    """`emph_conv1d_split` with layers = 1 on segments shorter than a quad, at
    a tile edge, one past two tiles and of two spans; noise between them."""
    frames = RAGGED_FRAMES
    plan = frame_plan(frames)
    spans = torch.from_numpy(plan.conv_spans()).cuda()
    assert spans.shape[0] > len(frames)          # 300 positions: two spans
    ld = plan.ld_frames
    generator = torch.Generator().manual_seed(3)
    x = torch.randn(80, ld, generator=generator)
    weight = torch.randn(80, 80, 3, generator=generator) * 0.1
    bias = torch.randn(80, generator=generator)
    pack = torch.from_numpy(runtime.conv_split_pack(weight.numpy())).cuda()
    x_device, bias_device = x.cuda(), bias.cuda()
    y = torch.full((80, ld), float('nan'), device='cuda:0')
    runtime.check(runtime.library().emph_conv1d_split(
        x_device.data_ptr(), ld, y.data_ptr(), ld, pack.data_ptr(),
        bias_device.data_ptr(), 1, 1, spans.data_ptr(), spans.shape[0], None,
        runtime.stream()), 'emph_conv1d_split')
    y = y.cpu().double()
    got, want, emulated, narrow = [], [], [], []
    conv = torch.nn.functional.conv1d
    for off, count in zip(plan.frame_off, frames):
        piece = x[None, :, off:off + count]
        got.append(y[:, off:off + count])
        want.append(torch.relu(conv(
            piece.double(), weight.double(), bias.double(), padding=1))[0])
        emulated.append(torch.relu(split_emulation.forward_product(
            piece.double(), weight.double()) + bias.double()[None, :, None])[0])
        narrow.append(torch.relu(
            conv(piece, weight, bias, padding=1))[0].double())
    error, allowed = conv_errors(
        *(torch.cat(part, dim=1) for part in (got, want, emulated, narrow)),
        'conv1d_split, one layer')
    assert error <= allowed


def test_conv_weight_grad_split_alone():
    """4 096 positions in 5 uneven segments against conv1d autograd in float64
    on the CPU; what surrounds the segments is noise, outputs and slabs start
    as NaN, two launches give the same bits."""
    frames = [1000, 37, 2047, 12, 1000]
    plan = frame_plan(frames)
    tiles = torch.from_numpy(plan.tiles(runtime.AXIS_FRAMES, 64)).cuda()
    n_tiles = tiles.shape[0]
    lib = runtime.library()
    parts = int(lib.emph_conv_weight_grad_parts(n_tiles))
    assert parts >= 3
    generator = torch.Generator().manual_seed(80)
    ld = plan.ld_frames
    dy = torch.randn(80, ld, generator=generator)
    x = torch.randn(80, ld, generator=generator)
    slabs = torch.full((parts * (80 * 3 * 80 + 80),), float('nan')).cuda()
    dweight = torch.full((80, 80, 3), float('nan')).cuda()
    dbias = torch.full((80,), float('nan')).cuda()
    dy_device, x_device = dy.cuda(), x.cuda()
    for launch in range(2):
        runtime.check(lib.emph_conv_weight_grad_split(
            dy_device.data_ptr(), ld, x_device.data_ptr(), ld, 80, 80, 3,
            tiles.data_ptr(), n_tiles, 64, slabs.data_ptr(),
            dweight.data_ptr(), dbias.data_ptr(), runtime.stream()),
            'emph_conv_weight_grad_split')
        if launch == 0:
            first = (dweight.clone(), dbias.clone())
            slabs.fill_(float('nan'))
    assert torch.equal(first[0], dweight) and torch.equal(first[1], dbias)
    assert not torch.isnan(dweight).any() and not torch.isnan(dbias).any()

    def autograd(dtype):
        weight = torch.zeros(80, 80, 3, dtype=dtype, requires_grad=True)
        bias = torch.zeros(80, dtype=dtype, requires_grad=True)
        for off, count in zip(plan.frame_off, frames):
            out = torch.nn.functional.conv1d(
                x[None, :, off:off + count].to(dtype), weight, bias,
                padding='same')
            out.backward(dy[None, :, off:off + count].to(dtype))
        return weight.grad.double(), bias.grad.double()
    exact = autograd(torch.float64)
    rounded = autograd(torch.float32)
    emulated = (sum(split_emulation.weight_gradient(
        dy[None, :, off:off + count].double(),
        x[None, :, off:off + count].double())
        for off, count in zip(plan.frame_off, frames)), exact[1])
    failed = []
    for name, got, want, rough, narrow in zip(
            ('dweight', 'dbias'), (dweight, dbias), exact, emulated, rounded):
        error, allowed = conv_errors(
            got.cpu().double(), want, rough, narrow, name)
        if not error <= allowed:
            failed.append((name, error, allowed))
    assert not failed, failed


@pytest.mark.parametrize('case', ['ragged', 'uniform'])
def test_gradients_match_the_reference(case):
    golden = train_data.golden()
    bound = bound_of(case)
    batch = train_data.collated(case)
    loss, gradients = trainer().loss_and_gradients(*batch)
    want_loss = float(golden[f'{case}/loss'])
    loss_error = abs(float(loss) - want_loss) / abs(want_loss)
    print(f'{case}: loss {float(loss):.9g} (reference {want_loss:.9g}), '
          f'error {loss_error:.3g}, bound {bound:.3g}')
    wanted = train_data.gradients(case)
    assert set(wanted) == set(gradients)
    worst = {}
    for name, want in wanted.items():
        got = gradients[name].cpu().numpy().astype(np.float64)
        worst[name] = np.abs(got - want).max() / np.abs(want).max()
        print(f'{case}: {name} error {worst[name]:.3g} '
              f'({worst[name] / bound:.2f} of the bound)')
    assert loss_error <= bound
    missed = {name: error for name, error in worst.items() if not error <= bound}
    assert not missed, (missed, bound)
    # the split path ran: not the f32 trainer's bits ...
    f32_loss, f32 = trainer('f32').loss_and_gradients(*batch)
    for name in train.split_layer_names(emphases_amd.DEFAULT):
        assert not torch.equal(
            gradients[f'{name}.weight'], f32[f'{name}.weight']), name
    # ... which are those of a trainer without the argument
    plain_loss, plain = train.Trainer(
        config=emphases_amd.DEFAULT, checkpoint=weights.DEFAULT_CHECKPOINT,
        gpu=0).loss_and_gradients(*batch)
    assert torch.equal(plain_loss, f32_loss)
    for name in plain:
        assert torch.equal(plain[name], f32[name]), name


def test_same_batch_twice_is_bitwise_the_same():
    batch = train_data.collated('ragged')
    first_loss, first = trainer().loss_and_gradients(*batch)
    second_loss, second = trainer().loss_and_gradients(*batch)
    assert torch.equal(first_loss, second_loss)
    for name in first:
        assert torch.equal(first[name], second[name]), name


def test_a_batch_of_an_f32_trainer_is_refused_by_name():
    """It carries no span table: refused before anything is launched."""
    prepared = trainer('f32').prepare(*train_data.collated('uniform'))
    before = trainer().parameters.clone()
    for call in (trainer().logits, trainer().loss_and_gradients,
                 trainer().step):
        with pytest.raises(ValueError, match="precision='f32'"):
            call(prepared)
    assert trainer().steps == 0 and torch.equal(trainer().parameters, before)
    # the other way round works: the f32 launches do not read the table
    split = trainer().prepare(*train_data.collated('uniform'))
    loss, _ = trainer('f32').loss_and_gradients(split)
    assert torch.equal(loss, trainer('f32').loss_and_gradients(prepared)[0])


def test_five_steps_follow_the_reference():
    golden, split = train_data.golden(), split_golden()
    runs = np.stack([golden[f'adam/{name}'] for name in (
        'float32', 'float64', 'float32_reversed')])
    model = train.Trainer(
        checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0, precision='bf16x3')
    prepared = model.prepare(*train_data.collated('ragged'))
    losses = [model.step(prepared) for _ in range(5)]
    losses.append(model.loss_and_gradients(prepared)[0])
    losses = np.array([float(loss) for loss in losses], dtype=np.float64)
    spread = runs.max(axis=0) - runs.min(axis=0)
    allowed = 4. * (spread + np.abs(split['adam/emulated'] - runs[1]))
    off = np.abs(runs - losses).max(axis=0)
    for step, loss in enumerate(losses):
        print(f'step {step}: loss {loss:.9g}, reference {runs[1, step]:.9g}, '
              f'emulated {split["adam/emulated"][step]:.9g}, off by '
              f'{off[step]:.3g}, bound {allowed[step]:.3g}')
    assert model.steps == 5
    assert np.all(np.diff(losses) < 0), losses
    assert abs(losses[0] - runs[1, 0]) / runs[1, 0] <= bound_of('ragged')
    for step in range(1, 6):
        assert off[step] <= allowed[step], (step, losses[step], runs[:, step])


def test_checkpoint_round_trip_between_precisions(tmp_path):
    batch = train_data.collated('ragged')
    model = train.Trainer(
        checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0, precision='bf16x3')
    for _ in range(2):
        model.step(*batch)
    path = tmp_path / '00000002.pt'
    model.save(path)
    saved = torch.load(path, map_location='cpu', weights_only=False)
    assert set(saved) == {'epoch', 'step', 'score', 'best', 'model', 'optimizer'}
    resumed = train.Trainer(checkpoint=str(path), gpu=0, precision='bf16x3')
    plain = train.Trainer(checkpoint=str(path), gpu=0, precision='f32')
    for other in (resumed, plain):
        assert other.steps == 2
        assert torch.equal(other.parameters, model.parameters)
        assert torch.equal(other.exp_avg, model.exp_avg)
        assert torch.equal(other.exp_avg_sq, model.exp_avg_sq)
        assert other.parameters.dtype == torch.float32
    assert torch.equal(resumed.step(*batch), model.step(*batch))
    assert torch.equal(resumed.step(*batch), model.step(*batch))
    assert torch.equal(resumed.parameters, model.parameters)
    assert torch.isfinite(plain.step(*batch))
    audio = torch.from_numpy(synth.audio(3, 211))
    alignment = emphases_amd.Alignment.from_frames(
        synth.word_frames(3, 211, 3, 40))
    for precision in ('f32', 'bf16x3'):
        scores = emphases_amd.from_alignment_and_audio(
            alignment, audio, emphases_amd.SAMPLE_RATE, checkpoint=str(path),
            gpu=0, precision=precision)
        assert scores.shape[-1] == len(alignment)
        assert torch.isfinite(scores).all()


def test_loop_at_bf16x3(tmp_path):
    partition_dir, cache_dir = loop_data.build_cache(str(tmp_path / 'cache'))
    first = {}
    for precision in ('f32', 'bf16x3'):
        directory = tmp_path / precision
        path = train.train(
            loop_data.DATASET, directory, 0, partition_dir=partition_dir,
            cache_dir=cache_dir, config=emphases_amd.DEFAULT,
            max_training_frames=600, num_steps=4, log_interval=2,
            precision=precision)
        assert path == str(directory / '00000004.pt')
        assert train.Trainer(checkpoint=path, gpu=0).steps == 4
        with open(directory / 'scalars.jsonl') as file:
            scalars = [json.loads(line) for line in file]
        assert [line['step'] for line in scalars] == [0, 2]
        for line in scalars:
            assert all(np.isfinite(value) for value in line.values())
        first[precision] = scalars[0]['loss/train']
        first[precision, 'model'] = torch.load(
            path, map_location='cpu', weights_only=False)['model']
    # four updates apart, the two precisions no longer hold the same weights
    assert not torch.equal(first['f32', 'model']['frame_encoder.0.weight'],
                           first['bf16x3', 'model']['frame_encoder.0.weight'])
    error = abs(first['bf16x3'] - first['f32']) / first['f32']
    print(f"first loss/train: f32 {first['f32']:.9g}, bf16x3 "
          f"{first['bf16x3']:.9g}, error {error:.3g}, "
          f"bound {bound_of('ragged'):.3g}")
    assert error <= bound_of('ragged')
