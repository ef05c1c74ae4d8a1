"""The differentiable operator seams on the MI355X: the three backward kernels
alone, `torch.library.opcheck` of the two ops, and `train.TorchModel` against
the reference's float64 gradients (tests/golden/train.npz) and against
`train.Trainer`.

Every bound is 4 x the error of the same computation in float32 on the CPU
against float64 (the project's standing allowance, `test_gpu_train`): torch's
for the kernels alone (computed here), the reference's own for the goldens
(`ref32_error`).  Each figure is printed before it is asserted.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import engine as engine_module  # noqa: E402
from emphases_amd import ops, runtime, session, synth, train, weights  # noqa: E402

pytestmark = pytest.mark.gpu

SEGMENTS = [200, 1, 17, 64, 65, 3, 130]
SHAPES = [(80, 80, 3), (80, 64, 5), (64, 64, 3), (128, 128, 7), (83, 128, 1),
          (80, 1, 3), (3, 7, 5)]


def device():
    return torch.device('cuda', 0)


###############################################################################
# emph_conv_weight_grad_any
###############################################################################


@pytest.mark.parametrize('c_in, c_out, k', SHAPES)
def test_conv_weight_grad_any(c_in, c_out, k):
    """Seven uneven segments against conv1d autograd in float64 on the CPU;
    what surrounds the segments is NaN."""
    layout = ops._layout(device(), np.array(SEGMENTS, dtype=np.int64))
    plan, ld = layout.plan, layout.plan.ld_frames
    tiles, n_tiles = layout.tiles(64)
    assert n_tiles == sum((n + 63) // 64 for n in SEGMENTS)
    generator = torch.Generator().manual_seed(1000 * c_in + 10 * c_out + k)
    dy = torch.full((c_out, ld), float('nan'))
    x = torch.full((c_in, ld), float('nan'))
    for off, count in zip(plan.frame_off, SEGMENTS):
        dy[:, off:off + count] = torch.randn(c_out, count, generator=generator)
        x[:, off:off + count] = torch.randn(c_in, count, generator=generator)
    lib = runtime.library()
    floats = int(lib.emph_conv_weight_grad_any_workspace(c_in, c_out, k, n_tiles))
    assert floats == int(lib.emph_conv_weight_grad_parts(n_tiles)) * \
        (c_out * c_in * k + c_out)
    slabs = torch.full((floats,), float('nan'), device=device())
    dweight = torch.full((c_out, c_in, k), float('nan'), device=device())
    dbias = torch.full((c_out,), float('nan'), device=device())
    dy_device, x_device = dy.to(device()), x.to(device())
    for launch in range(2):
        runtime.check(lib.emph_conv_weight_grad_any(
            dy_device.data_ptr(), ld, x_device.data_ptr(), ld, c_in, c_out, k,
            tiles.data_ptr(), n_tiles, 64, slabs.data_ptr(),
            dweight.data_ptr(), dbias.data_ptr(), runtime.stream()),
            'emph_conv_weight_grad_any')
        if launch == 0:
            first = (dweight.clone(), dbias.clone())
            dweight.fill_(float('nan'))
            dbias.fill_(float('nan'))
    assert torch.equal(first[0], dweight) and torch.equal(first[1], dbias)
    assert torch.isfinite(dweight).all() and torch.isfinite(dbias).all()

    def autograd(dtype):
        weight = torch.zeros(c_out, c_in, k, dtype=dtype, requires_grad=True)
        bias = torch.zeros(c_out, dtype=dtype, requires_grad=True)
        for off, count in zip(plan.frame_off, SEGMENTS):
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
        print(f'({c_in}, {c_out}, {k}) d{name}: error {error:.3g}, '
              f'bound {allowed:.3g}')
        assert error <= allowed, (name, error, allowed)


def test_conv_weight_grad_any_refuses_other_shapes():
    """Return codes of calls that launch nothing."""
    lib = runtime.library()
    layout = ops._layout(device(), np.array([64], dtype=np.int64))
    tiles, n_tiles = layout.tiles(64)
    buffer = torch.zeros(1 << 16, device=device())
    for c_in, c_out, k, tile in ((129, 80, 3, 64), (80, 129, 3, 64),
                                 (0, 80, 3, 64), (80, 80, 9, 64),
                                 (80, 80, 4, 64), (80, 80, 3, 32)):
        assert lib.emph_conv_weight_grad_any(
            buffer.data_ptr(), 128, buffer.data_ptr(), 128, c_in, c_out, k,
            tiles.data_ptr(), n_tiles, tile, buffer.data_ptr(),
            buffer.data_ptr(), buffer.data_ptr(), runtime.stream()) == -2


###############################################################################
# emph_segment_reduce_backward
###############################################################################

REDUCE_FRAMES = np.array([200, 40, 150], dtype=np.int64)
REDUCE_WORDS = np.array([3, 0, 5], dtype=np.int64)
# segment 0: a one-frame word, a word across the 64-frame edge, a 130-frame
# word (frames 1, 2 uncovered); segment 1: no word; segment 2: a one-frame
# word, then the four tie cases of 'max' (frames 0..4, 6..9, 30..59, 140..149
# uncovered)
REDUCE_BOUNDS = np.array([[0, 3, 70, 5, 10, 60, 68, 100],
                          [1, 70, 200, 6, 30, 68, 100, 140]], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def reduce_case(channels):
    """(x, dword) on the CPU, back to back: noise, with the maxima of the tie
    cases planted."""
    generator = torch.Generator().manual_seed(channels)
    x = torch.randn(channels, int(REDUCE_FRAMES.sum()), generator=generator)
    second = 240                              # first column of segment 2
    x[:, 66] = 9.                             # word [3, 70): only past the edge
    x[:, 75] = x[:, 150] = x[:, 195] = 10.    # [70, 200): in three tiles
    x[:, second + 12] = x[:, second + 20] = 10.   # the maximum occurs twice
    x[:, second + 60] = 10.                   # ... at the first frame
    x[:, second + 99] = 10.                   # ... at the last frame
    x[:, second + 100:second + 140] = 1.5     # an all-equal word
    dword = torch.randn(channels, REDUCE_BOUNDS.shape[1], generator=generator)
    return x, dword


def reduce_reference(x, dword, mode, dtype):
    """torch CPU autograd of the reference formula (`core.py:426-469`)."""
    x = x.detach().clone().to(dtype).requires_grad_(True)
    first_frame = np.cumsum(REDUCE_FRAMES) - REDUCE_FRAMES
    columns, word = [], 0
    for offset, count in zip(first_frame, REDUCE_WORDS):
        for _ in range(int(count)):
            start, end = (int(v) + int(offset) for v in REDUCE_BOUNDS[:, word])
            piece = x[:, start:end]
            columns.append({
                'sum': lambda: piece.sum(dim=1),
                'average': lambda: piece.mean(dim=1),
                'max': lambda: piece.max(dim=1).values,
                'center': lambda: x[:, (start + end) // 2]}[mode]())
            word += 1
    torch.stack(columns, dim=1).backward(dword.to(dtype))
    return x.grad


@pytest.mark.parametrize('mode', ['sum', 'average', 'max', 'center'])
@pytest.mark.parametrize('channels', [80, 7])
def test_segment_reduce_backward(channels, mode):
    x, dword = reduce_case(channels)
    layout = ops._layout(device(), REDUCE_FRAMES, REDUCE_WORDS, REDUCE_BOUNDS)
    plan = layout.plan
    lib = runtime.library()
    nan = float('nan')
    packed = torch.full((channels, plan.ld_frames), nan, device=device())
    packed[:, layout.frame_columns] = x.to(device())
    packed_dword = torch.full((channels, plan.ld_words), nan, device=device())
    packed_dword[:, layout.word_columns] = dword.to(device())
    top = torch.full((channels, plan.ld_words), nan, device=device())
    runtime.check(lib.emph_segment_reduce(
        packed.data_ptr(), plan.ld_frames, layout.view('bounds').data_ptr(),
        top.data_ptr(), plan.ld_words, channels,
        layout.view('table').data_ptr(), layout.view('word_segment').data_ptr(),
        plan.ld_words, runtime.REDUCTIONS[mode], runtime.stream()),
        'emph_segment_reduce')
    tiles, n_tiles = layout.tiles(64)
    results = []
    for launch in range(2):
        dx = torch.full((channels, plan.ld_frames), nan, device=device())
        runtime.check(lib.emph_segment_reduce_backward(
            packed_dword.data_ptr(), plan.ld_words,
            layout.view('bounds').data_ptr(), packed.data_ptr(),
            plan.ld_frames, top.data_ptr(), dx.data_ptr(), plan.ld_frames,
            channels, layout.view('table').data_ptr(), tiles.data_ptr(),
            n_tiles, runtime.REDUCTIONS[mode], runtime.stream()),
            'emph_segment_reduce_backward')
        results.append(dx[:, layout.frame_columns].cpu())
    got = results[0]
    assert torch.equal(got, results[1])
    narrow = reduce_reference(x, dword, mode, torch.float32)
    assert torch.isfinite(got).all()
    # frames no word covers, and the segment without words
    for column in (1, 2, 200, 239, 240, 244, 246, 249, 270, 380, 389):
        assert not got[:, column].any(), column
    if mode == 'max':
        # torch's tie rule, on the CPU: the first of equal maxima
        assert torch.equal(narrow[:, 252], dword[:, 4])
        assert not narrow[:, 260].any()
        assert torch.equal(narrow[:, 340], dword[:, 7])
        assert not narrow[:, 341:380].any()
        assert torch.equal(narrow[:, 75], dword[:, 2])
        assert not narrow[:, 150].any() and not narrow[:, 195].any()
    if mode == 'average':
        exact = reduce_reference(x, dword, mode, torch.float64)
        scale = exact.abs().max()
        allowed = 4. * float((narrow.double() - exact).abs().max() / scale)
        error = float((got.double() - exact).abs().max() / scale)
        print(f'average, {channels} channels: error {error:.3g}, '
              f'bound {allowed:.3g}')
        assert error <= allowed, (error, allowed)
    else:
        assert torch.equal(got, narrow), \
            (got - narrow).abs().max()


def test_segment_reduce_backward_refuses_unsorted_words():
    x = torch.randn(7, 40, device=device(), requires_grad=True)
    bounds = torch.tensor([[0, 8], [10, 20]])
    cu_frames, cu_words = torch.tensor([0, 40]), torch.tensor([0, 2])
    out = torch.ops.emphases_amd.segment_reduce(
        x, bounds, cu_frames, cu_words, 'sum')        # the forward accepts them
    with pytest.raises(ValueError, match='overlap'):
        out.sum().backward()


###############################################################################
# emph_activation_gradient
###############################################################################


@pytest.mark.parametrize('activation', ['relu', 'leaky_relu', 'gelu', 'silu'])
def test_activation_gradient(activation):
    tiny = float(np.finfo(np.float32).tiny)
    generator = torch.Generator().manual_seed(5)
    special = torch.tensor([0., -0., tiny, -tiny, 20., -20., 1., -1.])
    values = torch.cat([special, 3. * torch.randn(1016, generator=generator)])
    gradient = torch.randn(values.numel(), generator=generator)
    function = {'relu': torch.nn.functional.relu,
                'leaky_relu': torch.nn.functional.leaky_relu,
                'gelu': torch.nn.functional.gelu,
                'silu': torch.nn.functional.silu}[activation]

    def autograd(dtype):
        leaf = values.detach().clone().to(dtype).requires_grad_(True)
        out = function(leaf)
        out.backward(gradient.to(dtype))
        return leaf.grad.double(), out.detach()
    exact, _ = autograd(torch.float64)
    narrow, output = autograd(torch.float32)
    # relu / leaky_relu read the saved output, gelu / silu the pre-activation
    source = output if activation in ('relu', 'leaky_relu') else values
    lib = runtime.library()
    got = gradient.to(device())
    runtime.check(lib.emph_activation_gradient(
        source.to(device()).data_ptr(), got.data_ptr(), got.numel(),
        runtime.ACTIVATIONS[activation], runtime.stream()),
        'emph_activation_gradient')
    scale = exact.abs().max()
    allowed = 4. * float((narrow - exact).abs().max() / scale)
    error = float((got.cpu().double() - exact).abs().max() / scale)
    print(f'{activation}: error {error:.3g}, bound {allowed:.3g}')
    assert error <= allowed, (error, allowed)
    if activation == 'relu':
        old = gradient.to(device())
        runtime.check(lib.emph_activation_backward(
            source.to(device()).data_ptr(), old.data_ptr(), old.numel(),
            runtime.ACTIVATIONS['relu'], runtime.stream()),
            'emph_activation_backward')
        assert torch.equal(old, got)
    # EMPH_ACT_NONE is a no-op; a count that is no multiple of 4 is refused
    same = gradient.to(device())
    assert lib.emph_activation_gradient(
        same.data_ptr(), same.data_ptr(), same.numel(), 0,
        runtime.stream()) == 0
    assert torch.equal(same.cpu(), gradient)
    assert lib.emph_activation_gradient(
        same.data_ptr(), same.data_ptr(), 6, 1, runtime.stream()) == -1


###############################################################################
# torch.library.opcheck
###############################################################################

OPCHECKS = ('test_schema', 'test_autograd_registration', 'test_faketensor')


@pytest.mark.parametrize('activation', ['relu', 'gelu'])
def test_opcheck_conv1d_same_act(activation):
    generator = torch.Generator().manual_seed(2)
    x = torch.randn(5, 70, generator=generator).to(device()).requires_grad_(True)
    weight = (0.2 * torch.randn(16, 5, 3, generator=generator)).to(
        device()).requires_grad_(True)
    bias = torch.randn(16, generator=generator).to(device()).requires_grad_(True)
    torch.library.opcheck(
        torch.ops.emphases_amd.conv1d_same_act.default,
        (x, weight, bias, torch.tensor([0, 3, 70]), activation),
        test_utils=OPCHECKS)


@pytest.mark.parametrize('mode', ['sum', 'max'])
def test_opcheck_segment_reduce(mode):
    x = torch.randn(7, 70, generator=torch.Generator().manual_seed(3)).to(
        device()).requires_grad_(True)
    torch.library.opcheck(
        torch.ops.emphases_amd.segment_reduce.default,
        (x, torch.tensor([[0, 2, 10], [2, 3, 67]]), torch.tensor([0, 3, 70]),
         torch.tensor([0, 1, 3]), mode),
        test_utils=OPCHECKS)


def test_second_backward_raises_and_unasked_gradients_are_skipped():
    generator = torch.Generator().manual_seed(4)
    x = torch.randn(5, 70, generator=generator).to(device())
    weight = (0.2 * torch.randn(16, 5, 3, generator=generator)).to(
        device()).requires_grad_(True)
    bias = torch.zeros(16, device=device())
    out = torch.ops.emphases_amd.conv1d_same_act(
        x, weight, bias, torch.tensor([0, 3, 70]), 'silu')
    assert out.shape == (16, 70) and out.requires_grad
    with pytest.raises(RuntimeError, match='differentiable once'):
        torch.autograd.grad(out.sum(), weight, create_graph=True)
    out = torch.ops.emphases_amd.conv1d_same_act(
        x, weight, bias, torch.tensor([0, 3, 70]), 'silu')
    gradient, = torch.autograd.grad(out.sum(), weight)
    assert gradient.shape == weight.shape and not gradient.requires_grad
    assert x.grad is None and bias.grad is None
    reduced = torch.ops.emphases_amd.segment_reduce(
        out, torch.tensor([[0, 4], [3, 60]]), torch.tensor([0, 3, 70]),
        torch.tensor([0, 1, 2]), 'max')
    with pytest.raises(RuntimeError, match='differentiable once'):
        torch.autograd.grad(reduced.sum(), weight, create_graph=True)


###############################################################################
# The device-packed path (a weight whose version has changed)
###############################################################################


@pytest.mark.parametrize('c_in, c_out, k, activation', [
    (80, 80, 3, 'relu'), (80, 64, 5, 'gelu'), (64, 128, 7, 'leaky_relu'),
    (83, 16, 1, 'silu')])
def test_device_packed_path_against_torch(c_in, c_out, k, activation):
    """After an in-place update the op packs the weight on the device
    (`emph_take`) and runs direct-form `emph_conv1d`: its output and its three
    gradients against torch in float64, a segment at a time."""
    generator = torch.Generator().manual_seed(100 * c_in + c_out + k)
    total = sum(SEGMENTS)
    x = torch.randn(c_in, total, generator=generator)
    weight = torch.randn(c_out, c_in, k, generator=generator) / (c_in * k) ** 0.5
    bias = torch.randn(c_out, generator=generator)
    upstream = torch.randn(c_out, total, generator=generator)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(SEGMENTS)]))
    function = {'relu': torch.nn.functional.relu,
                'leaky_relu': torch.nn.functional.leaky_relu,
                'gelu': torch.nn.functional.gelu,
                'silu': torch.nn.functional.silu}[activation]

    def run_torch(dtype):
        leaves = [t.detach().clone().to(dtype).requires_grad_(True)
                  for t in (x, weight, bias)]
        out = torch.cat([function(torch.nn.functional.conv1d(
            leaves[0][None, :, first:first + count], leaves[1], leaves[2],
            padding='same'))[0]
            for first, count in zip(cu[:-1].tolist(), SEGMENTS)], dim=1)
        out.backward(upstream.to(dtype))
        return [out.detach().double()] + [leaf.grad.double() for leaf in leaves]
    exact, narrow = run_torch(torch.float64), run_torch(torch.float32)

    leaves = [t.to(device()).requires_grad_(True) for t in (x, weight, bias)]
    assert not ops._weight_changes(leaves[1])
    with torch.no_grad():
        leaves[1].add_(0)                      # what an optimizer step does
    assert ops._weight_changes(leaves[1])
    out = torch.ops.emphases_amd.conv1d_same_act(*leaves, cu, activation)
    out.backward(upstream.to(device()))
    got = [out.detach()] + [leaf.grad for leaf in leaves]
    for name, value, want, rounded in zip(
            ('out', 'dx', 'dweight', 'dbias'), got, exact, narrow):
        scale = want.abs().max()
        allowed = 4. * float((rounded - want).abs().max() / scale)
        error = float((value.cpu().double() - want).abs().max() / scale)
        print(f'device path ({c_in}, {c_out}, {k}, {activation}) {name}: '
              f'error {error:.3g}, bound {allowed:.3g}')
        assert error <= allowed, (name, error, allowed)


def test_host_pack_cache_answers_for_its_own_weight_alone():
    """The host-pack path (untouched weights): a transposed view of a square
    weight shares address, version and shape with it and must get a pack of
    its own; an entry keeps no weight alive; and a new weight - very likely
    at the dropped one's address - is convolved with its own values."""
    import gc
    import weakref
    generator = torch.Generator().manual_seed(8080)
    segments = [40, 23]
    cu = torch.tensor([0, 40, 63])
    x = torch.randn(80, sum(segments), generator=generator).to(device())
    bias = torch.randn(80, generator=generator).to(device())

    def conv(weight):
        assert not ops._weight_changes(weight)
        return torch.ops.emphases_amd.conv1d_same_act(
            x, weight, bias, cu, 'relu')
    w = (torch.randn(80, 80, 3, generator=generator) / 240 ** 0.5).to(device())
    first = conv(w)
    turned = conv(w.transpose(0, 1))
    assert torch.equal(turned, conv(w.transpose(0, 1).contiguous()))
    assert not torch.equal(turned, first)
    alive = weakref.ref(w.untyped_storage())
    del w
    gc.collect()
    assert alive() is None
    values = torch.randn(80, 80, 3, generator=generator) / 240 ** 0.5
    fresh, copy = values.to(device()), values.to(device())
    assert torch.equal(conv(fresh), conv(copy))


###############################################################################
# TorchModel
###############################################################################


def ragged():
    """The `ragged` case of tests/golden/train.npz, back to back on the
    device: (features, cu_frames, bounds, cu_words), targets."""
    data = train_data.golden()
    frames, words = data['ragged/frames'], data['ragged/words']
    cu = lambda counts: torch.from_numpy(  # noqa: E731
        np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    return (torch.from_numpy(data['ragged/features']).to(device()),
            cu(frames), torch.from_numpy(data['ragged/bounds']), cu(words)), \
        torch.from_numpy(data['ragged/targets']).to(device())


def loss_and_gradients(model, batch, targets):
    model.zero_grad(set_to_none=True)
    loss = train.loss_fn(model(*batch), targets, model.config.loss)
    loss.backward()
    return loss.detach(), {
        name: parameter.grad.clone()
        for name, parameter in model.named_parameters()}


def test_torch_model_matches_the_reference_and_the_trainer():
    golden = train_data.golden()
    reference_error = float(golden['ragged/ref32_error'])
    batch, targets = ragged()
    model = train.TorchModel(
        emphases_amd.DEFAULT, checkpoint=weights.DEFAULT_CHECKPOINT).to(device())
    loss, gradients = loss_and_gradients(model, batch, targets)
    again_loss, again = loss_and_gradients(model, batch, targets)
    assert torch.equal(loss, again_loss)
    for name in gradients:
        assert torch.equal(gradients[name], again[name]), name

    fused_loss, fused = train.Trainer(
        checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0).loss_and_gradients(
            *train_data.collated('ragged'))
    want_loss = float(golden['ragged/loss'])
    loss_error = abs(float(loss) - want_loss) / abs(want_loss)
    loss_apart = abs(float(loss) - float(fused_loss)) / abs(want_loss)
    print(f'loss {float(loss):.9g} (reference {want_loss:.9g}, trainer '
          f'{float(fused_loss):.9g}): error {loss_error:.3g}, apart '
          f'{loss_apart:.3g}, ref32_error {reference_error:.3g}')
    wanted = train_data.gradients('ragged')
    assert set(wanted) == set(gradients) == set(fused)
    missed = {}
    for name, want in wanted.items():
        got = gradients[name].cpu().numpy().astype(np.float64)
        other = fused[name].cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        scale = np.abs(want).max()
        error = np.abs(got - want).max() / scale
        apart = np.abs(got - other).max() / scale
        print(f'{name}: error {error / reference_error:.2f}, apart from the '
              f'trainer {apart / reference_error:.2f} (x ref32_error)')
        if not (error <= 4. * reference_error and
                apart <= 2. * reference_error):
            missed[name] = (error, apart)
    assert loss_error <= 4. * reference_error
    assert loss_apart <= 2. * reference_error
    assert not missed, (missed, reference_error)


def test_torch_model_trains_and_saves(tmp_path):
    """Five Adam steps lower the loss at every step; the saved state scores as
    the same weights loaded any other way."""
    batch, targets = ragged()
    model = train.TorchModel(
        emphases_amd.DEFAULT, checkpoint=weights.DEFAULT_CHECKPOINT).to(device())
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(5):
        optimizer.zero_grad(set_to_none=True)
        loss = train.loss_fn(model(*batch), targets, 'bce')
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(train.loss_fn(model(*batch), targets, 'bce')))
    print('losses', ' '.join(f'{loss:.9g}' for loss in losses))
    assert np.all(np.diff(losses) < 0), losses

    path = tmp_path / '00000005.pt'
    train.write_checkpoint(path, model.state_dict(), optimizer.state_dict(),
                           step=5)
    audio = torch.from_numpy(synth.audio(3, 211))
    alignment = emphases_amd.Alignment.from_frames(
        synth.word_frames(3, 211, 3, 40))
    from_file = emphases_amd.from_alignment_and_audio(
        alignment, audio, emphases_amd.SAMPLE_RATE, checkpoint=str(path), gpu=0)
    direct = session.Session(engine_module.Engine(
        emphases_amd.DEFAULT, weights.load(model.state_dict()), 0)).run(
            [alignment], [audio], on_device=True)[0]
    assert from_file.shape == direct.shape and from_file.shape[1] > 1
    assert torch.equal(from_file, direct)
    shipped = emphases_amd.from_alignment_and_audio(
        alignment, audio, emphases_amd.SAMPLE_RATE, gpu=0)
    assert not torch.equal(from_file, shipped)


###############################################################################
# The grid variants against the unmodified reference
###############################################################################

GRID = {
    'max': dict(downsample_method='max'),
    'center_loss': dict(downsample_method='center', downsample_location='loss'),
    'average_loss_mse': dict(downsample_method='average',
                             downsample_location='loss', loss='mse'),
    'gelu': dict(activation='gelu'),
    'silu': dict(activation='silu'),
    'leaky_relu': dict(activation='leaky_relu'),
    'c64_k5_k1': dict(channels=64, encoder_kernel_size=5, decoder_kernel_size=1),
    'c128_k7': dict(channels=128, encoder_kernel_size=7),
}


@pytest.mark.parametrize('variant', list(GRID))
def test_grid_variant_matches_the_reference(variant):
    """tests/golden/grid_<variant>.npz (tests/golden/generate_grid.py): two
    layers from the reference's initialisation under the stored seed, held to
    4 x the variant's own ref32_error."""
    with np.load(os.path.join(train_data.GOLDEN, f'grid_{variant}.npz')) as file:
        golden = {name: file[name] for name in file.files}
    config = emphases_amd.Config(layers=2, **GRID[variant])
    model = train.TorchModel(config, seed=int(golden['seed']))
    for name, parameter in model.named_parameters():
        value = parameter.detach().double().numpy()
        assert np.array_equal(
            golden[f'init/{name}'], [value.sum(), (value ** 2).sum()]), name
    model = model.to(device())
    batch, targets = ragged()
    loss, gradients = loss_and_gradients(model, batch, targets)
    bound = 4. * float(golden['ref32_error'])
    want_loss = float(golden['loss'])
    loss_error = abs(float(loss) - want_loss) / abs(want_loss)
    print(f'{variant}: loss {float(loss):.9g} (reference {want_loss:.9g}), '
          f'error {loss_error:.3g}, bound {bound:.3g}')
    wanted = {name[len('grad/'):]: value.astype(np.float64)
              for name, value in golden.items() if name.startswith('grad/')}
    assert wanted and set(wanted) <= set(gradients)
    if variant != 'c128_k7':
        assert set(wanted) == set(gradients)
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
