"""The backward of `ops.logmel` (`emph_logmel_backward`, csrc/frontend_grad.hip)
on the GPU against torch autograd of the float64 oracle on the CPU.

Yardstick (the project's for every gradient): with `want` the oracle's gradient
in float64 and `narrow` the same in float32,

    error = max|got - want| / max|want|
    bound = 4 * max|narrow - want| / max|want|

per signal.  Every comparison prints `logmel_backward <case>: error ... bound
... ratio ...`; profiles/logmel_backward_tests.txt holds those lines of one
run."""
import functools

import numpy as np
import pytest
import torch

import frontend_signals as fs
import logmel_grad_reference as reference
import emphases_amd
from emphases_amd import engine as engine_module, ops, runtime, synth, train
from emphases_amd.data.preprocess import mels
from oracle import prominence as oracle

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'
MARGIN = 4.
LENGTHS = (433, 864, 865, 5920, 16000, 16077)
SIGNALS = ('tone_440', 'dc_max', 'nyquist', 'chirp', 'noise_lsb')


def cu(counts):
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64)


def noise(samples, seed, amplitude=0.1):
    rng = np.random.default_rng(seed)
    return (amplitude * rng.standard_normal(samples)).astype(np.float32)


def cotangent(frames, seed):
    return np.random.default_rng(1000 + seed).standard_normal(
        (80, frames)).astype(np.float32)


def oracle_gradient(audio, weights, dtype, basis=None):
    """d sum(weights * logmel(audio)) / d audio by torch autograd on the CPU:
    audio float32 [S], weights float32 [80, F] (both widened exactly)."""
    leaf = torch.from_numpy(audio).to(dtype)[None].requires_grad_()
    out = oracle.log_of_mel(oracle.mel(leaf, basis))
    gradient, = torch.autograd.grad(
        (out * torch.from_numpy(weights).to(dtype)).sum(), leaf)
    return gradient[0]


@functools.lru_cache(maxsize=None)
def named_signal(name):
    """float32 [16000]."""
    if name == 'tone_440':
        n = np.arange(16000, dtype=np.float64)
        return fs.as_float(fs._pcm(fs.FULL * np.sin(2. * np.pi * 440. * n / 16000.)))
    return fs.as_float(fs.signals()[name][:16000])


def judge(case, got, want, narrow):
    """Print and assert the yardstick; returns error / bound."""
    want = want.double()
    scale = float(want.abs().max())
    assert scale > 0.
    error = float((got.double().cpu() - want).abs().max()) / scale
    bound = MARGIN * float((narrow.double() - want).abs().max()) / scale
    print(f'logmel_backward {case}: error {error:.3e} bound {bound:.3e} '
          f'ratio {error / bound:.3f}')
    assert error <= bound, (case, error, bound)
    return error / bound


def device_gradient(audio, weights, counts=None):
    """The gradient of the packed float32 audio through the op."""
    leaf = torch.from_numpy(audio).to(DEVICE).requires_grad_()
    out = ops.logmel(leaf, cu(counts or [len(audio)]))
    assert out.shape == weights.shape
    gradient, = torch.autograd.grad(
        (out * torch.from_numpy(weights).to(DEVICE)).sum(), leaf)
    return gradient


###############################################################################
# 1. before and after
###############################################################################


def test_the_gradient_exists():
    audio = torch.from_numpy(noise(16000, 1)).to(DEVICE).requires_grad_()
    out = torch.ops.emphases_amd.logmel(audio, cu([16000]))
    assert out.requires_grad
    gradient, = torch.autograd.grad(out.sum(), audio)
    assert gradient.shape == audio.shape and gradient.dtype == torch.float32
    assert bool(torch.isfinite(gradient).all())
    assert float(gradient.abs().max()) > 0.


###############################################################################
# 2. one chunk alone against the oracle
###############################################################################


@pytest.mark.parametrize('samples', LENGTHS)
def test_noise_of_every_length(samples):
    audio = noise(samples, samples)
    weights = cotangent(reference.frames_of(samples), samples)
    got = device_gradient(audio, weights)
    judge(f'noise S={samples}', got, oracle_gradient(audio, weights, torch.float64),
          oracle_gradient(audio, weights, torch.float32))


@pytest.mark.parametrize('samples', LENGTHS)
def test_one_row_of_one_frame(samples):
    """A cotangent that is zero but for one cell: a misplaced frame or bin is
    a wrong support."""
    audio = noise(samples, 7 + samples)
    frames = reference.frames_of(samples)
    weights = np.zeros((80, frames), dtype=np.float32)
    frame, row = (frames * 2) // 3, 5 + samples % 70
    weights[row, frame] = 1.5
    got = device_gradient(audio, weights)
    want = oracle_gradient(audio, weights, torch.float64)
    judge(f'one cell S={samples}', got, want,
          oracle_gradient(audio, weights, torch.float32))
    # outside the frame's samples (and their mirror images) the oracle's
    # gradient is exactly 0, and so is the device's
    outside = want == 0.
    padded = np.zeros(samples + 864, dtype=bool)
    padded[160 * frame:160 * frame + 1024] = True
    touched = np.zeros(samples, dtype=bool)
    np.logical_or.at(touched, reference.reflect_index(samples)[padded], True)
    assert bool(outside[torch.from_numpy(~touched)].all())
    assert bool((got.cpu()[outside] == 0.).all())
    assert bool((got.cpu()[torch.from_numpy(touched)] != 0.).any())


@pytest.mark.parametrize('name', SIGNALS)
def test_hard_signals(name):
    audio = named_signal(name)
    weights = cotangent(100, len(name))
    got = device_gradient(audio, weights)
    judge(name, got, oracle_gradient(audio, weights, torch.float64),
          oracle_gradient(audio, weights, torch.float32))


def test_silence_has_no_gradient():
    audio = np.zeros(16000, dtype=np.float32)
    weights = cotangent(100, 3)
    want = oracle_gradient(audio, weights, torch.float64)
    assert bool((want == 0.).all())
    got = device_gradient(audio, weights)
    assert bool((got == 0.).all())


###############################################################################
# 3. a batch
###############################################################################


BATCH = [16000, 5920, 40000]


@functools.lru_cache(maxsize=None)
def the_batch():
    """(audios, cotangents, the gradient of the three chunks back to back)."""
    audios = [synth.audio(7 + i, n // 160)[0, :n].astype(np.float32)
              for i, n in enumerate(BATCH)]
    weights = [cotangent(n // 160, 20 + i) for i, n in enumerate(BATCH)]
    together = device_gradient(
        np.concatenate(audios), np.concatenate(weights, axis=1), BATCH)
    return audios, weights, together


def test_a_batch_has_the_bits_of_its_chunks():
    audios, weights, together = the_batch()
    again = device_gradient(
        np.concatenate(audios), np.concatenate(weights, axis=1), BATCH)
    assert torch.equal(together, again)
    start = 0
    for index, (audio, weight) in enumerate(zip(audios, weights)):
        own = together[start:start + len(audio)]
        start += len(audio)
        assert torch.equal(own, device_gradient(audio, weight)), index


@pytest.mark.parametrize('index', range(len(BATCH)))
def test_every_chunk_of_a_batch_is_within_its_bound(index):
    """Chunk 2 (synth 9) has half a second of digital silence: the first
    frame after it has all of its energy in its last 30 samples, where the
    float32 `torch.hann_window` of the oracle and the exact Hann of the
    forward's table are 5.5e-4 relative apart, over a mel floor of 6.6e-5.  In
    float64 the two windows' gradients differ by 3.6e-6 of the largest element
    there - more than this bound - which is why the op's backward takes the
    reference's window (`ops._backward_table`)."""
    audios, weights, together = the_batch()
    start = sum(BATCH[:index])
    judge(f'batch chunk {index} S={BATCH[index]}',
          together[start:start + BATCH[index]],
          oracle_gradient(audios[index], weights[index], torch.float64),
          oracle_gradient(audios[index], weights[index], torch.float32))


def test_a_chunk_across_two_runs_of_the_tile_table():
    """More tiles than one run of the workspace holds (4094): a chunk that
    straddles the boundary has the bits it has alone."""
    long, short = 160 * 8 * 4000 + 77, 160 * 8 * 200 + 5
    generator = torch.Generator().manual_seed(5)
    first = 0.1 * torch.randn(long, generator=generator)
    second = 0.1 * torch.randn(short, generator=generator)
    weights = torch.randn((80, long // 160 + short // 160), generator=generator)

    def gradient(audio, counts, weight):
        leaf = audio.to(DEVICE).requires_grad_()
        out = ops.logmel(leaf, cu(counts))
        return torch.autograd.grad((out * weight.to(DEVICE)).sum(), leaf)[0]

    together = gradient(torch.cat([first, second]), [long, short], weights)
    alone = gradient(second, [short], weights[:, long // 160:])
    assert torch.equal(together[long:], alone)
    assert bool(torch.isfinite(together).all())
    # ... and the long one, which spans the boundary itself, against itself
    # behind the short one (its tiles then fall elsewhere in the runs)
    swapped = gradient(
        torch.cat([second, first]), [short, long],
        torch.cat([weights[:, long // 160:], weights[:, :long // 160]], dim=1))
    assert torch.equal(swapped[short:], together[:long])


###############################################################################
# 4. the forward is untouched
###############################################################################


def test_the_forward_has_the_bits_it_had():
    audio = torch.from_numpy(noise(16077, 4)).to(DEVICE)
    plain = ops.logmel(audio, cu([16077]))
    assert not plain.requires_grad
    tracked = ops.logmel(audio.clone().requires_grad_(), cu([16077]))
    assert tracked.requires_grad
    assert torch.equal(plain, tracked.detach())
    named = mels.from_audio(audio[None])
    named_tracked = mels.from_audio(audio[None].clone().requires_grad_())
    assert named_tracked.requires_grad and not named.requires_grad
    assert torch.equal(named, named_tracked.detach())
    assert torch.equal(named, plain)
    pcm = (audio * 32767.).round().to(torch.int16)
    assert not ops.logmel(pcm, cu([16077])).requires_grad


def test_from_audio_is_differentiable():
    leaf = torch.from_numpy(noise(5920, 9)).to(DEVICE)[None].requires_grad_()
    out = mels.from_audio(leaf)
    gradient, = torch.autograd.grad(out.sum(), leaf)
    assert gradient.shape == leaf.shape
    direct = device_gradient(noise(5920, 9), np.ones((80, 37), dtype=np.float32))
    assert torch.equal(gradient[0], direct)


###############################################################################
# 5. once
###############################################################################


def test_create_graph_raises():
    audio = torch.from_numpy(noise(1600, 2)).to(DEVICE).requires_grad_()
    out = ops.logmel(audio, cu([1600]))
    with pytest.raises(RuntimeError, match='differentiable once'):
        torch.autograd.grad(out.sum(), audio, create_graph=True)


###############################################################################
# 6. the clamp, through the C ABI
###############################################################################


@pytest.fixture(scope='module')
def engine():
    return engine_module.Engine(device=0)


def test_the_clamp_stops_the_gradient(engine):
    """The bundled basis scaled by 0.015: on quiet noise whose second half is
    30 times louder, 3 % of the cells clamp; a second, silent chunk clamps in
    every row."""
    scale, seed, samples, silent = np.float32(0.015), 24, 8000, 1600
    audio = noise(samples, seed, 1e-3)
    audio[samples // 2:] *= 30
    basis = oracle.mel_basis() * scale                       # float32
    mel = oracle.mel(torch.from_numpy(audio).double()[None], basis.double())
    clamped = mel < 1e-5
    assert int(clamped.sum()) >= 0.01 * mel.numel()
    assert float(((mel - 1e-5).abs() / 1e-5).min()) > 1e-3
    quiet = oracle.mel(torch.zeros((1, silent), dtype=torch.float64), basis.double())
    assert bool((quiet < 1e-5).all())

    lib = runtime.library()
    chunks = [samples, silent]
    frames = [fs.frames_of(n) for n in chunks]
    lead, gap = 5, 3
    table = np.zeros((2, runtime.SEG_FIELDS), dtype=np.int64)
    tiles, cursor, offset = [], lead, 3
    for index, (n, count) in enumerate(zip(chunks, frames)):
        table[index, runtime.SEG_AUDIO_OFF] = offset
        table[index, runtime.SEG_AUDIO_LEN] = n
        table[index, runtime.SEG_START] = 432
        table[index, runtime.SEG_LENGTH] = n
        table[index, runtime.SEG_FRAME_OFF] = cursor
        table[index, runtime.SEG_FRAMES] = count
        tiles += [(index, first, cursor, count) for first in range(0, count, 8)]
        cursor += count + gap
        offset += n + 7
    ld = cursor + 8
    assert int(lib.emph_frontend_block()) == 8
    host = np.full(offset + 5, np.nan, dtype=np.float32)     # NaN between the chunks
    host[3:3 + samples] = audio
    host[3 + samples + 7:3 + samples + 7 + silent] = 0.
    weights = [cotangent(count, 40 + i) for i, count in enumerate(frames)]
    dmel = np.full((80, ld), np.nan, dtype=np.float32)
    for index, weight in enumerate(weights):
        first = int(table[index, runtime.SEG_FRAME_OFF])
        dmel[:, first:first + weight.shape[1]] = weight
    sentinel = -777.
    to = lambda array: torch.from_numpy(np.ascontiguousarray(array)).to(DEVICE)
    audio_dev, seg_dev, dmel_dev = to(host), to(table), to(dmel)
    tiles_dev = to(np.array(tiles, dtype=np.int32))
    values = engine.mel_values * float(scale)
    daudio = torch.full_like(audio_dev, sentinel)
    workspace = torch.empty(int(lib.emph_logmel_backward_workspace(len(tiles))),
                            dtype=torch.float32, device=DEVICE)
    runtime.check(lib.emph_logmel_backward(
        audio_dev.data_ptr(), seg_dev.data_ptr(), tiles_dev.data_ptr(), len(tiles),
        engine.table.data_ptr(), engine.mel_start.data_ptr(),
        engine.mel_count.data_ptr(), engine.mel_offset.data_ptr(),
        values.data_ptr(), engine.mel_nnz, dmel_dev.data_ptr(), ld, 0,
        workspace.data_ptr(), daudio.data_ptr(), None), 'emph_logmel_backward')
    torch.cuda.synchronize()
    got = daudio.cpu()
    # samples outside every chunk are not touched
    inside = np.zeros(len(host), dtype=bool)
    inside[3:3 + samples] = True
    inside[3 + samples + 7:3 + samples + 7 + silent] = True
    assert bool((got[torch.from_numpy(~inside)] == sentinel).all())
    judge('clamp', got[3:3 + samples],
          oracle_gradient(audio, weights[0], torch.float64, basis.double()),
          oracle_gradient(audio, weights[0], torch.float32, basis))
    assert bool((got[3 + samples + 7:3 + samples + 7 + silent] == 0.).all())


###############################################################################
# 7. end to end
###############################################################################


def test_the_gradient_of_the_logits_reaches_the_audio():
    config = emphases_amd.Config(layers=2)
    model = train.TorchModel(config, seed=3).to(DEVICE)
    audio = synth.audio(11, 100)[0, :16000].astype(np.float32)
    bounds = np.array([[2, 30, 61], [30, 58, 100]], dtype=np.int64)
    leaf = torch.from_numpy(audio).to(DEVICE).requires_grad_()
    features = ops.logmel(leaf, cu([16000]))
    logits = model(features, cu([100]), torch.from_numpy(bounds).to(DEVICE), cu([3]))
    got, = torch.autograd.grad(logits.sum(), leaf)

    def composition(dtype):
        state = {name: value.detach().cpu().to(dtype)
                 for name, value in model.state_dict().items()}
        source = torch.from_numpy(audio).to(dtype)[None].requires_grad_()
        x = oracle.logmel(source)

        def conv(x, name):
            weight = state[f'{name}.weight']
            module = torch.nn.Conv1d(weight.shape[1], weight.shape[0],
                                     weight.shape[2], padding='same', dtype=dtype)
            module.load_state_dict({'weight': weight, 'bias': state[f'{name}.bias']})
            return module(x[None])[0]

        x = conv(x, 'input_layer')
        for i in range(config.layers):
            x = torch.relu(conv(x, f'frame_encoder.{2 * i}'))
        x = oracle.downsample(x, bounds, config.downsample_method)
        for i in range(config.layers):
            x = torch.relu(conv(x, f'word_decoder.{2 * i}'))
        x = conv(x, 'output_layer')[0]
        gradient, = torch.autograd.grad(x.sum(), source)
        return gradient[0], x.detach()

    want, want_logits = composition(torch.float64)
    narrow, _ = composition(torch.float32)
    assert float((logits.detach().cpu().double() - want_logits).abs().max()) < 1e-3
    judge('end to end', got, want, narrow)
