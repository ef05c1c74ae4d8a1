"""GPU: the input layer and the first encoder layer as ONE 5-tap layer
(emph_conv_compose_pack + emph_conv1d_stack_composed, Winograd F(4,5)) against
float64, against the two F(4,3) layers it replaces, and through the engine."""
import numpy as np
import pytest
import torch

from emphases_amd import batch, runtime, synth
from emphases_amd import config as cfg
from emphases_amd import engine as engine_module

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'

# 1 and 2: the two edge corrections overlap; 252 / 253 and 504 / 505 straddle
# span ownership; 1000: the workload's four spans
FRAMES = [1, 2, 3, 4, 5, 6, 37, 64, 65, 252, 253, 256, 257, 504, 505, 1000]


def ragged_plan(frames):
    segments = []
    for index, count in enumerate(frames):
        bounds = synth.word_frames(index, count, 1, 25)
        segments.append(batch.Segment(
            index, 0, bounds.shape[1], 0, 0, count, bounds))
    return batch.Plan(segments, [0] * len(frames), [0] * len(frames))


_SETUP = {}


def setup():
    """Plan, input (NaN in all padding), weights and the float64 reference of
    conv -> conv -> ReLU with the intermediate zero-padded: built once."""
    if _SETUP:
        return _SETUP
    plan = ragged_plan(FRAMES)
    x = torch.from_numpy(synth.weights(31, (80, plan.ld_frames), 1.0))
    x[:, :batch.LEAD] = float('nan')
    x[:, -batch.TAIL:] = float('nan')
    segments = list(zip(plan.frame_off, plan.frames))
    for off, count in segments:
        x[:, off + count:off + count + (-count) % 16] = float('nan')
    weights = [synth.weights(40 + l, (80, 80, 3), 0.12) for l in range(4)]
    biases = [synth.weights(50 + l, (80,), 0.3) for l in range(4)]
    want = []
    for off, count in segments:
        value = x[None, :, off:off + count].double()
        for l in range(2):
            value = torch.nn.functional.conv1d(
                value, torch.from_numpy(weights[l]).double(),
                torch.from_numpy(biases[l]).double(), padding=1)
        want.append(torch.relu(value)[0])
    spans_host = plan.conv_spans()
    _SETUP.update(
        plan=plan, x=x.to(DEVICE), segments=segments, weights=weights,
        biases=biases, want=want, n_spans=len(spans_host),
        spans=torch.from_numpy(spans_host).to(DEVICE),
        compose=torch.from_numpy(runtime.conv_compose_pack(
            weights[0], biases[0], weights[1], biases[1])).to(DEVICE),
        packs=torch.from_numpy(np.concatenate(
            [runtime.conv_winograd4_pack(w) for w in weights])).to(DEVICE),
        biases_dev=torch.from_numpy(np.concatenate(biases)).to(DEVICE))
    return _SETUP


def composed(s, source, layers, relu_mask):
    """emph_conv1d_stack_composed of the model layers 0 .. layers."""
    lib, ld = runtime.library(), s['plan'].ld_frames
    pack = s['packs'].numel() // 4
    y = torch.full((80, ld), 7.0, device=DEVICE)
    runtime.check(lib.emph_conv1d_stack_composed(
        source.data_ptr(), ld, y.data_ptr(), ld, s['compose'].data_ptr(),
        s['packs'][2 * pack:].data_ptr() if layers > 1 else None,
        s['biases_dev'][160:].data_ptr() if layers > 1 else None,
        layers, relu_mask, s['spans'].data_ptr(), s['n_spans'], None, None),
        'emph_conv1d_stack_composed')
    return y


def stacked(s, source, first, layers, relu_mask):
    """emph_conv1d_stack of the model layers first .. first + layers - 1."""
    lib, ld = runtime.library(), s['plan'].ld_frames
    pack = s['packs'].numel() // 4
    y = torch.full((80, ld), 7.0, device=DEVICE)
    runtime.check(lib.emph_conv1d_stack(
        source.data_ptr(), ld, y.data_ptr(), ld,
        s['packs'][first * pack:].data_ptr(),
        s['biases_dev'][80 * first:].data_ptr(), layers, relu_mask,
        s['spans'].data_ptr(), s['n_spans'], None, None), 'emph_conv1d_stack')
    return y


def test_composed_layer_against_float64():
    """One composed layer against conv -> conv -> ReLU in float64 (intermediate
    zero-padded: what the edge terms restore).  The bound is not a constant:
    1.5 x the largest error of today's launch of the two F(4,3) layers on the
    same inputs (an emulation of both in float32 with sequential accumulation
    gives 1.17 x; the margin is for the MFMA's order of accumulation).  The
    first and the last column of every segment meet that same bound
    separately - a wrong edge term is off by 0.1 and more.

    Measured (MI355X): all columns 3.87e-6 against the pair's 5.28e-6 (0.73 x);
    last columns 1.96e-6 (pair: 2.39e-6); first columns 3.10e-6, where the
    pair's own first columns are at 7.4e-7: a segment's first position is
    always output 0 of its quad, F(4,3)'s most accurate output and, through
    the cancellation among eight products, one of F(4,5)'s two least accurate
    (interior quads, float32 emulation: 1.7e-6 / 0.8e-6 / 0.9e-6 / 1.7e-6 for
    outputs 0 .. 3 of F(4,5), 1.0e-6 / 0.7e-6 / 1.2e-6 / 2.2e-6 for the
    pair) - the rounding of the layer, not of the edge term."""
    s = setup()
    got = composed(s, s['x'], 1, 0b1).cpu()
    pair = stacked(s, s['x'], 0, 2, 0b10).cpu()
    errors = {'all': [0., 0.], 'first': [0., 0.], 'last': [0., 0.]}
    for (off, count), want in zip(s['segments'], s['want']):
        for slot, y in enumerate((got, pair)):
            delta = (y[:, off:off + count].double() - want).abs()
            assert bool(torch.isfinite(delta).all()), count
            errors['all'][slot] = max(errors['all'][slot], float(delta.max()))
            errors['first'][slot] = max(
                errors['first'][slot], float(delta[:, 0].max()))
            errors['last'][slot] = max(
                errors['last'][slot], float(delta[:, -1].max()))
    for name, (new, old) in errors.items():
        print(f'{name}: |composed - f64| {new:.3e}, |two F(4,3) - f64| {old:.3e}, '
              f'ratio {new / old:.2f}')
    bound = 1.5 * errors['all'][1]
    for name, (new, _) in errors.items():
        assert new <= bound, (name, new, bound)
    # columns outside every segment are left untouched
    inside = torch.zeros(got.shape[1], dtype=torch.bool)
    for off, count in s['segments']:
        inside[off:off + count] = True
    assert bool((got[:, ~inside] == 7.0).all())


def test_three_layers_equal_one_plus_two():
    """The halo argument in bits: composed + F(4,3) + F(4,3) in one launch ==
    the composed layer alone followed by emph_conv1d_stack of the two."""
    s = setup()
    one = composed(s, s['x'], 3, 0b111)
    first = composed(s, s['x'], 1, 0b1)
    two = stacked(s, first, 2, 2, 0b11)
    one, two = one.cpu(), two.cpu()
    for off, count in s['segments']:
        assert torch.equal(one[:, off:off + count], two[:, off:off + count]), \
            (count, float((one[:, off:off + count] -
                           two[:, off:off + count]).abs().max()))


def utterances(frames):
    audios = [synth.audio(60 + i, n) for i, n in enumerate(frames)]
    bounds = [synth.word_frames(60 + i, n, 1, 25) for i, n in enumerate(frames)]
    return audios, bounds


def run(engine, audios, bounds, timed=False):
    """Scores per utterance of one ragged batch."""
    counts = [a.shape[1] // 160 for a in audios]
    segments = [batch.Segment(i, 0, b.shape[1], 432, n * 160, n, b)
                for i, (n, b) in enumerate(zip(counts, bounds))]
    lengths = [a.shape[1] for a in audios]
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    plan = batch.Plan(segments, offsets, lengths)
    packed = torch.cat(
        [torch.from_numpy(a).reshape(-1) for a in audios]).to(DEVICE)
    meta = engine.upload(plan)
    names = None
    if timed:
        engine.timers = []
    try:
        scores, _ = engine.forward(packed, plan, meta)
    finally:
        if timed:
            names = [name for name, *_ in engine.timers]
            engine.timers = None
    scores = scores.cpu()
    out = [scores[o:o + n].clone() for o, n in zip(plan.word_off, plan.words)]
    return out, names


def test_engine_compose_switch(monkeypatch):
    """EMPHASES_CONV_COMPOSE=1 (default) against =0 with the bundled
    checkpoint on utterances of 1, 37 and 1000 frames: scores within 1e-6; an
    utterance alone has the bits it has inside the batch; two conv launches
    per pass with the switch on, three with it off."""
    audios, bounds = utterances([1, 37, 1000])
    monkeypatch.setenv('EMPHASES_CONV_COMPOSE', '0')
    plain = engine_module.Engine(cfg.DEFAULT, None, 0)
    monkeypatch.setenv('EMPHASES_CONV_COMPOSE', '1')
    engine = engine_module.Engine(cfg.DEFAULT, None, 0)
    assert engine.compose and not plain.compose
    # (one frame per word: the two F(4,3) layers stay)
    assert not engine_module.Engine(
        cfg.Config(downsample_method='max'), None, 0).compose
    assert engine.model.compose and not plain.model.compose
    want, _ = run(plain, audios, bounds)
    got, _ = run(engine, audios, bounds)
    worst = 0.
    for a, b in zip(got, want):
        assert a.shape == b.shape and bool(torch.isfinite(a).all())
        worst = max(worst, float((a - b).abs().max()))
    print(f'max |score(compose) - score(two layers)| = {worst:.3e}')
    assert worst < 1e-6
    for index in range(len(audios)):
        alone, _ = run(engine, audios[index:index + 1], bounds[index:index + 1])
        assert torch.equal(alone[0], got[index]), index
    # step by step (timers on): the same launches, the same bits
    stepped, names = run(engine, audios, bounds, timed=True)
    assert names.count('conv1d_stack_frames_80x80_k3') == 2
    for a, b in zip(stepped, got):
        assert torch.equal(a, b)
    _, names = run(plain, audios, bounds, timed=True)
    assert names.count('conv1d_stack_frames_80x80_k3') == 3
