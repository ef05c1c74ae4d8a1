"""Every path `Engine` can take, at every precision, against the float64 oracle.

`Engine` picks its kernels through a dozen gates (configuration, precision,
EMPHASES_* switches).  Each row of `ROWS` is one configuration and
environment; it names the path the engine must take, asserted before any
number is looked at, so that a later gate change cannot quietly drop a path
from coverage.  Per row and precision:

  - the logits and scores of the production `forward` (no `stages`) against
    `oracle.forward` in float64, fed the engine's own features (upcast) and
    the row's weights (upcast), with an output gain that keeps max |logit| in
    (2, 4] so that no score is saturated;
  - batch invariance: a segment alone, in the batch and in the reversed batch
    gives the same bits;
  - determinism: two passes give the same bits.

The batch straddles the engine's thresholds: 16 / 17 frames, 127 / 128 / 129
(GROUPED_FROM), 255 / 256 / 257 (ATTENTION_GROUP), 64 and 65 words in one
segment (FUSED_WORDS), one-word segments, one-frame words, words that end on
the last frame, a chunked long utterance and, for the Transformer, a segment of
MAX_POSITIONS frames.

`test_packed_axis_boundary` runs one utterance of about 12 hours, whose
packed frame axis crosses 2^22 columns (the limit of the 16-position split
kernels; `Engine.sub_plans`).
"""
import functools
import gc
import math

import numpy as np
import pytest
import torch

import emphases_amd
from emphases_amd import batch, config as cfg, engine as engine_module
from emphases_amd import synth, weights
from oracle import prominence as oracle

PRECISIONS = ['f32', 'bf16x3', 'bf16x3_fast', 'bf16x6']
# |logit - float64 oracle| / max |logit|; the split precisions keep the
# budgets the existing tests hold their scores to against the f32 engine
BUDGETS = {'f32': 5e-6, 'bf16x3': 1e-5, 'bf16x3_fast': 5e-5, 'bf16x6': 3e-6}
SPLIT = ('bf16x3', 'bf16x3_fast')      # the split conv's precisions


def conv(name, path, env=None, **overrides):
    """`path`: quad (F(4,3) frame-rate convs), stack (emph_conv1d_stack /
    emph_conv1d_split), fold (the word sums in the last layer's epilogue)."""
    return dict(name=name, overrides=overrides, env=env or {}, path=path)


def transformer(name, path, env=None, **overrides):
    """`path`: quad (the input layer on F(4,3)), block (the fused fp32
    position-wise block on the frame encoder), split (its split-bf16 form at
    the opt-in precisions), words (the one-launch word decoder), attention
    (emph_attention_split for the long segments at the opt-in precisions)."""
    return dict(name=name, overrides=dict(architecture='transformer',
                                          **overrides),
                env=env or {}, path=path)


FAST = dict(quad=True, stack=True, fold=True)
QUAD = dict(quad=True, stack=False, fold=False)
DIRECT = dict(quad=False, stack=False, fold=False)
T80 = dict(quad=True, block=True, split=True, words=True, attention=True)

ROWS = [
    conv('conv', FAST),
    conv('conv_layers0', dict(quad=True, stack=True, fold=False), layers=0),
    *[conv(f'conv_layers{n}', FAST, layers=n) for n in (1, 2, 3, 4, 5, 8)],
    conv('conv_channels64', dict(quad=True, stack=False, fold=True),
         channels=64),
    conv('conv_channels128', DIRECT, channels=128),
    conv('conv_kernel5', DIRECT, encoder_kernel_size=5),
    conv('conv_gelu', DIRECT, activation='gelu'),
    conv('conv_leaky_relu', DIRECT, activation='leaky_relu'),
    conv('conv_max', dict(quad=True, stack=True, fold=False),
         downsample_method='max'),
    conv('conv_center', dict(quad=True, stack=True, fold=False),
         downsample_method='center'),
    conv('conv_input', QUAD, downsample_location='input'),
    conv('conv_inference', FAST, downsample_location='inference'),
    conv('conv_loss', FAST, downsample_location='loss'),
    conv('conv_no_stack', dict(quad=True, stack=False, fold=True),
         env=dict(EMPHASES_CONV_STACK='0')),
    conv('conv_no_fold', dict(quad=True, stack=True, fold=False),
         env=dict(EMPHASES_FOLD_WORD_SUMS='0')),
    transformer('tf', T80),
    transformer('tf_64x2', dict(quad=True, block=True, split=False,
                                words=True, attention=False),
                channels=64, heads=2),
    transformer('tf_64x1', dict(quad=True, block=True, split=False,
                                words=False, attention=False),
                channels=64, heads=1),
    transformer('tf_128x2', dict(quad=False, block=False, split=False,
                                 words=False, attention=False),
                channels=128, heads=2),
    transformer('tf_128x4', dict(quad=False, block=False, split=False,
                                 words=False, attention=False),
                channels=128, heads=4),
    transformer('tf_120x3', dict(quad=False, block=False, split=False,
                                 words=False, attention=True),
                channels=120, heads=3),
    transformer('tf_40x1', dict(quad=True, block=False, split=False,
                                words=False, attention=True),
                channels=40, heads=1),
    transformer('tf_layers1', T80, layers=1),
    transformer('tf_layers2', T80, layers=2),
    # the (location, method) pairs the reference goldens leave out
    *[transformer(f'tf_{location}_{method}',
                  dict(T80, words=location == 'intermediate'),
                  downsample_location=location, downsample_method=method)
      for location, method in (
          ('intermediate', 'average'), ('intermediate', 'max'),
          ('intermediate', 'center'), ('inference', 'sum'),
          ('inference', 'max'), ('inference', 'center'), ('loss', 'sum'),
          ('loss', 'average'), ('loss', 'max'), ('loss', 'center'))],
    *[transformer(f'tf_input_{method}', T80, downsample_location='input',
                  downsample_method=method)
      for method in ('average', 'max')],
    transformer('tf_split_tile32', T80, env=dict(EMPHASES_SPLIT_TILE='32')),
    transformer('tf_no_fuse_qkv', T80, env=dict(EMPHASES_FUSE_QKV='0')),
]

REFUSED = [
    (dict(architecture='transformer', channels=80, heads=4),
     'head dimension 20'),
    (dict(architecture='transformer', channels=80, heads=1),
     'head dimension 80'),
    (dict(architecture='transformer', channels=96), 'head dimension 48'),
    (dict(architecture='transformer', channels=256, heads=4),
     'channels 256 > 128'),
    (dict(channels=120), 'channels 120 not a multiple of 16'),
    (dict(architecture='transformer', channels=120, heads=3,
          downsample_location='inference'), 'channels 120 not a multiple'),
    (dict(architecture='transformer', channels=40, heads=1,
          downsample_location='loss'), 'channels 40 not a multiple'),
    (dict(decoder_kernel_size=7), 'decoder kernel size 7'),
    (dict(layers=17), '17 convolution layers'),
    (dict(layers=16, decoder_kernel_size=5), 'receptive field'),
]


def cases():
    for row in ROWS:
        transformer_row = row['overrides'].get('architecture') == 'transformer'
        for precision in PRECISIONS:
            if precision == 'bf16x3_fast' and not transformer_row:
                continue          # (the conv path: bf16x3's kernels again)
            yield pytest.param(row, precision, id=f'{row["name"]}-{precision}')


###############################################################################
# the batch
###############################################################################


def _words(*lengths):
    ends = np.cumsum(lengths)
    return np.stack([ends - np.asarray(lengths), ends]).astype(np.int64)


def utterances(transformer_row):
    """(frames, word bounds in frames, batch_size) of every utterance."""
    rows = [
        (16, _words(5, 11), None),                       # a word ends on 16
        (17, _words(17), None),                          # one word
        (127, _words(*[1] * 63, 64), None),              # 64 words
        (128, _words(*[1] * 64, 64), None),              # 65 words
        (129, synth.word_frames(5, 129, 2, 40), None),
        (255, synth.word_frames(6, 255), None),
        (256, _words(256), None),                        # one word of 256
        (257, synth.word_frames(8, 257, 1, 30), None),
        (1500, synth.word_frames(9, 1500), 400),         # chunked
    ]
    if transformer_row:
        rows.append((cfg.MAX_POSITIONS, synth.word_frames(10, cfg.MAX_POSITIONS),
                     None))
    return rows


class Batch:
    def __init__(self, transformer_row, device):
        self.segments, lengths, audios = [], [], []
        for index, (frames, bounds, batch_size) in enumerate(
                utterances(transformer_row)):
            audios.append(synth.audio(60 + index, frames)[0])
            lengths.append(frames * 160)
            self.segments.extend(batch.chunk_utterance(
                emphases_amd.Alignment.from_frames(bounds), frames * 160,
                batch_size, index))
        self.offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        self.lengths = lengths
        self.audio = torch.from_numpy(np.concatenate(audios)).to(device)
        self.plan = self.plan_of(self.segments)
        frames = sorted(s.frames for s in self.segments)
        words = sorted(s.bounds.shape[1] for s in self.segments)
        for count in (16, 17, 127, 128, 129, 255, 256, 257):
            assert count in frames
        assert 64 in words and 65 in words and 1 in words
        if transformer_row:
            assert cfg.MAX_POSITIONS in frames
        assert sum(s.utterance == 8 for s in self.segments) > 2

    def plan_of(self, segments):
        return batch.Plan(segments, self.offsets, self.lengths)


@functools.lru_cache(maxsize=None)
def the_batch_of(transformer_row):
    return Batch(transformer_row, torch.device('cuda', 0))


def segment_logits(plan, logits):
    """Per segment, its words' entries of a packed word-axis vector."""
    values = logits.cpu().numpy()
    return [values[o:o + n] for o, n in zip(plan.word_off, plan.words)]


def double(state):
    return {k: torch.from_numpy(np.asarray(v)).double()
            for k, v in state.items()}


###############################################################################
# the float64 reference of a row
###############################################################################


_REFERENCE = {}


def reference(row, config, the_batch):
    """(gained float32 state, float64 oracle logits per segment) of a row:
    built once, from the features of an f32 engine's stage dump."""
    if row['name'] in _REFERENCE:
        return _REFERENCE[row['name']]
    state = weights.random_state(config, seed=17)
    engine = engine_module.Engine(config, state, 0)
    stages = {}
    engine.forward(the_batch.audio, the_batch.plan, stages=stages)
    features = stages['features'].cpu().double()
    del engine
    plan = the_batch.plan
    features = [features[:, o:o + n]
                for o, n in zip(plan.frame_off, plan.frames)]
    gain, want, scale, floor = oracle_logits(
        state, features, plan.segments, row['overrides'])
    gained = weights.random_state(config, seed=17, output_gain=gain)
    _REFERENCE[row['name']] = (gained, want, scale, features, floor)
    return _REFERENCE[row['name']]


def oracle_logits(state, features, segments, overrides):
    """(gain, float64 logits per segment with that output gain, their scale,
    floor): `floor` is the float32 oracle's own |dlogit| / scale on the same inputs - the
    conditioning floor: how far ANY float32 evaluation of this model may be
    from float64 (the reference's own arithmetic is that far)."""
    state64 = double(state)
    state32 = {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}
    want = [oracle.forward(f, segment.bounds, state64, overrides)
            for f, segment in zip(features, segments)]
    single = [oracle.forward(f.float(), segment.bounds, state32, overrides)
              for f, segment in zip(features, segments)]
    largest = max(float(v.abs().max()) for v in want)
    # the goldens' rule: a power of two that puts max |logit| in (2, 4]
    gain = 2.0 ** math.floor(math.log2(4.0 / largest))
    scale = largest * gain
    assert 2. < scale <= 4.
    floor = max(float((a.double() - b).abs().max())
                for a, b in zip(single, want)) / largest
    return gain, [(v * gain).numpy() for v in want], scale, floor


def assert_path(engine, row, precision):
    path, config = row['path'], engine.config
    opt_in = precision != 'f32'
    assert engine.precision == precision
    assert engine.quad == path['quad']
    if config.architecture == 'convolution':
        assert engine.stack == path['stack']
        assert engine.fold == path['fold']
        assert engine.split_conv == (path['stack'] and precision in SPLIT)
        return
    assert not engine.stack and not engine.fold and not engine.split_conv
    assert (engine.word_transformer is not None) == path['words']
    layers = engine.frame_encoder
    assert [layer['block'] is not None for layer in layers] == \
        [path['block']] * config.layers
    assert [layer['block_split'] is not None for layer in layers] == \
        [path['split'] and opt_in] * config.layers
    assert (engine.attention_pieces != 0 and
            config.channels // config.heads == 40) == \
        (path['attention'] and opt_in)
    assert engine.split_tile == int(
        row['env'].get('EMPHASES_SPLIT_TILE', 16))
    assert engine.fuse_qkv == (row['env'].get('EMPHASES_FUSE_QKV') != '0')


# (row, precision) -> (|dlogit| / scale measured on an MI355X, cause): the cells
# over their budget.  Each stays an expected failure only while it is over the
# budget (within budget: drop it here) and within 10 % of what was measured
SPLIT_CONV = ('two bf16 pieces per operand (2^-17 each) through every frame-rate '
              'layer: bf16x3 by design; it grows with the layers (1 layer: 5e-6, '
              '8: 2.8e-5) and with max / center pooling, which average nothing')
DECODER = ('the float64 decoder itself amplifies the frame stage\'s error of the '
           'word embeddings (3e-7 at f32, the default row\'s) to this: the word '
           'stage alone, fed the engine\'s embeddings, is 3.7e-6 - 6.3e-6')
CONV_FP32 = ('bf16x6 leaves the conv path in fp32: bitwise the f32 cell, which '
             'is within the f32 budget')
MAX_POOL = ('max pooling hands the f32 frame encoder\'s per-element error '
            '(2.3e-6 of its maximum, as in every Transformer row) to the '
            'output layer unaveraged; sum pooling of the same encoder: 8.1e-7')
FINDINGS = {
    ('conv', 'bf16x3'): (1.75e-05, SPLIT_CONV),
    ('conv_layers8', 'bf16x3'): (2.83e-05, SPLIT_CONV),
    ('conv_max', 'bf16x3'): (5.20e-05, SPLIT_CONV),
    ('conv_center', 'bf16x3'): (5.97e-05, SPLIT_CONV),
    ('conv_inference', 'bf16x3'): (1.18e-05, SPLIT_CONV),
    ('conv_loss', 'bf16x3'): (1.18e-05, SPLIT_CONV),
    ('conv_no_fold', 'bf16x3'): (1.77e-05, SPLIT_CONV),
    ('boundary_convolution', 'bf16x3'): (1.16e-05, SPLIT_CONV),
    ('conv_leaky_relu', 'bf16x6'): (3.34e-06, CONV_FP32),
    ('conv_center', 'bf16x6'): (3.29e-06, CONV_FP32),
    ('tf_64x2', 'f32'): (1.79e-05, DECODER),
    ('tf_64x2', 'bf16x3'): (1.79e-05, DECODER),
    ('tf_64x2', 'bf16x6'): (1.79e-05, DECODER),
    ('tf_layers1', 'f32'): (5.31e-06, DECODER),
    ('tf_layers1', 'bf16x3'): (6.23e-05, DECODER),
    ('tf_layers1', 'bf16x3_fast'): (1.06e-04, DECODER),
    ('tf_layers1', 'bf16x6'): (1.12e-05, DECODER),
    ('tf_layers2', 'f32'): (1.15e-05, DECODER),
    ('tf_layers2', 'bf16x3'): (4.49e-05, DECODER),
    ('tf_layers2', 'bf16x3_fast'): (9.40e-05, DECODER),
    ('tf_layers2', 'bf16x6'): (4.40e-06, DECODER),
    ('tf_inference_max', 'f32'): (5.70e-06, MAX_POOL),
    ('tf_inference_max', 'bf16x6'): (3.41e-06, MAX_POOL),
    ('tf_loss_max', 'f32'): (5.70e-06, MAX_POOL),
    ('tf_loss_max', 'bf16x6'): (3.41e-06, MAX_POOL),
    ('tf_120x3', 'bf16x6'): (3.18e-06, 'within 1.3x the float32 oracle\'s own '
                             'error on the same inputs (2.4e-6)'),
}


def within_budget(relative, score, precision, name):
    """The row budget (BUDGETS), or the cell's entry in FINDINGS."""
    budget = BUDGETS[precision]
    if (name, precision) not in FINDINGS:
        assert relative < budget and score < budget, (relative, score, budget)
        return
    measured, cause = FINDINGS[name, precision]
    assert relative >= budget, \
        f'{name} {precision}: {relative:.2e} is within budget now'
    assert relative < 1.1 * measured and score < 1.1 * measured, \
        (relative, score, measured)
    pytest.xfail(f'{relative:.2e} over the {budget:.0e} budget: {cause}')


@pytest.mark.gpu
@pytest.mark.parametrize('row,precision', list(cases()))
def test_path_against_float64_oracle(row, precision, monkeypatch):
    for key, value in row['env'].items():
        monkeypatch.setenv(key, value)
    config = cfg.Config(**row['overrides'])
    transformer_row = config.architecture == 'transformer'
    the_batch = the_batch_of(transformer_row)
    state, want, scale, features, floor = reference(row, config, the_batch)
    engine = engine_module.Engine(config, state, 0, precision=precision)
    try:
        assert_path(engine, row, precision)
        plan = the_batch.plan
        # the features this precision sees are the ones the oracle was fed
        stages = {}
        engine.forward(the_batch.audio, plan, stages=stages)
        seen = stages['features'].cpu().double()
        for o, n, fed in zip(plan.frame_off, plan.frames, features):
            assert torch.equal(seen[:, o:o + n], fed)
        # the production path: no stage dump
        scores, logits = engine.forward(the_batch.audio, plan)
        scores, logits = scores.clone(), logits.clone()
        worst, worst_score = 0., 0.
        for got, got_scores, reference_logits in zip(
                segment_logits(plan, logits), segment_logits(plan, scores),
                want):
            worst = max(worst, float(np.abs(got - reference_logits).max()))
            reference_scores = oracle.postprocess(
                torch.from_numpy(reference_logits), config.loss).numpy()
            worst_score = max(worst_score, float(
                np.abs(got_scores - reference_scores).max()))
        # determinism (the word columns: padding is undefined)
        columns = torch.from_numpy(plan.word_columns()).to(scores.device)
        again, _ = engine.forward(the_batch.audio, plan)
        assert torch.equal(again[columns], scores[columns])
        # a segment alone, in the batch, in the reversed batch
        segments = the_batch.segments
        reverse = the_batch.plan_of(segments[::-1])
        backwards = segment_logits(
            reverse, engine.forward(the_batch.audio, reverse)[0])[::-1]
        batched = segment_logits(plan, scores)
        for index in (1, 6, len(segments) - 1):
            alone = the_batch.plan_of([segments[index]])
            single = segment_logits(
                alone, engine.forward(the_batch.audio, alone)[0])[0]
            assert np.array_equal(single, batched[index]), index
            assert np.array_equal(single, backwards[index]), index
        # bf16x6 leaves the conv path in fp32: bitwise the f32 engine
        if precision == 'bf16x6' and not transformer_row:
            plain = engine_module.Engine(config, state, 0)
            assert torch.equal(
                plain.forward(the_batch.audio, plan)[0][columns],
                scores[columns])
            del plain
        print(f'{row["name"]} {precision}: |dlogit| / scale '
              f'{worst / scale:.2e} (budget {BUDGETS[precision]:.0e}; the '
              f'float32 oracle: {floor:.2e}), |dscore| {worst_score:.2e}')
        within_budget(worst / scale, worst_score, precision, row['name'])
    finally:
        del engine
        gc.collect()


@pytest.mark.parametrize('overrides,message', REFUSED)
def test_unsupported_configuration_is_refused(overrides, message):
    """Configurations no kernel set can run are refused by the constructor,
    before a device is touched - not by the first kernel in `forward`."""
    config = cfg.Config(**overrides)
    with pytest.raises(ValueError, match=message):
        engine_module.Engine(config, weights.random_state(config), 0)


###############################################################################
# a packed frame axis past 2^22 columns
###############################################################################


BOUNDARY_FRAMES = 4_300_000     # about 11.9 hours
BOUNDARY_CHUNK = 4000           # frames per chunk: inside the position table


@pytest.fixture(scope='module')
def long_utterance():
    """One ~12 h utterance as 16-bit PCM (a 20 s synthetic clip tiled), and
    its word bounds: 1.4 GB of audio rather than 2.8 GB of float32."""
    clip = np.rint(synth.audio(77, 2000)[0] * 32768.).astype(np.int16)
    pcm = np.tile(clip, -(-BOUNDARY_FRAMES * 160 // clip.size))[
        :BOUNDARY_FRAMES * 160]
    bounds = synth.word_frames(77, BOUNDARY_FRAMES)
    segments = batch.chunk_utterance(
        emphases_amd.Alignment.from_frames(bounds), pcm.size, BOUNDARY_CHUNK)
    return torch.from_numpy(pcm), segments


@pytest.mark.gpu
@pytest.mark.parametrize('architecture', ['convolution', 'transformer'])
@pytest.mark.parametrize('precision', ['f32', 'bf16x3'])
def test_packed_axis_boundary(long_utterance, architecture, precision):
    """One utterance whose chunked plan packs more than 2^22 frame columns:
    the first, a middle and the last segment score bitwise as in a plan of
    their own, and within the row budget of the float64 oracle.  (The
    16-position split kernels address rows with 32-bit byte offsets: the
    engine runs such a plan as sub-plans below the limit; the f32 kernels
    take it in one pass, with qk buffers past 2^31 bytes.)"""
    pcm, segments = long_utterance
    config = cfg.Config(architecture=architecture)
    chosen = (0, len(segments) // 2, len(segments) - 1)
    plans = [batch.Plan([segments[i]], [0], [pcm.numel()]) for i in chosen]
    audio = pcm.to(torch.device('cuda', 0))
    # the float64 oracle of the chosen segments, on the engine's features
    state = weights.random_state(config, seed=21)
    engine = engine_module.Engine(config, state, 0)
    features = []
    for alone in plans:
        stages = {}
        engine.forward(audio, alone, stages=stages)
        features.append(stages['features'][:, alone.frame_off[0]:][
            :, :alone.frames[0]].cpu().double())
    del engine
    gain, want, scale, floor = oracle_logits(
        state, features, [segments[i] for i in chosen],
        {'architecture': architecture})
    state = weights.random_state(config, seed=21, output_gain=gain)
    engine = engine_module.Engine(config, state, 0, precision=precision)
    try:
        plan = batch.Plan(segments, [0], [pcm.numel()])
        assert plan.ld_frames > 1 << 22
        runs = engine.sub_plans(plan)
        if architecture == 'transformer' and precision != 'f32':
            assert runs is not None and len(runs) > 1
        else:
            assert runs is None
        scores, logits = engine.forward(audio, plan)
        scores = segment_logits(plan, scores)
        logits = segment_logits(plan, logits)
        if runs is not None:
            # the features entry point (`Model.forward`) takes the same runs
            packed = engine.features(audio, plan, engine.upload(plan)).clone()
            via = segment_logits(
                plan, engine.forward(None, plan, features=packed)[0])
            del packed
            for index in chosen:
                assert np.array_equal(via[index], scores[index]), index
        worst, worst_score = 0., 0.
        for index, alone, reference_logits in zip(chosen, plans, want):
            single = segment_logits(alone, engine.forward(audio, alone)[0])[0]
            assert np.array_equal(single, scores[index]), index
            worst = max(worst, float(
                np.abs(logits[index] - reference_logits).max()))
            worst_score = max(worst_score, float(np.abs(
                scores[index] - torch.sigmoid(
                    torch.from_numpy(reference_logits)).numpy()).max()))
        print(f'{architecture} {precision} past 2^22 columns: |dlogit| / '
              f'scale {worst / scale:.2e} (float32 floor {floor:.2e})')
        within_budget(worst / scale, worst_score, precision,
                      f'boundary_{architecture}')
    finally:
        del engine, audio
        gc.collect()
        torch.cuda.empty_cache()


@pytest.mark.parametrize('location', ['intermediate', 'input'])
def test_sub_plans_stay_below_the_limit(location):
    """`Engine.sub_plans` (host arithmetic): consecutive runs that cover every
    segment once, each packing fewer frame (and word-piece) columns than the
    limit; None when the plan fits."""
    the_batch = Batch(True, torch.device('cpu'))
    stub = engine_module.Engine.__new__(engine_module.Engine)
    stub.config = cfg.Config(downsample_location=location)
    stub.max_columns = engine_module.SPLIT16_COLUMNS
    assert stub.sub_plans(the_batch.plan) is None
    stub.max_columns = 6000 if location != 'input' else 12000
    runs = stub.sub_plans(the_batch.plan)
    assert len(runs) > 1
    assert runs[0][0] == 0 and runs[-1][1] == len(the_batch.segments)
    assert all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    for first, end in runs:
        part = the_batch.plan_of(the_batch.segments[first:end])
        assert part.ld_frames < stub.max_columns or end - first == 1
        if location == 'input':
            assert part.pieces('sum').plan.ld_frames < stub.max_columns
    stub.max_columns = 4096        # the 5000-frame segment alone is too long
    with pytest.raises(ValueError, match='one segment'):
        stub.sub_plans(the_batch.plan)
