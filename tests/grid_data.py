"""A float64 restatement of the convolution model's training loss over the
whole of `GridTrainer`'s grid, the `ABUT` layout, and the cases of the
whole-step tests on hard layouts (tests/test_grid_data.py anchors the
restatement to the reference's recorded gradients and checks everything else
here without a device; tests/test_gpu_grid_hard.py holds the HIP step to it).

`word_rate_data.restatement` is ReLU, `sum` / `average` and no dropout; this
one takes its shapes from the state and covers every activation, reduction,
channel count, kernel size and layer count of `STEP_RULES['GridTrainer']`,
with the dropout masks of `emphases_amd/train/dropout.py`.

`ABUT` is six utterances whose segments touch on both axes (the packed plan
aligns every segment to 16 columns, so a count that is a multiple of 16 leaves
no padding column before the next segment):

  utterance  frames  words
  0          64      33    abuts utterance 1; one word past the 32-wide tile
  1          128     64    abuts 2 on the frame AND on the word axis
  2          16      1     abuts 3; one word over all 16 frames
  3          1       1     one frame
  4          48      16    abuts 5 on both axes
  5          192     65    one word past the 64-wide gradient tile

Every worded utterance is tiled by its words (`word_rate_data._tiled`).  A
convolution of kernel size 5 or 7 reads two or three columns past a segment's
end: here those columns hold the neighbour's values, not padding, and only the
segment table makes them zero.

The cases cross several fields of the grid that no golden covers at once:

  A  gelu        48 channels  k 5 / 5  max      mse          layers 2
  B  silu        112          k 7 / 7  center   dropout 0.5  layers 2
  C  leaky_relu  16           k 1 / 7  average  dropout 0.1  layers 2
  D  relu        96           k 3 / 5  max      dropout 0.1  layers 3
  E  gelu        32           k 5 / 3  center                layers 0
  F  relu        128          k 7 / 1  sum      mse          layers 1

all six on `HARD` (tests/word_rate_data.py), B, D and F on `ABUT`, the masks at
STEP = 3.

A ReLU that flips or an argmax that moves between float32 and float64 moves a
gradient by about 1e-3, so the inputs keep the float64 restatement clear of
both.  `SEEDS[case, layout]` is the first of 0, 1, 2, .. whose restatement has

  kink margin >= MARGIN   over the ReLU / LeakyReLU layers, the smallest
                          |pre-activation| over the layer's largest (infinite
                          for GELU and SiLU);
  max gap >= MARGIN       under `max`, over the words of more than one frame,
                          the smallest gap between a word's largest and
                          second-largest value over the largest |value|.  A
                          tie at exactly zero is skipped: behind ReLU or a
                          mask it carries no gradient, whichever frame wins.

MARGIN is `word_rate_data.MARGIN`, 1e-6, by the reasoning stated there: ten
times what a float32 dot product of a few hundred terms is off by.  Measured
with this file (`margins(case, layout, seed)`, kink / gap):

  A HARD  seed 0  inf / 1.22e-4
  B HARD  seed 0  inf / inf
  C HARD  seed 0  3.15e-6 / inf
  D HARD  seed 0  1.33e-6 / 1.55e-5
  E HARD  seed 0  inf / inf
  F HARD  seed 3  1.48e-6 / inf    (seeds 0..2: 9.17e-8, 6.06e-7, 4.33e-7)
  B ABUT  seed 0  inf / inf
  D ABUT  seed 1  1.13e-6 / 3.84e-5    (seed 0: 6.31e-7)
  F ABUT  seed 0  4.34e-6 / inf
"""
import collections
import functools

import numpy as np
import torch

import emphases_amd
from emphases_amd import core as api
from emphases_amd import train
from emphases_amd.train import dropout as spec

import word_rate_data
from word_rate_data import HARD, REVERSED, Utterance, collate  # noqa: F401

MARGIN = word_rate_data.MARGIN
STEP = 3

ABUT_FRAMES = [64, 128, 16, 1, 48, 192]
ABUT_WORDS = [33, 64, 1, 1, 16, 65]


def _abut():
    rng = np.random.default_rng(20261020)
    return tuple(
        Utterance(key, frames, word_rate_data._tiled(rng, frames, words))
        for key, (frames, words) in enumerate(zip(ABUT_FRAMES, ABUT_WORDS)))


ABUT = _abut()
ABUT_REVERSED = ABUT[::-1]
LAYOUTS = {'hard': HARD, 'reversed': REVERSED, 'abut': ABUT,
           'abut_reversed': ABUT_REVERSED}

CASES = {
    'A': dict(activation='gelu', channels=48, encoder_kernel_size=5,
              decoder_kernel_size=5, downsample_method='max', loss='mse',
              layers=2),
    'B': dict(activation='silu', channels=112, encoder_kernel_size=7,
              decoder_kernel_size=7, downsample_method='center', dropout=0.5,
              layers=2),
    'C': dict(activation='leaky_relu', channels=16, encoder_kernel_size=1,
              decoder_kernel_size=7, downsample_method='average', dropout=0.1,
              layers=2),
    'D': dict(activation='relu', channels=96, encoder_kernel_size=3,
              decoder_kernel_size=5, downsample_method='max', dropout=0.1,
              layers=3),
    'E': dict(activation='gelu', channels=32, encoder_kernel_size=5,
              decoder_kernel_size=3, downsample_method='center', layers=0),
    'F': dict(activation='relu', channels=128, encoder_kernel_size=7,
              decoder_kernel_size=1, downsample_method='sum', loss='mse',
              layers=1),
}
# (case, layout) -> seed: the first that meets both margins (see above)
SEEDS = {
    ('A', 'hard'): 0, ('B', 'hard'): 0, ('C', 'hard'): 0, ('D', 'hard'): 0,
    ('E', 'hard'): 0, ('F', 'hard'): 3,
    ('B', 'abut'): 0, ('D', 'abut'): 1, ('F', 'abut'): 0,
}
PAIRS = tuple(SEEDS)

ACTIVATIONS = {
    'relu': torch.relu, 'gelu': torch.nn.functional.gelu,
    'silu': torch.nn.functional.silu,
    'leaky_relu': torch.nn.functional.leaky_relu}
KINKED = ('relu', 'leaky_relu')
# the deliberate defects of `restatement(defect=...)`
HALO, CENTER = 'halo', 'center'

Restated = collections.namedtuple('Restated', 'loss gradients kink gap')


def stack_names(config, prefix):
    """The conv layers of a stack in forward order, internal names."""
    return [f'{prefix}.{2 * i}' for i in range(config.layers)]


def config_of(case):
    return emphases_amd.Config(**CASES[case])


def plan_of_batch(batch):
    """The packed plan `GridTrainer.prepare` gives a collated batch."""
    frames, words, bounds = train.check_batch(*batch)
    return api._packed_plan(frames, torch.from_numpy(bounds), words)


def layer_masks(config, plan, name, seed, step):
    """[utterance] -> bool tensor [channels, n_u]: the kept elements of layer
    `name`, its mask over the packed buffer [channels, ld] cut at each
    utterance's columns."""
    frame_rate = name.startswith('frame_encoder')
    ld = plan.ld_frames if frame_rate else plan.ld_words
    offsets = plan.frame_off if frame_rate else plan.word_off
    counts = plan.frames if frame_rate else plan.words
    whole = spec.keep_mask(
        seed, spec.stream_of(config, name), step, config.channels * ld,
        config.dropout).reshape(config.channels, ld)
    return [torch.from_numpy(np.ascontiguousarray(
        whole[:, int(off):int(off) + int(count)]))
        for off, count in zip(offsets, counts)]


def restatement(config, state, batch, seed=0, step=0, dtype=torch.float64,
                defect=None):
    """The training loss of the convolution model at `config`, one utterance
    at a time with plain `conv1d(padding='same')` and autograd:

        input_layer (no activation); conv, activation and dropout per
        frame_encoder layer; per word `sum`, `mean`, `torch.max` or the frame
        `n // 2` of its n frames; conv, activation and dropout per
        word_decoder layer; output_layer; the mean over ALL words of the batch
        of BCE-with-logits or squared error.

    state: {internal name: array} (`train.initial_state`), whose shapes are
    the model's; batch: the five collated items; seed, step: of the dropout
    masks (`layer_masks`), which scale by 1 / (1 - p) of the Python float in
    float64 and by `dropout.scale(p)` in float32.  An utterance without words
    goes through the encoder and contributes nothing.

    defect: None, or a deliberate mistake for the tests of the bound - HALO:
    utterances 0, 1 and 2 go through the encoder as ONE sequence (their
    segments must abut in the packed plan, so that the masks are the plan's);
    CENTER: `center` takes frame (n - 1) // 2.

    Returns `Restated`: the loss as float, {name: gradient in float64}, the
    kink margin and the max gap (see the module docstring)."""
    conv = torch.nn.functional.conv1d
    activation = ACTIVATIONS[config.activation]
    method, layers = config.downsample_method, config.layers
    p = float(config.dropout or 0.)
    parameters = {
        name: torch.as_tensor(np.asarray(value)).to(dtype).requires_grad_()
        for name, value in state.items()}
    features, frame_lengths, word_bounds, word_lengths, targets = batch
    frame_lengths = [int(n) for n in frame_lengths]
    word_lengths = [int(n) for n in word_lengths]
    plan = plan_of_batch(batch)
    names = stack_names(config, 'frame_encoder') + \
        stack_names(config, 'word_decoder')
    masks = {name: layer_masks(config, plan, name, seed, step)
             for name in names} if p else {}
    scale = torch.tensor(1. / (1. - p), dtype=torch.float64) \
        if dtype == torch.float64 else torch.tensor(spec.scale(p))
    extremes = collections.defaultdict(lambda: [np.inf, 0.])
    gaps = [np.inf, 0.]

    def layer(name, x, mask):
        x = conv(x, parameters[f'{name}.weight'], parameters[f'{name}.bias'],
                 padding='same')
        if config.activation in KINKED:
            with torch.no_grad():
                size = x.abs()
                extremes[name][0] = min(extremes[name][0], float(size.min()))
                extremes[name][1] = max(extremes[name][1], float(size.max()))
        x = activation(x)
        if p:
            x = x * mask.to(dtype)[None] * scale
        return x

    def encoded(group):
        """The encoder's output of the utterances `group` as one sequence."""
        x = torch.cat([features[i, :, :frame_lengths[i]] for i in group],
                      dim=1)[None].to(dtype)
        x = conv(x, parameters['input_layer.weight'],
                 parameters['input_layer.bias'], padding='same')
        for name in stack_names(config, 'frame_encoder'):
            mask = torch.cat([masks[name][i] for i in group], dim=1) \
                if p else None
            x = layer(name, x, mask)
        return torch.split(x, [frame_lengths[i] for i in group], dim=2)

    def pooled(piece):
        n = piece.shape[2]
        if method == 'sum':
            return piece.sum(dim=2)
        if method == 'average':
            return piece.mean(dim=2)
        if method == 'center':
            return piece[:, :, (n - 1) // 2 if defect == CENTER else n // 2]
        assert method == 'max'
        if n > 1:
            with torch.no_grad():
                top = torch.topk(piece, 2, dim=2).values
                gap = top[..., 0] - top[..., 1]
                tied_at_zero = (top[..., 0] == 0) & (top[..., 1] == 0)
                if not tied_at_zero.all():
                    gaps[0] = min(gaps[0], float(gap[~tied_at_zero].min()))
        return torch.max(piece, dim=2).values

    items = list(range(len(frame_lengths)))
    groups = [[i] for i in items]
    if defect == HALO:
        for first, second in ((0, 1), (1, 2)):
            assert plan.frame_off[first] + plan.frames[first] == \
                plan.frame_off[second]
        groups = [[0, 1, 2]] + [[i] for i in items[3:]]
    encoder_output = {}
    for group in groups:
        for i, x in zip(group, encoded(group)):
            encoder_output[i] = x
    logits, wanted = [], []
    for i in items:
        x, words = encoder_output[i], word_lengths[i]
        gaps[1] = max(gaps[1], float(x.detach().abs().max()))
        if not words:
            continue
        x = torch.stack([
            pooled(x[:, :, int(start):int(end)])
            for start, end in word_bounds[i, :, :words].T], dim=2)
        for name in stack_names(config, 'word_decoder'):
            x = layer(name, x, masks[name][i] if p else None)
        x = conv(x, parameters['output_layer.weight'],
                 parameters['output_layer.bias'], padding='same')
        logits.append(x[0, 0])
        wanted.append(targets[i, 0, :words].to(dtype))
    function = torch.nn.functional.binary_cross_entropy_with_logits \
        if config.loss == 'bce' else torch.nn.functional.mse_loss
    value = function(torch.cat(logits), torch.cat(wanted))
    value.backward()
    gradients = {name: parameter.grad.double()
                 for name, parameter in parameters.items()}
    kink = min([low / high for low, high in extremes.values()] or [np.inf])
    gap = gaps[0] / gaps[1] if np.isfinite(gaps[0]) else np.inf
    assert len(names) == 2 * layers
    return Restated(float(value.detach()), gradients, kink, gap)


@functools.lru_cache(maxsize=None)
def batch_of(layout, seed):
    """`collate(LAYOUTS[layout], seed)`, made once and left unchanged."""
    return collate(LAYOUTS[layout], seed)


@functools.lru_cache(maxsize=None)
def exact(case, layout, seed, step=STEP, defect=None):
    """The float64 restatement of a case on a layout from
    `train.initial_state(config, seed)`, made once and left unchanged."""
    config = config_of(case)
    return restatement(
        config, train.initial_state(config, seed), batch_of(layout, seed),
        seed, step, torch.float64, defect)


def margins(case, layout, seed):
    """(kink margin, max gap) of a case on a layout under `seed`."""
    found = exact(case, layout, seed)
    return found.kink, found.gap


def worst_error(got, want):
    """The worst over the tensors of max |got - want| / max |want|."""
    return max(
        float((got[name].double() - value).abs().max() / value.abs().max())
        for name, value in want.items())


@functools.lru_cache(maxsize=None)
def reference(case, layout):
    """(config, seed, state, `Restated` in float64, ref32) of a (case, layout)
    under its recorded seed: `ref32` is the worst over the tensors of the
    float32 restatement's error against the float64 one, over max |want|."""
    config, seed = config_of(case), SEEDS[case, layout]
    state = train.initial_state(config, seed)
    want = exact(case, layout, seed)
    narrow = restatement(
        config, state, batch_of(layout, seed), seed, STEP, torch.float32)
    return config, seed, state, want, worst_error(narrow.gradients,
                                                  want.gradients)
