"""The training step of the convolution model.

What the reference does per batch (`emphases/train/core.py:105-142`: forward
in train mode, `loss`, `backward`, `optimizer.step`) as launches of the HIP
library on one stream.  Deliberate, documented deviations:

* no `torch.autocast`, no `GradScaler` (`train/core.py:78,111,136-142`):
  float32 throughout by default, as inference (`core.inference_context`).
  `precision='bf16x3'` is the mixed precision of this package instead: the
  Conv1d(80, 80, 3) layers on the frame axis - forward, data gradient and
  weight gradient - multiply on the bf16 matrix pipe with every float32
  operand split into two bf16 pieces (three products per term, float32
  accumulation: `emph_conv1d_split`, `emph_conv_weight_grad_split`), while
  the word-rate layers, the output layer, the loss and Adam stay float32, as
  do the parameters, the gradients and the moments;
* `Config.dropout` (`torch.nn.Dropout` after every activation of the two conv
  stacks, `model/layers/convolution.py:29-30`) draws its masks from Philox
  counters keyed by the trainer's seed, the layer and the step count
  (`train/dropout.py`), not from torch's generator: a step can be repeated
  and a resumed run continues the same masks;
* every utterance is trained alone, with its own zero halo, exactly as
  inference runs it; the reference's padded batch leaks bias + ReLU of the
  padding into the last frames and words of every shorter utterance
  (`model/layers/convolution.py:35-37` ignores lengths).  The loss is the mean
  over all valid words of the batch, as the reference's masked loss is.

`EncoderTrainer` is the same step for the models without a word decoder
(`DOWNSAMPLE_LOCATION` 'inference' and 'loss', `model/core.py:28-30,109-138`):
the frame encoder goes straight to `output_layer`, at word rate behind the
reduce for 'loss', at frame rate against targets that `emphases.upsample`
spreads over the frames for 'inference' (`train/core.py:324-353`).  It keeps
`Trainer`'s semantics: every utterance is trained alone, with its own zero
halo; the 'inference' loss is the mean over all frames of the batch, the
'loss' loss the mean over all words; the output layer, the loss and Adam
stay float32 at either precision.

`PieceTrainer` is the same step for `DOWNSAMPLE_LOCATION` 'input'
(`model/core.py:41-87`, `core.py:552-586`): every word is cut out of the
features and zero-padded to the longest word, every piece is encoded as a
sequence of its own and pooled over the PADDED axis into its word's column;
the word decoder, the output layer and the loss are `Trainer`'s.  Its
deviation is the one above in this model's terms: every utterance is alone,
so a word is padded to the longest word of ITS OWN utterance (what
`batch.Pieces` lays out and what the reference's inference sees, one
utterance per call), not to the longest word of the batch as the reference's
padded training batch does.  `Config.dropout` is refused there.

`GridTrainer` is the same step for the rest of the reference's hyperparameter
grid at 'intermediate' (`config/hparam-search/*.py`,
`config/downsample/{max,center}-intermediate.py`): any of the four
activations and reductions, channels a multiple of 16 up to 128, kernel sizes
1, 3, 5, 7, with or without dropout, in float32.  It runs the general kernels
(`emph_conv1d` at the layer's own shape, `emph_conv_weight_grad_any`,
`emph_segment_reduce_backward`, `emph_output_layer_backward_any`), keeps the
pre-activation where the activation's derivative reads it (GELU, SiLU) and
regenerates the dropout masks in the backward.  `select_trainer` picks a
specialised step where one covers the configuration - which then keeps its
bits - and `GridTrainer` where none does.

How the module is laid out.  What a step supports is data: `STEP_RULES`, one
table of rules per class, walked by `refusal`; `step_class` is the one place
that maps a downsample_location to a class (`STEP_OF_LOCATION`), and
`select_trainer`, `trainer_for` and `make_trainer` are that dispatch with
fewer candidates.  `_Step` holds the state, the batch layout, the workspace
cache and every launch that more than one step issues; `_DecoderStep` is the
one forward / backward skeleton of the three steps with a word decoder.  The
classes differ by the methods they override - the reduce and its backward,
the activation's backward, the buffers of their own - and by two entry-point
names, never by a branch on the class: `Trainer` keeps its specialised
kernels, `GridTrainer` the general ones, and neither stands in for the other.

All parameters live in ONE flat device buffer in `weights.parameter_shapes`
order (the order of `Model.parameters()`); gradients and the two Adam moments
are buffers of the same shape.  The MFMA weight packs of the forward kernel
(`emph_conv1d`) and of the data gradient (the same kernel on
W'[ci][co][j] = W[co][ci][2 - j]) are rebuilt after every update by ONE
gather launch (`emph_take`) through a table made once on the host; under
'bf16x3' one more launch (`emph_conv_split_pack_device`) splits the weights
of the layers in scope into the packs of `emph_conv1d_split`, both ways.
"""
import collections
import math
import os

import numpy as np
import torch

from .. import config as cfg
from .. import core as api
from .. import runtime
from .. import weights as weights_module
from . import dropout as dropout_module

FRAME_TILE = 64      # emph_conv1d, emph_conv_weight_grad, emph_segment_broadcast
WORD_TILE = 32       # emph_conv1d on the word axis
GRAD_TILE = 64       # emph_conv_weight_grad on either axis
PRECISIONS = ('f32', 'bf16x3')
SPLIT_CHANNELS = 80  # emph_conv1d_split, emph_conv_weight_grad_split
GRID_CHANNELS = tuple(range(16, 129, 16))   # `TorchModel`'s rule
GRID_KERNEL_SIZES = (1, 3, 5, 7)


def _rules(**changes):
    """The rules of a step, in the order they are tested: {field: (the
    accepted values or a predicate, the text that names them)}.  `Trainer`'s,
    with the fields of `changes` replaced (None: not tested) or appended."""
    rules = {
        'method': (('neural',), "'neural'"),
        'architecture': (('convolution',), "'convolution'"),
        'downsample_location': (('intermediate',), "'intermediate'"),
        'downsample_method': (('sum', 'average'), "'sum' or 'average'"),
        'activation': (('relu',), "'relu'"),
        'loss': (('bce', 'mse'), "'bce' or 'mse'"),
        'channels': ((80,), '80'),
        'encoder_kernel_size': ((3,), '3'),
        'decoder_kernel_size': ((3,), '3'),
        'layers': (lambda layers: 0 <= layers <= 16, '0..16'),
        'mel_feature': (bool, 'True (80..83 input features)')}
    rules.update(changes)
    return {field: rule for field, rule in rules.items() if rule is not None}


_ALL_METHODS = (('sum', 'average', 'max', 'center'),
                "'sum', 'average', 'max' or 'center'")
# class -> (the step's name in a refusal, its rules)
STEP_RULES = {
    'Trainer': ('training step', _rules()),
    'EncoderTrainer': ('encoder training step', _rules(
        downsample_location=(('inference', 'loss'), "'inference' or 'loss'"),
        downsample_method=None,
        decoder_kernel_size=((3,), "3 (the output layer's kernel size)"))),
    'PieceTrainer': ('piece training step', _rules(
        downsample_location=(('input',), "'input'"),
        downsample_method=_ALL_METHODS,
        dropout=(lambda p: p is None,
                 'None (no mask is specified for the piece layout)'))),
    'GridTrainer': ('grid training step', _rules(
        downsample_method=_ALL_METHODS,
        activation=(('relu', 'gelu', 'silu', 'leaky_relu'),
                    "'relu', 'gelu', 'silu' or 'leaky_relu'"),
        channels=(GRID_CHANNELS, 'a multiple of 16 in 16..128'),
        encoder_kernel_size=(GRID_KERNEL_SIZES, '1, 3, 5 or 7'),
        decoder_kernel_size=(GRID_KERNEL_SIZES, '1, 3, 5 or 7'),
        dropout=(lambda p: p is None or 0. <= p < 1.,
                 'None or a probability 0 <= p < 1')))}
# downsample_location -> the class of its specialised step
STEP_OF_LOCATION = {
    'intermediate': 'Trainer', 'inference': 'EncoderTrainer',
    'loss': 'EncoderTrainer', 'input': 'PieceTrainer'}


def refusal(step, config):
    """What refuses `config` for the step of class `step`, naming the first
    field outside its rules; None where the step covers it."""
    name, rules = STEP_RULES[step]
    for field, (accepted, supported) in rules.items():
        value = getattr(config, field)
        if not (accepted(value) if callable(accepted) else value in accepted):
            return (f'the {name} supports {field} {supported} only, not '
                    f'{field}={value!r}')
    return None


def _check(step, config):
    message = refusal(step, config)
    if message is not None:
        raise NotImplementedError(message)


def check_supported(config):
    """NotImplementedError, naming the field, for a configuration `Trainer`
    does not cover - before anything is allocated or launched."""
    _check('Trainer', config)


def check_encoder_supported(config):
    """`check_supported` for `EncoderTrainer`: the models without a word
    decoder, downsample_location 'inference' or 'loss'."""
    _check('EncoderTrainer', config)


def check_pieces_supported(config):
    """`check_supported` for `PieceTrainer`: downsample_location 'input', all
    four reductions, no dropout."""
    _check('PieceTrainer', config)


def check_grid_supported(config):
    """`check_supported` for `GridTrainer`: the reference's hyperparameter
    grid at downsample_location 'intermediate' - any activation, reduction,
    channel count (a multiple of 16 up to 128) and odd kernel size up to 7."""
    _check('GridTrainer', config)


def check_precision(precision):
    """'f32' or 'bf16x3'; NotImplementedError for the inference precisions the
    step does not cover, ValueError for anything else - before a GPU is
    needed."""
    from .. import engine
    if not isinstance(precision, str):
        raise ValueError(
            f'precision must be one of {sorted(engine.PRECISIONS)}, not '
            f'{precision!r}')
    if precision in PRECISIONS:
        return precision
    if precision in engine.PRECISIONS:
        raise NotImplementedError(
            f'the training step supports precision {PRECISIONS} only, not '
            f'precision={precision!r}')
    raise ValueError(
        f'precision {precision!r} is not one of {sorted(engine.PRECISIONS)}')


def check_grid_precision(precision):
    """`check_precision` for `GridTrainer`: 'f32' only.  The split kernels of
    'bf16x3' are Conv1d(80, 80, 3) with a ReLU flag and nothing else."""
    if check_precision(precision) != 'f32':
        raise NotImplementedError(
            "the grid training step supports precision 'f32' only, not "
            f'precision={precision!r}: the bf16 split kernels are '
            'Conv1d(80, 80, 3) with ReLU')
    return precision


def step_class(config, precision=None, grid=True, locations=None):
    """The class of the step that trains `config`, every check made and
    nothing constructed: the specialised step of the configuration's location
    first, `GridTrainer` where that refuses and `check_grid_supported` passes,
    otherwise the specialised step's refusal.  `precision`: checked as well
    unless None.  `grid=False`: never `GridTrainer`.  `locations`: the ones
    the caller dispatches over; any other gets `Trainer`'s refusal of its
    downsample_location.  The class is looked up in this module at the call."""
    location = config.downsample_location
    if locations is not None and location not in locations:
        location = 'intermediate'
    step, check = STEP_OF_LOCATION[location], check_precision
    message = refusal(step, config)
    if message is not None:
        if not grid or refusal('GridTrainer', config) is not None:
            raise NotImplementedError(message)
        step, check = 'GridTrainer', check_grid_precision
    if precision is not None:
        check(precision)
    return globals()[step]


def split_layer_names(config):
    """The layers of `layer_names` that run on the bf16 pipe under
    precision='bf16x3': the Conv1d(80, 80, 3) on the frame axis (the input
    layer only when it has exactly 80 feature rows)."""
    names = ['input_layer'] if config.num_features == SPLIT_CHANNELS else []
    return names + stack_names(config, 'frame_encoder')


def stack_names(config, prefix):
    """The conv layers of the stack `prefix` ('frame_encoder' or
    'word_decoder'), in forward order: modules 0, 2, .. of its Sequential."""
    return [f'{prefix}.{2 * i}' for i in range(config.layers)]


def layer_names(config):
    """The conv layers in forward order (no word decoder at
    downsample_location 'inference' and 'loss', `model/core.py:28-30`)."""
    names = ['input_layer'] + stack_names(config, 'frame_encoder')
    if config.has_decoder:
        names += stack_names(config, 'word_decoder')
    return names


def checkpoint_names(config):
    """Internal parameter name -> its name in a saved file: the reference's
    `Convolution` is `Sequential(conv, activation[, Dropout])` per layer
    (`convolution.py:25-33`, `DROPOUT is not None`, 0. included), so under
    `Config.dropout` layer i of a stack is module 3 i, not 2 i.  `weights.load`
    reads either numbering."""
    stride = 2 if config.dropout is None else 3
    names = collections.OrderedDict()
    for name in weights_module.parameter_shapes(config):
        prefix, _, rest = name.partition('.')
        names[name] = name
        if prefix in ('frame_encoder', 'word_decoder'):
            index, kind = rest.split('.')
            names[name] = f'{prefix}.{int(index) // 2 * stride}.{kind}'
    return names


def parameter_offsets(config):
    """name -> (first element, shape) in the flat parameter buffer."""
    offsets = collections.OrderedDict()
    cursor = 0
    for name, shape in weights_module.parameter_shapes(config).items():
        offsets[name] = (cursor, tuple(shape))
        cursor += int(np.prod(shape))
    return offsets, cursor


def initial_state(config=cfg.DEFAULT, seed=0):
    """Bitwise the parameters of the reference's `emphases.Model()` after
    `torch.manual_seed(seed)`: `torch.nn.Conv1d` modules built on the CPU in
    the reference's construction order (`model/core.py:16-37`,
    `model/layers/convolution.py:22-33`).  The caller's generator is left
    as it was."""
    step_class(config)
    state = collections.OrderedDict()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)

        def conv(name, c_in, c_out, kernel_size):
            module = torch.nn.Conv1d(
                c_in, c_out, kernel_size=kernel_size, padding='same')
            state[f'{name}.weight'] = module.weight.detach().numpy().copy()
            state[f'{name}.bias'] = module.bias.detach().numpy().copy()
        conv('input_layer', config.num_features, config.channels,
             config.encoder_kernel_size)
        for prefix, kernel_size in (
                ('frame_encoder', config.encoder_kernel_size),
                ('word_decoder', config.decoder_kernel_size)):
            if prefix == 'word_decoder' and not config.has_decoder:
                continue
            for i in range(config.layers):
                conv(f'{prefix}.{2 * i}', config.channels, config.channels,
                     kernel_size)
        conv('output_layer', config.channels, 1, config.decoder_kernel_size)
    assert list(state) == list(weights_module.parameter_shapes(config))
    return state


def _tile_count(tiles):
    """The rows of a device tile table (`Plan.tiles`)."""
    return tiles.numel() // runtime.TILE_FIELDS


def gather_tables(config=cfg.DEFAULT):
    """The `emph_take` table of every pack of a step: int32 `index` into the
    flat parameter buffer (-1: zero), and {layer: (first, size)} of the forward
    packs (every layer) and of the data-gradient packs
    W'[ci][co][j] = W[co][ci][k - 1 - j] (every layer but the input layer,
    whose input needs no gradient)."""
    step_class(config)
    offsets, _ = parameter_offsets(config)
    pieces, forward, backward = [], {}, {}
    cursor = 0
    for direction, table in (('forward', forward), ('backward', backward)):
        for name in layer_names(config):
            if direction == 'backward' and name == 'input_layer':
                continue
            first, shape = offsets[f'{name}.weight']
            indices = first + np.arange(
                int(np.prod(shape)), dtype=np.int64).reshape(shape)
            if direction == 'backward':
                indices = np.ascontiguousarray(
                    indices.transpose(1, 0, 2)[:, :, ::-1])
            piece = runtime.conv_pack_indices(indices)
            table[name] = (cursor, piece.size)
            pieces.append(piece)
            cursor += piece.size
    index = np.concatenate(pieces).astype(np.int32)
    return {'index': index, 'forward': forward, 'backward': backward}


def split_pack_tables(config=cfg.DEFAULT):
    """The `emph_conv_split_pack_device` table of a step at 'bf16x3': int32
    `index` [packs][23 040] into the flat parameter buffer, and {layer: pack
    number} of the forward packs (`split_layer_names`) and of the
    data-gradient packs W'[ci][co][j] = W[co][ci][2 - j] (the same layers but
    the input layer).  Element ((tap * 5 + block) * 3 + m) * 512 + lane * 8 +
    e of a pack is weight [32 m + lane % 32][16 block + 8 (lane / 32) + e]
    [tap] of its layer, -1 (zeros) for rows 80 .. 95: the layout of
    `emph_conv_split_pack`."""
    step_class(config)
    offsets, _ = parameter_offsets(config)
    tap, block, m, lane, e = np.meshgrid(
        np.arange(3), np.arange(5), np.arange(3), np.arange(64), np.arange(8),
        indexing='ij')
    row = 32 * m + lane % 32
    channel = 16 * block + 8 * (lane // 32) + e
    inside = row < SPLIT_CHANNELS
    row = np.minimum(row, SPLIT_CHANNELS - 1)
    pieces, forward, backward = [], {}, {}
    for direction, table in (('forward', forward), ('backward', backward)):
        for name in split_layer_names(config):
            if direction == 'backward' and name == 'input_layer':
                continue
            first, shape = offsets[f'{name}.weight']
            assert tuple(shape) == (SPLIT_CHANNELS, SPLIT_CHANNELS, 3)
            if direction == 'forward':
                source = (row * SPLIT_CHANNELS + channel) * 3 + tap
            else:
                source = (channel * SPLIT_CHANNELS + row) * 3 + 2 - tap
            table[name] = len(pieces)
            pieces.append(np.where(inside, first + source, -1).ravel())
    index = np.stack(pieces).astype(np.int32) if pieces else \
        np.zeros((0, tap.size), dtype=np.int32)
    return {'index': index, 'forward': forward, 'backward': backward}


def check_batch(features, frame_lengths, word_bounds, word_lengths, targets,
                config=cfg.DEFAULT):
    """ValueError for a malformed batch (the first five items of the
    reference's `emphases.data.collate`), before any launch.  Returns the
    lengths as lists of int and the bounds as int64 numpy [B, 2, Wmax]."""
    if features.dim() != 3 or features.shape[1] != config.num_features:
        raise ValueError(
            f'features must be [B, {config.num_features}, T], not '
            f'{tuple(features.shape)}')
    items = features.shape[0]
    frames = [int(n) for n in frame_lengths]
    words = [int(n) for n in word_lengths]
    if len(frames) != items or len(words) != items or \
            word_bounds.shape[0] != items or targets.shape[0] != items:
        raise ValueError('the batch items disagree on the batch size')
    if word_bounds.dim() != 3 or word_bounds.shape[1] != 2:
        raise ValueError('word_bounds must be [B, 2, W]')
    if targets.dim() != 3 or targets.shape[1] != 1:
        raise ValueError('targets must be [B, 1, W]')
    bounds = np.asarray(word_bounds.cpu(), dtype=np.int64)
    for index, (count, length) in enumerate(zip(frames, words)):
        if not 1 <= count <= features.shape[2]:
            raise ValueError(
                f'item {index}: frame length {count} outside the features '
                f'(1..{features.shape[2]})')
        if not 0 <= length <= bounds.shape[2]:
            raise ValueError(
                f'item {index}: word length {length} outside word_bounds')
        if length > targets.shape[2]:
            raise ValueError(
                f'item {index}: targets hold {targets.shape[2]} words, '
                f'word_lengths asks for {length}')
        starts, ends = bounds[index, 0, :length], bounds[index, 1, :length]
        if np.any(ends <= starts):
            raise ValueError(f'item {index}: a word with end <= start')
        if np.any(starts < 0) or np.any(ends > count):
            raise ValueError(
                f'item {index}: word bounds past its {count} frames')
        if np.any(starts[1:] < ends[:-1]):
            raise ValueError(
                f'item {index}: words overlap or are not in order')
    if sum(words) == 0:
        raise ValueError('the batch has no word')
    return frames, words, bounds


def adam_state_dict(config, steps, exp_avg, exp_avg_sq, lr=1e-3,
                    betas=(0.9, 0.999), eps=1e-8):
    """`torch.optim.Adam.state_dict()` layout from the flat CPU moment
    buffers: parameter i of `Model.parameters()` order under key i (no state
    before the first step, as torch), the param group of this torch's Adam."""
    offsets, _ = parameter_offsets(config)
    shells = [torch.nn.Parameter(torch.zeros(shape))
              for _, shape in offsets.values()]
    template = torch.optim.Adam(
        shells, lr=lr, betas=tuple(betas), eps=eps).state_dict()
    state = {}
    if steps:
        for index, (first, shape) in enumerate(offsets.values()):
            size = int(np.prod(shape))
            state[index] = {
                'step': torch.tensor(float(steps)),
                'exp_avg': exp_avg[first:first + size].view(shape).clone(),
                'exp_avg_sq':
                    exp_avg_sq[first:first + size].view(shape).clone()}
    return {'state': state, 'param_groups': template['param_groups']}


def write_checkpoint(path, model, optimizer, epoch=0, step=0, score=0.,
                     best=0.):
    """The dict of `torchutil.checkpoint.save(file, model, optimizer,
    **kwargs)`: the keys of the reference's shipped checkpoint.pt."""
    torch.save({
        'epoch': epoch, 'step': step, 'score': score, 'best': best,
        'model': model, 'optimizer': optimizer}, os.fspath(path))


class Batch:
    """A collated batch on the device in packed ragged form (`Trainer.prepare`):
    the plan, its metadata, the features [C, ld_frames] and the targets
    [ld_words]."""

    def __init__(self, plan, meta, features, targets):
        self.plan = plan
        self.meta = meta
        self.features = features
        self.targets = targets


class _State:
    """The state of a trainer and what does not depend on how its step is
    computed: parameters, both Adam moments and the step count in flat device
    buffers in `weights.parameter_shapes` order, the checkpoint
    (`optimizer_state_dict`, `save`, and reading one back), and `prepare`, the
    packed layout of a collated batch.  A subclass gives `metadata(plan)` and
    `state_dict()`.  `_Step` (the fused steps) and `TransformerTrainer`
    (`train/transformer_step.py`) are built on it."""

    def _settings(self, lr, betas, eps, seed):
        self.lr, self.betas, self.eps = float(lr), tuple(betas), float(eps)
        self.steps = 0
        self.seed = int(seed)

    def _read(self, checkpoint, initial):
        """(the parameters as numpy arrays by name, the optimizer state or
        None) of `checkpoint`: None (`initial(config, seed)`), a state dict,
        or a file `weights.load` reads; a file written by `save` carries the
        optimizer state."""
        if checkpoint is None:
            return initial(self.config, self.seed), None
        optimizer = None
        if not isinstance(checkpoint, dict) and \
                not str(checkpoint).endswith('.npz'):
            checkpoint = torch.load(
                os.fspath(checkpoint), map_location='cpu',
                weights_only=False)
        if isinstance(checkpoint, dict) and 'model' in checkpoint:
            optimizer = checkpoint.get('optimizer')
            checkpoint = checkpoint['model']
        return weights_module.load(checkpoint, self.config), optimizer

    def _allocate(self, state, optimizer):
        """The flat device buffers of `state` (inside the device's context);
        `optimizer`: the moments and the step count restored from it."""
        flat = np.concatenate([state[name].ravel() for name in self.offsets])
        self.parameters = torch.from_numpy(flat).to(self.device)
        self.exp_avg = torch.zeros_like(self.parameters)
        self.exp_avg_sq = torch.zeros_like(self.parameters)
        if optimizer is not None and optimizer.get('state'):
            self._restore(optimizer)

    def _view(self, buffer, name):
        first, shape = self.offsets[name]
        return buffer[first:first + int(np.prod(shape))].view(shape)

    def _restore(self, optimizer):
        moments = optimizer['state']
        steps = set()
        for index, name in enumerate(self.offsets):
            entry = moments[index]
            self._view(self.exp_avg, name).copy_(entry['exp_avg'])
            self._view(self.exp_avg_sq, name).copy_(entry['exp_avg_sq'])
            steps.add(int(entry['step']))
        if len(steps) != 1:
            raise ValueError('the optimizer state holds several step counts')
        self.steps = steps.pop()
        group = optimizer['param_groups'][0]
        self.lr, self.eps = float(group['lr']), float(group['eps'])
        self.betas = tuple(float(b) for b in group['betas'])

    def optimizer_state_dict(self):
        """`torch.optim.Adam.state_dict()` of the reference's optimizer
        (`train/core.py:48`): parameters in `Model.parameters()` order."""
        return adam_state_dict(
            self.config, self.steps, self.exp_avg.cpu(), self.exp_avg_sq.cpu(),
            self.lr, self.betas, self.eps)

    def save(self, path, epoch=0, step=None, score=0., best=0.):
        """The file `torchutil.checkpoint.save` writes in the reference's loop
        (`train/core.py:162-169,189-196`): every inference entry point takes it
        as `checkpoint=`, the same class with `checkpoint=path` resumes from
        it."""
        write_checkpoint(
            path, self.state_dict(), self.optimizer_state_dict(), epoch,
            self.steps if step is None else step, score, best)

    ###########################################################################
    # Batches
    ###########################################################################

    def prepare(self, features, frame_lengths, word_bounds, word_lengths,
                targets):
        """Validate a collated batch (host or device tensors) and lay it out
        on the device: one copy of the integer metadata, one gather launch
        each for the features and the targets."""
        config = self.config
        frames, words, bounds = check_batch(
            features, frame_lengths, word_bounds, word_lengths, targets,
            config)
        plan = api._packed_plan(frames, torch.from_numpy(bounds), words)
        meta = self.metadata(plan)
        # emph_gather_columns pieces: (source column, length, target column,
        # columns to write; the rest zero) of every item, frames then words
        align = lambda n: (n + 15) // 16 * 16  # noqa: E731
        items, t_max, w_max = len(frames), features.shape[2], targets.shape[2]
        pieces = np.array(
            [(i * t_max, frames[i], plan.frame_off[i], align(frames[i]))
             for i in range(items)] +
            [(i * w_max, words[i], plan.word_off[i], align(words[i]))
             for i in range(items)], dtype=np.int64)
        with torch.cuda.device(self.device):
            table = torch.from_numpy(pieces).to(self.device)
            source = features.to(self.device, torch.float32).permute(
                1, 0, 2).reshape(config.num_features, items * t_max).contiguous()
            packed = torch.zeros(
                (config.num_features, plan.ld_frames), dtype=torch.float32,
                device=self.device)
            runtime.check(self.lib.emph_gather_columns(
                source.data_ptr(), source.shape[1], packed.data_ptr(),
                plan.ld_frames, config.num_features, table.data_ptr(), items,
                runtime.stream()), 'emph_gather_columns')
            source = targets.to(self.device, torch.float32).reshape(
                1, items * w_max).contiguous()
            packed_targets = torch.zeros(
                plan.ld_words, dtype=torch.float32, device=self.device)
            runtime.check(self.lib.emph_gather_columns(
                source.data_ptr(), source.shape[1], packed_targets.data_ptr(),
                plan.ld_words, 1, table[items:].data_ptr(), items,
                runtime.stream()), 'emph_gather_columns')
        return Batch(plan, meta, packed, packed_targets)


class _Step(_State):
    """What every fused step shares on top of `_State`: the batch's integer
    tables, Adam, the workspace (`_buffers`) and every launch that more than
    one step issues - a conv layer and a conv stack forward and backward, the
    frame encoder, the reduce, and the word tail (output layer, loss, output
    layer's backward).  A subclass names its `_check` and gives `_forward`
    (whose buffers' 'logits' then hold the packed word logits) and
    `_forward_backward` (which leaves the loss in `self.loss` and every
    gradient in `self.gradients`)."""

    _check = staticmethod(check_supported)

    def __init__(self, config=None, checkpoint=None, gpu=None, lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, seed=0, precision='f32'):
        """precision: 'f32' (default) or 'bf16x3' (see the module docstring);
        a choice of the configuration, never of the batch, and not part of
        the checkpoint: a run saved at one resumes at the other.
        seed: of the initialisation (without a checkpoint) and of the dropout
        masks (always; `Config.dropout`).
        checkpoint: None (the reference's initialisation under `seed`), a
        state dict, or a file `weights.load` reads; a file written by `save`
        also restores the Adam moments and the step count."""
        self.config = config = config or api.active_config()
        self._check(config)
        self.precision = check_precision(precision)
        self._settings(lr, betas, eps, seed)
        # (None and 0. launch nothing: torch.nn.Dropout(0.) is the identity)
        self.dropout = float(config.dropout or 0.)
        state, optimizer = self._read(checkpoint, initial_state)
        self.offsets, self.count = parameter_offsets(config)
        tables = gather_tables(config)
        self.device = runtime.require_gpu(gpu)
        self.lib = runtime.library()
        with torch.cuda.device(self.device):
            self._allocate(state, optimizer)
            self.gradients = torch.zeros_like(self.parameters)
            self.take_index = torch.from_numpy(tables['index']).to(self.device)
            self.packs = torch.zeros(
                tables['index'].size, dtype=torch.float32, device=self.device)
            self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
            self._forward_packs = tables['forward']
            self._backward_packs = tables['backward']
            self._workspace = {}
            self._split_forward, self._split_backward = {}, {}
            if self.precision == 'bf16x3':
                tables = split_pack_tables(config)
                self._split_forward = tables['forward']
                self._split_backward = tables['backward']
                self._split_bytes = int(
                    self.lib.emph_conv_split_pack_size())
                assert tables['index'].shape[1] * 4 == self._split_bytes
                self.split_index = torch.from_numpy(
                    tables['index']).to(self.device)
                self.split_packs = torch.zeros(
                    (tables['index'].shape[0], self._split_bytes),
                    dtype=torch.uint8, device=self.device)
                self._zero_bias = torch.zeros(
                    SPLIT_CHANNELS, dtype=torch.float32, device=self.device)
            self._repack()

    ###########################################################################
    # State
    ###########################################################################

    def state_dict(self):
        """The parameters under the reference's names (`checkpoint_names`)
        and shapes (CPU)."""
        flat = self.parameters.cpu()
        saved = checkpoint_names(self.config)
        return collections.OrderedDict(
            (saved[name], self._view(flat, name).clone())
            for name in self.offsets)

    def _upload(self, tables):
        """Host tables [(int32 array, {name: (first element, size)})], every
        one a whole number of 16 bytes, in ONE copy to the device: the device
        buffer and, per table, its views by name."""
        host = np.concatenate([table for table, _ in tables])
        with torch.cuda.device(self.device):
            buffer = torch.from_numpy(host).to(self.device)
        views, first = [], 0
        for table, offsets in tables:
            assert table.size % 4 == 0
            views.append({
                name: buffer[first + start:first + start + size]
                for name, (start, size) in offsets.items()})
            first += table.size
        return buffer, views

    def metadata(self, plan):
        """The integer tables of a step for a packed layout on the device: one
        copy, views by name (`Batch.meta`)."""
        requests = [(runtime.AXIS_FRAMES, FRAME_TILE),
                    (runtime.AXIS_WORDS, WORD_TILE),
                    (runtime.AXIS_WORDS, GRAD_TILE)]
        buffer, (meta,) = self._upload([plan.pack_metadata(
            list(dict.fromkeys(requests)), spans=self.precision == 'bf16x3')])
        meta['_buffer'] = buffer
        return meta

    def _frame_meta(self, batch):
        """The tables of the layout the frame-rate layers run on."""
        return batch.meta

    def _batch(self, arguments):
        if len(arguments) == 1 and isinstance(arguments[0], Batch):
            meta = self._frame_meta(arguments[0])
            if self._split_forward and 'conv_spans' not in meta:
                raise ValueError(
                    "the batch was prepared by a trainer at precision='f32' "
                    "and carries no span table: prepare it with this "
                    f"trainer (precision={self.precision!r})")
            return arguments[0]
        return self.prepare(*arguments)

    ###########################################################################
    # Launches
    ###########################################################################

    def _repack(self):
        runtime.check(self.lib.emph_take(
            self.parameters.data_ptr(), self.take_index.data_ptr(),
            self.packs.data_ptr(), self.packs.numel(), runtime.stream()),
            'emph_take')
        if self._split_forward:
            runtime.check(self.lib.emph_conv_split_pack_device(
                self.parameters.data_ptr(), self.split_index.data_ptr(),
                self.split_packs.data_ptr(), self.split_packs.shape[0],
                runtime.stream()), 'emph_conv_split_pack_device')

    def _parameter(self, name):
        return self.parameters.data_ptr() + 4 * self.offsets[name][0]

    def _gradient(self, name):
        return self.gradients.data_ptr() + 4 * self.offsets[name][0]

    def _layer_shape(self, name):
        """(c_in, kernel size) of conv layer `name`."""
        _, shape = self.offsets[f'{name}.weight']
        return shape[1], shape[2]

    def _mask(self, name):
        """(seed, stream, step) of the dropout mask of layer `name` at this
        step (`train/dropout.py`)."""
        return (self.seed & (1 << 64) - 1,
                dropout_module.stream_of(self.config, name), self.steps)

    def _conv(self, packs, name, bias, x, y, ld, activation, tiles, tile):
        """`emph_conv1d` at the shape of layer `name` with its pack of
        `packs`: the forward's, or the data gradient's (no input layer there,
        so c_in is the layer's own either way)."""
        c_in, kernel_size = self._layer_shape(name)
        runtime.check(self.lib.emph_conv1d(
            x.data_ptr(), ld, y.data_ptr(), ld,
            self.packs.data_ptr() + 4 * packs[name][0], bias, c_in,
            self.config.channels, kernel_size,
            runtime.ACTIVATIONS[activation], tiles.data_ptr(),
            _tile_count(tiles), tile, 0, runtime.stream()), 'emph_conv1d')

    def _conv_split(self, pack, bias, x, y, ld, relu, spans):
        """One Conv1d(80, 80, 3) on the frame axis as bf16x3: a launch of
        `emph_conv1d_split` with a single layer, whose output is kept."""
        runtime.check(self.lib.emph_conv1d_split(
            x.data_ptr(), ld, y.data_ptr(), ld,
            self.split_packs.data_ptr() + pack * self._split_bytes, bias, 1,
            1 if relu else 0, spans.data_ptr(), spans.numel() // 8, None,
            runtime.stream()), 'emph_conv1d_split')

    def _layer(self, name, x, y, ld, activation, meta, axis, tile):
        """Forward of conv layer `name` at the trainer's precision."""
        bias = self._parameter(f'{name}.bias')
        if name in self._split_forward:
            self._conv_split(self._split_forward[name], bias, x, y, ld,
                             activation == 'relu', meta['conv_spans'])
        else:
            self._conv(self._forward_packs, name, bias, x, y, ld, activation,
                       meta[('tiles', axis, tile)], tile)

    def _dropout(self, name, y):
        """`torch.nn.Dropout` on the kept output of layer `name`, in place:
        the mask of this layer at this step."""
        runtime.check(self.lib.emph_dropout(
            y.data_ptr(), y.numel(), 0, self.dropout, *self._mask(name),
            runtime.stream()), 'emph_dropout')

    def _forward_stack(self, meta, names, outputs, pre, ld, axis, tile,
                       training):
        """A conv stack (`model/layers/convolution.py:22-37`): outputs[i + 1]
        = dropout(act(conv(outputs[i]))), every output kept.  `pre`: None, or
        where the pre-activations are kept in training for an activation
        whose derivative reads them - the activation is then a pass of its
        own, which applies the mask too."""
        activation = self.config.activation
        drop = training and self.dropout > 0.
        for i, name in enumerate(names):
            if training and pre is not None:
                self._layer(name, outputs[i], pre[i], ld, None, meta, axis,
                            tile)
                runtime.check(self.lib.emph_activation_dropout(
                    pre[i].data_ptr(), outputs[i + 1].data_ptr(),
                    pre[i].numel(), runtime.ACTIVATIONS[activation],
                    self.dropout if drop else 0., *self._mask(name),
                    runtime.stream()), 'emph_activation_dropout')
                continue
            self._layer(name, outputs[i], outputs[i + 1], ld, activation,
                        meta, axis, tile)
            if drop:
                self._dropout(name, outputs[i + 1])

    def _encoder_forward(self, view, buffers, training):
        """input_layer and the frame encoder (model/core.py:91-94) on the
        layout of `view`, every layer's output kept: buffers['frames'][0 ..
        layers]."""
        h, ld_f = buffers['frames'], view.plan.ld_frames
        self._layer('input_layer', view.features, h[0], ld_f, None, view.meta,
                    runtime.AXIS_FRAMES, FRAME_TILE)
        self._forward_stack(
            view.meta, stack_names(self.config, 'frame_encoder'), h,
            buffers.get('pre_frames'), ld_f, runtime.AXIS_FRAMES, FRAME_TILE,
            training)

    def _segment_reduce(self, x, ld_x, bounds, table, segment, y, ld_y):
        """The words y [channels, ld_y] of the frames x, `segment` naming the
        table row of every word column."""
        runtime.check(self.lib.emph_segment_reduce(
            x.data_ptr(), ld_x, bounds.data_ptr(), y.data_ptr(), ld_y,
            self.config.channels, table.data_ptr(), segment.data_ptr(), ld_y,
            runtime.REDUCTIONS[self.config.downsample_method],
            runtime.stream()), 'emph_segment_reduce')

    def _reduce(self, view, batch, buffers):
        """The encoder's output to the words (model/core.py:96-104):
        buffers['words'][0]."""
        meta = batch.meta
        self._segment_reduce(
            buffers['frames'][self.config.layers], batch.plan.ld_frames,
            meta['bounds'], meta['table'], meta['word_segment'],
            buffers['words'][0], batch.plan.ld_words)

    def _word_logits(self, batch, words, buffers):
        """output_layer on `words` [channels, ld_words] (model/core.py:138):
        buffers['logits']."""
        meta, ld_w = batch.meta, batch.plan.ld_words
        runtime.check(self.lib.emph_output_layer(
            words.data_ptr(), ld_w, self._parameter('output_layer.weight'),
            self._parameter('output_layer.bias'), self.config.channels,
            self.config.decoder_kernel_size, meta['table'].data_ptr(),
            meta['word_segment'].data_ptr(), ld_w, runtime.AXIS_WORDS, 0,
            buffers['logits'].data_ptr(), None, runtime.stream()),
            'emph_output_layer')

    _output_layer_backward = 'emph_output_layer_backward'

    def _word_loss_backward(self, batch, words, buffers):
        """The loss of buffers['logits'] on the words (train/core.py:315-353)
        into `self.loss`, and output_layer's backward: its gradients and the
        gradient of `words` in buffers['word_grad'][0]."""
        config, ld_w = self.config, batch.plan.ld_words
        word_segment, dlogit = batch.meta['word_segment'], buffers['dlogit']
        runtime.check(self.lib.emph_loss_grad(
            buffers['logits'].data_ptr(), batch.targets.data_ptr(),
            word_segment.data_ptr(), ld_w, batch.plan.total_words,
            runtime.BCE_FORMS[config.loss], self.loss.data_ptr(),
            dlogit.data_ptr(), runtime.stream()), 'emph_loss_grad')
        entry = self._output_layer_backward
        runtime.check(getattr(self.lib, entry)(
            dlogit.data_ptr(), words.data_ptr(), ld_w,
            self._parameter('output_layer.weight'), word_segment.data_ptr(),
            config.channels, config.decoder_kernel_size, ld_w,
            self._gradient('output_layer.weight'),
            self._gradient('output_layer.bias'),
            buffers['word_grad'][0].data_ptr(), ld_w, runtime.stream()), entry)

    def _activation_backward(self, name, y, pre, dy):
        """dy times the derivative of layer `name`'s activation (and its
        dropout mask), in place: off the kept output `y`, which is zero where
        ReLU or the mask cut."""
        activation = runtime.ACTIVATIONS[self.config.activation]
        if self.dropout > 0.:
            runtime.check(self.lib.emph_activation_dropout_backward(
                y.data_ptr(), dy.data_ptr(), dy.numel(), activation,
                self.dropout, runtime.stream()),
                'emph_activation_dropout_backward')
        else:
            runtime.check(self.lib.emph_activation_backward(
                y.data_ptr(), dy.data_ptr(), dy.numel(), activation,
                runtime.stream()), 'emph_activation_backward')

    _weight_grad_kernel = 'emph_conv_weight_grad'

    def _weight_grad(self, dy, x, ld, name, tiles, buffers):
        entry = 'emph_conv_weight_grad_split' \
            if name in self._split_forward else self._weight_grad_kernel
        c_in, kernel_size = self._layer_shape(name)
        runtime.check(getattr(self.lib, entry)(
            dy.data_ptr(), ld, x.data_ptr(), ld, c_in, self.config.channels,
            kernel_size, tiles.data_ptr(), _tile_count(tiles), GRAD_TILE,
            buffers['slabs'].data_ptr(), self._gradient(f'{name}.weight'),
            self._gradient(f'{name}.bias'), runtime.stream()), entry)

    def _backward_stack(self, meta, buffers, names, outputs, pre, gradient,
                        ld, axis, tile):
        """Backward of a conv stack, from the gradient of the last output
        (gradient[0]) down to the gradient of outputs[0]; returns the buffer
        that holds it."""
        grad_tiles = meta[('tiles', axis, GRAD_TILE)]
        current = 0
        for i in range(len(names) - 1, -1, -1):
            name = names[i]
            dy = gradient[current]
            self._activation_backward(
                name, outputs[i + 1], None if pre is None else pre[i], dy)
            self._weight_grad(dy, outputs[i], ld, name, grad_tiles, buffers)
            if name in self._split_backward:
                self._conv_split(
                    self._split_backward[name], self._zero_bias.data_ptr(),
                    dy, gradient[1 - current], ld, False, meta['conv_spans'])
            else:
                self._conv(self._backward_packs, name, None, dy,
                           gradient[1 - current], ld, None,
                           meta[('tiles', axis, tile)], tile)
            current = 1 - current
        return gradient[current]

    def _encoder_backward(self, view, buffers):
        """From the gradient of the encoder's output (buffers['frame_grad'][0])
        to the gradients of the frame encoder and the input layer."""
        ld_f = view.plan.ld_frames
        dinput = self._backward_stack(
            view.meta, buffers, stack_names(self.config, 'frame_encoder'),
            buffers['frames'], buffers.get('pre_frames'),
            buffers['frame_grad'], ld_f, runtime.AXIS_FRAMES, FRAME_TILE)
        self._weight_grad(
            dinput, view.features, ld_f, 'input_layer',
            view.meta[('tiles', runtime.AXIS_FRAMES, GRAD_TILE)], buffers)

    def _reduce_backward(self, view, batch, buffers, dword):
        """The gradient `dword` of buffers['words'][0] back through the
        reduce, into buffers['frame_grad'][0]: every reduction (max reads the
        encoder's output and the pooled words, both kept)."""
        meta, plan = batch.meta, batch.plan
        tiles = meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
        runtime.check(self.lib.emph_segment_reduce_backward(
            dword.data_ptr(), plan.ld_words, meta['bounds'].data_ptr(),
            buffers['frames'][self.config.layers].data_ptr(), plan.ld_frames,
            buffers['words'][0].data_ptr(),
            buffers['frame_grad'][0].data_ptr(), plan.ld_frames,
            self.config.channels, meta['table'].data_ptr(), tiles.data_ptr(),
            _tile_count(tiles),
            runtime.REDUCTIONS[self.config.downsample_method],
            runtime.stream()), 'emph_segment_reduce_backward')

    ###########################################################################
    # Workspace
    ###########################################################################

    def _frame_plan(self, plan):
        """The layout the frame-rate layers run on."""
        return plan

    def _workspace_needs(self, frame_tiles, word_tiles):
        """{name: number}: what of a layout's tile counts the sizes of the
        buffers depend on (part of the cache key)."""
        counts = (frame_tiles, word_tiles) if self.config.has_decoder else \
            (frame_tiles,)
        return {'parts': max(
            int(self.lib.emph_conv_weight_grad_parts(n)) for n in counts)}

    def _slab_floats(self, needs):
        """The size of 'slabs', the workspace of the weight gradients."""
        channels = self.config.channels
        slab = channels * 3 * self.config.num_features + channels
        return max(needs['parts'], 1) * slab

    _buffer_dtypes = {}     # name -> dtype of the buffers that are not float32

    def _buffer_shapes(self, ld_frames, ld_words, needs):
        """{name: shape} of the step's buffers, in the order in which they
        are allocated."""
        channels, layers = self.config.channels, self.config.layers
        decoder = self.config.has_decoder
        return {
            'frames': (layers + 1, channels, ld_frames),
            'words': (layers + 1 if decoder else 1, channels, ld_words),
            'frame_grad': (2, channels, ld_frames),
            'word_grad': (2 if decoder else 1, channels, ld_words),
            'logits': (ld_words,),
            'dlogit': (ld_words,),
            'slabs': (self._slab_floats(needs),)}

    def _buffers(self, plan, frame_plan=None):
        """The activations and gradients of a step for a packed layout, kept
        between steps (zero at first, so that padding columns stay finite);
        one set at a time."""
        frame_plan = frame_plan or self._frame_plan(plan)
        needs = self._workspace_needs(
            len(frame_plan.tiles(runtime.AXIS_FRAMES, GRAD_TILE)),
            len(plan.tiles(runtime.AXIS_WORDS, GRAD_TILE)))
        ld_frames, ld_words = frame_plan.ld_frames, plan.ld_words
        key = (ld_frames, ld_words) + tuple(needs.values())
        found = self._workspace.get(key)
        if found is None:
            self._workspace.clear()
            shapes = self._buffer_shapes(ld_frames, ld_words, needs)
            found = self._workspace[key] = {
                name: torch.zeros(
                    shape, dtype=self._buffer_dtypes.get(name, torch.float32),
                    device=self.device)
                for name, shape in shapes.items()}
        return found

    ###########################################################################
    # API
    ###########################################################################

    def logits(self, batch):
        """The model's logits of a prepared `Batch`: the forward launches of a
        step alone (no loss, no gradient, no update).  Compact float32
        [total_words] on the device, the words of the items in order."""
        batch = self._batch((batch,))
        with torch.cuda.device(self.device):
            packed = self._forward(batch)['logits']
            columns = torch.from_numpy(
                batch.plan.word_columns()).to(self.device)
            return packed[columns]

    def loss_and_gradients(self, *batch):
        """(loss, {name: gradient}) of a collated batch (or a prepared
        `Batch`), device tensors; the parameters are left as they are."""
        batch = self._batch(batch)
        with torch.cuda.device(self.device):
            self._forward_backward(batch)
            flat = self.gradients.clone()
            loss = self.loss[0].clone()
        return loss, collections.OrderedDict(
            (name, self._view(flat, name)) for name in self.offsets)

    def step(self, *batch):
        """Forward, loss, backward, Adam and the next step's packs on the
        current stream; returns the loss (before the update) as a 0-dim device
        tensor without synchronising."""
        batch = self._batch(batch)
        with torch.cuda.device(self.device):
            self._forward_backward(batch)
            loss = self.loss[0].clone()
            self.steps += 1
            beta1, beta2 = self.betas
            correction1 = 1. - beta1 ** self.steps
            correction2 = 1. - beta2 ** self.steps
            runtime.check(self.lib.emph_adam_step(
                self.parameters.data_ptr(), self.gradients.data_ptr(),
                self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                self.count, beta1, beta2, self.lr / correction1,
                math.sqrt(correction2), self.eps, runtime.stream()),
                'emph_adam_step')
            self._repack()
        return loss


class _DecoderStep(_Step):
    """The step of the models with a word decoder, in the order of
    `model/core.py:41-107,138` and back: input layer, frame encoder, reduce,
    word decoder, output layer, loss, and their backwards in reverse.  A
    subclass overrides the launches that are its own: `_enter`, `_reduce` and
    `_reduce_backward`, `_activation_backward`, the two entry points
    `_weight_grad_kernel` and `_output_layer_backward`, and its buffers."""

    def _enter(self, batch):
        """(the step's buffers, the batch as the frame-rate layers see it)."""
        return self._buffers(batch.plan), batch

    def _forward_view(self, batch, training):
        config, ld_w = self.config, batch.plan.ld_words
        buffers, view = self._enter(batch)
        d = buffers['words']
        # ---- forward, every layer's output kept (model/core.py:91-107,138)
        self._encoder_forward(view, buffers, training)
        self._reduce(view, batch, buffers)
        self._forward_stack(
            batch.meta, stack_names(config, 'word_decoder'), d,
            buffers.get('pre_words'), ld_w, runtime.AXIS_WORDS, WORD_TILE,
            training)
        self._word_logits(batch, d[config.layers], buffers)
        return buffers, view

    def _forward(self, batch, training=False):
        """The forward launches of a step; returns the step's buffers, whose
        'logits' then hold the packed logits [ld_words].  `training`: the
        train-mode forward, which keeps what the backward reads and applies
        the dropout masks of the step (never for validation)."""
        return self._forward_view(batch, training)[0]

    def _forward_backward(self, batch):
        config, ld_w = self.config, batch.plan.ld_words
        buffers, view = self._forward_view(batch, True)
        d = buffers['words']
        # ---- loss (train/core.py:315-353) and backward
        self._word_loss_backward(batch, d[config.layers], buffers)
        dword = self._backward_stack(
            batch.meta, buffers, stack_names(config, 'word_decoder'), d,
            buffers.get('pre_words'), buffers['word_grad'], ld_w,
            runtime.AXIS_WORDS, WORD_TILE)
        self._reduce_backward(view, batch, buffers, dword)
        self._encoder_backward(view, buffers)


class Trainer(_DecoderStep):
    """`Trainer(...).step(*batch[:5])` is one iteration of the reference's loop
    (`train/core.py:105-142`) for the convolution model; see the module
    docstring for the two deviations."""

    def _reduce_backward(self, view, batch, buffers, dword):
        """'sum' and 'average' need nothing kept: every frame takes its
        word's gradient."""
        meta, plan = batch.meta, batch.plan
        tiles = meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
        runtime.check(self.lib.emph_segment_broadcast(
            dword.data_ptr(), plan.ld_words, meta['bounds'].data_ptr(),
            buffers['frame_grad'][0].data_ptr(), plan.ld_frames,
            self.config.channels, meta['table'].data_ptr(), tiles.data_ptr(),
            _tile_count(tiles),
            runtime.REDUCTIONS[self.config.downsample_method],
            runtime.stream()), 'emph_segment_broadcast')


class EncoderTrainer(_Step):
    """`Trainer` for the models without a word decoder, downsample_location
    'inference' and 'loss' (`check_encoder_supported`); see the module
    docstring.  The same interface: `data.Loader` and `train.evaluate` take
    either.  `logits` is the model in eval mode for both locations
    (`model/core.py:109-138`): encoder, reduce, word-rate output layer, no
    dropout."""

    _check = staticmethod(check_encoder_supported)

    def _workspace_needs(self, frame_tiles, word_tiles):
        return dict(
            super()._workspace_needs(frame_tiles, word_tiles),
            head_parts=int(self.lib.emph_frame_head_parts(frame_tiles)),
            frame_tiles=frame_tiles)

    def _slab_floats(self, needs):
        """... and of the frame head's backward."""
        return max(
            super()._slab_floats(needs),
            max(needs['head_parts'], 1) * (3 * self.config.channels + 1))

    _buffer_dtypes = {'partials': torch.float64}

    def _buffer_shapes(self, ld_frames, ld_words, needs):
        shapes = super()._buffer_shapes(ld_frames, ld_words, needs)
        slabs = shapes.pop('slabs')
        return dict(
            shapes, frame_logits=(ld_frames,), frame_dlogit=(ld_frames,),
            partials=(max(needs['frame_tiles'], 1),), slabs=slabs)

    def _forward(self, batch, training=False):
        """The forward launches; returns the step's buffers.  In training at
        'inference' (`model/core.py:117-122`) their 'frame_logits' hold the
        packed frame logits [ld_frames]; everywhere else - 'loss', and both
        locations in eval mode, `model/core.py:109-138` - their 'logits' hold
        the packed word logits [ld_words].  `training`: with the dropout
        masks of the step."""
        config, layers = self.config, self.config.layers
        buffers = self._buffers(batch.plan)
        self._encoder_forward(batch, buffers, training)
        if training and config.downsample_location == 'inference':
            tiles = batch.meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
            runtime.check(self.lib.emph_frame_head(
                buffers['frames'][layers].data_ptr(), batch.plan.ld_frames,
                self._parameter('output_layer.weight'),
                self._parameter('output_layer.bias'), config.channels, 3,
                tiles.data_ptr(), _tile_count(tiles),
                buffers['frame_logits'].data_ptr(), runtime.stream()),
                'emph_frame_head')
            return buffers
        self._reduce(batch, batch, buffers)
        self._word_logits(batch, buffers['words'][0], buffers)
        return buffers

    def _forward_backward(self, batch):
        config, lib, plan, meta = self.config, self.lib, batch.plan, batch.meta
        channels, layers = config.channels, config.layers
        ld_f, ld_w = plan.ld_frames, plan.ld_words
        frame_tiles = meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
        n_tiles = _tile_count(frame_tiles)
        if config.downsample_location == 'inference' and \
                (len(plan.words) == 0 or int(min(plan.words)) < 1):
            raise ValueError(
                "downsample_location 'inference' interpolates the targets of "
                'every utterance from its words: an utterance has none')
        buffers = self._forward(batch, training=True)
        stream = runtime.stream()
        h, dh = buffers['frames'], buffers['frame_grad']
        if config.downsample_location == 'inference':
            # ---- loss on the frames (train/core.py:324-353) and the head
            logits, dlogit = buffers['frame_logits'], buffers['frame_dlogit']
            runtime.check(lib.emph_frame_loss_grad(
                logits.data_ptr(), batch.targets.data_ptr(),
                meta['bounds'].data_ptr(), ld_w, meta['table'].data_ptr(),
                frame_tiles.data_ptr(), n_tiles, plan.total_frames,
                runtime.BCE_FORMS[config.loss],
                runtime.UPSAMPLE_METHODS[config.upsample_method],
                buffers['partials'].data_ptr(), self.loss.data_ptr(),
                dlogit.data_ptr(), stream), 'emph_frame_loss_grad')
            runtime.check(lib.emph_frame_head_backward(
                dlogit.data_ptr(), h[layers].data_ptr(), ld_f,
                self._parameter('output_layer.weight'), channels, 3,
                frame_tiles.data_ptr(), n_tiles, buffers['slabs'].data_ptr(),
                self._gradient('output_layer.weight'),
                self._gradient('output_layer.bias'), dh[0].data_ptr(), ld_f,
                stream), 'emph_frame_head_backward')
        else:
            # ---- loss on the words (train/core.py:341-353), the head and
            # the reduce
            self._word_loss_backward(batch, buffers['words'][0], buffers)
            self._reduce_backward(
                batch, batch, buffers, buffers['word_grad'][0])
        self._encoder_backward(batch, buffers)


class PieceTrainer(Trainer):
    """`Trainer` for downsample_location 'input' (`check_pieces_supported`);
    see the module docstring.  The same interface: `data.Loader` and
    `train.evaluate` take it.  A batch carries the features on the frame
    layout, as everywhere; the step gathers them into the piece layout
    (`batch.Pieces`), runs the frame-rate layers there, and pools every piece
    into the word column of the batch's own plan."""

    _check = staticmethod(check_pieces_supported)

    def metadata(self, plan):
        """`Trainer.metadata` plus, under 'pieces', the tables of the piece
        layout: its segment table, its frame tiles (and spans at 'bf16x3'),
        the gather table, the piece bounds, `word_piece` and `piece_column` -
        all in ONE copy to the device."""
        pieces = plan.pieces(self.config.downsample_method)
        tables = [
            plan.pack_metadata(list(dict.fromkeys(
                [(runtime.AXIS_WORDS, WORD_TILE),
                 (runtime.AXIS_WORDS, GRAD_TILE)]))),
            pieces.plan.pack_metadata(
                list(dict.fromkeys([(runtime.AXIS_FRAMES, FRAME_TILE),
                                    (runtime.AXIS_FRAMES, GRAD_TILE)])),
                spans=self.precision == 'bf16x3')]
        # (every part starts on a 16-byte boundary, the int64 tables included)
        for name, array in (('gather', pieces.gather.view(np.int32).ravel()),
                            ('piece_bounds', pieces.bounds.ravel()),
                            ('word_piece', pieces.word_piece),
                            ('piece_column', pieces.piece_column)):
            padded = np.zeros(-(-max(array.size, 1) // 4) * 4, dtype=np.int32)
            padded[:array.size] = array
            tables.append((padded, {name: (0, array.size)}))
        buffer, (meta, piece_meta, *extras) = self._upload(tables)
        for extra in extras:
            piece_meta.update(extra)
        piece_meta['plan'] = pieces.plan
        meta['pieces'] = piece_meta
        meta['_buffer'] = buffer
        return meta

    def _frame_meta(self, batch):
        pieces = batch.meta.get('pieces')
        if pieces is None:
            raise ValueError(
                'the batch carries no piece tables: prepare it with this '
                "trainer (downsample_location='input')")
        return pieces

    def _frame_plan(self, plan):
        return plan.pieces(self.config.downsample_method).plan

    def _buffer_shapes(self, ld_frames, ld_words, needs):
        """The frame-rate buffers are on the piece layout, the word-rate ones
        on the batch's own; 'piece_features': the features gathered there."""
        return {'piece_features': (self.config.num_features, ld_frames),
                **super()._buffer_shapes(ld_frames, ld_words, needs)}

    def _enter(self, batch):
        """Gathers the features into the piece layout (`model/core.py:41-87`):
        the view is the batch there."""
        pieces = batch.meta['pieces']
        piece_plan = pieces['plan']
        buffers = self._buffers(batch.plan, piece_plan)
        gathered = buffers['piece_features']
        runtime.check(self.lib.emph_gather_columns(
            batch.features.data_ptr(), batch.plan.ld_frames,
            gathered.data_ptr(), piece_plan.ld_frames,
            self.config.num_features, pieces['gather'].data_ptr(),
            len(piece_plan), runtime.stream()), 'emph_gather_columns')
        return buffers, Batch(piece_plan, pieces, gathered, None)

    def _reduce(self, view, batch, buffers):
        """Every piece pooled over its PADDED axis into its word's column."""
        pieces = view.meta
        self._segment_reduce(
            buffers['frames'][self.config.layers], view.plan.ld_frames,
            pieces['piece_bounds'], pieces['table'], pieces['word_piece'],
            buffers['words'][0], batch.plan.ld_words)

    def _reduce_backward(self, view, batch, buffers, dword):
        """The pooled words back to the columns of their pieces."""
        ld_p = view.plan.ld_frames
        tiles = view.meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
        runtime.check(self.lib.emph_piece_pool_backward(
            dword.data_ptr(), batch.plan.ld_words,
            view.meta['gather'].data_ptr(),
            view.meta['piece_column'].data_ptr(), len(view.plan),
            buffers['frames'][self.config.layers].data_ptr(), ld_p,
            buffers['words'][0].data_ptr(),
            buffers['frame_grad'][0].data_ptr(), ld_p, self.config.channels,
            tiles.data_ptr(), _tile_count(tiles),
            runtime.REDUCTIONS[self.config.downsample_method],
            runtime.stream()), 'emph_piece_pool_backward')


class GridTrainer(_DecoderStep):
    """`Trainer` for the reference's hyperparameter grid at
    downsample_location 'intermediate' (`check_grid_supported`): every
    activation, reduction, channel count and kernel size of
    `config/hparam-search` and `config/downsample/*-intermediate.py`, at
    precision 'f32'.  The same interface and the same deviations as `Trainer`;
    the launches are the general kernels (`emph_conv1d` with the layer's own
    shape, `emph_conv_weight_grad_any`, `emph_segment_reduce_backward`,
    `emph_output_layer_backward_any`), so at the default configuration it
    computes what `Trainer` computes but not with its bits.

    ReLU and LeakyReLU differentiate off the kept output; GELU and SiLU need
    the pre-activation, which the convolution then writes into a second set
    of buffers ('pre_frames', 'pre_words') and `emph_activation_dropout` turns
    into the layer's output: one pass more per layer, never a second
    convolution.  Under dropout the backward regenerates the mask
    (`emph_activation_dropout_gradient`)."""

    _check = staticmethod(check_grid_supported)
    _weight_grad_kernel = 'emph_conv_weight_grad_any'
    _output_layer_backward = 'emph_output_layer_backward_any'

    def __init__(self, config=None, checkpoint=None, gpu=None, lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, seed=0, precision='f32'):
        check_grid_precision(precision)
        super().__init__(config, checkpoint, gpu, lr, betas, eps, seed,
                         precision)

    def _workspace_needs(self, frame_tiles, word_tiles):
        config = self.config
        channels = config.channels
        shapes = [(config.num_features, config.encoder_kernel_size, frame_tiles)]
        if config.layers:
            shapes += [(channels, config.encoder_kernel_size, frame_tiles),
                       (channels, config.decoder_kernel_size, word_tiles)]
        return {'workspace': max(
            int(self.lib.emph_conv_weight_grad_any_workspace(
                c_in, channels, kernel_size, tiles))
            for c_in, kernel_size, tiles in shapes)}

    def _slab_floats(self, needs):
        return max(needs['workspace'], 1)

    def _buffer_shapes(self, ld_frames, ld_words, needs):
        """... and the pre-activations, where the activation's derivative
        reads them."""
        shapes = super()._buffer_shapes(ld_frames, ld_words, needs)
        if self.config.activation in ('gelu', 'silu'):
            channels, layers = self.config.channels, self.config.layers
            shapes['pre_frames'] = (layers, channels, ld_frames)
            shapes['pre_words'] = (layers, channels, ld_words)
        return shapes

    def _activation_backward(self, name, y, pre, dy):
        """Off the pre-activation where it is kept, off the kept output
        otherwise; under dropout with the regenerated mask."""
        source = y if pre is None else pre
        activation = runtime.ACTIVATIONS[self.config.activation]
        if self.dropout > 0.:
            runtime.check(self.lib.emph_activation_dropout_gradient(
                source.data_ptr(), dy.data_ptr(), dy.numel(), activation,
                self.dropout, *self._mask(name), runtime.stream()),
                'emph_activation_dropout_gradient')
        else:
            runtime.check(self.lib.emph_activation_gradient(
                source.data_ptr(), dy.data_ptr(), dy.numel(), activation,
                runtime.stream()), 'emph_activation_gradient')


def _build(config, arguments, **dispatch):
    config = config or api.active_config()
    return step_class(config, **dispatch)(config, **arguments)


def select_trainer(config=None, **arguments):
    """The fused step that trains `config`: what `trainer_for` returns where
    a specialised step covers it (so such a configuration keeps that step and
    its bits), a `GridTrainer` where none does and `check_grid_supported`
    passes; otherwise the specialised step's refusal.  Every check comes
    before anything is constructed or a GPU is needed."""
    return _build(config, arguments,
                  precision=arguments.get('precision', 'f32'))


MADE_LOCATIONS = ('intermediate', 'inference', 'loss')


def trainer_for(config=None, **arguments):
    """The step that trains `config` at any downsample_location, never the
    grid step: a `PieceTrainer` at 'input' where `check_pieces_supported` and
    `check_precision` pass, `make_trainer(...)` everywhere else; the refusal
    that names the offending field comes first, before a GPU is needed."""
    config = config or api.active_config()
    if config.downsample_location in MADE_LOCATIONS:
        return make_trainer(config, **arguments)
    return _build(config, arguments, grid=False,
                  precision=arguments.get('precision', 'f32'))


def make_trainer(config=None, **arguments):
    """The step that trains `config`: a `Trainer` where `check_supported`
    passes, an `EncoderTrainer` at downsample_location 'inference' and 'loss'
    where `check_encoder_supported` passes; otherwise the refusal that names
    the offending field, before a GPU is needed."""
    return _build(config, arguments, grid=False, locations=MADE_LOCATIONS)
