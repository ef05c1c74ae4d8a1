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


def check_supported(config):
    """NotImplementedError, naming the field, for a configuration the step does
    not cover - before anything is allocated or launched."""
    def refuse(field, supported):
        raise NotImplementedError(
            f'the training step supports {field} {supported} only, not '
            f'{field}={getattr(config, field)!r}')
    if config.method != 'neural':
        refuse('method', "'neural'")
    if config.architecture != 'convolution':
        refuse('architecture', "'convolution'")
    if config.downsample_location != 'intermediate':
        refuse('downsample_location', "'intermediate'")
    if config.downsample_method not in ('sum', 'average'):
        refuse('downsample_method', "'sum' or 'average'")
    if config.activation != 'relu':
        refuse('activation', "'relu'")
    if config.loss not in ('bce', 'mse'):
        refuse('loss', "'bce' or 'mse'")
    if config.channels != 80:
        refuse('channels', '80')
    if config.encoder_kernel_size != 3:
        refuse('encoder_kernel_size', '3')
    if config.decoder_kernel_size != 3:
        refuse('decoder_kernel_size', '3')
    if not 0 <= config.layers <= 16:
        refuse('layers', '0..16')
    if not config.mel_feature:
        refuse('mel_feature', 'True (80..83 input features)')


def check_encoder_supported(config):
    """`check_supported` for `EncoderTrainer`: the models without a word
    decoder, downsample_location 'inference' or 'loss'."""
    def refuse(field, supported):
        raise NotImplementedError(
            f'the encoder training step supports {field} {supported} only, '
            f'not {field}={getattr(config, field)!r}')
    if config.method != 'neural':
        refuse('method', "'neural'")
    if config.architecture != 'convolution':
        refuse('architecture', "'convolution'")
    if config.downsample_location not in ('inference', 'loss'):
        refuse('downsample_location', "'inference' or 'loss'")
    if config.activation != 'relu':
        refuse('activation', "'relu'")
    if config.loss not in ('bce', 'mse'):
        refuse('loss', "'bce' or 'mse'")
    if config.channels != 80:
        refuse('channels', '80')
    if config.encoder_kernel_size != 3:
        refuse('encoder_kernel_size', '3')
    if config.decoder_kernel_size != 3:
        refuse('decoder_kernel_size', "3 (the output layer's kernel size)")
    if not 0 <= config.layers <= 16:
        refuse('layers', '0..16')
    if not config.mel_feature:
        refuse('mel_feature', 'True (80..83 input features)')


def check_pieces_supported(config):
    """`check_supported` for `PieceTrainer`: downsample_location 'input', all
    four reductions, no dropout."""
    def refuse(field, supported):
        raise NotImplementedError(
            f'the piece training step supports {field} {supported} only, '
            f'not {field}={getattr(config, field)!r}')
    if config.method != 'neural':
        refuse('method', "'neural'")
    if config.architecture != 'convolution':
        refuse('architecture', "'convolution'")
    if config.downsample_location != 'input':
        refuse('downsample_location', "'input'")
    if config.downsample_method not in ('sum', 'average', 'max', 'center'):
        refuse('downsample_method', "'sum', 'average', 'max' or 'center'")
    if config.activation != 'relu':
        refuse('activation', "'relu'")
    if config.loss not in ('bce', 'mse'):
        refuse('loss', "'bce' or 'mse'")
    if config.channels != 80:
        refuse('channels', '80')
    if config.encoder_kernel_size != 3:
        refuse('encoder_kernel_size', '3')
    if config.decoder_kernel_size != 3:
        refuse('decoder_kernel_size', '3')
    if not 0 <= config.layers <= 16:
        refuse('layers', '0..16')
    if not config.mel_feature:
        refuse('mel_feature', 'True (80..83 input features)')
    if config.dropout is not None:
        refuse('dropout', 'None (no mask is specified for the piece layout)')


GRID_CHANNELS = tuple(range(16, 129, 16))   # `TorchModel`'s rule
GRID_KERNEL_SIZES = (1, 3, 5, 7)


def check_grid_supported(config):
    """`check_supported` for `GridTrainer`: the reference's hyperparameter
    grid at downsample_location 'intermediate' - any activation, reduction,
    channel count (a multiple of 16 up to 128) and odd kernel size up to 7."""
    def refuse(field, supported):
        raise NotImplementedError(
            f'the grid training step supports {field} {supported} only, not '
            f'{field}={getattr(config, field)!r}')
    if config.method != 'neural':
        refuse('method', "'neural'")
    if config.architecture != 'convolution':
        refuse('architecture', "'convolution'")
    if config.downsample_location != 'intermediate':
        refuse('downsample_location', "'intermediate'")
    if config.downsample_method not in ('sum', 'average', 'max', 'center'):
        refuse('downsample_method', "'sum', 'average', 'max' or 'center'")
    if config.activation not in ('relu', 'gelu', 'silu', 'leaky_relu'):
        refuse('activation', "'relu', 'gelu', 'silu' or 'leaky_relu'")
    if config.loss not in ('bce', 'mse'):
        refuse('loss', "'bce' or 'mse'")
    if config.channels not in GRID_CHANNELS:
        refuse('channels', 'a multiple of 16 in 16..128')
    if config.encoder_kernel_size not in GRID_KERNEL_SIZES:
        refuse('encoder_kernel_size', '1, 3, 5 or 7')
    if config.decoder_kernel_size not in GRID_KERNEL_SIZES:
        refuse('decoder_kernel_size', '1, 3, 5 or 7')
    if not 0 <= config.layers <= 16:
        refuse('layers', '0..16')
    if not config.mel_feature:
        refuse('mel_feature', 'True (80..83 input features)')
    if config.dropout is not None and not 0. <= config.dropout < 1.:
        refuse('dropout', 'None or a probability 0 <= p < 1')


def check_grid_precision(precision):
    """`check_precision` for `GridTrainer`: 'f32' only.  The split kernels of
    'bf16x3' are Conv1d(80, 80, 3) with a ReLU flag and nothing else."""
    if check_precision(precision) != 'f32':
        raise NotImplementedError(
            "the grid training step supports precision 'f32' only, not "
            f'precision={precision!r}: the bf16 split kernels are '
            'Conv1d(80, 80, 3) with ReLU')
    return precision


def _check_step(config):
    """The check of the step that trains `config`: `PieceTrainer`'s at
    downsample_location 'input', `Trainer`'s with a word decoder otherwise
    (`GridTrainer`'s where that refuses), `EncoderTrainer`'s without one."""
    if config.downsample_location == 'input':
        check_pieces_supported(config)
    elif config.has_decoder:
        try:
            check_supported(config)
        except NotImplementedError:
            try:
                check_grid_supported(config)
            except NotImplementedError:
                pass
            else:
                return
            raise
    else:
        check_encoder_supported(config)


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


def split_layer_names(config):
    """The layers of `layer_names` that run on the bf16 pipe under
    precision='bf16x3': the Conv1d(80, 80, 3) on the frame axis (the input
    layer only when it has exactly 80 feature rows)."""
    names = ['input_layer'] if config.num_features == SPLIT_CHANNELS else []
    return names + [f'frame_encoder.{2 * i}' for i in range(config.layers)]


def layer_names(config):
    """The Conv1d(., 80, 3) layers in forward order (no word decoder at
    downsample_location 'inference' and 'loss', `model/core.py:28-30`)."""
    prefixes = ('frame_encoder', 'word_decoder') if config.has_decoder else \
        ('frame_encoder',)
    return ['input_layer'] + [
        f'{prefix}.{2 * i}' for prefix in prefixes
        for i in range(config.layers)]


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
    _check_step(config)
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


def _pack_indices(indices):
    """`emph_conv_pack` of an index array [c_out, c_in, k] (int, < 2^24): the
    pack is a pure permutation with zero padding, so packing the indices + 1
    gives, minus 1, where every element of a pack comes from (-1: padding)."""
    assert indices.max() + 1 < 1 << 24
    packed = runtime.conv_pack((indices + 1).astype(np.float32))
    return packed.astype(np.int64) - 1


def gather_tables(config=cfg.DEFAULT):
    """The `emph_take` table of every pack of a step: int32 `index` into the
    flat parameter buffer (-1: zero), and {layer: (first, size)} of the forward
    packs (every layer) and of the data-gradient packs
    W'[ci][co][j] = W[co][ci][k - 1 - j] (every layer but the input layer,
    whose input needs no gradient)."""
    _check_step(config)
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
            piece = _pack_indices(indices)
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
    _check_step(config)
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


class _Step:
    """What `Trainer` and `EncoderTrainer` share: the flat state, the batch
    layout, the frame encoder's launches, Adam and the checkpoint.  A
    subclass names its `_check` and gives `_buffers`, `_forward` (whose
    buffers' 'logits' then hold the packed word logits) and
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
        self.lr, self.betas, self.eps = float(lr), tuple(betas), float(eps)
        self.steps = 0
        self.seed = int(seed)
        # (None and 0. launch nothing: torch.nn.Dropout(0.) is the identity)
        self.dropout = float(config.dropout or 0.)
        optimizer = None
        if checkpoint is None:
            state = initial_state(config, seed)
        else:
            if not isinstance(checkpoint, dict) and \
                    not str(checkpoint).endswith('.npz'):
                checkpoint = torch.load(
                    os.fspath(checkpoint), map_location='cpu',
                    weights_only=False)
            if isinstance(checkpoint, dict) and 'model' in checkpoint:
                optimizer = checkpoint.get('optimizer')
                checkpoint = checkpoint['model']
            state = weights_module.load(checkpoint, config)
        self.offsets, self.count = parameter_offsets(config)
        tables = gather_tables(config)
        self.device = runtime.require_gpu(gpu)
        self.lib = runtime.library()
        with torch.cuda.device(self.device):
            flat = np.concatenate([state[name].ravel() for name in self.offsets])
            self.parameters = torch.from_numpy(flat).to(self.device)
            self.gradients = torch.zeros_like(self.parameters)
            self.exp_avg = torch.zeros_like(self.parameters)
            self.exp_avg_sq = torch.zeros_like(self.parameters)
            if optimizer is not None and optimizer.get('state'):
                self._restore(optimizer)
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

    def state_dict(self):
        """The parameters under the reference's names (`checkpoint_names`)
        and shapes (CPU)."""
        flat = self.parameters.cpu()
        saved = checkpoint_names(self.config)
        return collections.OrderedDict(
            (saved[name], self._view(flat, name).clone())
            for name in self.offsets)

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

    def metadata(self, plan):
        """The integer tables of a step for a packed layout on the device: one
        copy, views by name (`Batch.meta`)."""
        requests = [(runtime.AXIS_FRAMES, FRAME_TILE),
                    (runtime.AXIS_WORDS, WORD_TILE),
                    (runtime.AXIS_WORDS, GRAD_TILE)]
        host, offsets = plan.pack_metadata(
            list(dict.fromkeys(requests)), spans=self.precision == 'bf16x3')
        with torch.cuda.device(self.device):
            device_meta = torch.from_numpy(host).to(self.device)
        meta = {name: device_meta[start:start + size]
                for name, (start, size) in offsets.items()}
        meta['_buffer'] = device_meta
        return meta

    def _batch(self, arguments):
        if len(arguments) == 1 and isinstance(arguments[0], Batch):
            if self._split_forward and 'conv_spans' not in arguments[0].meta:
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

    def _conv(self, pack, bias, x, y, ld, c_in, activation, tiles, tile):
        runtime.check(self.lib.emph_conv1d(
            x.data_ptr(), ld, y.data_ptr(), ld,
            self.packs.data_ptr() + 4 * pack[0], bias, c_in,
            self.config.channels, 3, runtime.ACTIVATIONS[activation],
            tiles.data_ptr(), tiles.numel() // runtime.TILE_FIELDS, tile, 0,
            runtime.stream()), 'emph_conv1d')

    def _conv_split(self, pack, bias, x, y, ld, relu, spans):
        """One Conv1d(80, 80, 3) on the frame axis as bf16x3: a launch of
        `emph_conv1d_split` with a single layer, whose output is kept."""
        runtime.check(self.lib.emph_conv1d_split(
            x.data_ptr(), ld, y.data_ptr(), ld,
            self.split_packs.data_ptr() + pack * self._split_bytes, bias, 1,
            1 if relu else 0, spans.data_ptr(), spans.numel() // 8, None,
            runtime.stream()), 'emph_conv1d_split')

    def _frame_conv(self, name, x, y, ld, c_in, activation, batch):
        """Forward of a frame-rate layer at the trainer's precision."""
        if name in self._split_forward:
            self._conv_split(
                self._split_forward[name], self._parameter(f'{name}.bias'),
                x, y, ld, activation == 'relu', batch.meta['conv_spans'])
        else:
            self._conv(
                self._forward_packs[name], self._parameter(f'{name}.bias'),
                x, y, ld, c_in, activation,
                batch.meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)],
                FRAME_TILE)

    def _dropout(self, name, y):
        """`torch.nn.Dropout` on the kept output of layer `name`, in place:
        the mask of this layer at this step (`train/dropout.py`)."""
        runtime.check(self.lib.emph_dropout(
            y.data_ptr(), y.numel(), 0, self.dropout,
            self.seed & (1 << 64) - 1,
            dropout_module.stream_of(self.config, name), self.steps,
            runtime.stream()), 'emph_dropout')

    def _encoder_forward(self, batch, h, drop):
        """input_layer and the frame encoder (model/core.py:91-94), every
        layer's output kept: h[0] .. h[layers]."""
        config, ld_f = self.config, batch.plan.ld_frames
        self._frame_conv('input_layer', batch.features, h[0], ld_f,
                         config.num_features, None, batch)
        for i in range(config.layers):
            name = f'frame_encoder.{2 * i}'
            self._frame_conv(name, h[i], h[i + 1], ld_f, config.channels,
                             'relu', batch)
            if drop:
                self._dropout(name, h[i + 1])

    def _backward_stack(self, batch, buffers, names, outputs, gradient, ld,
                        grad_tiles, tiles, tile):
        """Backward of a conv stack, from the gradient of the last output
        (gradient[0]) down to the gradient of outputs[0]; returns the buffer
        that holds it."""
        lib, channels, stream = self.lib, self.config.channels, runtime.stream()
        current = 0
        for i in range(len(names) - 1, -1, -1):
            name = names[i]
            dy = gradient[current]
            if self.dropout > 0.:
                runtime.check(lib.emph_activation_dropout_backward(
                    outputs[i + 1].data_ptr(), dy.data_ptr(), dy.numel(),
                    runtime.ACTIVATIONS['relu'], self.dropout, stream),
                    'emph_activation_dropout_backward')
            else:
                runtime.check(lib.emph_activation_backward(
                    outputs[i + 1].data_ptr(), dy.data_ptr(), dy.numel(),
                    runtime.ACTIVATIONS['relu'], stream),
                    'emph_activation_backward')
            self._weight_grad(dy, outputs[i], ld, channels, name,
                              grad_tiles, buffers)
            if name in self._split_backward:
                self._conv_split(
                    self._split_backward[name],
                    self._zero_bias.data_ptr(), dy, gradient[1 - current],
                    ld, False, batch.meta['conv_spans'])
            else:
                self._conv(self._backward_packs[name], None, dy,
                           gradient[1 - current], ld, channels, None,
                           tiles, tile)
            current = 1 - current
        return gradient[current]

    def _encoder_backward(self, batch, buffers):
        """From the gradient of the encoder's output (buffers['frame_grad'][0])
        to the gradients of the frame encoder and the input layer."""
        config, ld_f = self.config, batch.plan.ld_frames
        frame_tiles = batch.meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
        encoder = [f'frame_encoder.{2 * i}' for i in range(config.layers)]
        dinput = self._backward_stack(
            batch, buffers, encoder, buffers['frames'], buffers['frame_grad'],
            ld_f, frame_tiles, frame_tiles, FRAME_TILE)
        self._weight_grad(dinput, batch.features, ld_f, config.num_features,
                          'input_layer', frame_tiles, buffers)

    def _weight_grad(self, dy, x, ld, c_in, name, tiles, buffers):
        split = name in self._split_forward
        entry = 'emph_conv_weight_grad_split' if split else \
            'emph_conv_weight_grad'
        runtime.check(getattr(self.lib, entry)(
            dy.data_ptr(), ld, x.data_ptr(), ld, c_in, self.config.channels, 3,
            tiles.data_ptr(), tiles.numel() // runtime.TILE_FIELDS, GRAD_TILE,
            buffers['slabs'].data_ptr(), self._gradient(f'{name}.weight'),
            self._gradient(f'{name}.bias'), runtime.stream()), entry)

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


class Trainer(_Step):
    """`Trainer(...).step(*batch[:5])` is one iteration of the reference's loop
    (`train/core.py:105-142`) for the convolution model; see the module
    docstring for the two deviations."""

    def _buffers(self, plan):
        """The activations and gradients of a step for a packed layout, kept
        between steps (zero at first, so that padding columns stay finite)."""
        frame_tiles = len(plan.tiles(runtime.AXIS_FRAMES, GRAD_TILE))
        word_tiles = len(plan.tiles(runtime.AXIS_WORDS, GRAD_TILE))
        parts = max(
            int(self.lib.emph_conv_weight_grad_parts(n))
            for n in (frame_tiles, word_tiles))
        key = (plan.ld_frames, plan.ld_words, parts)
        found = self._workspace.get(key)
        if found is None:
            self._workspace.clear()
            channels, layers = self.config.channels, self.config.layers
            zeros = lambda *shape: torch.zeros(  # noqa: E731
                shape, dtype=torch.float32, device=self.device)
            slab = channels * 3 * self.config.num_features + channels
            found = {
                'frames': zeros(layers + 1, channels, plan.ld_frames),
                'words': zeros(layers + 1, channels, plan.ld_words),
                'frame_grad': zeros(2, channels, plan.ld_frames),
                'word_grad': zeros(2, channels, plan.ld_words),
                'logits': zeros(plan.ld_words),
                'dlogit': zeros(plan.ld_words),
                'slabs': zeros(max(parts, 1) * slab)}
            self._workspace[key] = found
        return found

    def _forward(self, batch, training=False):
        """The forward launches of a step; returns the step's buffers, whose
        'logits' then hold the packed logits [ld_words].  `training`: with
        the dropout masks of the step (never for validation)."""
        config, lib, plan, meta = self.config, self.lib, batch.plan, batch.meta
        channels, layers = config.channels, config.layers
        ld_f, ld_w = plan.ld_frames, plan.ld_words
        frames, words = runtime.AXIS_FRAMES, runtime.AXIS_WORDS
        buffers = self._buffers(plan)
        stream = runtime.stream()
        drop = training and self.dropout > 0.
        word_tiles = meta[('tiles', words, WORD_TILE)]
        table, bounds = meta['table'], meta['bounds']
        word_segment = meta['word_segment']
        mode = runtime.REDUCTIONS[config.downsample_method]
        decoder = [f'word_decoder.{2 * i}' for i in range(layers)]

        # ---- forward, every layer's output kept (model/core.py:91-107,138)
        h, d = buffers['frames'], buffers['words']
        self._encoder_forward(batch, h, drop)
        runtime.check(lib.emph_segment_reduce(
            h[layers].data_ptr(), ld_f, bounds.data_ptr(), d[0].data_ptr(),
            ld_w, channels, table.data_ptr(), word_segment.data_ptr(), ld_w,
            mode, stream), 'emph_segment_reduce')
        for i, name in enumerate(decoder):
            self._conv(self._forward_packs[name],
                       self._parameter(f'{name}.bias'), d[i], d[i + 1], ld_w,
                       channels, 'relu', word_tiles, WORD_TILE)
            if drop:
                self._dropout(name, d[i + 1])
        logits = buffers['logits']
        runtime.check(lib.emph_output_layer(
            d[layers].data_ptr(), ld_w, self._parameter('output_layer.weight'),
            self._parameter('output_layer.bias'), channels, 3,
            table.data_ptr(), word_segment.data_ptr(), ld_w, words, 0,
            logits.data_ptr(), None, stream), 'emph_output_layer')
        return buffers

    def _forward_backward(self, batch):
        config, lib, plan, meta = self.config, self.lib, batch.plan, batch.meta
        channels, layers = config.channels, config.layers
        ld_f, ld_w = plan.ld_frames, plan.ld_words
        buffers = self._forward(batch, training=True)
        stream = runtime.stream()
        frame_tiles = meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
        word_tiles = meta[('tiles', runtime.AXIS_WORDS, WORD_TILE)]
        word_grad_tiles = meta[('tiles', runtime.AXIS_WORDS, GRAD_TILE)]
        table, bounds = meta['table'], meta['bounds']
        word_segment = meta['word_segment']
        mode = runtime.REDUCTIONS[config.downsample_method]
        decoder = [f'word_decoder.{2 * i}' for i in range(layers)]
        d = buffers['words']
        logits, dlogit = buffers['logits'], buffers['dlogit']

        # ---- loss (train/core.py:315-353) and backward
        runtime.check(lib.emph_loss_grad(
            logits.data_ptr(), batch.targets.data_ptr(),
            word_segment.data_ptr(), ld_w, plan.total_words,
            runtime.BCE_FORMS[config.loss], self.loss.data_ptr(),
            dlogit.data_ptr(), stream), 'emph_loss_grad')
        dd, dh = buffers['word_grad'], buffers['frame_grad']
        runtime.check(lib.emph_output_layer_backward(
            dlogit.data_ptr(), d[layers].data_ptr(), ld_w,
            self._parameter('output_layer.weight'), word_segment.data_ptr(),
            channels, 3, ld_w, self._gradient('output_layer.weight'),
            self._gradient('output_layer.bias'), dd[0].data_ptr(), ld_w,
            stream), 'emph_output_layer_backward')

        dword = self._backward_stack(
            batch, buffers, decoder, d, dd, ld_w, word_grad_tiles, word_tiles,
            WORD_TILE)
        runtime.check(lib.emph_segment_broadcast(
            dword.data_ptr(), ld_w, bounds.data_ptr(), dh[0].data_ptr(), ld_f,
            channels, table.data_ptr(), frame_tiles.data_ptr(),
            frame_tiles.numel() // runtime.TILE_FIELDS, mode, stream),
            'emph_segment_broadcast')
        self._encoder_backward(batch, buffers)


class EncoderTrainer(_Step):
    """`Trainer` for the models without a word decoder, downsample_location
    'inference' and 'loss' (`check_encoder_supported`); see the module
    docstring.  The same interface: `data.Loader` and `train.evaluate` take
    either.  `logits` is the model in eval mode for both locations
    (`model/core.py:109-138`): encoder, reduce, word-rate output layer, no
    dropout."""

    _check = staticmethod(check_encoder_supported)

    def _buffers(self, plan):
        """The activations and gradients of a step for a packed layout, kept
        between steps (zero at first, so that padding columns stay finite)."""
        frame_tiles = len(plan.tiles(runtime.AXIS_FRAMES, GRAD_TILE))
        parts = int(self.lib.emph_conv_weight_grad_parts(frame_tiles))
        head_parts = int(self.lib.emph_frame_head_parts(frame_tiles))
        key = (plan.ld_frames, plan.ld_words, parts, head_parts, frame_tiles)
        found = self._workspace.get(key)
        if found is None:
            self._workspace.clear()
            channels, layers = self.config.channels, self.config.layers
            zeros = lambda *shape, dtype=torch.float32: torch.zeros(  # noqa: E731
                shape, dtype=dtype, device=self.device)
            slab = channels * 3 * self.config.num_features + channels
            found = {
                'frames': zeros(layers + 1, channels, plan.ld_frames),
                'words': zeros(1, channels, plan.ld_words),
                'frame_grad': zeros(2, channels, plan.ld_frames),
                'word_grad': zeros(1, channels, plan.ld_words),
                'logits': zeros(plan.ld_words),
                'dlogit': zeros(plan.ld_words),
                'frame_logits': zeros(plan.ld_frames),
                'frame_dlogit': zeros(plan.ld_frames),
                'partials': zeros(max(frame_tiles, 1), dtype=torch.float64),
                'slabs': zeros(max(
                    max(parts, 1) * slab,
                    max(head_parts, 1) * (3 * channels + 1)))}
            self._workspace[key] = found
        return found

    def _forward(self, batch, training=False):
        """The forward launches; returns the step's buffers.  In training at
        'inference' (`model/core.py:117-122`) their 'frame_logits' hold the
        packed frame logits [ld_frames]; everywhere else - 'loss', and both
        locations in eval mode, `model/core.py:109-138` - their 'logits' hold
        the packed word logits [ld_words].  `training`: with the dropout
        masks of the step."""
        config, lib, plan, meta = self.config, self.lib, batch.plan, batch.meta
        channels, layers = config.channels, config.layers
        ld_f, ld_w = plan.ld_frames, plan.ld_words
        buffers = self._buffers(plan)
        stream = runtime.stream()
        h = buffers['frames']
        self._encoder_forward(batch, h, training and self.dropout > 0.)
        if training and config.downsample_location == 'inference':
            tiles = meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
            runtime.check(lib.emph_frame_head(
                h[layers].data_ptr(), ld_f,
                self._parameter('output_layer.weight'),
                self._parameter('output_layer.bias'), channels, 3,
                tiles.data_ptr(), tiles.numel() // runtime.TILE_FIELDS,
                buffers['frame_logits'].data_ptr(), stream), 'emph_frame_head')
            return buffers
        table, word_segment = meta['table'], meta['word_segment']
        d = buffers['words']
        runtime.check(lib.emph_segment_reduce(
            h[layers].data_ptr(), ld_f, meta['bounds'].data_ptr(),
            d[0].data_ptr(), ld_w, channels, table.data_ptr(),
            word_segment.data_ptr(), ld_w,
            runtime.REDUCTIONS[config.downsample_method], stream),
            'emph_segment_reduce')
        runtime.check(lib.emph_output_layer(
            d[0].data_ptr(), ld_w, self._parameter('output_layer.weight'),
            self._parameter('output_layer.bias'), channels, 3,
            table.data_ptr(), word_segment.data_ptr(), ld_w,
            runtime.AXIS_WORDS, 0, buffers['logits'].data_ptr(), None, stream),
            'emph_output_layer')
        return buffers

    def _forward_backward(self, batch):
        config, lib, plan, meta = self.config, self.lib, batch.plan, batch.meta
        channels, layers = config.channels, config.layers
        ld_f, ld_w = plan.ld_frames, plan.ld_words
        frame_tiles = meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
        n_tiles = frame_tiles.numel() // runtime.TILE_FIELDS
        table, bounds = meta['table'], meta['bounds']
        word_segment = meta['word_segment']
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
                bounds.data_ptr(), ld_w, table.data_ptr(),
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
            d, dd = buffers['words'], buffers['word_grad']
            logits, dlogit = buffers['logits'], buffers['dlogit']
            runtime.check(lib.emph_loss_grad(
                logits.data_ptr(), batch.targets.data_ptr(),
                word_segment.data_ptr(), ld_w, plan.total_words,
                runtime.BCE_FORMS[config.loss], self.loss.data_ptr(),
                dlogit.data_ptr(), stream), 'emph_loss_grad')
            runtime.check(lib.emph_output_layer_backward(
                dlogit.data_ptr(), d[0].data_ptr(), ld_w,
                self._parameter('output_layer.weight'),
                word_segment.data_ptr(), channels, 3, ld_w,
                self._gradient('output_layer.weight'),
                self._gradient('output_layer.bias'), dd[0].data_ptr(), ld_w,
                stream), 'emph_output_layer_backward')
            runtime.check(lib.emph_segment_reduce_backward(
                dd[0].data_ptr(), ld_w, bounds.data_ptr(),
                h[layers].data_ptr(), ld_f, d[0].data_ptr(), dh[0].data_ptr(),
                ld_f, channels, table.data_ptr(), frame_tiles.data_ptr(),
                n_tiles, runtime.REDUCTIONS[config.downsample_method], stream),
                'emph_segment_reduce_backward')
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
        tile = (runtime.AXIS_FRAMES, FRAME_TILE)
        word_host, word_offsets = plan.pack_metadata(list(dict.fromkeys(
            [(runtime.AXIS_WORDS, WORD_TILE), (runtime.AXIS_WORDS, GRAD_TILE)])))
        piece_host, piece_offsets = pieces.plan.pack_metadata(
            list(dict.fromkeys([tile, (runtime.AXIS_FRAMES, GRAD_TILE)])),
            spans=self.precision == 'bf16x3')
        extras = [('gather', pieces.gather.view(np.int32).ravel()),
                  ('piece_bounds', pieces.bounds.ravel()),
                  ('word_piece', pieces.word_piece),
                  ('piece_column', pieces.piece_column)]
        # (every part starts on a 16-byte boundary, the int64 tables included)
        parts, cursor, extra_offsets = [word_host, piece_host], \
            word_host.size + piece_host.size, {}
        assert word_host.size % 4 == 0 and piece_host.size % 4 == 0
        for name, array in extras:
            extra_offsets[name] = (cursor, array.size)
            padded = np.zeros(-(-max(array.size, 1) // 4) * 4, dtype=np.int32)
            padded[:array.size] = array
            parts.append(padded)
            cursor += padded.size
        host = np.concatenate(parts)
        with torch.cuda.device(self.device):
            device_meta = torch.from_numpy(host).to(self.device)
        meta = {name: device_meta[start:start + size]
                for name, (start, size) in word_offsets.items()}
        piece_meta = {
            name: device_meta[word_host.size + start:][:size]
            for name, (start, size) in piece_offsets.items()}
        piece_meta.update(
            (name, device_meta[start:start + size])
            for name, (start, size) in extra_offsets.items())
        piece_meta['plan'] = pieces.plan
        meta['pieces'] = piece_meta
        meta['_buffer'] = device_meta
        return meta

    def _batch(self, arguments):
        if len(arguments) == 1 and isinstance(arguments[0], Batch):
            pieces = arguments[0].meta.get('pieces')
            if pieces is None:
                raise ValueError(
                    'the batch carries no piece tables: prepare it with this '
                    "trainer (downsample_location='input')")
            if self._split_forward and 'conv_spans' not in pieces:
                raise ValueError(
                    "the batch was prepared by a trainer at precision='f32' "
                    "and carries no span table: prepare it with this "
                    f"trainer (precision={self.precision!r})")
            return arguments[0]
        return self.prepare(*arguments)

    def _buffers(self, plan, piece_plan=None):
        """The activations and gradients of a step, kept between steps (zero
        at first, so that padding columns stay finite): the frame-rate ones on
        the piece layout, the word-rate ones on the batch's own."""
        if piece_plan is None:
            piece_plan = plan.pieces(self.config.downsample_method).plan
        frame_tiles = len(piece_plan.tiles(runtime.AXIS_FRAMES, GRAD_TILE))
        word_tiles = len(plan.tiles(runtime.AXIS_WORDS, GRAD_TILE))
        parts = max(
            int(self.lib.emph_conv_weight_grad_parts(n))
            for n in (frame_tiles, word_tiles))
        key = (piece_plan.ld_frames, plan.ld_words, parts)
        found = self._workspace.get(key)
        if found is None:
            self._workspace.clear()
            channels, layers = self.config.channels, self.config.layers
            zeros = lambda *shape: torch.zeros(  # noqa: E731
                shape, dtype=torch.float32, device=self.device)
            slab = channels * 3 * self.config.num_features + channels
            found = {
                'piece_features': zeros(
                    self.config.num_features, piece_plan.ld_frames),
                'frames': zeros(layers + 1, channels, piece_plan.ld_frames),
                'words': zeros(layers + 1, channels, plan.ld_words),
                'frame_grad': zeros(2, channels, piece_plan.ld_frames),
                'word_grad': zeros(2, channels, plan.ld_words),
                'logits': zeros(plan.ld_words),
                'dlogit': zeros(plan.ld_words),
                'slabs': zeros(max(parts, 1) * slab)}
            self._workspace[key] = found
        return found

    def _forward(self, batch, training=False):
        """The forward launches of a step (`model/core.py:41-87,138`); returns
        the step's buffers, whose 'logits' then hold the packed logits
        [ld_words] and whose 'view' is the batch on the piece layout."""
        config, lib, plan, meta = self.config, self.lib, batch.plan, batch.meta
        channels, layers = config.channels, config.layers
        pieces = meta['pieces']
        piece_plan = pieces['plan']
        ld_f, ld_w, ld_p = plan.ld_frames, plan.ld_words, piece_plan.ld_frames
        buffers = self._buffers(plan, piece_plan)
        stream = runtime.stream()
        word_tiles = meta[('tiles', runtime.AXIS_WORDS, WORD_TILE)]
        table, word_segment = meta['table'], meta['word_segment']
        decoder = [f'word_decoder.{2 * i}' for i in range(layers)]

        gathered = buffers['piece_features']
        runtime.check(lib.emph_gather_columns(
            batch.features.data_ptr(), ld_f, gathered.data_ptr(), ld_p,
            config.num_features, pieces['gather'].data_ptr(), len(piece_plan),
            stream), 'emph_gather_columns')
        view = buffers['view'] = Batch(piece_plan, pieces, gathered, None)
        h, d = buffers['frames'], buffers['words']
        self._encoder_forward(view, h, False)
        runtime.check(lib.emph_segment_reduce(
            h[layers].data_ptr(), ld_p, pieces['piece_bounds'].data_ptr(),
            d[0].data_ptr(), ld_w, channels, pieces['table'].data_ptr(),
            pieces['word_piece'].data_ptr(), ld_w,
            runtime.REDUCTIONS[config.downsample_method], stream),
            'emph_segment_reduce')
        for i, name in enumerate(decoder):
            self._conv(self._forward_packs[name],
                       self._parameter(f'{name}.bias'), d[i], d[i + 1], ld_w,
                       channels, 'relu', word_tiles, WORD_TILE)
        runtime.check(lib.emph_output_layer(
            d[layers].data_ptr(), ld_w, self._parameter('output_layer.weight'),
            self._parameter('output_layer.bias'), channels, 3,
            table.data_ptr(), word_segment.data_ptr(), ld_w,
            runtime.AXIS_WORDS, 0, buffers['logits'].data_ptr(), None, stream),
            'emph_output_layer')
        return buffers

    def _forward_backward(self, batch):
        config, lib, plan, meta = self.config, self.lib, batch.plan, batch.meta
        channels, layers = config.channels, config.layers
        ld_w = plan.ld_words
        buffers = self._forward(batch, training=True)
        view = buffers['view']
        ld_p = view.plan.ld_frames
        stream = runtime.stream()
        piece_tiles = view.meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
        word_tiles = meta[('tiles', runtime.AXIS_WORDS, WORD_TILE)]
        word_grad_tiles = meta[('tiles', runtime.AXIS_WORDS, GRAD_TILE)]
        word_segment = meta['word_segment']
        decoder = [f'word_decoder.{2 * i}' for i in range(layers)]
        h, d = buffers['frames'], buffers['words']
        logits, dlogit = buffers['logits'], buffers['dlogit']

        # ---- loss (train/core.py:315-353) and the word-rate backward
        runtime.check(lib.emph_loss_grad(
            logits.data_ptr(), batch.targets.data_ptr(),
            word_segment.data_ptr(), ld_w, plan.total_words,
            runtime.BCE_FORMS[config.loss], self.loss.data_ptr(),
            dlogit.data_ptr(), stream), 'emph_loss_grad')
        dd, dh = buffers['word_grad'], buffers['frame_grad']
        runtime.check(lib.emph_output_layer_backward(
            dlogit.data_ptr(), d[layers].data_ptr(), ld_w,
            self._parameter('output_layer.weight'), word_segment.data_ptr(),
            channels, 3, ld_w, self._gradient('output_layer.weight'),
            self._gradient('output_layer.bias'), dd[0].data_ptr(), ld_w,
            stream), 'emph_output_layer_backward')
        dword = self._backward_stack(
            batch, buffers, decoder, d, dd, ld_w, word_grad_tiles, word_tiles,
            WORD_TILE)
        # ---- the pooled words back to the columns of their pieces
        runtime.check(lib.emph_piece_pool_backward(
            dword.data_ptr(), ld_w, view.meta['gather'].data_ptr(),
            view.meta['piece_column'].data_ptr(), len(view.plan),
            h[layers].data_ptr(), ld_p, d[0].data_ptr(), dh[0].data_ptr(),
            ld_p, channels, piece_tiles.data_ptr(),
            piece_tiles.numel() // runtime.TILE_FIELDS,
            runtime.REDUCTIONS[config.downsample_method], stream),
            'emph_piece_pool_backward')
        self._encoder_backward(view, buffers)


class GridTrainer(_Step):
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

    def __init__(self, config=None, checkpoint=None, gpu=None, lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, seed=0, precision='f32'):
        check_grid_precision(precision)
        super().__init__(config, checkpoint, gpu, lr, betas, eps, seed,
                         precision)
        self._keeps_pre = self.config.activation in ('gelu', 'silu')

    def _layer_shape(self, name):
        """(c_in, kernel size) of conv layer `name`."""
        _, shape = self.offsets[f'{name}.weight']
        return shape[1], shape[2]

    def _buffers(self, plan):
        """The activations and gradients of a step for a packed layout, kept
        between steps (zero at first, so that padding columns stay finite)."""
        config = self.config
        frame_tiles = len(plan.tiles(runtime.AXIS_FRAMES, GRAD_TILE))
        word_tiles = len(plan.tiles(runtime.AXIS_WORDS, GRAD_TILE))
        channels, layers = config.channels, config.layers
        shapes = [(config.num_features, config.encoder_kernel_size, frame_tiles)]
        if layers:
            shapes += [(channels, config.encoder_kernel_size, frame_tiles),
                       (channels, config.decoder_kernel_size, word_tiles)]
        workspace = max(
            int(self.lib.emph_conv_weight_grad_any_workspace(
                c_in, channels, kernel_size, tiles))
            for c_in, kernel_size, tiles in shapes)
        key = (plan.ld_frames, plan.ld_words, workspace)
        found = self._workspace.get(key)
        if found is None:
            self._workspace.clear()
            zeros = lambda *shape: torch.zeros(  # noqa: E731
                shape, dtype=torch.float32, device=self.device)
            found = {
                'frames': zeros(layers + 1, channels, plan.ld_frames),
                'words': zeros(layers + 1, channels, plan.ld_words),
                'frame_grad': zeros(2, channels, plan.ld_frames),
                'word_grad': zeros(2, channels, plan.ld_words),
                'logits': zeros(plan.ld_words),
                'dlogit': zeros(plan.ld_words),
                'slabs': zeros(max(workspace, 1))}
            if self._keeps_pre:
                found['pre_frames'] = zeros(layers, channels, plan.ld_frames)
                found['pre_words'] = zeros(layers, channels, plan.ld_words)
            self._workspace[key] = found
        return found

    def _grid_conv(self, pack, bias, x, y, ld, c_in, kernel_size, activation,
                   tiles, tile):
        runtime.check(self.lib.emph_conv1d(
            x.data_ptr(), ld, y.data_ptr(), ld,
            self.packs.data_ptr() + 4 * pack[0], bias, c_in,
            self.config.channels, kernel_size,
            runtime.ACTIVATIONS[activation], tiles.data_ptr(),
            tiles.numel() // runtime.TILE_FIELDS, tile, 0, runtime.stream()),
            'emph_conv1d')

    def _forward_stack(self, names, outputs, pre, ld, tiles, tile, training):
        """A conv stack (`model/layers/convolution.py:22-37`): outputs[i + 1]
        = dropout(act(conv(outputs[i]))), every output kept, and the
        pre-activation too where the activation's derivative reads it."""
        activation = self.config.activation
        drop = training and self.dropout > 0.
        for i, name in enumerate(names):
            c_in, kernel_size = self._layer_shape(name)
            bias = self._parameter(f'{name}.bias')
            pack = self._forward_packs[name]
            if training and self._keeps_pre:
                self._grid_conv(pack, bias, outputs[i], pre[i], ld, c_in,
                                kernel_size, None, tiles, tile)
                runtime.check(self.lib.emph_activation_dropout(
                    pre[i].data_ptr(), outputs[i + 1].data_ptr(),
                    pre[i].numel(), runtime.ACTIVATIONS[activation],
                    self.dropout if drop else 0., self.seed & (1 << 64) - 1,
                    dropout_module.stream_of(self.config, name), self.steps,
                    runtime.stream()), 'emph_activation_dropout')
                continue
            self._grid_conv(pack, bias, outputs[i], outputs[i + 1], ld, c_in,
                            kernel_size, activation, tiles, tile)
            if drop:
                self._dropout(name, outputs[i + 1])

    def _forward(self, batch, training=False):
        """The forward launches of a step; returns the step's buffers, whose
        'logits' then hold the packed logits [ld_words].  `training`: the
        train-mode forward, which keeps what the backward reads and applies
        the dropout masks of the step; without it the eval model, whose GELU
        and SiLU run in the convolution's epilogue (the same function, the
        same bits)."""
        config, lib, plan, meta = self.config, self.lib, batch.plan, batch.meta
        channels, layers = config.channels, config.layers
        ld_f, ld_w = plan.ld_frames, plan.ld_words
        buffers = self._buffers(plan)
        stream = runtime.stream()
        frame_tiles = meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
        word_tiles = meta[('tiles', runtime.AXIS_WORDS, WORD_TILE)]
        table, word_segment = meta['table'], meta['word_segment']
        h, d = buffers['frames'], buffers['words']

        self._grid_conv(
            self._forward_packs['input_layer'],
            self._parameter('input_layer.bias'), batch.features, h[0], ld_f,
            config.num_features, config.encoder_kernel_size, None,
            frame_tiles, FRAME_TILE)
        self._forward_stack(
            [f'frame_encoder.{2 * i}' for i in range(layers)], h,
            buffers.get('pre_frames'), ld_f, frame_tiles, FRAME_TILE, training)
        runtime.check(lib.emph_segment_reduce(
            h[layers].data_ptr(), ld_f, meta['bounds'].data_ptr(),
            d[0].data_ptr(), ld_w, channels, table.data_ptr(),
            word_segment.data_ptr(), ld_w,
            runtime.REDUCTIONS[config.downsample_method], stream),
            'emph_segment_reduce')
        self._forward_stack(
            [f'word_decoder.{2 * i}' for i in range(layers)], d,
            buffers.get('pre_words'), ld_w, word_tiles, WORD_TILE, training)
        runtime.check(lib.emph_output_layer(
            d[layers].data_ptr(), ld_w, self._parameter('output_layer.weight'),
            self._parameter('output_layer.bias'), channels,
            config.decoder_kernel_size, table.data_ptr(),
            word_segment.data_ptr(), ld_w, runtime.AXIS_WORDS, 0,
            buffers['logits'].data_ptr(), None, stream), 'emph_output_layer')
        return buffers

    def _grid_weight_grad(self, dy, x, ld, name, tiles, buffers):
        c_in, kernel_size = self._layer_shape(name)
        runtime.check(self.lib.emph_conv_weight_grad_any(
            dy.data_ptr(), ld, x.data_ptr(), ld, c_in, self.config.channels,
            kernel_size, tiles.data_ptr(),
            tiles.numel() // runtime.TILE_FIELDS, GRAD_TILE,
            buffers['slabs'].data_ptr(), self._gradient(f'{name}.weight'),
            self._gradient(f'{name}.bias'), runtime.stream()),
            'emph_conv_weight_grad_any')

    def _grid_backward_stack(self, buffers, names, outputs, pre, gradient, ld,
                             grad_tiles, tiles, tile):
        """Backward of a conv stack, from the gradient of the last output
        (gradient[0]) down to the gradient of outputs[0]; returns the buffer
        that holds it."""
        lib, config, stream = self.lib, self.config, runtime.stream()
        activation = runtime.ACTIVATIONS[config.activation]
        current = 0
        for i in range(len(names) - 1, -1, -1):
            name = names[i]
            dy = gradient[current]
            source = pre[i] if self._keeps_pre else outputs[i + 1]
            if self.dropout > 0.:
                runtime.check(lib.emph_activation_dropout_gradient(
                    source.data_ptr(), dy.data_ptr(), dy.numel(), activation,
                    self.dropout, self.seed & (1 << 64) - 1,
                    dropout_module.stream_of(config, name), self.steps,
                    stream), 'emph_activation_dropout_gradient')
            else:
                runtime.check(lib.emph_activation_gradient(
                    source.data_ptr(), dy.data_ptr(), dy.numel(), activation,
                    stream), 'emph_activation_gradient')
            self._grid_weight_grad(dy, outputs[i], ld, name, grad_tiles,
                                   buffers)
            _, kernel_size = self._layer_shape(name)
            self._grid_conv(self._backward_packs[name], None, dy,
                            gradient[1 - current], ld, config.channels,
                            kernel_size, None, tiles, tile)
            current = 1 - current
        return gradient[current]

    def _forward_backward(self, batch):
        config, lib, plan, meta = self.config, self.lib, batch.plan, batch.meta
        channels, layers = config.channels, config.layers
        ld_f, ld_w = plan.ld_frames, plan.ld_words
        buffers = self._forward(batch, training=True)
        stream = runtime.stream()
        frame_tiles = meta[('tiles', runtime.AXIS_FRAMES, FRAME_TILE)]
        word_tiles = meta[('tiles', runtime.AXIS_WORDS, WORD_TILE)]
        word_grad_tiles = meta[('tiles', runtime.AXIS_WORDS, GRAD_TILE)]
        table, bounds = meta['table'], meta['bounds']
        word_segment = meta['word_segment']
        h, d = buffers['frames'], buffers['words']
        dh, dd = buffers['frame_grad'], buffers['word_grad']
        logits, dlogit = buffers['logits'], buffers['dlogit']

        # ---- loss (train/core.py:315-353) and the word-rate backward
        runtime.check(lib.emph_loss_grad(
            logits.data_ptr(), batch.targets.data_ptr(),
            word_segment.data_ptr(), ld_w, plan.total_words,
            runtime.BCE_FORMS[config.loss], self.loss.data_ptr(),
            dlogit.data_ptr(), stream), 'emph_loss_grad')
        runtime.check(lib.emph_output_layer_backward_any(
            dlogit.data_ptr(), d[layers].data_ptr(), ld_w,
            self._parameter('output_layer.weight'), word_segment.data_ptr(),
            channels, config.decoder_kernel_size, ld_w,
            self._gradient('output_layer.weight'),
            self._gradient('output_layer.bias'), dd[0].data_ptr(), ld_w,
            stream), 'emph_output_layer_backward_any')
        dword = self._grid_backward_stack(
            buffers, [f'word_decoder.{2 * i}' for i in range(layers)], d,
            buffers.get('pre_words'), dd, ld_w, word_grad_tiles, word_tiles,
            WORD_TILE)
        # ---- the reduce (max reads the encoder's output and the pooled
        # words, both kept), the frame encoder and the input layer
        runtime.check(lib.emph_segment_reduce_backward(
            dword.data_ptr(), ld_w, bounds.data_ptr(), h[layers].data_ptr(),
            ld_f, d[0].data_ptr(), dh[0].data_ptr(), ld_f, channels,
            table.data_ptr(), frame_tiles.data_ptr(),
            frame_tiles.numel() // runtime.TILE_FIELDS,
            runtime.REDUCTIONS[config.downsample_method], stream),
            'emph_segment_reduce_backward')
        dinput = self._grid_backward_stack(
            buffers, [f'frame_encoder.{2 * i}' for i in range(layers)], h,
            buffers.get('pre_frames'), dh, ld_f, frame_tiles, frame_tiles,
            FRAME_TILE)
        self._grid_weight_grad(dinput, batch.features, ld_f, 'input_layer',
                               frame_tiles, buffers)


def _select(config, precision):
    """The class of the step that trains `config`, every check made and
    nothing constructed: the specialised step of the configuration's location
    (what `trainer_for` builds) first, `GridTrainer` where that refuses and
    `check_grid_supported` passes, otherwise the specialised step's refusal."""
    location = config.downsample_location
    if location == 'input':
        check, name = check_pieces_supported, 'PieceTrainer'
    elif location in ('inference', 'loss'):
        check, name = check_encoder_supported, 'EncoderTrainer'
    else:
        check, name = check_supported, 'Trainer'
    try:
        check(config)
    except NotImplementedError:
        try:
            check_grid_supported(config)
        except NotImplementedError:
            pass
        else:
            check_grid_precision(precision)
            return globals()['GridTrainer']
        raise
    check_precision(precision)
    return globals()[name]


def select_trainer(config=None, **arguments):
    """The fused step that trains `config`: what `trainer_for` returns where
    a specialised step covers it (so such a configuration keeps that step and
    its bits), a `GridTrainer` where none does and `check_grid_supported`
    passes; otherwise the specialised step's refusal.  Every check comes
    before anything is constructed or a GPU is needed."""
    config = config or api.active_config()
    return _select(config, arguments.get('precision', 'f32'))(
        config, **arguments)


def trainer_for(config=None, **arguments):
    """The step that trains `config` at any downsample_location: a
    `PieceTrainer` at 'input' where `check_pieces_supported` passes,
    `make_trainer(...)` everywhere else; the refusal that names the offending
    field comes first, before a GPU is needed."""
    config = config or api.active_config()
    if config.downsample_location == 'input':
        check_pieces_supported(config)
        check_precision(arguments.get('precision', 'f32'))
        return PieceTrainer(config, **arguments)
    return make_trainer(config, **arguments)


def make_trainer(config=None, **arguments):
    """The step that trains `config`: a `Trainer` where `check_supported`
    passes, an `EncoderTrainer` at downsample_location 'inference' and 'loss'
    where `check_encoder_supported` passes; otherwise the refusal that names
    the offending field, before a GPU is needed."""
    config = config or api.active_config()
    if config.downsample_location in ('inference', 'loss'):
        check_encoder_supported(config)
        return EncoderTrainer(config, **arguments)
    check_supported(config)
    return Trainer(config, **arguments)
