"""The reference's `emphases.Model` under ARCHITECTURE = 'transformer'
(`emphases/model/core.py:11-138`, `model/layers/transformer.py:13-52`) as a
`torch.nn.Module` on the differentiable operator seams: `conv1d_same_act` for
the input and output layers, `encoder_layer` once per layer of a stack,
`segment_reduce` between the frames and the words.  At downsample_location
'intermediate' the word decoder is a second Transformer over the words; at
'loss' there is none.

Every utterance runs alone, as inference runs it: attention stays within an
utterance, and the sinusoidal table (`weights.positional_encoding`) is
gathered by the position inside the utterance.

Dropout.  The reference's `TransformerEncoderLayer` trains with its internal
dropout of 0.1 (attention weights, both residual branches, the feed-forward)
and its `PositionalEncoding` with another 0.1: constants of the architecture.
By default (`reference_dropout=False`) none of them is drawn and `train()`
and `eval()` compute the same function - a deliberate deviation, kept as the
default so that what exists keeps its bits.  With `reference_dropout=True` a
model in training mode draws all five, as specified masks
(`train/dropout.py`: `transformer_stream`, `keep_mask`,
`attention_keep_mask`) of (`seed`, site, `self.steps`), through
`ops.dropout` and `ops.encoder_layer_dropout`; in `eval()` it drops nothing.
`Config.dropout` (the conv stacks' switch) is refused either way.

Precision.  `precision='bf16x3'` routes every layer of both stacks through
`ops.encoder_layer_split`: the attention core of every segment of at least
128 positions (the frame axis, in practice) runs on the bf16 matrix pipe,
forward and backward; shorter segments (the words) and everything else stay
float32.  The default 'f32' calls exactly what it always called.
"""
import collections
import functools

import numpy as np
import torch

from .. import config as cfg
from .. import core as api
from .. import ops  # noqa: F401  (registers torch.ops.emphases_amd)
from .. import weights as weights_module
from . import dropout as spec

CHANNELS, HEADS = 80, 2     # the backward of encoder_layer


LOCATIONS = ('intermediate', 'loss')                    # TransformerModel
ALL_LOCATIONS = ('input', 'intermediate', 'inference', 'loss')


def check_transformer_supported(config, _locations=LOCATIONS):
    """NotImplementedError, naming the field, for a configuration
    `TransformerModel` does not cover (`_locations`: private, what
    `TransformerLocationsModel` admits)."""
    def refuse(field, supported):
        raise NotImplementedError(
            f'TransformerModel supports {field} {supported} only, not '
            f'{field}={getattr(config, field)!r}')
    if config.method != 'neural':
        refuse('method', "'neural'")
    if config.architecture != 'transformer':
        refuse('architecture', "'transformer'")
    if config.downsample_location not in _locations:
        # 'inference' needs `upsample` of the targets; 'input' the key-padding
        # mask over zero-padded word pieces (emph_attention's key_counts),
        # which emph_attention_backward does not take: both are
        # TransformerLocationsModel's
        refuse('downsample_location', "'intermediate' or 'loss'")
    if config.channels != CHANNELS:
        refuse('channels', str(CHANNELS))
    if config.heads != HEADS:
        refuse('heads', str(HEADS))
    if config.dropout is not None:
        refuse('dropout', 'None')
    if config.loss not in ('bce', 'mse'):
        refuse('loss', "'bce' or 'mse'")
    if not config.mel_feature:
        refuse('mel_feature', 'True (80..83 input features)')


def check_reference_dropout(precision, reference_dropout):
    """NotImplementedError for `reference_dropout=True` off precision 'f32':
    the one refusal `TransformerModel` and `TransformerTrainer.check` make."""
    if reference_dropout and precision != 'f32':
        raise NotImplementedError(
            'TransformerModel supports reference_dropout=True at '
            f"precision 'f32' only, not precision={precision!r}: the "
            'masked attention kernels are float32')


_LAYER_ORDER = ('self_attn.in_proj_weight', 'self_attn.in_proj_bias',
                'self_attn.out_proj.weight', 'self_attn.out_proj.bias',
                'linear1.weight', 'linear1.bias', 'linear2.weight',
                'linear2.bias', 'norm1.weight', 'norm1.bias', 'norm2.weight',
                'norm2.bias')


def initial_transformer_state(config, seed=0, _locations=LOCATIONS):
    """Bitwise the parameters of the reference's `emphases.Model()` after
    `torch.manual_seed(seed)`: the torch modules built on the CPU in the
    reference's construction order (`model/core.py:13-37`; a stack is ONE
    `TransformerEncoderLayer` cloned `layers` times, so its layers start
    equal; `PositionalEncoding` draws nothing).  The caller's generator is
    left as it was.  (`_locations`: private, as `check_transformer_supported`
    takes it.)"""
    check_transformer_supported(config, _locations)
    state = collections.OrderedDict()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)

        def conv(name, c_in, c_out, kernel_size):
            module = torch.nn.Conv1d(
                c_in, c_out, kernel_size=kernel_size, padding='same')
            state[f'{name}.weight'] = module.weight.detach().numpy().copy()
            state[f'{name}.bias'] = module.bias.detach().numpy().copy()

        def stack(prefix):
            module = torch.nn.TransformerEncoder(
                torch.nn.TransformerEncoderLayer(
                    config.channels, HEADS, dim_feedforward=config.channels),
                config.layers, enable_nested_tensor=False)
            values = dict(module.named_parameters())
            for i in range(config.layers):
                for name in _LAYER_ORDER:
                    state[f'{prefix}.model.layers.{i}.{name}'] = \
                        values[f'layers.{i}.{name}'].detach().numpy().copy()
        conv('input_layer', config.num_features, config.channels,
             config.encoder_kernel_size)
        stack('frame_encoder')
        if config.has_decoder:
            stack('word_decoder')
        conv('output_layer', config.channels, 1, config.decoder_kernel_size)
    assert list(state) == list(weights_module.parameter_shapes(config))
    return state


class _Parameters(torch.nn.Module):
    """A module that holds `name -> Parameter` (and sub-modules) in order."""

    def __init__(self, **tensors):
        super().__init__()
        for name, value in tensors.items():
            setattr(self, name, torch.nn.Parameter(
                torch.from_numpy(np.array(value, dtype=np.float32))))


class _Layer(torch.nn.Module):
    """The parameters of one `nn.TransformerEncoderLayer`, under its names and
    in the order of `weights.parameter_shapes`."""

    def __init__(self, state, prefix):
        super().__init__()
        self.self_attn = _Parameters(
            in_proj_weight=state[prefix + 'self_attn.in_proj_weight'],
            in_proj_bias=state[prefix + 'self_attn.in_proj_bias'])
        self.self_attn.out_proj = _Parameters(
            weight=state[prefix + 'self_attn.out_proj.weight'],
            bias=state[prefix + 'self_attn.out_proj.bias'])
        for name in ('linear1', 'linear2', 'norm1', 'norm2'):
            setattr(self, name, _Parameters(
                weight=state[f'{prefix}{name}.weight'],
                bias=state[f'{prefix}{name}.bias']))

    def forward(self, x, cu, dropout=None, precision='f32', key_counts=None):
        """`dropout` = (seed, stream_base, step): the layer in training mode
        under the reference's dropout.  `precision` other than 'f32': the
        plain layer through `encoder_layer_split`.  `key_counts`: the layer
        behind the key-padding mask, `encoder_layer_padded` (f32, no
        dropout)."""
        attention = self.self_attn
        tensors = (
            attention.in_proj_weight, attention.in_proj_bias,
            attention.out_proj.weight, attention.out_proj.bias,
            self.norm1.weight, self.norm1.bias, self.linear1.weight,
            self.linear1.bias, self.linear2.weight, self.linear2.bias,
            self.norm2.weight, self.norm2.bias)
        if key_counts is not None:
            return torch.ops.emphases_amd.encoder_layer_padded(
                x, *tensors, cu, key_counts, HEADS)
        if precision != 'f32':
            return torch.ops.emphases_amd.encoder_layer_split(
                x, *tensors, cu, HEADS, precision)
        if dropout is None:
            return torch.ops.emphases_amd.encoder_layer(x, *tensors, cu, HEADS)
        seed, stream_base, step = dropout
        return torch.ops.emphases_amd.encoder_layer_dropout(
            x, *tensors, cu, HEADS, spec.TRANSFORMER_LAYER_DROPOUT, seed,
            stream_base, step)


@functools.lru_cache(maxsize=16)
def _positions(key, device='cpu'):
    counts = np.diff(np.frombuffer(key, dtype=np.int64))
    if counts.size and int(counts.max()) > cfg.MAX_POSITIONS:
        # transformer.py:40,51-52: the encoding table has 5000 rows
        raise ValueError(
            f'a segment of {int(counts.max())} positions exceeds the '
            f'{cfg.MAX_POSITIONS}-entry positional encoding')
    if not counts.size:
        return torch.zeros(0, dtype=torch.int64, device=device)
    return torch.from_numpy(np.concatenate(
        [np.arange(count, dtype=np.int64) for count in counts])).to(device)


class _Transformer(torch.nn.Module):
    """`Transformer` (`transformer.py:13-30`): x + encoding[position in the
    segment], then the layers (`model.layers.<i>`)."""

    def __init__(self, config, prefix, state, precision='f32'):
        super().__init__()
        self.precision = precision
        self.streams = (
            spec.transformer_stream(config, prefix),
            [spec.transformer_stream(config, prefix, i, 'attention')
             for i in range(config.layers)])
        self.model = torch.nn.Module()
        self.model.layers = torch.nn.ModuleList(
            _Layer(state, f'{prefix}.model.layers.{i}.')
            for i in range(config.layers))
        self.register_buffer('encoding', torch.from_numpy(
            weights_module.positional_encoding(
                cfg.MAX_POSITIONS, config.channels)).t().contiguous(),
            persistent=False)

    def forward(self, x, cu, dropout=None, key_counts=None):
        """`dropout` = (seed, step): training under the reference's dropout
        (`PositionalEncoding`'s after the sum, then every layer's four).
        `key_counts` (int64 host tensor, one per segment): the segments end
        in padding that is no key (`encoder_layer_padded`)."""
        host = cu.detach().cpu().to(torch.int64).numpy()
        index = _positions(np.ascontiguousarray(host).tobytes(), str(x.device))
        x = x + self.encoding.index_select(1, index)
        if key_counts is not None:
            for layer in self.model.layers:
                x = layer(x, cu, key_counts=key_counts)
            return x
        if dropout is None:
            for layer in self.model.layers:
                x = layer(x, cu, precision=self.precision)
            return x
        seed, step = dropout
        position, layers = self.streams
        x = torch.ops.emphases_amd.dropout(
            x, spec.TRANSFORMER_POSITION_DROPOUT, seed, position, step)
        for layer, stream_base in zip(self.model.layers, layers):
            x = layer(x, cu, (seed, stream_base, step))
        return x


class TransformerModel(torch.nn.Module):
    """`TransformerModel(config, checkpoint=None, seed=0,
    reference_dropout=False, precision='f32')`; `forward(features
    [C_in, sum T], cu_frames, bounds [2, sum W], cu_words) -> logits [sum W]`,
    the utterances back to back (`cu_*`: N + 1 prefix sums, on the host), as
    `TorchModel`; `train.loss_fn` serves unchanged.

    downsample_location 'intermediate' or 'loss', every downsample_method;
    80 channels, 2 heads.  `reference_dropout=True` trains with the
    reference's five dropouts (module docstring): the masks are a function
    of `seed`, the site and `self.steps`, a plain int (0 at first; not a
    parameter, not in `state_dict()`) that the caller sets or advances once
    per optimizer update, so the same batch at the same `steps` gives the
    same bits.  In `eval()`, and with the default False, nothing is dropped.
    `precision='bf16x3'` (module docstring; `train.check_precision` names the
    others) trains and infers with the long segments' attention on the bf16
    matrix pipe; `train()` and `eval()` compute the same function, the
    checkpoints do not record it and are interchangeable with 'f32'; with
    `reference_dropout=True` it raises NotImplementedError (the masked
    kernels are float32).
    The parameters carry
    the reference's names and order (`weights.parameter_shapes`):
    `state_dict()` is read by `weights.load` and by every inference entry
    point's `checkpoint=`.  Without a checkpoint they are bitwise
    `initial_transformer_state(config, seed)`.  A segment longer than the
    5000-entry positional encoding raises ValueError."""

    _locations = LOCATIONS

    def __init__(self, config=None, checkpoint=None, seed=0,
                 reference_dropout=False, precision='f32'):
        super().__init__()
        from .core import check_precision
        self.config = config = config or api.active_config()
        check_transformer_supported(config, self._locations)
        self.precision = check_precision(precision)
        self.reference_dropout = bool(reference_dropout)
        check_reference_dropout(self.precision, self.reference_dropout)
        self.seed, self.steps = int(seed), 0
        if checkpoint is None:
            state = initial_transformer_state(config, seed, self._locations)
        else:
            state = weights_module.load(checkpoint, config)
        self.input_layer = _Parameters(
            weight=state['input_layer.weight'], bias=state['input_layer.bias'])
        self.frame_encoder = _Transformer(
            config, 'frame_encoder', state, self.precision)
        if config.has_decoder:
            self.word_decoder = _Transformer(
                config, 'word_decoder', state, self.precision)
        self.output_layer = _Parameters(
            weight=state['output_layer.weight'],
            bias=state['output_layer.bias'])

    def forward(self, features, cu_frames, bounds, cu_words):
        conv = torch.ops.emphases_amd.conv1d_same_act
        x = conv(features, self.input_layer.weight, self.input_layer.bias,
                 cu_frames, 'none')
        dropout = None
        if self.reference_dropout and self.training:
            dropout = (self.seed, int(self.steps))
        x = self.frame_encoder(x, cu_frames, dropout)
        x = torch.ops.emphases_amd.segment_reduce(
            x, bounds, cu_frames, cu_words, self.config.downsample_method)
        if self.config.has_decoder:
            x = self.word_decoder(x, cu_words, dropout)
        x = conv(x, self.output_layer.weight, self.output_layer.bias,
                 cu_words, 'none')
        return x[0]


def check_locations_supported(config, precision='f32',
                              reference_dropout=False):
    """Every refusal of `TransformerLocationsModel`, by field name: what
    `TransformerModel` refuses but for the location, and at 'input' - where
    the layers are `encoder_layer_padded` - `precision` other than 'f32' and
    `reference_dropout=True` (the bf16 and the masked attention kernels take
    no key-padding mask)."""
    check_transformer_supported(config, ALL_LOCATIONS)
    check_reference_dropout(precision, reference_dropout)
    if config.downsample_location == 'input':
        if precision != 'f32':
            raise NotImplementedError(
                "TransformerLocationsModel supports precision 'f32' only at "
                f"downsample_location 'input', not precision={precision!r}")
        if reference_dropout:
            raise NotImplementedError(
                'TransformerLocationsModel supports reference_dropout=False '
                "only at downsample_location 'input', not "
                'reference_dropout=True')


@functools.lru_cache(maxsize=16)
def _piece_tables(cu_frames, bounds, cu_words, center, device='cpu'):
    """The piece layout of a batch as index tables (the arguments: the bytes
    of the int64 host arrays).  Every word is a piece padded to the longest
    word of its UTTERANCE, as `batch.Pieces` builds it: (gather index into
    the feature columns with one zero column appended [sum padded] on
    `device`, cu_pieces, key_counts, the pooling bounds [2, P], the prefix
    sums of one word per piece) - the last four on the host."""
    cu_frames = np.frombuffer(cu_frames, dtype=np.int64)
    cu_words = np.frombuffer(cu_words, dtype=np.int64)
    bounds = np.frombuffer(bounds, dtype=np.int64).reshape(2, -1)
    words = np.diff(cu_words)
    count = int(bounds.shape[1])
    if int(cu_words[-1]) != count:
        raise ValueError('cu_words does not cover the columns of bounds')
    item = np.repeat(np.arange(words.size), words)
    starts, ends = bounds[0], bounds[1]
    lengths = ends - starts
    frames = np.diff(cu_frames)
    if count and (np.any(starts < 0) or np.any(ends > frames[item]) or
                  np.any(lengths < 1)):
        raise ValueError(
            "downsample_location 'input' takes words of at least one frame "
            'inside their utterance')
    longest = np.zeros(words.size, dtype=np.int64)
    np.maximum.at(longest, item, lengths)
    padded = longest[item]
    cu_pieces = np.concatenate([[0], np.cumsum(padded)]).astype(np.int64)
    total = int(cu_pieces[-1])
    piece = np.repeat(np.arange(count), padded)
    position = np.arange(total, dtype=np.int64) - cu_pieces[:-1][piece]
    real = position < lengths[piece]
    # (a padded position reads the zero column behind the features)
    index = np.where(real, cu_frames[:-1][item][piece] + starts[piece] +
                     position, int(cu_frames[-1]))
    end = lengths if center else padded
    pool = np.stack([np.zeros(count, dtype=np.int64), end])
    return (torch.from_numpy(index.astype(np.int64)).to(device),
            torch.from_numpy(cu_pieces), torch.from_numpy(lengths.copy()),
            torch.from_numpy(np.ascontiguousarray(pool)),
            torch.arange(count + 1, dtype=torch.int64))


class TransformerLocationsModel(TransformerModel):
    """`TransformerModel` at all four DOWNSAMPLE_LOCATIONs; the same
    constructor, parameters, checkpoints and `forward` arguments.  At
    'intermediate' and 'loss' it IS the parent, bit for bit.

    'input' (`model/core.py:41-87`): every word is cut out of the features
    into a piece of its own, zero-padded to the longest word of its utterance
    (the project's piece layout, `batch.Pieces`); `input_layer` runs over the
    pieces, the positional encoding counts from each piece's start, the frame
    encoder's layers are `encoder_layer_padded` with the words' real lengths
    as `key_counts`, and `segment_reduce` pools every piece over its padded
    axis ('center' takes length // 2, 'average' divides by the padded
    length); then the word decoder and `output_layer` over the words.
    'f32' without `reference_dropout` only.

    'inference' (`model/core.py:117-130`): in `train()` the logits are at
    FRAME rate, [sum T], `output_layer` on the frame embeddings (the loss
    takes upsampled targets); in `eval()` the embeddings are reduced first
    and the logits are at word rate, [sum W].  The layers are the parent's:
    'f32', 'bf16x3' and `reference_dropout=True`."""

    _locations = ALL_LOCATIONS

    def __init__(self, config=None, checkpoint=None, seed=0,
                 reference_dropout=False, precision='f32'):
        check_locations_supported(
            config or api.active_config(), precision, reference_dropout)
        super().__init__(config, checkpoint, seed, reference_dropout,
                         precision)

    def forward(self, features, cu_frames, bounds, cu_words):
        location = self.config.downsample_location
        if location in LOCATIONS:
            return super().forward(features, cu_frames, bounds, cu_words)
        conv = torch.ops.emphases_amd.conv1d_same_act
        reduce = torch.ops.emphases_amd.segment_reduce
        method = self.config.downsample_method
        if location == 'input':
            host = [np.ascontiguousarray(
                t.detach().cpu().to(torch.int64).numpy()).tobytes()
                for t in (cu_frames, bounds, cu_words)]
            index, cu_pieces, key_counts, pool, cu_one = _piece_tables(
                *host, method == 'center', str(features.device))
            pieces = torch.cat(
                [features, features.new_zeros(features.shape[0], 1)],
                dim=1).index_select(1, index)
            x = conv(pieces, self.input_layer.weight, self.input_layer.bias,
                     cu_pieces, 'none')
            x = self.frame_encoder(x, cu_pieces, key_counts=key_counts)
            x = reduce(x, pool, cu_pieces, cu_one, method)
            x = self.word_decoder(x, cu_words)
            x = conv(x, self.output_layer.weight, self.output_layer.bias,
                     cu_words, 'none')
            return x[0]
        x = conv(features, self.input_layer.weight, self.input_layer.bias,
                 cu_frames, 'none')
        dropout = None
        if self.reference_dropout and self.training:
            dropout = (self.seed, int(self.steps))
        x = self.frame_encoder(x, cu_frames, dropout)
        cu = cu_frames
        if not self.training:
            x = reduce(x, bounds, cu_frames, cu_words, method)
            cu = cu_words
        x = conv(x, self.output_layer.weight, self.output_layer.bias, cu,
                 'none')
        return x[0]
