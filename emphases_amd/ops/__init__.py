"""The operator seams of SURVEY §8b as `torch.library` custom ops over the C ABI:
`at::Tensor` in, `at::Tensor` out, ragged ("varlen") axes described by `cu_*`
prefix sums, so that a caller of the reference's ATen ops
(the reference's `emphases/model/core.py:93-138`) needs no `ctypes`:

    torch.ops.emphases_amd.logmel(audio_packed, cu_samples)            mels.py:16-109
    torch.ops.emphases_amd.conv1d_same_act(x, w, b, cu_T, act)         convolution.py:25-37
    torch.ops.emphases_amd.segment_reduce(x, bounds, cu_frames, cu_words, mode)
                                                                       core.py:426-469
    torch.ops.emphases_amd.encoder_layer(x, in_w, in_b, out_w, out_b, norm1_w, norm1_b,
                                         ff1_w, ff1_b, ff2_w, ff2_b, norm2_w, norm2_b,
                                         cu_T, heads)                  transformer.py:18-30
    torch.ops.emphases_amd.encoder_layer_dropout(x, <the same twelve>, cu_T, heads,
                                         p, seed, stream_base, step)   the same in .train()
    torch.ops.emphases_amd.encoder_layer_split(x, <the same twelve>, cu_T, heads,
                                         precision)                    the plain layer, its
                                         attention core on the bf16 matrix pipe
    torch.ops.emphases_amd.encoder_layer_padded(x, <the same twelve>, cu_T, key_counts,
                                         heads)                        transformer.py:26-29:
                                         the plain layer behind src_key_padding_mask
    torch.ops.emphases_amd.dropout(x, p, seed, stream, step)           transformer.py:51-52
    torch.ops.emphases_amd.prominence_forward(audio_packed, cu_samples, bounds, cu_words)
                                                                       core.py:295-342

The package: this module holds the nine ops, their fakes and their autograd
registrations; `layout` the prefix sums, the plans, `_Layout` and the plan LRU;
`packs` the launch helper `_call`, `_ByStorage` and everything kept per weight;
`layer` the launchers an op shares with its backward and `_LayerRun`.

Conventions: every segment keeps its OWN zero halo (the
reference's B = 1 semantics); inputs are borrowed, contiguous, on the op's HIP
device; outputs are freshly allocated on the current stream; `cu_*` are int32 /
int64 tensors of N + 1 prefix sums (on the host, or on the device at the price
of a synchronising copy - the table of a batch is built on the host).  The
ops run the library's kernels on the library's packed layout (segments start
16-aligned) and gather the result back into the caller's back-to-back layout;
callers that own the layout use `engine.Engine` directly and skip both copies.
No CPU implementation is registered: on a host tensor the dispatcher raises.

Autograd.  `conv1d_same_act` (gradients of `x`, `weight`, `bias`) and
`segment_reduce` (gradient of `x`) are differentiable once
(`torch.library.register_autograd`; a backward under `create_graph=True`,
the way to a second backward, raises) and carry a
`register_fake` shape rule; so is `encoder_layer` (gradients of `x` and of
all twelve parameters; 80 channels in 2 heads, its dropouts the identity:
see its docstring; `encoder_layer_dropout` is the same layer in training mode
under the reference's four dropouts as specified masks - one body serves
both, `dropout=None` being the plain layer; `encoder_layer_split` is the
plain layer at `precision='bf16x3'`, the third caller of that body: the
attention core of every segment of at least 128 positions on the bf16 matrix
pipe, forward and backward; `encoder_layer_padded` is the plain layer whose
segments end in zero padding that is no key, the fourth caller, walked back
through `emph_attention_backward_keys` - and `dropout` the mask alone) and `logmel` (gradient of a float `audio_packed`: the
waveform end of the chain, so d(prominence)/d(audio) exists on the seams; no
`register_fake` - its shape depends on the values of `cu_samples`);
`prominence_forward` alone stays non-differentiable.  The backward runs on
the library's kernels (`emph_activation_gradient`,
`emph_conv_weight_grad_any`, `emph_conv1d` on the flipped pack,
`emph_segment_reduce_backward`, `emph_attention_backward`,
`emph_add_layernorm_backward`, `emph_logmel_backward`), without atomics: the
same inputs give the same bits.

Two paths of `conv1d_same_act`.  A weight that has never changed since the op
first saw it (inference) takes the kernels it always took, its packs made
once on the host.  A weight whose version has changed since (an optimizer
updates it in place) is packed ON THE DEVICE (`emph_take` through an index
table made once per weight shape, no device-to-host copy) and runs as
direct-form `emph_conv1d` on 64-position tiles, as `train.Trainer` does.  The
two paths differ at float32 rounding (Winograd against direct form).

Two paths of `encoder_layer`, in the same way.  A parameter set of which no
tensor has changed since the op first saw it runs on the layer's fused
inference engine (packs made once on the host; the bits it always gave,
whether or not anything requires grad).  Once a tensor's version has changed,
the layer runs as the unfused sequence of launches that its backward also
recomputes, on weights packed on the device: no `Engine` is rebuilt and
nothing is copied to the host per step.  The two paths differ at float32
rounding (fused chain against separate launches).

One cache rule for whatever is derived from weights (`packs._ByStorage`: the
device packs, the first version seen, the host packs of a convolution, the
one-layer engine): the key is the address, shape, strides and device of every
tensor involved, with the versions; an entry answers only while every storage
it was made from is alive and is the asking tensor's, and keeps none alive.

One plan per batch: the packed layout of a set of `cu_*` (and `bounds`)
values, its device metadata and its device column indices are kept in a small
LRU keyed by the bytes of those arrays and the device, so the layers of a
model and their backwards share one upload.
"""
import functools

import numpy as np
import torch

from .. import config as cfg
from .. import core
from .. import engine as engine_module
from .. import runtime
from .layer import (  # noqa: F401
    LAYER_CHANNELS, LAYER_HEADS, SPLIT_PIECES, _LayerRun, _conv1d,
    _weight_grad)
from .layout import (  # noqa: F401
    DIRECT_TILE, GRAD_TILE, SPLIT_TILE, _Layout, _chunk_plan, _counts, _device_index,
    _frame_plan, _layout, _logmel_plan)
from .packs import (  # noqa: F401
    _ByStorage, _call, _device_pack, _first, _first_versions, _float32, _host_conv,
    _layer_engine, _weight_changes, mark_trained, pack_index_tables)

__all__ = ['logmel', 'conv1d_same_act', 'segment_reduce', 'encoder_layer',
           'encoder_layer_dropout', 'encoder_layer_split',
           'encoder_layer_padded', 'dropout', 'prominence_forward']


@torch.library.custom_op('emphases_amd::logmel', mutates_args=())
def logmel(audio_packed: torch.Tensor, cu_samples: torch.Tensor) -> torch.Tensor:
    """`mels.from_audio` (`mels.py:16-109`) of N chunks back to back: float32
    (or int16 PCM) `[sum S_i]` -> float32 `[80, sum F_i]`, F_i = 1 + (S_i -
    160) // 160 as in the reference (reflect padding of 432 per chunk).

    Backward (once, `emph_logmel_backward`): the gradient of a float
    `audio_packed`; nothing is saved but the inputs - the spectrum is
    recomputed from the audio.  int16 PCM has no gradient (the output does not
    require grad)."""
    index = _device_index(audio_packed)
    plan, columns = _logmel_plan(cu_samples, audio_packed.device)
    engine = core.get_engine(None, index, cfg.DEFAULT)
    with torch.cuda.device(index), engine.lock:
        meta = engine.upload(plan)
        packed = engine.features(audio_packed.contiguous(), plan, meta)
        return packed.index_select(1, columns)


def _activation(activation):
    activation = None if activation in ('none', '') else activation
    if activation is not None and activation not in cfg.ACTIVATIONS:
        raise ValueError(f'Activation {activation} is not defined')
    return activation


def _conv_layout(x, cu_T):
    counts, _ = _counts(cu_T)
    if int(counts.sum()) != x.shape[1]:
        raise ValueError('cu_T does not cover the columns of x')
    return _layout(x.device, counts)


@torch.library.custom_op('emphases_amd::conv1d_same_act', mutates_args=())
def conv1d_same_act(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                    cu_T: torch.Tensor, activation: str) -> torch.Tensor:
    """`Conv1d(C_in, C_out, k, padding='same')` + activation
    (`convolution.py:25-37`) over N segments back to back, each with its own
    zero halo: x `[C_in, sum T_i]`, weight `[C_out, C_in, k]`, bias `[C_out]`
    -> `[C_out, sum T_i]`.  activation: 'none' | 'relu' | 'gelu' | 'silu' |
    'leaky_relu'.  The packed weights are cached per (weight storage,
    version): on the host for a weight that never changed, on the device
    (direct-form `emph_conv1d`) for one that has - see the module docstring.

    Backward (once): the activation gradient is applied to dy in place - from
    the saved output for relu / leaky_relu; for gelu / silu the
    pre-activation is RECOMPUTED by one `emph_conv1d` with no activation;
    dW / db come from `emph_conv_weight_grad_any` for every shape (Conv1d(.,
    80, 3) included: one kernel for the general path, the specialised
    `emph_conv_weight_grad` stays `Trainer`'s); dx is `emph_conv1d` on the
    device pack of W'[ci][co][j] = W[co][ci][k - 1 - j] without bias.  Only
    the gradients `needs_input_grad` asks for are computed."""
    index = _device_index(x)
    activation = _activation(activation)
    layout = _conv_layout(x, cu_T)
    plan = layout.plan
    engine = core.get_engine(None, index, cfg.DEFAULT)
    with torch.cuda.device(index), engine.lock:
        packed = layout.scatter(x, layout.frame_columns, plan.ld_frames)
        out = torch.zeros((weight.shape[0], plan.ld_frames),
                          dtype=torch.float32, device=x.device)
        first = _first(weight)
        if first.version != weight._version:
            c_out, c_in, kernel_size = weight.shape
            _conv1d(packed, out, plan.ld_frames,
                    _device_pack(weight, index, False), _float32(bias), c_in,
                    c_out, kernel_size, activation, layout)
        else:
            layer = _host_conv(first, weight, bias, index)
            tile = 64 if (layer.winograd4 is not None and engine.quad and
                          activation in (None, 'relu')) else \
                32 if layer.winograd is not None else 16
            layout.tiles(tile)
            engine._conv(layer, packed, plan.ld_frames, out, plan.ld_frames,
                         layout.meta, runtime.AXIS_FRAMES, tile, activation)
        return out.index_select(1, layout.frame_columns)


@conv1d_same_act.register_fake
def _conv1d_same_act_fake(x, weight, bias, cu_T, activation):
    return x.new_empty((weight.shape[0], x.shape[1]), dtype=torch.float32)


def _once(name):
    """The backward of `name` runs on HIP kernels that record no graph: asking
    for one (`create_graph=True`, the way to a second backward) raises."""
    if torch.is_grad_enabled():
        raise RuntimeError(
            f'emphases_amd::{name} is differentiable once: its backward '
            'records no graph (create_graph=True / a second backward is not '
            'supported)')


@functools.lru_cache(maxsize=8)
def _backward_table(index):
    """The front-end's table with the window the REFERENCE has: `torch.stft`
    in `mels.py:39-48` is given `torch.hann_window` as torch evaluates it in
    float32, up to 5.5e-4 relative (1.8e-7 absolute) away, at a frame's ends,
    from the exact periodic Hann rounded to float32 that
    `emph_frontend_table_fill` holds.  The forward keeps its table and its
    bits; the backward differentiates the reference's function, so that the
    gradient is the one the reference's autograd gives (after half a second of
    digital silence the two windows' gradients are 3.6e-6 of the largest
    element apart).  The table holds the window halved, an exact operation."""
    engine = core.get_engine(None, index, cfg.DEFAULT)
    table = engine.table.clone()
    window = torch.hann_window(cfg.NUM_FFT, dtype=torch.float32)
    table[:cfg.NUM_FFT] = (0.5 * window).to(table.device)
    return table


def _logmel_setup(ctx, inputs, output):
    audio_packed, cu_samples = inputs
    ctx.save_for_backward(audio_packed, cu_samples)


def _logmel_backward(ctx, grad):
    _once('logmel')
    audio_packed, cu_samples = ctx.saved_tensors
    if not ctx.needs_input_grad[0]:
        return None, None
    index = _device_index(grad)
    plan, columns = _logmel_plan(cu_samples, grad.device)
    engine = core.get_engine(None, index, cfg.DEFAULT)
    with torch.cuda.device(index), engine.lock:
        meta = engine.upload(plan)
        tiles, size = meta[
            ('tiles', runtime.AXIS_FRAMES, engine_module.FRONTEND_BLOCK)]
        n_tiles = size // runtime.TILE_FIELDS
        audio = _float32(audio_packed)
        dmel = _Layout.scatter(grad, columns, plan.ld_frames)
        # (samples outside every chunk - behind the last prefix sum - get 0)
        daudio = torch.zeros_like(audio)
        workspace = torch.empty(
            int(runtime.library().emph_logmel_backward_workspace(n_tiles)),
            dtype=torch.float32, device=audio.device)
        _call('emph_logmel_backward', audio, meta['table'][0], tiles, n_tiles,
              _backward_table(index), engine.mel_start, engine.mel_count,
              engine.mel_offset, engine.mel_values, engine.mel_nnz, dmel,
              plan.ld_frames, 0, workspace, daudio)
    return daudio.to(audio_packed.dtype).reshape(audio_packed.shape), None


logmel.register_autograd(_logmel_backward, setup_context=_logmel_setup)


def _conv_setup(ctx, inputs, output):
    x, weight, bias, cu_T, activation = inputs
    ctx.activation = activation
    # (only relu / leaky_relu read the saved output)
    ctx.save_for_backward(
        x, weight, bias, cu_T,
        output if activation in ('relu', 'leaky_relu') else None)


def _conv_backward(ctx, grad):
    _once('conv1d_same_act')
    x, weight, bias, cu_T, output = ctx.saved_tensors
    need_x, need_weight, need_bias = ctx.needs_input_grad[:3]
    index = _device_index(grad)
    activation = _activation(ctx.activation)
    layout = _conv_layout(x, cu_T)
    ld = layout.plan.ld_frames
    c_out, c_in, kernel_size = weight.shape
    dx = dweight = dbias = None
    with torch.cuda.device(index):
        dy = layout.scatter(grad, layout.frame_columns, ld)
        packed = None
        if need_weight or need_bias or activation in ('gelu', 'silu'):
            packed = layout.scatter(x, layout.frame_columns, ld)
        if activation in ('relu', 'leaky_relu'):
            source = layout.scatter(output, layout.frame_columns, ld)
        elif activation is not None:
            source = torch.zeros_like(dy)
            _conv1d(packed, source, ld, _device_pack(weight, index, False),
                    _float32(bias), c_in, c_out, kernel_size, None, layout)
        if activation is not None:
            _call('emph_activation_gradient', source, dy, dy.numel(),
                  runtime.ACTIVATIONS[activation])
        if need_weight or need_bias:
            dweight = torch.empty((c_out, c_in, kernel_size),
                                  dtype=torch.float32, device=grad.device)
            dbias = torch.empty(c_out, dtype=torch.float32, device=grad.device)
            _weight_grad(dy, packed, ld, c_in, c_out, kernel_size, layout,
                         dweight, dbias)
            dweight = dweight.to(weight.dtype) if need_weight else None
            dbias = dbias.to(bias.dtype) if need_bias else None
        if need_x:
            dpacked = torch.zeros((c_in, ld), dtype=torch.float32,
                                  device=grad.device)
            _conv1d(dy, dpacked, ld, _device_pack(weight, index, True), None,
                    c_out, c_in, kernel_size, None, layout)
            dx = dpacked.index_select(1, layout.frame_columns).to(x.dtype)
    return dx, dweight, dbias, None, None


conv1d_same_act.register_autograd(_conv_backward, setup_context=_conv_setup)


def _reduce_layout(x, bounds, cu_frames, cu_words, mode):
    if mode not in cfg.DOWNSAMPLE_METHODS:
        raise ValueError(f'Interpolation method {mode} is not defined')
    frames, _ = _counts(cu_frames)
    words, _ = _counts(cu_words)
    if len(frames) != len(words):
        raise ValueError('cu_frames and cu_words describe different numbers of segments')
    host_bounds = np.ascontiguousarray(
        bounds.detach().cpu().to(torch.int64).numpy().reshape(2, -1))
    layout = _layout(x.device, frames, words, host_bounds)
    if ('forward', mode) not in layout.checked:
        engine_module.check_bounds(layout.plan, mode)
        layout.checked['forward', mode] = True
    return layout


def check_backward_bounds(plan):
    """ValueError unless the words of every segment are sorted, non-empty and
    do not overlap: what `emph_segment_reduce_backward` needs to give every
    frame one word at the most (the forward accepts any words)."""
    first = 0
    for index, count in enumerate(plan.words):
        starts, ends = plan.segment_bounds[:, first:first + int(count)]
        first += int(count)
        if np.any(ends <= starts):
            raise ValueError(
                f'segment {index}: a word with end <= start has no backward')
        if np.any(starts[1:] < ends[:-1]):
            raise ValueError(
                f'segment {index}: words overlap or are not in order; the '
                'backward of segment_reduce needs sorted, disjoint words')


@torch.library.custom_op('emphases_amd::segment_reduce', mutates_args=())
def segment_reduce(x: torch.Tensor, bounds: torch.Tensor, cu_frames: torch.Tensor,
                   cu_words: torch.Tensor, mode: str) -> torch.Tensor:
    """`emphases.downsample` (`core.py:426-469`): x `[C, sum F_i]`, bounds int
    `[2, sum W_i]` (frames relative to the word's own segment), mode 'sum' |
    'average' | 'max' | 'center' -> `[C, sum W_i]`.  An empty word: 0 (sum),
    NaN (average), as in the reference; 'max' of an empty word raises.

    Backward (once, `emph_segment_reduce_backward`): the gradient of x; it
    raises ValueError on the host if the words of a segment overlap, are out
    of order or include a word with end <= start, all of which the forward
    accepts: the backward finds a frame's word by bisection over the starts,
    and an empty word would hide the word around it."""
    index = _device_index(x)
    layout = _reduce_layout(x, bounds, cu_frames, cu_words, mode)
    plan = layout.plan
    with torch.cuda.device(index):
        packed = layout.scatter(x, layout.frame_columns, plan.ld_frames)
        out = torch.zeros((x.shape[0], plan.ld_words), dtype=torch.float32,
                          device=x.device)
        _call('emph_segment_reduce', packed, plan.ld_frames,
              layout.view('bounds'), out, plan.ld_words, x.shape[0],
              layout.view('table'), layout.view('word_segment'), plan.ld_words,
              runtime.REDUCTIONS[mode])
        return out.index_select(1, layout.word_columns)


@segment_reduce.register_fake
def _segment_reduce_fake(x, bounds, cu_frames, cu_words, mode):
    return x.new_empty((x.shape[0], bounds.shape[1]), dtype=torch.float32)


def _reduce_setup(ctx, inputs, output):
    x, bounds, cu_frames, cu_words, mode = inputs
    ctx.mode = mode
    ctx.save_for_backward(x, bounds, cu_frames, cu_words,
                          output if mode == 'max' else None)


def _reduce_backward(ctx, grad):
    _once('segment_reduce')
    x, bounds, cu_frames, cu_words, output = ctx.saved_tensors
    if not ctx.needs_input_grad[0]:
        return None, None, None, None, None
    index = _device_index(grad)
    mode = ctx.mode
    layout = _reduce_layout(x, bounds, cu_frames, cu_words, mode)
    if 'backward' not in layout.checked:
        check_backward_bounds(layout.plan)
        layout.checked['backward'] = True
    plan = layout.plan
    with torch.cuda.device(index):
        dword = layout.scatter(grad, layout.word_columns, plan.ld_words)
        packed = top = None
        if mode == 'max':
            packed = layout.scatter(x, layout.frame_columns, plan.ld_frames)
            top = layout.scatter(output, layout.word_columns, plan.ld_words)
        dpacked = torch.zeros((x.shape[0], plan.ld_frames), dtype=torch.float32,
                              device=grad.device)
        tiles, n_tiles = layout.tiles(GRAD_TILE)
        _call('emph_segment_reduce_backward', dword, plan.ld_words,
              layout.view('bounds'), packed, plan.ld_frames, top, dpacked,
              plan.ld_frames, x.shape[0], layout.view('table'), tiles, n_tiles,
              runtime.REDUCTIONS[mode])
        dx = dpacked.index_select(1, layout.frame_columns).to(x.dtype)
        if dx.shape[1] < x.shape[1]:      # (columns past the last segment)
            dx = torch.nn.functional.pad(dx, (0, x.shape[1] - dx.shape[1]))
    return dx, None, None, None, None


segment_reduce.register_autograd(_reduce_backward, setup_context=_reduce_setup)


def _check_layer_shape(name, channels, heads):
    if channels != LAYER_CHANNELS:
        raise NotImplementedError(
            f'{name} supports x of {LAYER_CHANNELS} channels only, not '
            f'{channels}')
    if heads != LAYER_HEADS:
        raise NotImplementedError(
            f'{name} supports heads={LAYER_HEADS} only, not heads={heads}')


def _mask_arguments(p, seed, stream, step):
    """(float32 p, seed mod 2^64, stream, step) as the C ABI carries them."""
    p = float(np.float32(p))
    if not 0. <= p < 1.:
        raise ValueError(f'p = {p} (0 <= p < 1)')
    if not (0 <= stream < 1 << 32 and 0 <= step < 1 << 32):
        raise ValueError('stream and step are unsigned 32-bit')
    return p, int(seed) & (1 << 64) - 1, int(stream), int(step)


def _layer_inputs(x, tensors, cu_T):
    """(device index, the twelve tensors as a tuple, the layout of `cu_T`)."""
    index = _device_index(x)
    counts, _ = _counts(cu_T)
    return index, tuple(tensors), _layout(x.device, counts)


def _split_pieces(precision):
    """The `pieces` code of `precision` for `encoder_layer_split`: 'bf16x3'
    alone.  'f32' is `encoder_layer`; the engine's other precisions raise
    NotImplementedError, anything else ValueError (`train.check_precision`)."""
    from ..train.core import check_precision
    if check_precision(precision) not in SPLIT_PIECES:
        raise ValueError(
            f"encoder_layer_split takes precision 'bf16x3', not "
            f'precision={precision!r}: encoder_layer is the float32 layer')
    return SPLIT_PIECES[precision]


def _key_counts(key_counts, layout):
    """The device table of `key_counts` (int host tensor [N], the real
    positions of every segment of `layout`), checked on the host when the
    layout does not hold these values already (the backward asks again)."""
    if key_counts.is_cuda or key_counts.is_floating_point():
        raise TypeError('key_counts is an integer host tensor, like cu_T')

    def check(counts):
        frames = np.asarray(layout.plan.frames, dtype=np.int64)
        if counts.shape != frames.shape:
            raise ValueError(
                f'key_counts has shape {tuple(counts.shape)}: one count for '
                f'each of the {frames.size} segments of cu_T')
        if np.any(counts < 1) or np.any(counts > frames):
            raise ValueError(
                'key_counts[i] must lie in 1 .. T_i (the real positions of '
                'segment i, at least one)')
    return layout.key_counts(
        key_counts.detach().to(torch.int64).numpy(), check)


def _layer_forward(x, tensors, cu_T, heads, dropout=None, precision=None,
                   key_counts=None):
    """The body of `encoder_layer` (`dropout` None), of
    `encoder_layer_dropout` (`dropout` = (p, seed, stream_base, step)), of
    `encoder_layer_split` (`precision`) and of `encoder_layer_padded`
    (`key_counts`)."""
    pieces = 0
    if precision is not None:
        pieces = _split_pieces(precision)
        _check_layer_shape('encoder_layer_split', int(x.shape[0]), int(heads))
    if dropout is not None:
        _check_layer_shape('encoder_layer_dropout', int(x.shape[0]), int(heads))
        dropout = _mask_arguments(*dropout)
    index, tensors, layout = _layer_inputs(x, tensors, cu_T)
    if key_counts is not None:
        _check_layer_shape('encoder_layer_padded', int(x.shape[0]), int(heads))
        if x.dtype != torch.float32:
            raise TypeError(f'encoder_layer_padded takes float32, not {x.dtype}')
        key_counts = _key_counts(key_counts, layout)
    # (the plain layer of a parameter set that never changed is the fused
    # engine's, which alone takes a `cu_T` that covers fewer columns)
    unfused = dropout is not None or pieces or key_counts is not None or \
        any([_weight_changes(tensor) for tensor in tensors])
    if unfused and layout.frame_columns.numel() != x.shape[1]:
        raise ValueError('cu_T does not cover the columns of x')
    if unfused:
        with torch.cuda.device(index):
            run = _LayerRun(x, tensors, heads, layout, index, dropout, pieces,
                            key_counts)
            return run.normed2.index_select(1, layout.frame_columns)
    engine = _layer_engine(tensors, index, int(x.shape[0]), int(heads))
    plan = layout.plan
    with torch.cuda.device(index), engine.lock:
        meta = engine.upload(plan)
        packed = layout.scatter(x, layout.frame_columns, plan.ld_frames)
        other = torch.zeros_like(packed)
        encoded = engine._stack_forward(
            engine.frame_encoder, packed, other, plan.ld_frames, plan, meta,
            runtime.AXIS_FRAMES, meta['tile'], 'op', positioned=True)
        return encoded.index_select(1, layout.frame_columns)


def _layer_fake(x, *rest):
    return x.new_empty(x.shape, dtype=torch.float32)


def _layer_setup(kind):
    """`setup_context` of the layer op `kind`: what follows `heads` in its
    inputs is nothing ('encoder_layer'), the four mask arguments
    ('encoder_layer_dropout') or `precision` ('encoder_layer_split');
    'encoder_layer_padded' has `key_counts` IN FRONT of `heads`."""
    def setup(ctx, inputs, output):
        ctx.kind = kind
        ctx.key_counts = None
        ctx.heads = inputs[14]
        ctx.extra = len(inputs) - 15
        if kind == 'encoder_layer_padded':
            ctx.key_counts, ctx.heads = inputs[14], inputs[15]
        ctx.dropout = tuple(inputs[15:19]) \
            if kind == 'encoder_layer_dropout' else None
        ctx.precision = inputs[15] if kind == 'encoder_layer_split' else None
        ctx.save_for_backward(*inputs[:14])
    return setup


def _layer_backward(ctx, grad):
    """The thirteen gradients, and a None for every other input of the op."""
    plain = ctx.dropout is None
    name = ctx.kind
    _once(name)
    saved = ctx.saved_tensors
    x, cu_T = saved[0], saved[13]
    need = list(ctx.needs_input_grad[:13])
    _check_layer_shape(
        'the backward of encoder_layer' if name == 'encoder_layer' else name,
        x.shape[0], ctx.heads)
    others = (None,) * (2 + ctx.extra)          # cu_T, heads, the op's own
    if not any(need):
        return (None,) * 13 + others
    index, tensors, layout = _layer_inputs(x, saved[1:13], cu_T)
    with torch.cuda.device(index):
        run = _LayerRun(
            x.detach(), tensors, ctx.heads, layout, index,
            None if plain else _mask_arguments(*ctx.dropout),
            0 if ctx.precision is None else _split_pieces(ctx.precision),
            None if ctx.key_counts is None
            else _key_counts(ctx.key_counts, layout))
        grads = run.backward(grad, need)
        if grads[0] is not None:
            grads[0] = grads[0].index_select(1, layout.frame_columns)
    grads = [None if g is None else g.to(source.dtype).reshape(source.shape)
             for g, source in zip(grads, saved[:13])]
    return (*grads, *others)


@torch.library.custom_op('emphases_amd::encoder_layer', mutates_args=())
def encoder_layer(x: torch.Tensor, in_proj_weight: torch.Tensor,
                  in_proj_bias: torch.Tensor, out_proj_weight: torch.Tensor,
                  out_proj_bias: torch.Tensor, norm1_weight: torch.Tensor,
                  norm1_bias: torch.Tensor, linear1_weight: torch.Tensor,
                  linear1_bias: torch.Tensor, linear2_weight: torch.Tensor,
                  linear2_bias: torch.Tensor, norm2_weight: torch.Tensor,
                  norm2_bias: torch.Tensor, cu_T: torch.Tensor,
                  heads: int) -> torch.Tensor:
    """One `nn.TransformerEncoderLayer` (post-LN, ReLU, eps 1e-5) as
    `transformer.py:18-30` stacks them, over N segments back to back
    (attention within a segment only): x `[C, sum T_i]` -> `[C, sum T_i]`; no
    positional encoding is added.

    DROPOUT IS THE IDENTITY, in the forward and in the backward: this op is
    the layer in `.eval()`.  The reference's layer TRAINS with its internal
    dropout of 0.1 (attention weights, both residual branches, the
    feed-forward); `encoder_layer_dropout` draws those, as specified masks.

    A parameter set that has never changed since the op first saw it runs on
    the fused inference engine of the layer (its packs made once on the host);
    one whose version has changed (an optimizer updates it in place) runs the
    unfused, device-packed sequence of `_LayerRun` - see the module docstring.

    Backward (once): the context saves the inputs only; the layer is
    recomputed by `_LayerRun`, which keeps every intermediate, and walked back
    through `emph_add_layernorm_backward`, `emph_attention_backward`,
    `emph_activation_gradient`, `emph_conv_weight_grad_any` (kernel_size 1;
    in_proj as three row slices of dQ | dK | dV) and `emph_conv1d` on the
    flipped device packs (in_proj: one launch, c_in 240).  Only the gradients
    `needs_input_grad` asks for are computed, and the walk stops where nothing
    upstream needs it.  Channels other than 80 or heads other than 2 raise
    NotImplementedError in the backward (the forward accepts what
    `emph_attention` does)."""
    return _layer_forward(
        x, (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias,
            norm1_weight, norm1_bias, linear1_weight, linear1_bias,
            linear2_weight, linear2_bias, norm2_weight, norm2_bias),
        cu_T, heads)


@torch.library.custom_op('emphases_amd::encoder_layer_dropout', mutates_args=())
def encoder_layer_dropout(
        x: torch.Tensor, in_proj_weight: torch.Tensor,
        in_proj_bias: torch.Tensor, out_proj_weight: torch.Tensor,
        out_proj_bias: torch.Tensor, norm1_weight: torch.Tensor,
        norm1_bias: torch.Tensor, linear1_weight: torch.Tensor,
        linear1_bias: torch.Tensor, linear2_weight: torch.Tensor,
        linear2_bias: torch.Tensor, norm2_weight: torch.Tensor,
        norm2_bias: torch.Tensor, cu_T: torch.Tensor, heads: int, p: float,
        seed: int, stream_base: int, step: int) -> torch.Tensor:
    """`encoder_layer` in TRAINING mode: the four dropouts of
    `nn.TransformerEncoderLayer` (the attention weights after the softmax,
    `dropout1` on the attention branch, `dropout` on the hidden layer after
    its ReLU, `dropout2` on the feed-forward branch), each with probability
    `p`, drawn as `train/dropout.py` specifies from (`seed`, `stream_base`
    + 0 .. 3, `step`): a pure function of its arguments.  The element-wise
    masks index the layer's packed buffer [rows, ld] of the frame plan of
    `cu_T`; the attention mask is `attention_keep_mask`.

    Always the unfused sequence of `_LayerRun` (`emph_attention_dropout`,
    `emph_dropout`).  Backward (once): recomputed with the same four
    integers, walked back through `emph_attention_dropout_backward` and the
    same masks on the gradients.  80 channels in 2 heads only."""
    return _layer_forward(
        x, (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias,
            norm1_weight, norm1_bias, linear1_weight, linear1_bias,
            linear2_weight, linear2_bias, norm2_weight, norm2_bias),
        cu_T, heads, (p, seed, stream_base, step))


@torch.library.custom_op('emphases_amd::encoder_layer_split', mutates_args=())
def encoder_layer_split(
        x: torch.Tensor, in_proj_weight: torch.Tensor,
        in_proj_bias: torch.Tensor, out_proj_weight: torch.Tensor,
        out_proj_bias: torch.Tensor, norm1_weight: torch.Tensor,
        norm1_bias: torch.Tensor, linear1_weight: torch.Tensor,
        linear1_bias: torch.Tensor, linear2_weight: torch.Tensor,
        linear2_bias: torch.Tensor, norm2_weight: torch.Tensor,
        norm2_bias: torch.Tensor, cu_T: torch.Tensor, heads: int,
        precision: str) -> torch.Tensor:
    """`encoder_layer` at `precision='bf16x3'`: the attention core on the
    bf16 matrix pipe, every fp32 operand split into bf16 pieces (the engine's
    rule for attention: three pieces and six products for the scores, two and
    three behind the softmax), fp32 accumulation.  The projections, the
    feed-forward, the LayerNorms stay the float32 kernels; dropout is the
    identity.

    Which kernels take a segment depends on its length alone
    (`engine.GROUPED_FROM` = 128): segments of at least 128 positions take
    `emph_split_kv` + `emph_attention_split` and, in the backward,
    `emph_attention_backward_split`; shorter ones `emph_attention` /
    `emph_attention_backward` through a tile table of their own - at most two
    launches per direction, and a batch without a long segment gives the bits
    of `encoder_layer` on updated parameters.  Always the unfused sequence of
    `_LayerRun`.  80 channels in 2 heads only (NotImplementedError);
    `precision` 'bf16x3' only: 'f32' is `encoder_layer` (ValueError),
    'bf16x3_fast' / 'bf16x6' raise NotImplementedError."""
    return _layer_forward(
        x, (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias,
            norm1_weight, norm1_bias, linear1_weight, linear1_bias,
            linear2_weight, linear2_bias, norm2_weight, norm2_bias),
        cu_T, heads, precision=precision)


@torch.library.custom_op('emphases_amd::encoder_layer_padded', mutates_args=())
def encoder_layer_padded(
        x: torch.Tensor, in_proj_weight: torch.Tensor,
        in_proj_bias: torch.Tensor, out_proj_weight: torch.Tensor,
        out_proj_bias: torch.Tensor, norm1_weight: torch.Tensor,
        norm1_bias: torch.Tensor, linear1_weight: torch.Tensor,
        linear1_bias: torch.Tensor, linear2_weight: torch.Tensor,
        linear2_bias: torch.Tensor, norm2_weight: torch.Tensor,
        norm2_bias: torch.Tensor, cu_T: torch.Tensor,
        key_counts: torch.Tensor, heads: int) -> torch.Tensor:
    """`encoder_layer` behind `src_key_padding_mask` (`transformer.py:26-29`):
    segment i of `cu_T` holds `key_counts[i]` real positions followed by zero
    padding (a word piece padded to the longest word, `batch.Pieces`).  Every
    position is a query and gets an output, the padded ones too; only the
    leading `key_counts[i]` are keys.  `key_counts`: integer host tensor [N]
    like `cu_T`, checked on the host, 1 <= key_counts[i] <= T_i (ValueError).

    Always the unfused sequence of `_LayerRun`, `emph_attention` taking the
    table; dropout is the identity.  Backward (once): recomputed and walked
    back through `emph_attention_backward_keys`, which writes dK and dV of a
    padded position as zeros, so in_proj's gradients take nothing from the
    padding's keys and values.  With `key_counts == T` everywhere the bits of
    `encoder_layer` on updated parameters.  float32 x, 80 channels in 2 heads
    only (TypeError, NotImplementedError)."""
    return _layer_forward(
        x, (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias,
            norm1_weight, norm1_bias, linear1_weight, linear1_bias,
            linear2_weight, linear2_bias, norm2_weight, norm2_bias),
        cu_T, heads, key_counts=key_counts)


for _kind, _op in (('encoder_layer', encoder_layer),
                   ('encoder_layer_dropout', encoder_layer_dropout),
                   ('encoder_layer_split', encoder_layer_split),
                   ('encoder_layer_padded', encoder_layer_padded)):
    _op.register_fake(_layer_fake)
    _op.register_autograd(
        _layer_backward, setup_context=_layer_setup(_kind))


def _masked(x, p, seed, stream, step):
    p, seed, stream, step = _mask_arguments(p, seed, stream, step)
    if x.dtype != torch.float32:
        raise TypeError(f'dropout takes float32, not {x.dtype}')
    index = _device_index(x)
    count = x.numel()
    if not count:
        return x.clone()
    # (emph_dropout works in whole quads: the tail is padded)
    out = torch.zeros((count + 3) // 4 * 4, dtype=torch.float32,
                      device=x.device)
    out[:count] = x.reshape(-1)
    with torch.cuda.device(index):
        _call('emph_dropout', out, out.numel(), 0, p, seed, stream, step)
    return out[:count].reshape(x.shape).clone()


@torch.library.custom_op('emphases_amd::dropout', mutates_args=())
def dropout(x: torch.Tensor, p: float, seed: int, stream: int,
            step: int) -> torch.Tensor:
    """The specified mask (`train/dropout.py`, `keep_mask`) on the flat index
    of a float32 tensor: a copy through `emph_dropout`, kept elements scaled
    by float32(1 / (1 - p)).  Differentiable: the same mask on the gradient.
    The positional site of `TransformerModel(reference_dropout=True)`."""
    return _masked(x, p, seed, stream, step)


@dropout.register_fake
def _dropout_fake(x, p, seed, stream, step):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


def _dropout_setup(ctx, inputs, output):
    ctx.mask = tuple(inputs[1:5])


def _dropout_backward(ctx, grad):
    _once('dropout')
    return _masked(grad.to(torch.float32), *ctx.mask), None, None, None, None


dropout.register_autograd(_dropout_backward, setup_context=_dropout_setup)


@torch.library.custom_op('emphases_amd::prominence_forward', mutates_args=())
def prominence_forward(audio_packed: torch.Tensor, cu_samples: torch.Tensor,
                       bounds: torch.Tensor, cu_words: torch.Tensor) -> torch.Tensor:
    """`infer` + `postprocess` (`core.py:295-342`) with the active
    configuration and the bundled checkpoint over N CHUNKS back to back (what
    `preprocess` hands to `infer`, `core.py:345-418`: the audio slice at the
    frame-quantised word times, bounds relative to the chunk): audio `[sum
    S_i]`, bounds int `[2, sum W_i]` -> scores float32 `[sum W_i]`."""
    index = _device_index(audio_packed)
    samples, edges = _counts(cu_samples)
    words, _ = _counts(cu_words)
    if len(samples) != len(words):
        raise ValueError('cu_samples and cu_words describe different numbers of chunks')
    host_bounds = bounds.detach().cpu().to(torch.int64).numpy().reshape(2, -1)
    engine = core.get_engine(None, index)
    plan = _chunk_plan(samples, edges, words, host_bounds)
    with torch.cuda.device(index), engine.lock:
        scores, _ = engine.forward(audio_packed.contiguous(), plan)
        columns = torch.from_numpy(plan.word_columns()).to(audio_packed.device)
        return scores[columns].clone()
