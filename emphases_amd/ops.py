"""The operator seams of SURVEY §8b as `torch.library` custom ops over the C ABI:
`at::Tensor` in, `at::Tensor` out, ragged ("varlen") axes described by `cu_*`
prefix sums, so that a caller of the reference's ATen ops
(`/root/reference/emphases/model/core.py:93-138`) needs no `ctypes`:

    torch.ops.emphases_amd.logmel(audio_packed, cu_samples)            mels.py:16-109
    torch.ops.emphases_amd.conv1d_same_act(x, w, b, cu_T, act)         convolution.py:25-37
    torch.ops.emphases_amd.segment_reduce(x, bounds, cu_frames, cu_words, mode)
                                                                       core.py:426-469
    torch.ops.emphases_amd.encoder_layer(x, in_w, in_b, out_w, out_b, norm1_w, norm1_b,
                                         ff1_w, ff1_b, ff2_w, ff2_b, norm2_w, norm2_b,
                                         cu_T, heads)                  transformer.py:18-30
    torch.ops.emphases_amd.encoder_layer_dropout(x, <the same twelve>, cu_T, heads,
                                         p, seed, stream_base, step)   the same in .train()
    torch.ops.emphases_amd.dropout(x, p, seed, stream, step)           transformer.py:51-52
    torch.ops.emphases_amd.prominence_forward(audio_packed, cu_samples, bounds, cu_words)
                                                                       core.py:295-342

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
under the reference's four dropouts as specified masks, and `dropout` the
mask alone) and `logmel` (gradient of a float `audio_packed`: the
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

One plan per batch: the packed layout of a set of `cu_*` (and `bounds`)
values, its device metadata and its device column indices are kept in a small
LRU keyed by the bytes of those arrays and the device, so the layers of a
model and their backwards share one upload.
"""
import collections
import functools
import threading
import weakref

import numpy as np
import torch

from . import batch
from . import config as cfg
from . import core
from . import engine as engine_module
from . import runtime
from . import weights as weights_module

__all__ = ['logmel', 'conv1d_same_act', 'segment_reduce', 'encoder_layer',
           'encoder_layer_dropout', 'dropout', 'prominence_forward']

GRAD_TILE = 64       # emph_conv_weight_grad_any, emph_segment_reduce_backward
DIRECT_TILE = 64     # emph_conv1d of the device-packed path and of the data gradient
PLAN_CACHE_SIZE = 16


def _counts(cu):
    """Per-segment counts (python ints) of a prefix-sum tensor."""
    values = cu.detach().cpu().to(torch.int64).numpy()
    if values.ndim != 1 or values.size < 1 or values[0] != 0 or \
            np.any(np.diff(values) < 0):
        raise ValueError('cu_* must be non-decreasing prefix sums that start at 0')
    return np.diff(values).astype(np.int64), values


def _frame_plan(frames, words=None, bounds=None):
    """`batch.Plan` of already-featurised segments of `frames[i]` positions."""
    segments = []
    word_first = 0
    for index, count in enumerate(frames):
        if words is None:
            own = np.zeros((2, 0), dtype=np.int64)
        else:
            own = bounds[:, word_first:word_first + int(words[index])]
            word_first += int(words[index])
        segments.append(batch.Segment(
            index, 0, own.shape[1], 0, 0, int(count), own))
    return batch.Plan(segments, [0] * len(segments), [0] * len(segments))


def _columns(offsets, counts, device):
    """The library's packed columns of N back-to-back segments, as one index."""
    if not len(counts):
        return torch.zeros(0, dtype=torch.int64, device=device)
    index = np.concatenate([np.arange(off, off + count, dtype=np.int64)
                            for off, count in zip(offsets, counts)])
    return torch.from_numpy(index).to(device)


def _scatter(x, plan, offsets, counts, ld):
    """Back-to-back columns -> the library's packed axis (one indexed copy, not
    one per segment: 64 segments cost 0.5 ms of launches, tools/ops_cost.py)."""
    packed = torch.zeros((x.shape[0], ld), dtype=torch.float32, device=x.device)
    index = _columns(offsets, counts, x.device)
    packed.index_copy_(1, index, x[:, :index.numel()].to(torch.float32))
    return packed


def _gather(packed, offsets, counts):
    """The library's packed axis -> back-to-back columns (a fresh tensor)."""
    return packed.index_select(1, _columns(offsets, counts, packed.device))


class _Layout:
    """What the ops of one batch share: the `batch.Plan`, its integer metadata
    on the device (name -> (view, size)), the frame tile tables (each uploaded
    when an op first asks for its width, so a plan costs no more to build
    than it did per call) and the device column indices of `_scatter` /
    `_gather`."""

    def __init__(self, plan, device):
        self.plan = plan
        host, offsets = plan.pack_metadata([])
        self.buffer = torch.from_numpy(host).to(device)
        self.meta = {name: (self.buffer[start:start + size], size)
                     for name, (start, size) in offsets.items()}
        self.meta['positions'] = (plan.total_frames, plan.total_words)
        self.frame_columns = _columns(plan.frame_off, plan.frames, device)
        self._word_columns = None
        self.checked = {}

    @property
    def word_columns(self):
        if self._word_columns is None:
            self._word_columns = _columns(
                self.plan.word_off, self.plan.words, self.buffer.device)
        return self._word_columns

    def view(self, name):
        return self.meta[name][0]

    def tiles(self, tile):
        """(device tile table of the frame axis `tile` wide, its rows)."""
        key = ('tiles', runtime.AXIS_FRAMES, tile)
        if key not in self.meta:
            host = np.ascontiguousarray(
                self.plan.tiles(runtime.AXIS_FRAMES, tile)).ravel()
            self.meta[key] = (
                torch.from_numpy(host).to(self.buffer.device), host.size)
        tiles, size = self.meta[key]
        return tiles, size // runtime.TILE_FIELDS

    def scatter(self, x, columns, ld):
        """Back-to-back columns -> the library's packed axis (zeros between)."""
        packed = torch.zeros((x.shape[0], ld), dtype=torch.float32,
                             device=x.device)
        packed.index_copy_(
            1, columns, x[:, :columns.numel()].to(torch.float32))
        return packed


_layouts = collections.OrderedDict()
_layouts_lock = threading.Lock()


def _layout(device, frames, words=None, bounds=None):
    """The `_Layout` of segments of `frames[i]` positions (and `words[i]` words
    with `bounds`), from a small LRU keyed by the VALUES of the arrays."""
    key = (device.index, frames.tobytes(),
           None if words is None else (words.tobytes(), bounds.tobytes()))
    with _layouts_lock:
        found = _layouts.get(key)
        if found is not None:
            _layouts.move_to_end(key)
            return found
    found = _Layout(_frame_plan(frames, words, bounds), device)
    with _layouts_lock:
        _layouts[key] = found
        while len(_layouts) > PLAN_CACHE_SIZE:
            _layouts.popitem(last=False)
    return found


def _device_index(tensor):
    if not tensor.is_cuda:
        raise runtime.LibraryError(
            'emphases_amd ops run on an MI355X / HIP device only (no CPU '
            'fallback): the tensor is on ' + str(tensor.device))
    return tensor.device.index


_logmel_plans = collections.OrderedDict()


def _logmel_plan(cu_samples):
    """The `batch.Plan` of N chunks back to back (a chunk = an utterance whose
    one segment starts behind the zero padding), from a small LRU keyed by the
    values of `cu_samples`: the forward and its backward share one."""
    samples, edges = _counts(cu_samples)
    key = edges.tobytes()
    with _layouts_lock:
        found = _logmel_plans.get(key)
        if found is not None:
            _logmel_plans.move_to_end(key)
            return found
    frames = [1 + (int(n) + 2 * cfg.PADDING - cfg.NUM_FFT) // cfg.HOPSIZE
              if n > cfg.PADDING else 0 for n in samples]
    if any(f <= 0 for f in frames):
        raise ValueError('a chunk needs more than 432 samples (reflect padding, mels.py:31-36)')
    segments = [batch.Segment(i, 0, 0, cfg.PADDING, int(n), f,
                              np.zeros((2, 0), dtype=np.int64))
                for i, (n, f) in enumerate(zip(samples, frames))]
    found = batch.Plan(segments, edges[:-1], samples)
    with _layouts_lock:
        _logmel_plans[key] = found
        while len(_logmel_plans) > PLAN_CACHE_SIZE:
            _logmel_plans.popitem(last=False)
    return found


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
    plan = _logmel_plan(cu_samples)
    engine = core.get_engine(None, index, cfg.DEFAULT)
    with torch.cuda.device(index), engine.lock:
        meta = engine.upload(plan)
        packed = engine.features(audio_packed.contiguous(), plan, meta)
        return _gather(packed, plan.frame_off, plan.frames)


class _Borrowed:
    """A tensor as an lru_cache argument that neither hashes nor compares."""

    def __init__(self, tensor):
        self.tensor = tensor

    def __hash__(self):
        return 0

    def __eq__(self, other):
        return True


def _cached_conv(weight, bias, index):
    return _conv_layer_cached(
        weight.data_ptr(), weight._version, tuple(weight.shape),
        None if bias is None else (bias.data_ptr(), bias._version), index,
        _Borrowed(weight), _Borrowed(bias))


@functools.lru_cache(maxsize=32)
def _conv_layer_cached(pointer, version, shape, bias_key, index, weight, bias):
    bias = bias.tensor
    return engine_module._Conv(
        weight.tensor.detach().cpu().numpy(),
        None if bias is None else bias.detach().cpu().numpy(),
        torch.device('cuda', index), winograd=True)


def pack_index_tables(shape):
    """The `emph_take` tables of a [c_out, c_in, k] weight (host, int32; -1:
    zero): of the direct-form pack of the weight itself and of the pack of
    W'[ci][co][j] = W[co][ci][k - 1 - j], whose `emph_conv1d` is the data
    gradient."""
    from .train import core as train_core
    indices = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    flipped = np.ascontiguousarray(indices.transpose(1, 0, 2)[:, :, ::-1])
    return (train_core._pack_indices(indices).astype(np.int32),
            train_core._pack_indices(flipped).astype(np.int32))


@functools.lru_cache(maxsize=32)
def _device_tables(shape, index):
    return tuple(torch.from_numpy(table).to(torch.device('cuda', index))
                 for table in pack_index_tables(shape))


class _ByStorage:
    """A small LRU keyed by a tensor's (address, shape, strides, ...) that can
    never answer for ANOTHER tensor: every entry holds a weak reference to the
    storage it was made from and is a hit only while that very storage is
    alive and is the asking tensor's.  (An address alone is not an identity:
    the caching allocator hands the address of a dropped weight to the next
    one of the same shape.)  Entries of dead storages are dropped as they are
    met.  One lock for every instance.  (Relies on torch returning the SAME
    Python object from `tensor.untyped_storage()` for as long as the storage
    lives; on a torch that made a new object per call every lookup would miss
    - still correct, but the weight would be packed again on every call.)"""

    lock = threading.Lock()

    def __init__(self, size):
        self.size = size
        self.entries = collections.OrderedDict()

    @staticmethod
    def key(tensor, *more):
        return (tensor.data_ptr(), tuple(tensor.shape), tuple(tensor.stride()),
                str(tensor.device)) + more

    def get(self, tensor, key):
        storage = tensor.untyped_storage()
        with self.lock:
            found = self.entries.get(key)
            if found is None:
                return None
            if found[0]() is not storage:
                del self.entries[key]       # another tensor lived here
                return None
            self.entries.move_to_end(key)
            return found[1]

    def put(self, tensor, key, value):
        with self.lock:
            self.entries[key] = (weakref.ref(tensor.untyped_storage()), value)
            self.entries.move_to_end(key)
            while len(self.entries) > self.size:
                self.entries.popitem(last=False)
        return value


_device_packs = _ByStorage(256)
_first_versions = _ByStorage(256)


def _device_pack(weight, index, flipped, rows=None):
    """The direct-form MFMA pack of `weight` (or of its flipped transpose),
    built on the device by one `emph_take`; kept per (storage, version).
    `rows` = (first, last): of those rows of a 2-D `weight` alone, as a
    kernel_size-1 convolution (the Linear layers of `encoder_layer`; None for
    a 2-D weight: all of its rows)."""
    key = _ByStorage.key(weight, weight._version, flipped, rows)
    found = _device_packs.get(weight, key)
    if found is not None:
        return found
    source = weight.detach()
    if source.dtype != torch.float32 or not source.is_contiguous():
        source = source.to(torch.float32).contiguous()
    if source.dim() == 2:
        first, last = rows or (0, source.shape[0])
        source = source[first:last].unsqueeze(2)
    table = _device_tables(tuple(source.shape), index)[1 if flipped else 0]
    pack = torch.empty(table.numel(), dtype=torch.float32, device=weight.device)
    runtime.check(runtime.library().emph_take(
        source.data_ptr(), table.data_ptr(), pack.data_ptr(), pack.numel(),
        runtime.stream()), 'emph_take')
    return _device_packs.put(weight, key, pack)


def _weight_changes(weight):
    """Whether the version of `weight` has changed since the op first saw its
    storage: the weight is being trained (the op cannot see `requires_grad`
    below the autograd key)."""
    key = _ByStorage.key(weight)
    first = _first_versions.get(weight, key)
    if first is None:
        first = _first_versions.put(weight, key, (weight._version,))
    return first[0] != weight._version


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


def _float_pointer(tensor, keep):
    """Device address of a float32 contiguous view of `tensor` (kept alive in
    the list `keep`); None for None."""
    if tensor is None:
        return None
    tensor = tensor.detach()
    if tensor.dtype != torch.float32 or not tensor.is_contiguous():
        tensor = tensor.to(torch.float32).contiguous()
    keep.append(tensor)
    return tensor.data_ptr()


def _direct_conv(packed, out, ld, pack, bias, c_in, c_out, kernel_size,
                 activation, layout):
    tiles, n_tiles = layout.tiles(DIRECT_TILE)
    runtime.check(runtime.library().emph_conv1d(
        packed.data_ptr(), ld, out.data_ptr(), ld, pack.data_ptr(), bias, c_in,
        c_out, kernel_size, runtime.ACTIVATIONS[activation], tiles.data_ptr(),
        n_tiles, DIRECT_TILE, 0, runtime.stream()), 'emph_conv1d')


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
        if _weight_changes(weight):
            c_out, c_in, kernel_size = weight.shape
            keep = []
            _direct_conv(packed, out, plan.ld_frames,
                         _device_pack(weight, index, False),
                         _float_pointer(bias, keep), c_in, c_out, kernel_size,
                         activation, layout)
        else:
            layer = _cached_conv(weight, bias, index)
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
    plan = _logmel_plan(cu_samples)
    engine = core.get_engine(None, index, cfg.DEFAULT)
    lib = runtime.library()
    with torch.cuda.device(index), engine.lock:
        meta = engine.upload(plan)
        tiles, size = meta[
            ('tiles', runtime.AXIS_FRAMES, engine_module.FRONTEND_BLOCK)]
        n_tiles = size // runtime.TILE_FIELDS
        audio = audio_packed.detach()
        if audio.dtype != torch.float32 or not audio.is_contiguous():
            audio = audio.to(torch.float32).contiguous()
        dmel = _scatter(grad, plan, plan.frame_off, plan.frames, plan.ld_frames)
        # (samples outside every chunk - behind the last prefix sum - get 0)
        daudio = torch.zeros_like(audio)
        workspace = torch.empty(
            int(lib.emph_logmel_backward_workspace(n_tiles)),
            dtype=torch.float32, device=audio.device)
        runtime.check(lib.emph_logmel_backward(
            audio.data_ptr(), meta['table'][0].data_ptr(), tiles.data_ptr(),
            n_tiles, _backward_table(index).data_ptr(), engine.mel_start.data_ptr(),
            engine.mel_count.data_ptr(), engine.mel_offset.data_ptr(),
            engine.mel_values.data_ptr(), engine.mel_nnz, dmel.data_ptr(),
            plan.ld_frames, 0, workspace.data_ptr(), daudio.data_ptr(),
            runtime.stream()), 'emph_logmel_backward')
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
    plan, ld = layout.plan, layout.plan.ld_frames
    c_out, c_in, kernel_size = weight.shape
    lib = runtime.library()
    dx = dweight = dbias = None
    with torch.cuda.device(index):
        stream = runtime.stream()
        dy = layout.scatter(grad, layout.frame_columns, ld)
        packed = None
        if need_weight or need_bias or activation in ('gelu', 'silu'):
            packed = layout.scatter(x, layout.frame_columns, ld)
        if activation in ('relu', 'leaky_relu'):
            source = layout.scatter(output, layout.frame_columns, ld)
        elif activation is not None:
            keep = []
            source = torch.zeros_like(dy)
            _direct_conv(packed, source, ld, _device_pack(weight, index, False),
                         _float_pointer(bias, keep), c_in, c_out, kernel_size,
                         None, layout)
        if activation is not None:
            runtime.check(lib.emph_activation_gradient(
                source.data_ptr(), dy.data_ptr(), dy.numel(),
                runtime.ACTIVATIONS[activation], stream),
                'emph_activation_gradient')
        if need_weight or need_bias:
            tiles, n_tiles = layout.tiles(GRAD_TILE)
            dweight = torch.empty((c_out, c_in, kernel_size),
                                  dtype=torch.float32, device=grad.device)
            dbias = torch.empty(c_out, dtype=torch.float32, device=grad.device)
            if n_tiles:
                workspace = torch.empty(
                    int(lib.emph_conv_weight_grad_any_workspace(
                        c_in, c_out, kernel_size, n_tiles)),
                    dtype=torch.float32, device=grad.device)
                runtime.check(lib.emph_conv_weight_grad_any(
                    dy.data_ptr(), ld, packed.data_ptr(), ld, c_in, c_out,
                    kernel_size, tiles.data_ptr(), n_tiles, GRAD_TILE,
                    workspace.data_ptr(), dweight.data_ptr(), dbias.data_ptr(),
                    stream), 'emph_conv_weight_grad_any')
            else:
                dweight.zero_()
                dbias.zero_()
            dweight = dweight.to(weight.dtype) if need_weight else None
            dbias = dbias.to(bias.dtype) if need_bias else None
        if need_x:
            dpacked = torch.zeros((c_in, ld), dtype=torch.float32,
                                  device=grad.device)
            _direct_conv(dy, dpacked, ld, _device_pack(weight, index, True),
                         None, c_out, c_in, kernel_size, None, layout)
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
    lib = runtime.library()
    with torch.cuda.device(index):
        packed = layout.scatter(x, layout.frame_columns, plan.ld_frames)
        out = torch.zeros((x.shape[0], plan.ld_words), dtype=torch.float32,
                          device=x.device)
        runtime.check(lib.emph_segment_reduce(
            packed.data_ptr(), plan.ld_frames, layout.view('bounds').data_ptr(),
            out.data_ptr(), plan.ld_words, x.shape[0],
            layout.view('table').data_ptr(),
            layout.view('word_segment').data_ptr(), plan.ld_words,
            runtime.REDUCTIONS[mode], runtime.stream()), 'emph_segment_reduce')
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
    lib = runtime.library()
    with torch.cuda.device(index):
        dword = layout.scatter(grad, layout.word_columns, plan.ld_words)
        packed = top = None
        if mode == 'max':
            packed = layout.scatter(x, layout.frame_columns, plan.ld_frames)
            top = layout.scatter(output, layout.word_columns, plan.ld_words)
        dpacked = torch.zeros((x.shape[0], plan.ld_frames), dtype=torch.float32,
                              device=grad.device)
        tiles, n_tiles = layout.tiles(GRAD_TILE)
        runtime.check(lib.emph_segment_reduce_backward(
            dword.data_ptr(), plan.ld_words, layout.view('bounds').data_ptr(),
            None if packed is None else packed.data_ptr(), plan.ld_frames,
            None if top is None else top.data_ptr(), dpacked.data_ptr(),
            plan.ld_frames, x.shape[0], layout.view('table').data_ptr(),
            tiles.data_ptr(), n_tiles, runtime.REDUCTIONS[mode],
            runtime.stream()), 'emph_segment_reduce_backward')
        dx = dpacked.index_select(1, layout.frame_columns).to(x.dtype)
        if dx.shape[1] < x.shape[1]:      # (columns past the last segment)
            dx = torch.nn.functional.pad(dx, (0, x.shape[1] - dx.shape[1]))
    return dx, None, None, None, None


segment_reduce.register_autograd(_reduce_backward, setup_context=_reduce_setup)


_LAYER_NAMES = ('self_attn.in_proj_weight', 'self_attn.in_proj_bias',
                'self_attn.out_proj.weight', 'self_attn.out_proj.bias',
                'norm1.weight', 'norm1.bias', 'linear1.weight', 'linear1.bias',
                'linear2.weight', 'linear2.bias', 'norm2.weight', 'norm2.bias')


@functools.lru_cache(maxsize=8)
def _layer_engine(key, index, channels, heads, tensors):
    config = cfg.Config(architecture='transformer', layers=1, channels=channels,
                        heads=heads)
    state = weights_module.random_state(config, seed=0)
    for name, tensor in zip(_LAYER_NAMES, tensors.tensor):
        state['frame_encoder.model.layers.0.' + name] = np.ascontiguousarray(
            tensor.detach().cpu().numpy(), dtype=np.float32)
    return engine_module.Engine(config, state, index)


LAYER_CHANNELS, LAYER_HEADS = 80, 2      # emph_attention_backward
LAYER_EPS = cfg.Config(architecture='transformer').layer_norm_eps


class _LayerRun:
    """One encoder layer as an UNFUSED sequence of launches on the packed
    layout that keeps every intermediate (what the backward walks back
    through, and the forward of a parameter set that is being trained): Q / K
    and V by `emph_conv1d` k = 1, `emph_attention`, out_proj,
    `emph_add_layernorm`, linear1 + ReLU, linear2, `emph_add_layernorm`.  The
    weights are packed on the device (`_device_pack`): nothing is copied to
    the host.

    `dropout` = (p, seed, stream_base, step) draws the reference's four
    dropouts of the layer (`train/dropout.py`): `emph_attention_dropout` in
    place of `emph_attention` under stream_base, and `emph_dropout` in place
    on `projected`, `hidden` and `fed` (whole packed buffers [rows, ld]) under
    stream_base + 1, + 2, + 3."""

    def __init__(self, x, tensors, heads, layout, index, dropout=None):
        (self.in_w, self.in_b, self.out_w, self.out_b, self.norm1_w,
         self.norm1_b, self.ff1_w, self.ff1_b, self.ff2_w, self.ff2_b,
         self.norm2_w, self.norm2_b) = tensors
        self.layout, self.index, self.heads = layout, index, int(heads)
        self.dropout = dropout
        self.ld = ld = layout.plan.ld_frames
        self.channels = channels = int(x.shape[0])
        self.device = x.device
        self.lib = runtime.library()
        self.keep = []
        self.tiles, self.n_tiles = layout.tiles(DIRECT_TILE)
        bias = _float_pointer(self.in_b, self.keep)
        self.x = layout.scatter(x, layout.frame_columns, ld)
        self.qk = self.zeros(2 * channels)
        self.conv(self.x, self.qk, self.pack(self.in_w, (0, 2 * channels)),
                  bias, channels, 2 * channels)
        self.v = torch.zeros((ld, channels), dtype=torch.float32,
                             device=self.device)
        self.conv(self.x, self.v,
                  self.pack(self.in_w, (2 * channels, 3 * channels)),
                  bias + 4 * 2 * channels, channels, channels, transpose=True)
        self.attended = self.zeros(channels)
        if dropout is None:
            runtime.check(self.lib.emph_attention(
                self.qk.data_ptr(), self.v.data_ptr(),
                self.attended.data_ptr(), ld, channels, self.heads,
                self.tiles.data_ptr(), self.n_tiles, DIRECT_TILE, None,
                runtime.stream()), 'emph_attention')
        else:
            p, seed, base, step = dropout
            runtime.check(self.lib.emph_attention_dropout(
                self.qk.data_ptr(), self.v.data_ptr(),
                self.attended.data_ptr(), ld, channels, self.heads,
                self.tiles.data_ptr(), self.n_tiles, GRAD_TILE, p, seed, base,
                step, runtime.stream()), 'emph_attention_dropout')
        self.projected = self.zeros(channels)
        self.conv(self.attended, self.projected, self.pack(self.out_w),
                  _float_pointer(self.out_b, self.keep), channels, channels)
        self.drop(self.projected, 1)
        self.normed1 = self.zeros(channels)
        self.add_layernorm(self.x, self.projected, self.normed1, self.norm1_w,
                           self.norm1_b)
        hidden = int(self.ff1_w.shape[0])
        self.hidden = self.zeros(hidden)
        self.conv(self.normed1, self.hidden, self.pack(self.ff1_w),
                  _float_pointer(self.ff1_b, self.keep), channels, hidden,
                  activation='relu')
        self.drop(self.hidden, 2)
        self.fed = self.zeros(channels)
        self.conv(self.hidden, self.fed, self.pack(self.ff2_w),
                  _float_pointer(self.ff2_b, self.keep), hidden, channels)
        self.drop(self.fed, 3)
        self.normed2 = self.zeros(channels)
        self.add_layernorm(self.normed1, self.fed, self.normed2, self.norm2_w,
                           self.norm2_b)

    def zeros(self, rows):
        return torch.zeros((rows, self.ld), dtype=torch.float32,
                           device=self.device)

    def pack(self, weight, rows=None, flipped=False):
        return _device_pack(weight, self.index, flipped, rows)

    def drop(self, buffer, site):
        """The mask of stream_base + `site` on a packed buffer or on its
        gradient, in place (nothing without `dropout`)."""
        if self.dropout is None:
            return
        p, seed, base, step = self.dropout
        runtime.check(self.lib.emph_dropout(
            buffer.data_ptr(), buffer.numel(), 0, p, seed, base + site, step,
            runtime.stream()), 'emph_dropout')

    def conv(self, x, y, pack, bias, c_in, c_out, activation=None,
             transpose=False):
        runtime.check(self.lib.emph_conv1d(
            x.data_ptr(), self.ld, y.data_ptr(),
            c_out if transpose else self.ld, pack.data_ptr(), bias, c_in,
            c_out, 1, runtime.ACTIVATIONS[activation], self.tiles.data_ptr(),
            self.n_tiles, DIRECT_TILE, int(transpose), runtime.stream()),
            'emph_conv1d')

    def add_layernorm(self, x, r, y, gamma, beta):
        runtime.check(self.lib.emph_add_layernorm(
            x.data_ptr(), r.data_ptr(), y.data_ptr(), self.ld, self.channels,
            _float_pointer(gamma, self.keep), _float_pointer(beta, self.keep),
            LAYER_EPS, 0, self.ld, runtime.stream()), 'emph_add_layernorm')

    # ---- the way back

    def layernorm_backward(self, summed, gamma, dy):
        """(ds, dgamma, dbeta) of `emph_add_layernorm_backward`."""
        ds = self.zeros(self.channels)
        dgamma = torch.empty(self.channels, dtype=torch.float32,
                             device=self.device)
        dbeta = torch.empty_like(dgamma)
        parts = int(self.lib.emph_add_layernorm_backward_parts(self.n_tiles))
        workspace = torch.empty(max(1, parts * 2 * self.channels),
                                dtype=torch.float32, device=self.device)
        runtime.check(self.lib.emph_add_layernorm_backward(
            summed.data_ptr(), _float_pointer(gamma, self.keep), dy.data_ptr(),
            ds.data_ptr(), self.ld, self.channels, LAYER_EPS,
            self.tiles.data_ptr(), self.n_tiles, GRAD_TILE,
            workspace.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
            runtime.stream()), 'emph_add_layernorm_backward')
        return ds, dgamma, dbeta

    def weight_grad(self, dy, x, c_in, c_out, dweight, dbias):
        """dweight [c_out, c_in] and dbias [c_out] (views to fill) of a Linear
        layer: `emph_conv_weight_grad_any` with kernel_size 1."""
        if not self.n_tiles:
            dweight.zero_()
            dbias.zero_()
            return
        workspace = torch.empty(
            int(self.lib.emph_conv_weight_grad_any_workspace(
                c_in, c_out, 1, self.n_tiles)),
            dtype=torch.float32, device=self.device)
        runtime.check(self.lib.emph_conv_weight_grad_any(
            dy.data_ptr(), self.ld, x.data_ptr(), self.ld, c_in, c_out, 1,
            self.tiles.data_ptr(), self.n_tiles, GRAD_TILE,
            workspace.data_ptr(), dweight.data_ptr(), dbias.data_ptr(),
            runtime.stream()), 'emph_conv_weight_grad_any')

    def backward(self, grad, need):
        """The thirteen gradients (packed dx gathered by the caller; None
        where `need` is False), walking back only as far as `need` asks."""
        channels, ld, device = self.channels, self.ld, self.device
        hidden = self.hidden.shape[0]
        out = [None] * 13

        def linear_grads(dy, x, weight, slot, rows=None):
            if not (need[slot] or need[slot + 1]):
                return
            c_out, c_in = weight.shape
            dweight = torch.empty((c_out, c_in), dtype=torch.float32,
                                  device=device)
            dbias = torch.empty(c_out, dtype=torch.float32, device=device)
            for first in range(0, c_out, rows or c_out):
                last = first + (rows or c_out)
                self.weight_grad(dy[first:last], x, c_in, last - first,
                                 dweight[first:last], dbias[first:last])
            out[slot] = dweight if need[slot] else None
            out[slot + 1] = dbias if need[slot + 1] else None

        dy = self.layout.scatter(grad, self.layout.frame_columns, ld)
        ds2, dgamma, dbeta = self.layernorm_backward(
            self.normed1 + self.fed, self.norm2_w, dy)
        dfed = ds2
        if self.dropout is not None:
            dfed = ds2.clone()
            self.drop(dfed, 3)
        out[11], out[12] = (dgamma if need[11] else None,
                            dbeta if need[12] else None)
        if not any(need[:11]):
            return out
        linear_grads(dfed, self.hidden, self.ff2_w, 9)
        if not any(need[:9]):
            return out
        dhidden = self.zeros(hidden)
        self.conv(dfed, dhidden, self.pack(self.ff2_w, flipped=True), None,
                  channels, hidden)
        # (the kept `hidden` is positive only where the ReLU passed AND the
        # mask kept: the activation gradient below selects by either)
        self.drop(dhidden, 2)
        runtime.check(self.lib.emph_activation_gradient(
            self.hidden.data_ptr(), dhidden.data_ptr(), dhidden.numel(),
            runtime.ACTIVATIONS['relu'], runtime.stream()),
            'emph_activation_gradient')
        linear_grads(dhidden, self.normed1, self.ff1_w, 7)
        if not any(need[:7]):
            return out
        dnormed1 = self.zeros(channels)
        self.conv(dhidden, dnormed1, self.pack(self.ff1_w, flipped=True), None,
                  hidden, channels)
        dnormed1 += ds2
        ds1, dgamma, dbeta = self.layernorm_backward(
            self.x + self.projected, self.norm1_w, dnormed1)
        out[5], out[6] = (dgamma if need[5] else None,
                          dbeta if need[6] else None)
        dprojected = ds1
        if self.dropout is not None:
            dprojected = ds1.clone()
            self.drop(dprojected, 1)
        linear_grads(dprojected, self.attended, self.out_w, 3)
        if not any(need[:3]):
            return out
        dattended = self.zeros(channels)
        self.conv(dprojected, dattended, self.pack(self.out_w, flipped=True),
                  None, channels, channels)
        dqkv = self.zeros(3 * channels)
        size = (self.lib.emph_attention_backward_workspace
                if self.dropout is None else
                self.lib.emph_attention_dropout_backward_workspace)
        workspace = torch.empty(max(1, int(size(ld, self.heads))),
                                dtype=torch.float32, device=device)
        if self.dropout is None:
            runtime.check(self.lib.emph_attention_backward(
                self.qk.data_ptr(), self.v.data_ptr(),
                self.attended.data_ptr(), dattended.data_ptr(),
                dqkv.data_ptr(), ld, channels, self.heads,
                self.tiles.data_ptr(), self.n_tiles, GRAD_TILE,
                workspace.data_ptr(), runtime.stream()),
                'emph_attention_backward')
        else:
            p, seed, base, step = self.dropout
            runtime.check(self.lib.emph_attention_dropout_backward(
                self.qk.data_ptr(), self.v.data_ptr(),
                self.attended.data_ptr(), dattended.data_ptr(),
                dqkv.data_ptr(), ld, channels, self.heads,
                self.tiles.data_ptr(), self.n_tiles, GRAD_TILE,
                workspace.data_ptr(), p, seed, base, step, runtime.stream()),
                'emph_attention_dropout_backward')
        linear_grads(dqkv, self.x, self.in_w, 1, rows=channels)
        if need[0]:
            dx = self.zeros(channels)
            self.conv(dqkv, dx, self.pack(self.in_w, flipped=True), None,
                      3 * channels, channels)
            dx += ds1
            out[0] = dx
        return out


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
    index = _device_index(x)
    counts, _ = _counts(cu_T)
    tensors = (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias,
               norm1_weight, norm1_bias, linear1_weight, linear1_bias,
               linear2_weight, linear2_bias, norm2_weight, norm2_bias)
    if any([_weight_changes(tensor) for tensor in tensors]):
        if int(counts.sum()) != x.shape[1]:
            raise ValueError('cu_T does not cover the columns of x')
        layout = _layout(x.device, counts)
        with torch.cuda.device(index):
            run = _LayerRun(x, tensors, heads, layout, index)
            return run.normed2.index_select(1, layout.frame_columns)
    key = tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in tensors)
    engine = _layer_engine(key, index, int(x.shape[0]), int(heads),
                           _Borrowed(tensors))
    plan = _frame_plan(counts)
    with torch.cuda.device(index), engine.lock:
        meta = engine.upload(plan)
        packed = _scatter(x.to(torch.float32), plan, plan.frame_off, plan.frames,
                          plan.ld_frames)
        other = torch.zeros_like(packed)
        encoded = engine._stack_forward(
            engine.frame_encoder, packed, other, plan.ld_frames, plan, meta,
            runtime.AXIS_FRAMES, meta['tile'], 'op', positioned=True)
        return _gather(encoded, plan.frame_off, plan.frames)


@encoder_layer.register_fake
def _encoder_layer_fake(x, in_proj_weight, in_proj_bias, out_proj_weight,
                        out_proj_bias, norm1_weight, norm1_bias, linear1_weight,
                        linear1_bias, linear2_weight, linear2_bias,
                        norm2_weight, norm2_bias, cu_T, heads):
    return x.new_empty(x.shape, dtype=torch.float32)


def _layer_setup(ctx, inputs, output):
    ctx.heads = inputs[14]
    ctx.save_for_backward(*inputs[:14])


def _layer_backward(ctx, grad):
    _once('encoder_layer')
    saved = ctx.saved_tensors
    x, tensors, cu_T = saved[0], saved[1:13], saved[13]
    need = list(ctx.needs_input_grad[:13])
    if x.shape[0] != LAYER_CHANNELS:
        raise NotImplementedError(
            f'the backward of encoder_layer supports x of {LAYER_CHANNELS} '
            f'channels only, not {x.shape[0]}')
    if ctx.heads != LAYER_HEADS:
        raise NotImplementedError(
            f'the backward of encoder_layer supports heads={LAYER_HEADS} '
            f'only, not heads={ctx.heads}')
    if not any(need):
        return (None,) * 15
    index = _device_index(grad)
    counts, _ = _counts(cu_T)
    layout = _layout(x.device, counts)
    with torch.cuda.device(index):
        run = _LayerRun(x.detach(), tensors, ctx.heads, layout, index)
        grads = run.backward(grad, need)
        if grads[0] is not None:
            grads[0] = grads[0].index_select(1, layout.frame_columns)
    grads = [None if g is None else g.to(source.dtype).reshape(source.shape)
             for g, source in zip(grads, saved[:13])]
    return (*grads, None, None)


encoder_layer.register_autograd(_layer_backward, setup_context=_layer_setup)


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
    _check_layer_shape('encoder_layer_dropout', int(x.shape[0]), int(heads))
    dropout = _mask_arguments(p, seed, stream_base, step)
    index = _device_index(x)
    counts, _ = _counts(cu_T)
    if int(counts.sum()) != x.shape[1]:
        raise ValueError('cu_T does not cover the columns of x')
    tensors = (in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias,
               norm1_weight, norm1_bias, linear1_weight, linear1_bias,
               linear2_weight, linear2_bias, norm2_weight, norm2_bias)
    layout = _layout(x.device, counts)
    with torch.cuda.device(index):
        run = _LayerRun(x, tensors, heads, layout, index, dropout)
        return run.normed2.index_select(1, layout.frame_columns)


@encoder_layer_dropout.register_fake
def _encoder_layer_dropout_fake(
        x, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias,
        norm1_weight, norm1_bias, linear1_weight, linear1_bias, linear2_weight,
        linear2_bias, norm2_weight, norm2_bias, cu_T, heads, p, seed,
        stream_base, step):
    return x.new_empty(x.shape, dtype=torch.float32)


def _layer_dropout_setup(ctx, inputs, output):
    ctx.heads = inputs[14]
    ctx.dropout = tuple(inputs[15:19])
    ctx.save_for_backward(*inputs[:14])


def _layer_dropout_backward(ctx, grad):
    _once('encoder_layer_dropout')
    saved = ctx.saved_tensors
    x, tensors, cu_T = saved[0], saved[1:13], saved[13]
    need = list(ctx.needs_input_grad[:13])
    if not any(need):
        return (None,) * 19
    index = _device_index(grad)
    counts, _ = _counts(cu_T)
    layout = _layout(x.device, counts)
    with torch.cuda.device(index):
        run = _LayerRun(x.detach(), tensors, ctx.heads, layout, index,
                        _mask_arguments(*ctx.dropout))
        grads = run.backward(grad, need)
        if grads[0] is not None:
            grads[0] = grads[0].index_select(1, layout.frame_columns)
    grads = [None if g is None else g.to(source.dtype).reshape(source.shape)
             for g, source in zip(grads, saved[:13])]
    return (*grads, None, None, None, None, None, None)


encoder_layer_dropout.register_autograd(
    _layer_dropout_backward, setup_context=_layer_dropout_setup)


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
        runtime.check(runtime.library().emph_dropout(
            out.data_ptr(), out.numel(), 0, p, seed, stream, step,
            runtime.stream()), 'emph_dropout')
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
    segments, first = [], 0
    for i, (n, w) in enumerate(zip(samples, words)):
        if n <= cfg.PADDING:
            raise ValueError('a chunk needs more than 432 samples (mels.py:31-36)')
        frames = 1 + (int(n) + 2 * cfg.PADDING - cfg.NUM_FFT) // cfg.HOPSIZE
        segments.append(batch.Segment(
            i, 0, int(w), cfg.PADDING, int(n), frames,
            host_bounds[:, first:first + int(w)]))
        first += int(w)
    plan = batch.Plan(segments, edges[:-1], samples)
    with torch.cuda.device(index), engine.lock:
        scores, _ = engine.forward(audio_packed.contiguous(), plan)
        columns = torch.from_numpy(plan.word_columns()).to(audio_packed.device)
        return scores[columns].clone()
