"""What the ops derive from a weight and keep: the launch helper, `_ByStorage`
(the one cache rule), the device packs of a weight that is being trained, the
host packs and the one-layer `Engine` of one that is not, and
`_weight_changes`, which tells the two apart."""
import collections
import ctypes
import functools
import threading
import weakref

import numpy as np
import torch

from .. import config as cfg
from .. import engine as engine_module
from .. import runtime
from .. import weights as weights_module

_Tensor = torch.Tensor


def _call(name, *arguments):
    """The library's entry point `name` on the current stream, checked:
    tensors go as their addresses, None and scalars as they are; a failure
    raises under `name`.  (By exact type, as `Engine._call`: isinstance() of a
    Tensor costs as much as all the rest; a Tensor subclass - a Parameter -
    is what ctypes refuses before it calls anything: then by isinstance.)"""
    function = getattr(runtime.library(), name)
    try:
        status = function(
            *[argument.data_ptr() if argument.__class__ is _Tensor
              else argument for argument in arguments], runtime.stream())
    except ctypes.ArgumentError:
        status = function(
            *[argument.data_ptr() if isinstance(argument, _Tensor)
              else argument for argument in arguments], runtime.stream())
    if status:
        runtime.check(status, name)


def _float32(tensor):
    """`tensor` detached, as float32 and contiguous (itself where it is both);
    None for None."""
    if tensor is None:
        return None
    tensor = tensor.detach()
    if tensor.dtype != torch.float32 or not tensor.is_contiguous():
        tensor = tensor.to(torch.float32).contiguous()
    return tensor


class _ByStorage:
    """A small LRU keyed by the (address, shape, strides, device, ...) of one
    tensor or of several that can never answer for ANOTHER tensor: every entry
    holds a weak reference to each storage it was made from and is a hit only
    while every one of those very storages is alive and is the asking
    tensor's.  (An address alone is not an identity: the caching allocator
    hands the address of a dropped weight to the next one of the same shape,
    and a transposed view of a square weight shares address, version and
    shape with it.)  Entries of dead storages are dropped as they are met,
    and no entry keeps a tensor alive.  `tensors`: a tensor, or a tuple / list
    of tensors (`key((w,))` is `key(w)`, and `get` / `put` treat the two
    alike).  One lock for every instance.  (Relies on torch
    returning the SAME Python object from `tensor.untyped_storage()` for as
    long as the storage lives; on a torch that made a new object per call
    every lookup would miss - still correct, but the weight would be packed
    again on every call.)"""

    lock = threading.Lock()

    def __init__(self, size):
        self.size = size
        self.entries = collections.OrderedDict()

    @staticmethod
    def key(tensors, *more):
        # (one tensor, the case of every launch, without a loop; a
        # `torch.Size` hashes and compares as the tuple it is)
        if tensors.__class__ in (tuple, list):
            parts = []
            for tensor in tensors:
                parts += (tensor.data_ptr(), tensor.shape, tensor.stride(),
                          tensor.device)
            return (*parts, *more)
        return (tensors.data_ptr(), tensors.shape, tensors.stride(),
                tensors.device) + more

    def get(self, tensors, key):
        with self.lock:
            found = self.entries.get(key)
            if found is None:
                return None
            made = found[0]
            if tensors.__class__ in (tuple, list):
                hit = len(made) == len(tensors)
                for reference, tensor in zip(made, tensors):
                    hit = hit and reference() is tensor.untyped_storage()
            else:
                hit = len(made) == 1 and \
                    made[0]() is tensors.untyped_storage()
            if not hit:
                del self.entries[key]       # another tensor lived here
                return None
            self.entries.move_to_end(key)
            return found[1]

    def put(self, tensors, key, value):
        if tensors.__class__ not in (tuple, list):
            tensors = (tensors,)
        made = [weakref.ref(tensor.untyped_storage()) for tensor in tensors]
        with self.lock:
            self.entries[key] = (made, value)
            self.entries.move_to_end(key)
            while len(self.entries) > self.size:
                self.entries.popitem(last=False)
        return value


_device_packs = _ByStorage(256)
_first_versions = _ByStorage(256)
_host_convs = _ByStorage(32)
_layer_engines = _ByStorage(8)


def pack_index_tables(shape):
    """The `emph_take` tables of a [c_out, c_in, k] weight (host, int32; -1:
    zero): of the direct-form pack of the weight itself and of the pack of
    W'[ci][co][j] = W[co][ci][k - 1 - j], whose `emph_conv1d` is the data
    gradient."""
    indices = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    flipped = np.ascontiguousarray(indices.transpose(1, 0, 2)[:, :, ::-1])
    return (runtime.conv_pack_indices(indices).astype(np.int32),
            runtime.conv_pack_indices(flipped).astype(np.int32))


@functools.lru_cache(maxsize=32)
def _device_tables(shape, index):
    return tuple(torch.from_numpy(table).to(torch.device('cuda', index))
                 for table in pack_index_tables(shape))


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
    source = _float32(weight)
    if source.dim() == 2:
        first, last = rows or (0, source.shape[0])
        source = source[first:last].unsqueeze(2)
    table = _device_tables(tuple(source.shape), index)[1 if flipped else 0]
    pack = torch.empty(table.numel(), dtype=torch.float32, device=weight.device)
    _call('emph_take', source, table, pack, pack.numel())
    return _device_packs.put(weight, key, pack)


class _First:
    """The version a weight had when the op first saw it.  One object per
    entry of `_first_versions`, so its identity stands for the weight - this
    view of this live storage - in the key of what is made from it."""

    __slots__ = ('version',)

    def __init__(self, version):
        self.version = version


def _first(weight):
    """The `_First` of `weight`, made when the op first sees its storage."""
    key = _ByStorage.key(weight)
    return _first_versions.get(weight, key) or \
        _first_versions.put(weight, key, _First(weight._version))


def _weight_changes(weight):
    """Whether the version of `weight` has changed since the op first saw its
    storage: the weight is being trained (the op cannot see `requires_grad`
    below the autograd key)."""
    return _first(weight).version != weight._version


def mark_trained(tensors, base=None):
    """Tells the ops that `tensors` are weights in training although their
    versions have not moved yet - those of a trainer restored from a
    checkpoint, whose first forward must take the path its later ones take.
    Every tensor is shown to `_first` as an op will see it (the same address,
    shape, strides and storage); then its version is advanced once, or -
    `base`: a tensor whose counter all of them share as its views - that of
    `base` alone.  Nothing is launched.  RuntimeError where a tensor still
    looks untouched afterwards: it does not share `base`'s counter, or the
    tensors outgrow the cache of first versions (256 entries, shared with
    every other weight the ops have seen in the process)."""
    for tensor in tensors:
        _first(tensor)
    for tensor in (tensors if base is None else [base]):
        torch.autograd.graph.increment_version(tensor)
    changed = all([_weight_changes(tensor) for tensor in tensors])
    if not changed:
        raise RuntimeError(
            'mark_trained: a tensor does not share the version counter that '
            'was advanced, or the weights outgrow the cache of first versions')


def _host_conv(first, weight, bias, index):
    """`engine._Conv` of a weight that never changed (its packs made once on
    the host), kept per (weight, bias, versions, device).  `first` =
    `_first(weight)`, found in this call: the cache rule has just answered
    for the weight, whose version is `first.version`, so `first` enters the
    key in its place and the lookup asks the rule again for the bias alone."""
    key = _ByStorage.key(bias, first, bias._version, index)
    found = _host_convs.get(bias, key)
    if found is not None:
        return found
    return _host_convs.put(bias, key, engine_module._Conv(
        weight.detach().cpu().numpy(), bias.detach().cpu().numpy(),
        torch.device('cuda', index), winograd=True))


_LAYER_NAMES = ('self_attn.in_proj_weight', 'self_attn.in_proj_bias',
                'self_attn.out_proj.weight', 'self_attn.out_proj.bias',
                'norm1.weight', 'norm1.bias', 'linear1.weight', 'linear1.bias',
                'linear2.weight', 'linear2.bias', 'norm2.weight', 'norm2.bias')


def _layer_engine(tensors, index, channels, heads):
    """The fused inference `Engine` of one encoder layer whose twelve
    `tensors` never changed, kept per (their storages, versions, device,
    channels, heads)."""
    key = _ByStorage.key(tensors, *[tensor._version for tensor in tensors],
                         index, channels, heads)
    found = _layer_engines.get(tensors, key)
    if found is not None:
        return found
    config = cfg.Config(architecture='transformer', layers=1, channels=channels,
                        heads=heads)
    state = weights_module.random_state(config, seed=0)
    for name, tensor in zip(_LAYER_NAMES, tensors):
        state['frame_encoder.model.layers.0.' + name] = np.ascontiguousarray(
            tensor.detach().cpu().numpy(), dtype=np.float32)
    return _layer_engines.put(
        tensors, key, engine_module.Engine(config, state, index))
