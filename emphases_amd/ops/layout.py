"""The layouts the ops of one batch share: prefix sums to counts, the
`batch.Plan` of featurised segments and of audio chunks, `_Layout` (a plan with
its device metadata, tile tables and column indices) and the small LRUs that
keep them per batch."""
import collections
import threading

import numpy as np
import torch

from .. import batch
from .. import config as cfg
from .. import packed
from .. import runtime

GRAD_TILE = 64       # emph_conv_weight_grad_any, emph_segment_reduce_backward
DIRECT_TILE = 64     # emph_conv1d of the device-packed path and of the data gradient
SPLIT_TILE = 256     # emph_attention_split, emph_attention_backward_split
PLAN_CACHE_SIZE = 16


def _counts(cu):
    """Per-segment counts (python ints) of a prefix-sum tensor."""
    values = cu.detach().cpu().to(torch.int64).numpy()
    if values.ndim != 1 or values.size < 1 or values[0] != 0 or \
            np.any(np.diff(values) < 0):
        raise ValueError('cu_* must be non-decreasing prefix sums that start at 0')
    return np.diff(values).astype(np.int64), values


def _device_index(tensor):
    if not tensor.is_cuda:
        raise runtime.LibraryError(
            'emphases_amd ops run on an MI355X / HIP device only (no CPU '
            'fallback): the tensor is on ' + str(tensor.device))
    return tensor.device.index


def _own_bounds(count, words, bounds):
    """The `bounds` columns of each of `count` segments ([2, 0] without words)."""
    if words is None:
        return [np.zeros((2, 0), dtype=np.int64)] * count
    cuts = np.concatenate([[0], np.cumsum(words)]).astype(np.int64)
    return [bounds[:, first:last] for first, last in zip(cuts[:-1], cuts[1:])]


_frame_plan = batch.frame_plan


def _chunk_plan(samples, edges, words=None, bounds=None,
                source='mels.py:31-36'):
    """`batch.Plan` of N audio chunks back to back (a chunk = an utterance
    whose one segment starts behind the zero padding), `words[i]` words with
    `bounds` in each; F_i = 1 + (S_i - 160) // 160 frames.  `source`: what the
    refusal of a chunk too short for the reflect padding cites."""
    if np.any(samples <= cfg.PADDING):
        raise ValueError(f'a chunk needs more than 432 samples ({source})')
    counts = [0] * len(samples) if words is None else words
    segments = [
        batch.Segment(
            index, 0, int(count), cfg.PADDING, int(length),
            1 + (int(length) + 2 * cfg.PADDING - cfg.NUM_FFT) // cfg.HOPSIZE,
            own)
        for index, (length, count, own) in enumerate(zip(
            samples, counts, _own_bounds(len(samples), words, bounds)))]
    return batch.Plan(segments, edges[:-1], samples)


_columns = packed.columns


class _Layout:
    """What the ops of one batch share: the `batch.Plan`, its integer metadata
    on the device (name -> (view, size)), the frame tile tables (each uploaded
    when an op first asks for its width, so a plan costs no more to build
    than it did per call) and the device column indices of the scatter and
    the gather."""

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

    def tiles(self, tile, select=()):
        """(device tile table of the frame axis `tile` wide, its rows);
        `select` = (least, most) positions: of the segments of that size."""
        key = ('tiles', runtime.AXIS_FRAMES, tile) + tuple(select)
        if key not in self.meta:
            host = np.ascontiguousarray(
                self.plan.tiles(runtime.AXIS_FRAMES, tile, *select)).ravel()
            self.meta[key] = (
                torch.from_numpy(host).to(self.buffer.device), host.size)
        tiles, size = self.meta[key]
        return tiles, size // runtime.TILE_FIELDS

    def key_counts(self, counts, check=None):
        """The int32 device table of `counts` (int64 host array, one per
        segment) that `emph_attention` indexes by `Tile.segment`.  The layout
        keeps its LAST table alone (a layer's forward, the layers behind it
        and their backwards ask for the same one; a training loop brings a
        new one with nearly every batch): `check(counts)` runs and the table
        is uploaded only when the values differ from the kept ones."""
        key = counts.tobytes()
        kept = self.meta.get('key_counts')
        if kept is None or kept[1] != key:
            if check is not None:
                check(counts)
            host = np.ascontiguousarray(counts, dtype=np.int32)
            kept = (torch.from_numpy(host).to(self.buffer.device), key)
            self.meta['key_counts'] = kept
        return kept[0]

    scatter = staticmethod(packed.scatter)


class _Recent:
    """A small LRU of what `make()` gives for a key (made outside the lock: a
    refusal caches nothing, and two threads may both make one)."""

    lock = threading.Lock()

    def __init__(self, size):
        self.size = size
        self.entries = collections.OrderedDict()

    def get(self, key, make):
        with self.lock:
            found = self.entries.get(key)
            if found is not None:
                self.entries.move_to_end(key)
                return found
        found = make()
        with self.lock:
            self.entries[key] = found
            while len(self.entries) > self.size:
                self.entries.popitem(last=False)
        return found


_layouts = _Recent(PLAN_CACHE_SIZE)
_logmel_plans = _Recent(PLAN_CACHE_SIZE)


def _layout(device, frames, words=None, bounds=None):
    """The `_Layout` of segments of `frames[i]` positions (and `words[i]` words
    with `bounds`), from a small LRU keyed by the VALUES of the arrays."""
    key = (device.index, frames.tobytes(),
           None if words is None else (words.tobytes(), bounds.tobytes()))
    return _layouts.get(
        key, lambda: _Layout(_frame_plan(frames, words, bounds), device))


def _logmel_plan(cu_samples, device):
    """(the chunk plan of `cu_samples`, its device frame columns), from a
    small LRU keyed by the values of `cu_samples`: the forward and its
    backward share one."""
    samples, edges = _counts(cu_samples)

    def make():
        plan = _chunk_plan(
            samples, edges, source='reflect padding, mels.py:31-36')
        return plan, _columns(plan.frame_off, plan.frames, device)
    return _logmel_plans.get((device.index, edges.tobytes()), make)
