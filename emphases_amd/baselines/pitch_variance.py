"""Pitch-variance baseline (`emphases/baselines/pitch_variance/core.py:12-53`).

Per utterance the reference tracks pitch once over the whole audio
(`penn.from_audio`, hop 10 ms), takes log2, and scores each word with
spread(word frames) - spread(all frames), spread(x) = torch.quantile(x, .95) -
torch.quantile(x, .05); the word's frames are pitch[0, start:end] with
start / end = int(seconds * 16000 // 160) of the word's ABSOLUTE times (the
float floor of `convert.seconds_to_frames`, not `Alignment.word_bounds`' rule)
and Python's slice clamping.

Here the tracker still runs once per utterance (the `pitch_tracker=` contract
of `core.from_alignments_and_audios`; default `penn`), the pitch rows go to the
device back to back, and ONE `emph_quantile_spreads` call computes every word
and utterance spread of the batch and the zero-centred scores (two launches,
no host sync between them).  The quantiles are bitwise torch.quantile's on
the same float32 values; log2 is taken on the device (`log2f`, within an ulp
of the CPU's).
"""
import numpy as np
import torch

from .. import config as cfg
from .. import runtime

EMPTY = 'quantile() input tensor must be non-empty'


def infer(alignment, audio, sample_rate, gpu=None, pitch_tracker=None):
    """`emphases.baselines.pitch_variance.infer`: float32 scores [1, W]."""
    return from_alignments_and_audios(
        [alignment], [audio], sample_rate, gpu, pitch_tracker)[0]


def word_times(alignment):
    """float64 [W, 2] (start, end) seconds of every word of an alignment
    object (or the array itself)."""
    if isinstance(alignment, np.ndarray):
        return alignment.reshape(-1, 2)
    if hasattr(alignment, 'times'):
        return alignment.times()
    return np.array([(word.start(), word.end()) for word in alignment],
                    dtype=np.float64).reshape(-1, 2)


def segment_table(times, frames):
    """int64 [W + U, 3] rows of `emph_quantile_spreads` for utterances with
    word times `times` (list of float64 [W_u, 2]) and `frames` pitch frames
    each, rows back to back: the W word rows (packed word order) name the row
    of their utterance, the U utterance rows follow.  Raises torch's
    RuntimeError for an empty slice (a word shorter than a frame, or one that
    starts past the end of the pitch) before anything is launched."""
    frames = np.asarray(frames, dtype=np.int64)
    counts = np.array([len(t) for t in times], dtype=np.int64)
    words, utterances = int(counts.sum()), len(frames)
    offsets = np.concatenate([[0], np.cumsum(frames)])
    if (frames < 1).any():
        raise RuntimeError(EMPTY)
    owner = np.repeat(np.arange(utterances), counts)
    table = np.empty((words + utterances, 3), dtype=np.int64)
    if words:
        seconds = np.concatenate([np.asarray(t, np.float64).reshape(-1, 2)
                                  for t in times])
        # convert.seconds_to_frames: (seconds * SAMPLE_RATE) // HOPSIZE, float64
        bounds = np.floor_divide(
            seconds * float(cfg.SAMPLE_RATE), float(cfg.HOPSIZE)).astype(np.int64)
        length = frames[owner]
        # pitch[0, start:end]: Python's slice clamping
        clamped = np.where(bounds < 0, np.maximum(bounds + length[:, None], 0),
                           np.minimum(bounds, length[:, None]))
        size = np.maximum(clamped[:, 1] - clamped[:, 0], 0)
        if (size == 0).any():
            raise RuntimeError(EMPTY)
        table[:words, 0] = offsets[owner] + clamped[:, 0]
        table[:words, 1] = size
        table[:words, 2] = words + owner
    table[words:, 0] = offsets[:-1]
    table[words:, 1] = frames
    table[words:, 2] = -1
    return table


def quantile_spreads(values, table, rows=0, transform=runtime.SPREAD_IDENTITY,
                     selected=False):
    """One `emph_quantile_spreads` call on the device tensor `values` (float32
    [ld]) with the host table `table` (int64 [S, 3], `segment_table`'s rows):
    returns (stats float32 [S, 3] = (quantile .05, quantile .95, spread),
    scores float32 [rows], the transformed values of the utterance rows
    float32 [ld] or None), all on `values`' device."""
    device = values.device
    values = values.reshape(-1).to(torch.float32).contiguous()
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
    ends = table[:, 0] + table[:, 1]
    if len(table) and ((table[:, 0] < 0) | (table[:, 1] < 1) |
                       (ends > values.numel())).any():
        raise ValueError('segment outside the packed axis, or empty')
    if len(table) and ((table[:rows, 2] < 0) |
                       (table[:rows, 2] >= len(table))).any():
        raise ValueError('a score row names no segment')
    with torch.cuda.device(device):
        segments = torch.from_numpy(table).pin_memory().to(
            device, non_blocking=True)
        stats = torch.empty((len(table), 3), dtype=torch.float32,
                            device=device)
        scores = torch.empty(max(rows, 1), dtype=torch.float32, device=device)
        chosen = torch.full_like(values, float('nan')) if selected else None
        runtime.check(runtime.library().emph_quantile_spreads(
            values.data_ptr(), values.numel(), segments.data_ptr(),
            len(table), transform, stats.data_ptr(),
            None if chosen is None else chosen.data_ptr(),
            scores.data_ptr() if rows else None, rows, runtime.stream()),
            'emph_quantile_spreads')
    return stats, scores[:rows], chosen


def _at_16k(audios, sample_rate, device):
    """1-D float32 host tensors at 16 kHz: the whole batch in one
    `emph_resample` launch (the resampler of `Session.resample`, without an
    engine: a baseline loads no model)."""
    from .. import load
    kernel, orig, new, width = load.resample_kernel(sample_rate)
    lengths = [int(audio.shape[0]) for audio in audios]
    targets = [load.resampled_length(n, orig, new) for n in lengths]
    source = np.cumsum([0] + lengths)
    target = np.cumsum([0] + targets)
    table = np.stack([source[:-1], lengths, target[:-1], targets],
                     axis=1).astype(np.int64)
    with torch.cuda.device(device):
        raw = torch.cat([audio.to(device) for audio in audios])
        out = torch.empty(max(int(target[-1]), 1), dtype=torch.float32,
                          device=device)
        rows = torch.from_numpy(table).to(device)
        taps = kernel.reshape(new, -1).contiguous().to(device)
        runtime.check(runtime.library().emph_resample(
            raw.data_ptr(), runtime.AUDIO_F32, rows.data_ptr(), len(lengths),
            max(targets + [0]), taps.data_ptr(), orig, new, width,
            out.data_ptr(), runtime.stream()), 'emph_resample')
        out = out.cpu()
    return list(out[:int(target[-1])].split(targets))


def from_alignments_and_audios(alignments, audios, sample_rate=cfg.SAMPLE_RATE,
                               gpu=None, pitch_tracker=None, on_device=None):
    """Pitch-variance scores of a batch: list of float32 [1, W_u] (on the
    device when `gpu` is given, else on the host; `on_device` overrides)."""
    from .. import core, session
    device = runtime.require_gpu(gpu)
    on_device = gpu is not None if on_device is None else on_device
    times = [word_times(alignment) for alignment in alignments]
    audios = [session.host_pcm_to_float(session.mono(audio))
              for audio in audios]
    if int(sample_rate) != cfg.SAMPLE_RATE:
        # (the reference hands `penn` the original rate, which resamples)
        audios = _at_16k(audios, sample_rate, device)
    tracker = pitch_tracker or core.penn_tracker(gpu)
    rows = [torch.as_tensor(tracker(audio.reshape(1, -1))[0]).reshape(-1)
            for audio in audios]
    frames = [int(row.numel()) for row in rows]
    table = segment_table(times, frames)
    words = int(sum(len(t) for t in times))
    with torch.cuda.device(device):
        if all(not row.is_cuda for row in rows):
            packed = np.concatenate(
                [row.numpy().astype(np.float32, copy=False) for row in rows])
            values = torch.from_numpy(packed).pin_memory().to(
                device, non_blocking=True)
        else:
            values = torch.cat([row.to(device, torch.float32) for row in rows])
        _, scores, _ = quantile_spreads(
            values, table, words, runtime.SPREAD_LOG2)
        scores = scores if on_device else scores.cpu()
    from . import dense
    return dense(scores, [len(t) for t in times])
