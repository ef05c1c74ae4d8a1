"""The paper's baselines behind the reference's `METHOD` switch
(`emphases/core.py:244-287`, `config/baselines/*.py`): `Config.method` picks
them, and every entry point that takes a `Config` dispatches here.

    'pitch-variance'      `pitch_variance`: exact quantile spreads of log2
                          pitch on the device (`emph_quantile_spreads`)
    'duration-variance'   `duration_variance`: host arithmetic over the
                          phoneme tier, vectorised over the batch
    'prominence'          the wavelet (CWT / LoMA) baseline: not provided

A baseline builds no model and loads no checkpoint; `batch_size`,
`checkpoint`, `precision` and `conv_tile` do not apply to it (the reference
ignores them too).  Scores are float32 [1, W] per utterance, every word
scored, on the device when `gpu` is given and on the host otherwise.
"""
import numpy as np
import torch

from . import duration_variance  # noqa: F401
from . import pitch_variance  # noqa: F401

BASELINES = ('pitch-variance', 'duration-variance', 'prominence')


def require(method):
    """Raise for a method that cannot run here."""
    if method == 'prominence':
        raise NotImplementedError(
            "METHOD = 'prominence' (the wavelet / LoMA baseline, "
            'emphases/baselines/prominence) is not provided: it needs the '
            'third-party `pycwt`, which is not installed, and '
            '`scipy.signal.gaussian`, which SciPy 1.13 removed, so the '
            "reference's own baseline does not run on this software stack "
            'either')


def from_alignments_and_audios(method, alignments, audios, sample_rate, gpu,
                               pitch_tracker=None):
    """Scores of a batch under a baseline `method`: a list of float32
    tensors [1, W_u] (on the device if `gpu` is not None)."""
    require(method)
    if method == 'duration-variance':
        return duration_variance.from_alignments(alignments, gpu)
    return pitch_variance.from_alignments_and_audios(
        alignments, audios, sample_rate, gpu, pitch_tracker)


def files_to_scores(method, text_files, audio_files, gpu=None,
                    utterances_per_batch=256, deliver_batch=None,
                    pitch_tracker=None):
    """The file loop of `core.files_to_scores` for a baseline: batches of
    `utterances_per_batch` files opened by the library (`files.FileBatch`),
    scored, and handed to `deliver_batch(opened, local indices, global
    indices, scores)` with the scores on the host."""
    from .. import files
    require(method)
    text_files, audio_files = list(text_files), list(audio_files)
    for first in range(0, len(text_files), utterances_per_batch):
        last = min(first + utterances_per_batch, len(text_files))
        opened = files.FileBatch(text_files[first:last],
                                 audio_files[first:last])
        try:
            if method == 'duration-variance':
                scores = duration_variance.from_file_batch(opened)
            else:
                scores = _pitch_variance_files(opened, gpu, pitch_tracker)
            deliver_batch(opened, range(opened.count), range(first, last),
                          scores)
        finally:
            opened.close()


def _pitch_variance_files(opened, gpu, pitch_tracker):
    """Scores of a `FileBatch`, one call per sample rate."""
    times = opened.all_times()
    scores = [None] * opened.count
    for rate, chosen, audios in opened.rate_groups():
        results = pitch_variance.from_alignments_and_audios(
            [times[i] for i in chosen],
            [audio if torch.is_tensor(audio) else audio.tensor()
             for audio in audios], rate,
            None if gpu is None else gpu, pitch_tracker, on_device=False)
        for index, result in zip(chosen, results):
            scores[index] = result
    return scores


def dense(flat, counts):
    """Per-utterance [1, W_u] views of one dense row (`session.Scores`)."""
    from .. import session
    return list(session.Scores(flat[None], np.asarray(counts, np.int64)))
