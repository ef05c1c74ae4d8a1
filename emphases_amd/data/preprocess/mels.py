"""`emphases/data/preprocess/mels.py:16-59` on the HIP front-end
(`emph_logmel`: reflect padding, STFT(1024, hop 160, periodic Hann),
magnitude, `librosa.filters.mel` basis, log - one kernel)."""
import dataclasses

import torch

from ... import core
from . import core as preprocess


def from_audio(audio):
    """Compute the log-mel spectrogram of audio [1, S] (16 kHz): float32
    [80, F], on the device the audio is on (a host tensor is featurised on the
    current HIP device and comes back on the host).  `NORMALIZE` of the active
    configuration applies (`mels.py:56-58`).

    A float device tensor that requires grad gives a differentiable result (as
    the reference's ATen ops do): it goes through `ops.logmel`, whose bits are
    those of the path without grad and whose backward is
    `emph_logmel_backward`.  Under `normalize=True` that raises
    NotImplementedError: the op has no such argument."""
    active = core.active_config()
    if torch.is_floating_point(audio) and audio.requires_grad:
        if active.normalize:
            raise NotImplementedError(
                'mels.from_audio of an audio that requires grad does not '
                'support normalize=True: the differentiable path is '
                'ops.logmel, which has no normalize argument')
        if audio.is_cuda:
            return _differentiable(audio)
    config = dataclasses.replace(
        active, mel_feature=True, pitch_feature=False,
        periodicity_feature=False, loudness_feature=False)
    result, _ = preprocess.features(audio, None, config)
    return result if audio.is_cuda else result.cpu()


def _differentiable(audio):
    from ... import ops
    if audio.dim() == 2:
        audio = audio[0]                        # channel 0 only (mels.py:48)
    if audio.dim() != 1:
        raise ValueError('audio must be [1, samples] or [samples]')
    samples = int(audio.shape[0])
    if samples <= preprocess.cfg.PADDING:
        raise preprocess.too_short(samples)
    return ops.logmel(audio.to(torch.float32),
                      torch.tensor([0, samples], dtype=torch.int64))


def from_file(audio_file):
    """Load audio and compute its log-mel spectrogram [80, F] (`mels.py` `from_file`)."""
    from ... import load
    return from_audio(load.audio(audio_file))


def from_file_to_file(audio_file, output_file):
    """`from_file`, saved to `output_file` (its directory is created)."""
    from_files_to_files([audio_file], [output_file])


def from_files_to_files(audio_files, output_files, gpu=None):
    """The log-mel spectrogram [80, F] of many files, saved to disk: the batched path
    (`data.preprocess.from_files_to_files`)."""
    preprocess.from_files_to_files(
        audio_files, mel_files=list(output_files), gpu=gpu)
