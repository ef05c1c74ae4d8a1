"""Adversarial input for the log-mel / loudness front-end, and the scale its
error is measured on.  A plain module (no fixtures): imported by
tests/test_oracle.py (CPU) and tests/test_gpu_frontend.py (GPU).

Signals.  Generated from `synth.splitmix64` / `synth.uniform` and closed
forms, never stored.  Each is int16 PCM [S]; the float32 form is `pcm / 32768`
(exact).  They are what the broadband, 0.16-of-full-scale `synth.audio` is
not: the extremes of the input range, energy in one bin beside 512 quiet
ones, the three bins the real-FFT split treats by hand (0, 256, 512), and a
chirp under which every one of the 513 bins is the loudest of some frame.

Metric.  A log-domain tolerance means something else on every signal: float32
arithmetic itself moves the log-mel by 3e-7 on a Nyquist alternation and by
5.7e-4 on a full-scale tone between two bins, where quiet mel rows sit
beside the leakage of a loud one.  So the mel rows are compared in the
MAGNITUDE domain, on the scale of what a float32 transform of the frame can
deliver:

    e[row, f] = |m - m64| / (rowsum(basis)[row] * (||w x_f||_2 + 1e-3))

with m = exp(log-mel), m64 the float64 oracle's mel before the log, w the
float32 Hann and x_f the frame's 1024 samples (1e-3 = sqrt(1e-6), the floor
of the magnitude).  No cell is left out: the smallest possible mel,
rowsum * 1e-3 > 6e-5, is above the 1e-5 clamp.
"""
import numpy as np
import torch

from emphases_amd import synth
from oracle import prominence as oracle

FULL = 32767
FRAMES = 300            # of every signal but the chirp
CHIRP_FRAMES = 1500     # 513 bins / 1500 frames: every bin leads some frame


def _pcm(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _tone(bin_, samples, phase=0.3):
    n = np.arange(samples, dtype=np.float64)
    return _pcm(FULL * np.sin(2.0 * np.pi * bin_ * n / 1024.0 + phase))


def _synth(index):
    return _pcm(synth.audio(index, FRAMES)[0].astype(np.float64) * 32768.0)


def signals():
    """{name: int16 [S]} in a fixed order."""
    samples = FRAMES * 160
    n = np.arange(samples)
    out = {}
    out['silence'] = np.zeros(samples, dtype=np.int16)
    out['dc_max'] = np.full(samples, 32767, dtype=np.int16)
    out['dc_min'] = np.full(samples, -32768, dtype=np.int16)
    out['dc_lsb'] = np.full(samples, 1, dtype=np.int16)
    out['nyquist'] = np.where(n % 2 == 0, 32767, -32768).astype(np.int16)
    impulse = np.zeros(samples, dtype=np.int16)
    impulse[20011] = 32767
    out['impulse'] = impulse
    out['tone_bin64'] = _tone(64.0, samples)
    out['tone_bin256'] = _tone(256.0, samples)
    out['tone_between'] = _tone(64.5, samples)
    # 200 Hz: 80 samples a period
    out['square'] = np.where(n % 80 < 40, 32767, -32768).astype(np.int16)
    step = np.zeros(samples, dtype=np.int16)
    step[24017:] = 32767
    out['step'] = step
    out['noise_full'] = synth.integers(
        4101, samples, -32768, 32767).astype(np.int16)
    out['noise_lsb'] = synth.integers(4102, samples, -1, 1).astype(np.int16)
    # linear chirp 0 -> 8 kHz: frequency n / (2 S) cycles per sample
    long = CHIRP_FRAMES * 160
    m = np.arange(long, dtype=np.float64)
    out['chirp'] = _pcm(FULL * np.sin(2.0 * np.pi * 0.25 * m * m / long))
    out['synth61'] = _synth(61)
    out['synth9'] = _synth(9)          # the one with the 0.5 s hole
    return out


def as_float(pcm):
    """int16 [S] -> float32 [S], exactly pcm / 32768."""
    return pcm.astype(np.float32) / np.float32(32768.0)


def as_double(pcm):
    """int16 [S] -> float64 torch [1, S]: the oracle's input."""
    return torch.from_numpy(pcm.astype(np.float64) / 32768.0)[None]


###############################################################################
# the metric
###############################################################################


def frame_norms(audio):
    """||w x_f||_2 of every frame of a chunk: float64 [1, S] -> [F]."""
    frames = oracle.reflect_pad(audio).unfold(
        0, oracle.WINDOW_SIZE, oracle.HOPSIZE)
    return (frames * oracle.hann_window(torch.float64)).norm(dim=1)


def mel_scale(audio):
    """What one unit of `e` is, per cell: float64 [80, F]."""
    rowsum = oracle.mel_basis().double().sum(dim=1)
    return rowsum[:, None] * (frame_norms(audio)[None] + 1e-3)


def mel_of_log(logmel, normalize):
    """exp of the log-mel rows (any float dtype) in float64."""
    logmel = logmel.double()
    if normalize:
        logmel = logmel * 10. - 10.
    return torch.exp(logmel)


def mel_error(logmel, audio, normalize=False, want=None):
    """e[row, f] of log-mel rows [80, F] against the float64 oracle on
    `audio` (float64 [1, S]); `want`: the oracle's mel when the caller has
    it."""
    want = oracle.mel(audio) if want is None else want
    assert want.dtype == torch.float64 and logmel.shape == want.shape
    return (mel_of_log(logmel, normalize) - want).abs() / mel_scale(audio)


def decibels(row, normalize):
    """The loudness row in dB, float64."""
    row = row.double()
    return row * 100. - 100. if normalize else row


def floors(names=None):
    """The float32 restatement against the float64 one over the signal set:
    {(quantity, normalize): worst gap}, quantity in 'mel' (the metric above),
    'db' (loudness row, dB) and 'peak' (relative).  What float32 arithmetic
    needs on these signals; the device is held to a multiple of it."""
    worst = {}
    for name, pcm in signals().items():
        if names is not None and name not in names:
            continue
        single = torch.from_numpy(as_float(pcm))[None]
        double = as_double(pcm)
        want = oracle.mel(double)
        power = oracle.power(double)
        for normalize in (False, True):
            gaps = {
                'mel': float(mel_error(
                    oracle.logmel(single, normalize), double, normalize,
                    want).max()),
                'db': float((
                    decibels(oracle.loudness(single, normalize), normalize) -
                    oracle.loudness_of_power(power)).abs().max())}
            for key, gap in gaps.items():
                worst[key, normalize] = max(worst.get((key, normalize), 0.), gap)
        peak = float(power.max())
        if peak > 0.:
            worst['peak'] = max(
                worst.get('peak', 0.),
                abs(float(oracle.peak_power(single)) - peak) / peak)
    return worst


###############################################################################
# the multi-chunk loudness batch
###############################################################################

# (kind, frames) of one cycle.  Every chunk has a full-scale one on one side at
# least: its peak is 110 dB (the +-1 LSB noise) or more (silence: no peak at
# all) away from both neighbours', so a `top_db` floor taken from the chunk
# next door moves the row by tens of dB whichever way it leaks.  Two quiet
# chunks side by side would hide it: noise and silence floor each other's
# rows at -100 dB either way.  Chunks of 2..7 frames are shorter than one tile
# of the kernel; the loud ones among them are DC, not tones: the reflections
# at both ends of so short a tone fill every bin to within 80 dB of its peak,
# and a floor that drops moves nothing (tests/test_oracle.py measures all
# this).
BATCH_CYCLE = [('tone', 1203), ('lsb', 5), ('dc', 3), ('silence', 1001),
               ('tone', 900), ('lsb', 1500), ('dc', 7), ('silence', 2)]
BATCH_CYCLES = 8        # 4656 tiles of 8 frames: more than the 3072 resident
                        # waves, so waves loop and change chunk on the way


def batch_chunks(cycles=BATCH_CYCLES):
    """[(kind, int16 [S])] of the batch, in launch order.  Lengths are odd,
    so that chunks packed back to back start on odd samples too."""
    chunks = []
    for cycle in range(cycles):
        for index, (kind, frames) in enumerate(BATCH_CYCLE):
            number = cycle * len(BATCH_CYCLE) + index
            samples = 160 * frames + ((37 * number) % 160 | 1)
            samples = max(samples, 433)       # the least the reflect pad takes
            if kind == 'tone':
                pcm = _tone((64.0, 64.5, 256.0, 300.25)[number // 4 % 4],
                            samples, phase=0.1 * number)
            elif kind == 'dc':
                pcm = np.full(samples, (-32768, 32767)[cycle % 2], np.int16)
            elif kind == 'lsb':
                pcm = synth.integers(
                    4200 + number, samples, -1, 1).astype(np.int16)
            else:
                pcm = np.zeros(samples, dtype=np.int16)
            chunks.append((kind, pcm))
    return chunks


def frames_of(samples):
    """Frames of a chunk of `samples` samples (mels.py:31-48)."""
    return 1 + (samples + 864 - 1024) // 160
