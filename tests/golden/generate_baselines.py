"""Capture golden vectors of the reference's variance baselines.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_baselines.py

Imports the UNMODIFIED reference `emphases` with the stand-ins of
`tests/golden/stubs/` (as `generate.py` does), replaces `penn.from_audio` with
a deterministic pitch stand-in (the pitch row of a case, looked up by the
number of samples it is handed) and drives
`emphases.baselines.pitch_variance.infer` and
`emphases.baselines.duration_variance.infer` with duck-typed alignments that
carry phonemes.

Output (committed; inputs and outputs only): tests/golden/baselines.npz
  pv_frames   int64 [U]        pitch frames per utterance (audio = 160 x frames
                               samples at 16 kHz; all different)
  pv_pitch    float32 [sum F]  the stand-in's pitch rows in Hz, back to back
  pv_words    int64 [U]        words per utterance
  pv_times    float64 [W, 2]   (start, end) seconds of every word
  pv_scores   float32 [W]      infer(...)[0] of every utterance, back to back
  dv_words    int64 [V]        words per alignment
  dv_times    float64 [X, 2]   word times
  dv_labels   str [X]          word labels ('<silent>' for silences)
  dv_phonemes int64 [X]        phonemes per word
  dv_phone_times float64 [P, 2]  phoneme times (equal parts of their word)
  dv_scores   float32 [X]      infer(alignment)[0], back to back
The GPU box never runs this script; it only reads the .npz file.
"""
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = '/root/reference'
sys.path[:0] = [os.path.join(HERE, 'stubs'), REFERENCE, ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases  # noqa: E402  (the reference)
import penn  # noqa: E402  (stand-in)

torch.set_num_threads(1)
SILENCE = '<silent>'


class Phoneme:
    def __init__(self, start, end):
        self._start, self._end = float(start), float(end)

    def start(self):
        return self._start

    def end(self):
        return self._end


class Word:
    """pypar.Word's accessors the baselines read: times and len() = phonemes"""

    def __init__(self, label, start, end, phonemes=0):
        self.label = label
        self._start, self._end = float(start), float(end)
        step = (self._end - self._start) / max(phonemes, 1)
        self.phonemes = [
            Phoneme(self._start + k * step,
                    self._end if k == phonemes - 1 else
                    self._start + (k + 1) * step)
            for k in range(phonemes)]

    def __len__(self):
        return len(self.phonemes)

    def start(self):
        return self._start

    def end(self):
        return self._end

    def duration(self):
        return self._end - self._start


class Alignment:
    def __init__(self, words):
        self._words = list(words)

    def __iter__(self):
        return iter(self._words)

    def __len__(self):
        return len(self._words)

    def start(self):
        return self._words[0].start()

    def end(self):
        return self._words[-1].end()

    def duration(self):
        return self.end() - self.start()

    def phonemes(self):
        return [p for word in self._words for p in word.phonemes]


###############################################################################
# Pitch variance
###############################################################################


def pitch_row(rng, frames, kind):
    """float32 Hz: a wandering contour, quantised (ties), or with 0 Hz
    frames / a NaN."""
    steps = rng.normal(0., 0.03, frames).cumsum()
    row = 150. * np.exp2(steps - steps.mean() + rng.normal(0., 0.05, frames))
    row = np.clip(row, 45., 540.)
    if kind == 'ties':
        row = np.array([100., 125., 150., 200.])[rng.integers(0, 4, frames)]
    elif kind == 'zeros':
        row[rng.choice(frames, frames // 10, replace=False)] = 0.
        row[40:52] = 0.
    elif kind == 'nan':
        row[frames // 3] = np.nan
    return row.astype(np.float32)


def words_over(rng, first, last, low, high):
    """Word times (seconds, frames / 100) tiling frames [first, last)."""
    edges = [first]
    while edges[-1] < last:
        edges.append(min(last, edges[-1] + int(rng.integers(low, high + 1))))
    return [(a / 100., b / 100.) for a, b in zip(edges[:-1], edges[1:])]


def pitch_cases():
    rng = np.random.default_rng(20260115)
    cases = [
        (1, 'plain', [(0., .01)]),
        (2, 'plain', [(0., .01), (.01, .02)]),
        (3, 'plain', [(0., .02), (.02, .03)]),
        (64, 'plain', words_over(rng, 5, 64, 1, 9)),      # starts at 0.05 s
        (65, 'ties', words_over(rng, 0, 65, 1, 12)),
        (1023, 'plain', words_over(rng, 0, 1023, 1, 60)),
        (1024, 'ties', words_over(rng, 3, 1024, 20, 90)),
        (1025, 'plain', words_over(rng, 0, 1025, 2, 40)),
        (30000, 'plain', words_over(rng, 0, 30000, 15, 120)),
        # the float floor of convert.seconds_to_frames at 8.03 s and 16.06 s
        (1700, 'plain', [(0., 8.03), (8.03, 16.06), (16.06, 17.)]),
        # the last word runs past the end of the pitch
        (500, 'plain', words_over(rng, 0, 480, 10, 40) + [(4.8, 6.)]),
        (300, 'zeros', words_over(rng, 0, 300, 1, 30)),
        (301, 'nan', words_over(rng, 0, 301, 5, 40)),
    ]
    return [(frames, pitch_row(rng, frames, kind), words)
            for frames, kind, words in cases]


def capture_pitch(out):
    cases = pitch_cases()
    rows = {frames: row for frames, row, _ in cases}
    assert len(rows) == len(cases)

    def from_audio(audio, sample_rate, **kwargs):
        assert sample_rate == 16000 and audio.shape[-1] % 160 == 0
        pitch = torch.from_numpy(rows[audio.shape[-1] // 160].copy())[None]
        return pitch, torch.ones_like(pitch)
    penn.from_audio = from_audio
    scores = []
    for frames, _, words in cases:
        alignment = Alignment([Word(f'w{i}', a, b)
                               for i, (a, b) in enumerate(words)])
        audio = torch.zeros(1, frames * 160)
        result = emphases.baselines.pitch_variance.infer(
            alignment, audio, 16000)
        assert result.dtype == torch.float32 and \
            result.shape == (1, len(words))
        scores.append(result[0].numpy())
    out['pv_frames'] = np.array([c[0] for c in cases], dtype=np.int64)
    out['pv_pitch'] = np.concatenate([c[1] for c in cases])
    out['pv_words'] = np.array([len(c[2]) for c in cases], dtype=np.int64)
    out['pv_times'] = np.array(
        [t for c in cases for t in c[2]], dtype=np.float64)
    out['pv_scores'] = np.concatenate(scores).astype(np.float32)


###############################################################################
# Duration variance
###############################################################################


def duration_cases():
    rng = np.random.default_rng(20260116)
    alignments = []
    for index in range(24):
        count = int(rng.integers(1, 40))
        # every third alignment does not start at 0
        time = 0. if index % 3 else float(rng.uniform(0.05, 3.))
        words = []
        for k in range(count):
            silent = rng.random() < 0.2
            length = round(float(rng.uniform(0.03, 0.8)), 2 + k % 3)
            phonemes = 1 if silent else int(rng.integers(1, 6))
            words.append(Word(SILENCE if silent else f'w{k}', time,
                              time + length, phonemes))
            time += length
        alignments.append(Alignment(words))
    return alignments


def capture_duration(out):
    alignments = duration_cases()
    scores = [emphases.baselines.duration_variance.infer(a) for a in alignments]
    for alignment, result in zip(alignments, scores):
        assert result.dtype == torch.float32 and \
            result.shape == (1, len(alignment))
    words = [w for a in alignments for w in a]
    out['dv_words'] = np.array([len(a) for a in alignments], dtype=np.int64)
    out['dv_times'] = np.array([(w.start(), w.end()) for w in words],
                               dtype=np.float64)
    out['dv_labels'] = np.array([w.label for w in words])
    out['dv_phonemes'] = np.array([len(w) for w in words], dtype=np.int64)
    out['dv_phone_times'] = np.array(
        [(p.start(), p.end()) for w in words for p in w.phonemes],
        dtype=np.float64)
    out['dv_scores'] = np.concatenate([s[0].numpy() for s in scores])


def main():
    out = {}
    capture_pitch(out)
    capture_duration(out)
    path = os.path.join(HERE, 'baselines.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    leaked = [
        root for root, dirs, _ in os.walk(REFERENCE) if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
