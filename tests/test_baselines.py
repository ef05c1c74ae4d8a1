"""The METHOD switch and the host side of the variance baselines (no GPU).

Goldens: tests/golden/baselines.npz (tests/golden/generate_baselines.py, the
unmodified reference's `baselines.*.infer`)."""
import os

import numpy as np
import pytest
import torch

import emphases_amd
from emphases_amd import Config, alignment as alignment_module
from emphases_amd.baselines import duration_variance, pitch_variance

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'baselines.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as data:
        return {key: data[key] for key in data.files}


def split(values, counts):
    edges = np.concatenate([[0], np.cumsum(counts)])
    return [values[a:b] for a, b in zip(edges[:-1], edges[1:])]


def duration_alignments(golden):
    """emphases_amd Alignments of the golden duration cases, phonemes
    attached."""
    phones = iter(golden['dv_phone_times'])
    alignments = []
    for labels, times, counts in zip(
            split(golden['dv_labels'], golden['dv_words']),
            split(golden['dv_times'], golden['dv_words']),
            split(golden['dv_phonemes'], golden['dv_words'])):
        words = []
        for label, (a, b), count in zip(labels, times, counts):
            phonemes = [alignment_module.Phoneme('p', *next(phones))
                        for _ in range(int(count))]
            words.append(alignment_module.Word(str(label), a, b, phonemes))
        alignments.append(alignment_module.Alignment(words))
    return alignments


def test_method_values():
    assert Config().method == 'neural'
    for method in ('neural', 'pitch-variance', 'duration-variance',
                   'prominence'):
        assert Config(method=method).method == method
    with pytest.raises(ValueError) as error:
        Config(method='loudness')
    assert str(error.value) == \
        'Emphasis annotation method loudness is not defined'
    with pytest.raises(ValueError):
        emphases_amd.configure(method='wavelet')
    assert emphases_amd.active_config().method == 'neural'


def test_prominence_raises_at_call_time():
    config = Config(method='prominence')         # accepted ...
    alignment = emphases_amd.Alignment.from_frames(np.array([[0], [10]]))
    with pytest.raises(NotImplementedError) as error:  # ... refused when run
        emphases_amd.from_alignments_and_audios(
            [alignment], [torch.zeros(1, 1600)], config=config)
    assert 'pycwt' in str(error.value) and 'gaussian' in str(error.value)


def test_duration_variance_bitwise(golden):
    alignments = duration_alignments(golden)
    want = split(golden['dv_scores'], golden['dv_words'])
    got = duration_variance.from_alignments(alignments)
    for a, b in zip(got, want):
        assert a.dtype == torch.float32 and a.shape == (1, len(b))
        assert np.array_equal(a[0].numpy().view(np.int32), b.view(np.int32))
    # the tensor API under the switch: host tensors for gpu=None, no GPU used
    api = emphases_amd.from_alignments_and_audios(
        alignments, [None] * len(alignments),
        config=Config(method='duration-variance'))
    for a, b in zip(api, got):
        assert not a.is_cuda and torch.equal(a, b)
    # the reference's importable name, one alignment at a time
    for alignment, b in zip(alignments, want):
        one = emphases_amd.baselines.duration_variance.infer(alignment)
        assert np.array_equal(one[0].numpy().view(np.int32), b.view(np.int32))


def test_duration_variance_errors(golden):
    bare = emphases_amd.Alignment.from_frames(np.array([[0, 10], [10, 30]]))
    with pytest.raises(ValueError, match='phoneme tier'):
        duration_variance.infer(bare)
    alignment = duration_alignments(golden)[0]
    words = alignment.words()
    words[0] = alignment_module.Word('w', words[0].start(), words[0].end(), [])
    with pytest.raises(ZeroDivisionError):
        duration_variance.infer(alignment_module.Alignment(words))


def test_duration_variance_files(golden, tmp_path):
    """TextGrids with a phones tier through from_files_to_files (the library's
    tables) and the command line's switch: the golden bits."""
    alignments = duration_alignments(golden)[:6]
    want = split(golden['dv_scores'], golden['dv_words'])
    texts, waves, prefixes = [], [], []
    from emphases_amd import load
    for index, alignment in enumerate(alignments):
        text = tmp_path / f'u{index}.TextGrid'
        wave = tmp_path / f'u{index}.wav'
        alignment.save(str(text))
        load.save_wav(str(wave), np.zeros((1, 1600), np.float32), 16000)
        texts.append(str(text))
        waves.append(str(wave))
        prefixes.append(str(tmp_path / f'out{index}'))
    previous = emphases_amd.active_config()
    emphases_amd.configure(method='duration-variance')
    try:
        emphases_amd.from_files_to_files(texts, waves, prefixes,
                                         utterances_per_batch=4)
    finally:
        emphases_amd.configure(previous)
    for prefix, b in zip(prefixes, want):
        got = torch.load(f'{prefix}.pt')
        assert np.array_equal(got[0].numpy().view(np.int32), b.view(np.int32))
        # the TextGrid goes back out with its phones tier
        again = emphases_amd.Alignment(f'{prefix}.TextGrid')
        assert all(word.phonemes for word in again)


def test_pitch_variance_segment_table(golden):
    """Word rows use the reference's float floor on absolute seconds and
    Python's slice clamping; an empty slice raises torch's error before any
    launch."""
    frames = golden['pv_frames']
    times = split(golden['pv_times'], golden['pv_words'])
    table = pitch_variance.segment_table(times, frames)
    offsets = np.concatenate([[0], np.cumsum(frames)])
    row = 0
    for u, (t, n) in enumerate(zip(times, frames)):
        for start, end in t:
            a = int((start * 16000) // 160)
            b = int((end * 16000) // 160)
            span = range(int(n))[a:b]
            assert table[row].tolist() == [
                offsets[u] + span.start, len(span), len(golden['pv_times']) + u]
            row += 1
    assert table[row:].tolist() == [
        [int(offsets[u]), int(n), -1] for u, n in enumerate(frames)]
    # 8.03 s and 16.06 s floor below the rounded frame
    assert int((8.03 * 16000) // 160) == 802
    with pytest.raises(RuntimeError, match='must be non-empty'):
        pitch_variance.segment_table([np.array([[0., .005]])], [10])
    with pytest.raises(RuntimeError, match='must be non-empty'):
        pitch_variance.segment_table([np.array([[.2, .3]])], [10])
