"""Duration-variance baseline (`emphases/baselines/duration_variance/core.py:
9-19`): a word's mean phoneme duration minus the utterance's,

    alignment.duration() / len(alignment.phonemes())      Python float64
    torch.tensor([word.duration() / len(word), ...])       rounded to float32
    (words - utterance)[None]                              float32: the float64
                                                           scalar is rounded to
                                                           float32 first

restated with numpy over a whole batch at once (the bits are the reference's:
the same float64 divisions, the same two roundings, one float32 subtraction).
No kernel: a few flops per word.  A word without phonemes raises
ZeroDivisionError as in the reference; an alignment without a phoneme tier
raises ValueError.
"""
import numpy as np
import torch

NO_TIER = ('duration-variance needs the phoneme tier of the alignment '
           '(a TextGrid "phones" tier, or "phonemes" in JSON): '
           'a word has no phonemes attached')


def infer(alignment):
    """`emphases.baselines.duration_variance.infer`: float32 CPU [1, W]."""
    return from_alignments([alignment])[0]


def phoneme_counts(alignment):
    """int64 [W] phonemes per word of an alignment object."""
    counts = []
    for word in alignment:
        phonemes = getattr(word, 'phonemes', None)
        if callable(phonemes):
            phonemes = phonemes()
        if phonemes is None:
            if not hasattr(word, '__len__'):
                raise ValueError(NO_TIER)
            counts.append(len(word))
        else:
            counts.append(len(phonemes))
    return np.array(counts, dtype=np.int64)


def scores(times, phonemes, words):
    """float32 [sum(words)] scores of utterances whose words have (start, end)
    seconds `times` (float64 [W, 2]) and `phonemes` phonemes each, `words[u]`
    words in utterance u, back to back."""
    words = np.asarray(words, dtype=np.int64)
    times = np.asarray(times, dtype=np.float64).reshape(-1, 2)
    phonemes = np.asarray(phonemes, dtype=np.int64)
    if (words < 1).any():
        # (an alignment without words has no phonemes either)
        raise ZeroDivisionError('division by zero')
    first = np.concatenate([[0], np.cumsum(words)[:-1]])
    last = first + words - 1
    # Alignment.duration() = end of the last word - start of the first
    total = np.add.reduceat(phonemes, first) if len(first) else phonemes[:0]
    if (total == 0).any() or (phonemes == 0).any():
        raise ZeroDivisionError('float division by zero')
    utterance = (times[last, 1] - times[first, 0]) / total
    word = (times[:, 1] - times[:, 0]) / phonemes
    owner = np.repeat(np.arange(len(words)), words)
    return word.astype(np.float32) - utterance.astype(np.float32)[owner]


def from_alignments(alignments, gpu=None):
    """Scores of a batch of alignment objects: list of float32 [1, W_u] (on
    the device when `gpu` is given)."""
    from . import dense
    times = [alignment.times() if hasattr(alignment, 'times') else
             np.array([(w.start(), w.end()) for w in alignment],
                      dtype=np.float64).reshape(-1, 2)
             for alignment in alignments]
    counts = [phoneme_counts(alignment) for alignment in alignments]
    words = [len(t) for t in times]
    flat = scores(np.concatenate(times) if times else np.zeros((0, 2)),
                  np.concatenate(counts) if counts else np.zeros(0, np.int64),
                  words)
    result = torch.from_numpy(flat)
    if gpu is not None:
        from .. import runtime
        result = result.to(runtime.require_gpu(gpu))
    return dense(result, words)


def from_file_batch(opened):
    """Scores of a `files.FileBatch` from the library's tables (word times,
    phonemes per word), nothing per word in Python; files the library did not
    parse (JSON alignments) are read as objects."""
    if (opened.status & 1).any():
        return from_alignments(
            [opened.alignment(i) for i in range(opened.count)])
    if (opened.sizes[:, 2] < 0).any():
        raise ValueError(NO_TIER)
    labels = opened.labels()
    words = opened.sizes[:, 1]
    # phone_word: the word of each phoneme, counted from its file's first word
    owner = np.repeat(opened.word_first[:-1], opened.sizes[:, 2]) + \
        labels['phone_word']
    phonemes = np.bincount(owner, minlength=int(words.sum()))
    from . import dense
    return dense(torch.from_numpy(scores(opened.times, phonemes, words)), words)
