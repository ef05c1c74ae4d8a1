"""The shared pieces of the host path, without a device: the run finder of
the staging code (`session.runs`), the aligned placement of a batch's files
(`files.aligned_placement`) and the one builder of a plan of featurised
segments (`batch.frame_plan`, reached through `core._packed_plan` and
`ops._frame_plan`)."""
import numpy as np
import pytest
import torch

from emphases_amd import core as api
from emphases_amd import files, ops, session


def _aligned(nbytes):
    """4-byte aligned back-to-back offsets, one entry at a time."""
    where, cursor = [], 0
    for n in nbytes:
        where.append(cursor)
        cursor += -(-n // 4) * 4
    return where


RUN_CASES = {
    'contiguous': ([0, 400, 1000, 1004], [400, 600, 4, 96]),
    # odd counts of 16-bit samples, placed 4-byte aligned: a gap of two bytes
    # behind every entry
    'gap_after_every_entry': (
        _aligned([2 * 48001, 2 * 31999, 2 * 80003]),
        [2 * 48001, 2 * 31999, 2 * 80003]),
    'gap_in_the_middle': ([0, 100, 300, 350, 400], [100, 100, 50, 50, 8]),
    'one_entry': ([12], [40]),
    'no_entry': ([], []),
    'out_of_address_order': ([500, 0, 100, 400, 300], [100, 100, 200, 100, 100]),
}


@pytest.mark.parametrize('name', list(RUN_CASES))
def test_runs_cover_every_entry_once_and_are_maximal(name):
    where, nbytes = RUN_CASES[name]
    first, last = session.runs(where, nbytes)
    # brute force: walk the entries, start a new run wherever the next entry
    # does not begin at the byte the one in front of it ends at
    expect = []
    for k in range(len(where)):
        if k and where[k] == where[k - 1] + nbytes[k - 1]:
            expect[-1][1] = k + 1
        else:
            expect.append([k, k + 1])
    assert [list(pair) for pair in zip(first.tolist(), last.tolist())] == expect
    # every entry in exactly one run, the runs in order
    covered = [k for lo, hi in zip(first, last) for k in range(lo, hi)]
    assert covered == list(range(len(where)))
    for lo, hi in zip(first.tolist(), last.tolist()):
        # a run is back to back inside ...
        for k in range(lo + 1, hi):
            assert where[k] == where[k - 1] + nbytes[k - 1]
        # ... and maximal: the entry behind it does not continue it
        if hi < len(where):
            assert where[hi] != where[hi - 1] + nbytes[hi - 1]
    if name == 'gap_after_every_entry':
        assert len(first) == 3
    if name == 'contiguous':
        assert len(first) == 1


def test_runs_in_two_address_spaces_break_where_either_does():
    """Source and destination at once: three files back to back in the
    pinned buffer whose places in the batch are 0, 2 and 3."""
    nbytes = [100, 60, 40]
    source = [0, 100, 160]
    target = [0, 500, 560]
    first, last = session.runs(np.stack([source, target], axis=1), nbytes)
    assert first.tolist() == [0, 1] and last.tolist() == [1, 3]


def test_aligned_placement_matches_audio_bytes():
    nbytes = [0, 1, 2, 3, 4, 96002]
    where, total = files.aligned_placement(nbytes)
    assert where.dtype == np.int64 and len(where) == len(nbytes)
    assert all(offset % 4 == 0 for offset in where.tolist())
    ends = where + np.asarray(nbytes)
    assert np.all(ends[:-1] <= where[1:])            # no overlap, in order
    assert total >= int(ends[-1]) and total % 4 == 0
    # what `FileBatch.audio_bytes` reports for files of these data sizes
    # (mono 16-bit PCM headers, every file readable)
    opened = files.FileBatch.__new__(files.FileBatch)
    opened.sizes = np.zeros((len(nbytes), 12), dtype=np.int64)
    opened.sizes[:, 5], opened.sizes[:, 6], opened.sizes[:, 8] = 1, 1, 16
    opened.sizes[:, 10] = nbytes
    opened._handle = None
    assert bool(opened.native_audio().all())
    assert total == opened.audio_bytes() == 0 + 4 + 4 + 4 + 4 + 96004
    empty, nothing = files.aligned_placement([])
    assert len(empty) == 0 and nothing == 0


def test_native_header_scalar_and_array_forms_agree():
    headers = [(1, 1, 16), (3, 1, 32), (1, 2, 16), (1, 1, 24), (3, 1, 64),
               (1, 1, 8), (3, 2, 32)]
    want = [True, True, False, False, False, False, False]
    assert [bool(files.native_header(*header)) for header in headers] == want
    code, channels, bits = np.array(headers).T
    assert files.native_header(code, channels, bits).tolist() == want


@pytest.mark.parametrize('with_words', [True, False])
def test_packed_plan_and_frame_plan_are_one_builder(with_words):
    frames = [5, 1, 64, 65]
    words = [2, 1, 3, 0] if with_words else [0, 0, 0, 0]
    width = max(max(words), 1)
    padded = np.full((len(frames), 2, width), -7, dtype=np.int64)
    own = []
    for index, (count, length) in enumerate(zip(frames, words)):
        edges = np.linspace(0, count, length + 1).astype(np.int64)
        bounds = np.stack([edges[:-1], edges[1:]])
        padded[index, :, :length] = bounds
        own.append(bounds)
    through_api = api._packed_plan(frames, torch.from_numpy(padded), words)
    if with_words:
        through_ops = ops._frame_plan(
            np.asarray(frames, dtype=np.int64),
            np.asarray(words, dtype=np.int64), np.concatenate(own, axis=1))
    else:
        through_ops = ops._frame_plan(np.asarray(frames, dtype=np.int64))
    for name in ('table', 'frame_off', 'word_off'):
        assert np.array_equal(
            getattr(through_api, name), getattr(through_ops, name)), name
    assert through_api.ld_frames == through_ops.ld_frames
    assert through_api.ld_words == through_ops.ld_words
    assert np.array_equal(through_api.bounds, through_ops.bounds)
    assert np.array_equal(through_api.word_segment, through_ops.word_segment)
    # the layout itself: 16 leading columns, every segment on a multiple of 16
    assert through_api.frame_off.tolist() == [16, 32, 48, 112]
    assert through_api.ld_frames == 16 + 16 + 16 + 64 + 80 + 128
    assert [s.frames for s in through_api.segments] == frames
    assert [s.bounds.shape[1] for s in through_api.segments] == words
