"""The host path on the device: one `Session.submit` whose utterances come
from every kind of source at once, and the padded/packed adapter of the step
API (`packed.Padded`) against per-item calls."""
import struct

import numpy as np
import pytest
import torch

import emphases_amd
from emphases_amd import core as api
from emphases_amd import files, session as session_module, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def default_engine():
    return emphases_amd.get_engine()


def _save_float32(file, audio):
    """A mono float32 WAVE file (its `FileBatch` entry stays a `FileAudio`)."""
    body = np.asarray(audio, dtype='<f4').tobytes()
    header = b'RIFF' + struct.pack('<I', 36 + len(body)) + b'WAVEfmt ' + \
        struct.pack('<IHHIIHH', 16, 3, 1, 16000, 64000, 4, 32) + \
        b'data' + struct.pack('<I', len(body))
    with open(file, 'wb') as handle:
        handle.write(header + body)


# where utterance k of the mixed batch comes from
SOURCES = ['host', 'staged', 'device', 'unstaged', 'strided', 'staged',
           'staged', 'host']


@pytest.mark.parametrize('frames', [
    # 0.2 .. 1 s, all different: one piece
    [20, 100, 37, 64, 81, 55, 93, 46],
    # 6 x 45 s of float32 = 17.3 MB: from 16 MiB on the piece loop splits
    # (pieces == 2, the smallest shape at which a piece edge can go wrong)
    [4500] * 6,
], ids=['one_piece', 'two_pieces'])
def test_mixed_sources_in_one_submit(default_engine, tmp_path, frames):
    """Host tensor, staged file, device tensor, file still on disk (from a
    second `FileBatch`), strided host tensor, then two staged files that lie
    back to back in their pinned buffer (a run of two) and a host tensor: the
    scores are those of the same utterances as plain host tensors - three
    times over, so that the layout cache and the graph replay see the mixed
    staging too."""
    sources = SOURCES[:len(frames)]
    audios = [torch.from_numpy(synth.audio(800 + i, n))[0]
              for i, n in enumerate(frames)]
    aligns = [emphases_amd.Alignment.from_frames(
        synth.word_frames(800 + i, n)) for i, n in enumerate(frames)]
    waves = []
    for index, audio in enumerate(audios):
        waves.append(tmp_path / f'u{index}.wav')
        _save_float32(waves[-1], audio.numpy())
    session = session_module.Session(default_engine, depth=2)
    want = session.run(aligns, audios)

    staged = [k for k, source in enumerate(sources) if source == 'staged']
    unstaged = [k for k, source in enumerate(sources) if source == 'unstaged']
    first = files.FileBatch(None, [waves[k] for k in staged])
    second = files.FileBatch(None, [waves[k] for k in unstaged])
    try:
        from_first = [audio for audio, _ in first.all_audios()]
        from_second = [audio for audio, _ in second.all_audios()]
        assert all(type(audio) is files.FileAudio
                   for audio in from_first + from_second)
        with torch.cuda.device(default_engine.device):
            first.read_all(session.file_buffer(0, first.audio_bytes()))
        assert all(audio.staged is not None for audio in from_first)
        assert all(audio.staged is None for audio in from_second)
        if len(staged) == 3:
            # (float32: no alignment gap, the files lie back to back)
            assert from_first[2].staged == \
                from_first[1].staged + 4 * frames[staged[1]] * 160
        mixed = []
        for k, source in enumerate(sources):
            if source == 'host':
                mixed.append(audios[k].clone())
            elif source == 'device':
                mixed.append(audios[k].cuda())
            elif source == 'strided':
                wide = torch.zeros(2 * len(audios[k]))
                wide[::2] = audios[k]
                mixed.append(wide[::2])
                assert not mixed[-1].is_contiguous()
            elif source == 'staged':
                mixed.append(from_first[staged.index(k)])
            else:
                mixed.append(from_second[unstaged.index(k)])
        nbytes = 4 * 160 * sum(frames)
        assert max(1, min(4, nbytes // (8 << 20))) == \
            (2 if len(frames) == 6 else 1)
        for _ in range(3):
            got = session.submit(aligns, mixed).result()
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert a.shape == b.shape and torch.equal(a, b)
    finally:
        first.close()
        second.close()


def _padded_case():
    """B = 3 items of 7, 64 and 65 frames with 1, 3 and 2 words."""
    frames, words = [7, 64, 65], [1, 3, 2]
    bounds = torch.full((3, 2, 3), -1, dtype=torch.int64)
    for item, (count, length) in enumerate(zip(frames, words)):
        edges = np.linspace(0, count, length + 1).astype(np.int64)
        bounds[item, 0, :length] = torch.from_numpy(edges[:-1])
        bounds[item, 1, :length] = torch.from_numpy(edges[1:])
    return frames, words, bounds


def _nan_behind(values, lengths):
    """`values` [B, C, T] with NaN behind every item's own length."""
    values = values.clone()
    for item, length in enumerate(lengths):
        values[item, :, length:] = float('nan')
    return values


def _check_against_items(whole, alone, lengths):
    """`whole` [B, C, max]: finite, item i equal to its own B = 1 call
    `alone[i]` [1, C, lengths[i]], zeros behind."""
    assert whole.shape[0] == len(lengths) and whole.shape[2] == max(lengths)
    assert bool(torch.isfinite(whole).all())
    for item, length in enumerate(lengths):
        assert alone[item].shape == (1, whole.shape[1], length)
        assert torch.equal(whole[item:item + 1, :, :length], alone[item])
        assert not bool(whole[item, :, length:].any())


def test_downsample_never_touches_the_padding():
    """`downsample` takes no frame lengths: every item is planned T frames
    wide, so the NaN tail of the input IS packed and it is the word bounds
    that keep the kernel off it.  What this pins of the adapter is the output
    side - the word columns behind an item's length come back as zeros, the
    others are the item's own call's; `upsample` and `Model.forward` below
    pin the input side."""
    frames, words, bounds = _padded_case()
    xs = _nan_behind(torch.randn(
        (3, 5, 65), generator=torch.Generator().manual_seed(1)), frames).cuda()
    whole = api.downsample(xs, bounds.cuda(), torch.tensor(words))
    alone = [api.downsample(
        xs[i:i + 1, :, :frames[i]], bounds[i:i + 1, :, :words[i]].cuda(),
        torch.tensor(words[i:i + 1])) for i in range(3)]
    _check_against_items(whole, alone, words)


def test_upsample_never_touches_the_padding():
    frames, words, bounds = _padded_case()
    xs = _nan_behind(torch.randn(
        (3, 5, 3), generator=torch.Generator().manual_seed(2)), words).cuda()
    whole = api.upsample(
        xs, bounds.cuda(), torch.tensor(words), torch.tensor(frames))
    alone = [api.upsample(
        xs[i:i + 1, :, :words[i]], bounds[i:i + 1, :, :words[i]].cuda(),
        torch.tensor(words[i:i + 1]), torch.tensor(frames[i:i + 1]))
        for i in range(3)]
    _check_against_items(whole, alone, frames)


def test_model_forward_never_touches_the_padding():
    frames, words, bounds = _padded_case()
    model = api.Model(gpu=0)
    features = _nan_behind(torch.randn(
        (3, 80, 65), generator=torch.Generator().manual_seed(3)), frames).cuda()
    whole = model(features, torch.tensor(frames), bounds, torch.tensor(words))
    alone = [model(
        features[i:i + 1, :, :frames[i]], torch.tensor(frames[i:i + 1]),
        bounds[i:i + 1, :, :words[i]], torch.tensor(words[i:i + 1]))
        for i in range(3)]
    _check_against_items(whole, alone, words)
