"""Dataset preprocessing without a device: the `.pt` writer of 2-D tensors,
the batch whole-audio plan, the table of `emph_unpack_rows` and the command
line (`emphases_amd/data/preprocess`, `csrc/files.hip`)."""
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest
import torch

import preprocess_data
from conftest import GOLDEN

from emphases_amd import batch, config as cfg, files, runtime, synth
from emphases_amd.data.preprocess import core as preprocess


def test_write_tensors_round_trip(tmp_path):
    """`emph_files_write_tensors`: `torch.load(weights_only=True)` returns the
    float32 tensor of the exact shape, contiguous and bitwise the input, from
    nested directories that did not exist; an unwritable path is reported
    for its file alone."""
    shapes = [(80, 129), (80, 1), (1, 2), (1, 1), (81, 400)]
    tensors = [synth.weights(300 + i, shape, 4.) for i, shape in
               enumerate(shapes)]
    tensors[1][0, 0] = np.float32('nan')
    tensors[2][0, 1] = np.float32('-inf')
    # blocks at odd offsets of one buffer, a gap of sentinels between them
    sizes = [t.size + 3 for t in tensors]
    first = np.cumsum(sizes) - sizes + 1
    data = np.full(int(sum(sizes)) + 1, 1234.5, dtype=np.float32)
    for offset, tensor in zip(first, tensors):
        data[offset:offset + tensor.size] = tensor.ravel()
    paths = [tmp_path / 'cache' / f'd{i}' / 'deeper' / f't{i}.pt'
             for i in range(len(shapes))]
    assert not (tmp_path / 'cache').exists()
    assert files.write_tensors(
        paths, data, first, [s[0] for s in shapes], [s[1] for s in shapes],
        threads=4) == []
    for path, tensor in zip(paths, tensors):
        loaded = torch.load(path, weights_only=True)
        assert loaded.dtype == torch.float32 and not loaded.is_cuda
        assert tuple(loaded.shape) == tensor.shape
        assert loaded.is_contiguous()
        assert loaded.numpy().tobytes() == tensor.tobytes()
    # a pinned-style host tensor as the source, one thread
    again = tmp_path / 'again.pt'
    assert files.write_tensors(
        [again], torch.from_numpy(data), first[:1], [80], [129], 1) == []
    assert torch.load(again, weights_only=True).numpy().tobytes() == \
        tensors[0].tobytes()
    # a path under a regular file cannot be written: reported for that file,
    # the others are written
    (tmp_path / 'plain').write_bytes(b'x')
    mixed = [tmp_path / 'ok0.pt', tmp_path / 'plain' / 'no.pt',
             tmp_path / 'ok2.pt']
    failed = files.write_tensors(
        mixed, data, first[[0, 1, 2]], [80, 80, 1], [129, 1, 2], 2)
    assert [k for k, _ in failed] == [1]
    assert 'plain' in failed[0][1]
    assert torch.load(mixed[0], weights_only=True).shape == (80, 129)
    assert torch.load(mixed[2], weights_only=True).shape == (1, 2)
    assert not os.path.exists(mixed[1])
    # what does not fit the buffer never reaches the library
    with pytest.raises(ValueError, match='outside'):
        files.write_tensors([tmp_path / 'x.pt'], data, [len(data) - 3],
                            [2], [2])
    assert files.write_tensors([], data, [], [], []) == []


def test_write_tensors_checksums(tmp_path):
    """The container's CRC-32 fields (`crc32_of`, slice-by-8) against zlib
    for payloads whose length leaves every remainder of 8."""
    import zipfile
    for columns in range(1, 20):
        tensor = synth.weights(500 + columns, (1, columns), 1.)
        path = tmp_path / f'c{columns}.pt'
        assert files.write_tensors([path], tensor.ravel(), [0], [1],
                                   [columns], 1) == []
        with zipfile.ZipFile(path) as archive:
            assert archive.testzip() is None
            info = archive.getinfo(f'c{columns}/data/0')
            assert info.CRC == zlib.crc32(tensor.tobytes())
            assert info.header_offset >= 0 and info.file_size == 4 * columns


def test_scores_writer_bytes_unchanged(tmp_path):
    """`emph_files_write` shares its container code with the tensor writer:
    its `.pt` of a [1, W] row is byte for byte what the build before the
    tensor writer wrote (tests/golden/pt_rows.npz: the files for W = 3 and
    300, SHA-256 for W = 0, 3, 300 and 70 000), and the tensor writer gives a
    [1, W] tensor the same bytes."""
    golden = np.load(os.path.join(GOLDEN, 'pt_rows.npz'))
    grid = tmp_path / 'a.TextGrid'
    grid.write_text(preprocess_data.TEXTGRID)
    wave = tmp_path / 'a.wav'
    preprocess_data.write_pcm_wav(wave, np.zeros(500, dtype=np.int16))
    opened = files.FileBatch([grid], [wave], threads=1)
    assert not opened.status.any()
    for width in (0, 3, 300, 70000):
        row = (np.arange(width, dtype=np.float32) / np.float32(7))[None]
        opened.write([0], [tmp_path / f'row{width}'], [torch.from_numpy(row)])
        written = (tmp_path / f'row{width}.pt').read_bytes()
        assert hashlib.sha256(written).hexdigest() == \
            str(golden[f'sha256/row{width}']), width
        if f'row{width}' in golden.files:
            assert written == golden[f'row{width}'].tobytes()
        if width:
            directory = tmp_path / 'tensors'
            assert files.write_tensors(
                [directory / f'row{width}.pt'], row.ravel(), [0], [1],
                [width], 1) == []
            assert (directory / f'row{width}.pt').read_bytes() == written


def test_file_batch_of_audio_alone(tmp_path):
    """`FileBatch(None, audio_files)`: headers walked, no alignment asked
    for, every status clear."""
    paths = []
    for index, samples in enumerate((500, 1601)):
        paths.append(tmp_path / f'{index}.wav')
        preprocess_data.write_pcm_wav(
            paths[-1], preprocess_data.to_pcm(
                synth.audio(index, 11)[0, :samples]))
    opened = files.FileBatch(None, paths, threads=2)
    assert opened.count == 2 and not opened.status.any()
    assert opened.staged_format(16000) == torch.int16
    assert (opened.sizes[:, 10] // 2).tolist() == [500, 1601]
    assert opened.times.shape == (0, 2)


def test_batch_plan_is_whole_audio_plan_per_file():
    """One segment per file: start 432, length S, S // 160 frames (S >= 160),
    the file's samples at the running offset - what `whole_audio_plan` gives
    for the file alone; a 432-sample file raises and names the file."""
    lengths = [433, 20731, 64000, 1599, 1600, 480159]
    plan = preprocess.batch_plan(lengths)
    assert len(plan) == len(lengths)
    offset = 0
    for index, samples in enumerate(lengths):
        alone = preprocess.whole_audio_plan(samples)
        assert len(alone) == 1
        row, want = plan.table[index], alone.table[0]
        assert row[runtime.SEG_START] == want[runtime.SEG_START] == cfg.PADDING
        assert row[runtime.SEG_LENGTH] == want[runtime.SEG_LENGTH] == samples
        assert row[runtime.SEG_FRAMES] == want[runtime.SEG_FRAMES] == \
            samples // 160 == 1 + (samples + 864 - 1024) // 160
        assert row[runtime.SEG_AUDIO_LEN] == samples
        assert row[runtime.SEG_AUDIO_OFF] == offset
        assert row[runtime.SEG_WORDS] == 0
        assert row[runtime.SEG_FRAME_OFF] % batch.ALIGN == 0
        assert plan.segments[index].utterance == index
        offset += samples
    assert plan.total_words == 0
    # the frame axis: segments back to back on multiples of 16 columns
    ends = plan.frame_off + plan.frames
    assert (plan.frame_off[1:] >= ends[:-1]).all()
    assert plan.ld_frames >= ends[-1]
    # the tile tables of the front-end come out of it as of any plan
    tiles = plan.tiles(runtime.AXIS_FRAMES, 64)
    assert sorted(set(tiles[:, 0].tolist())) == list(range(len(lengths)))
    with pytest.raises(RuntimeError, match='432'):
        preprocess.whole_audio_plan(432)
    with pytest.raises(RuntimeError, match='clip_b.wav.*432 samples'):
        preprocess.batch_plan([500, 432, 9000],
                              ['clip_a.wav', 'clip_b.wav', 'clip_c.wav'])


def test_unpack_table_reproduces_the_slices():
    """The table built for a plan, through the numpy restatement of the
    gather, gives every file's slice of a random packed matrix."""
    lengths = [433, 20731, 64000, 1599, 1600, 800]
    plan = preprocess.batch_plan(lengths)
    packed = synth.weights(77, (81, plan.ld_frames), 9.)
    for groups in ([(0, 80), (80, 1)], [(0, 80)], [(0, 1)]):
        rows = sum(count for _, count in groups)
        table, floats = preprocess.unpack_table(plan, groups)
        assert table.dtype == np.int64 and table.shape == (
            len(lengths) * len(groups), 5)
        flat = np.full(floats, -7., dtype=np.float32)
        preprocess_data.gather(packed[:rows], table, flat)
        got = preprocess_data.blocks(table, flat)
        # blocks do not overlap and start on the alignment asked for
        ends = table[:, 4] + table[:, 1] * table[:, 3]
        assert (table[1:, 4] >= ends[:-1]).all() and floats >= ends[-1]
        assert (table[:, 4] % preprocess.BLOCK_ALIGN == 0).all()
        for index in range(len(lengths)):
            first, frames = int(plan.frame_off[index]), int(plan.frames[index])
            for g, (row, count) in enumerate(groups):
                want = packed[row:row + count, first:first + frames]
                assert np.array_equal(got[index * len(groups) + g], want)
    unaligned, floats = preprocess.unpack_table(plan, [(0, 80), (80, 1)], 1)
    assert floats == 81 * int(plan.frames.sum())
    assert (unaligned[:, 4] % 16 != 0).any()


def test_survey_checks_every_header_first(tmp_path):
    """Lengths and routes from the headers alone: a missing file and a file of
    432 samples raise before anything else happens."""
    paths = {}
    audio = synth.audio(3, 12)
    paths['pcm'] = tmp_path / 'pcm.wav'
    preprocess_data.write_pcm_wav(
        paths['pcm'], preprocess_data.to_pcm(audio[0, :1601]))
    paths['float'] = tmp_path / 'float.wav'
    preprocess_data.write_float_wav(paths['float'], audio[:, :1000])
    paths['stereo'] = tmp_path / 'stereo.wav'
    preprocess_data.write_float_wav(
        paths['stereo'], np.concatenate([audio, audio])[:, :900])
    paths['slow'] = tmp_path / 'slow.wav'
    preprocess_data.write_pcm_wav(
        paths['slow'], preprocess_data.to_pcm(audio[0, :801]), 8000)
    order = ['pcm', 'float', 'stereo', 'slow']
    opened = files.FileBatch(None, [paths[k] for k in order])
    lengths, formats = preprocess.survey(opened)
    assert lengths.tolist() == [1601, 1000, 900, 1602]
    assert formats == [torch.int16, torch.float32, None, None]
    short = tmp_path / 'short.wav'
    preprocess_data.write_float_wav(short, audio[:, :432])
    with pytest.raises(RuntimeError, match='short.wav.*432'):
        preprocess.survey(files.FileBatch(None, [paths['pcm'], short]))
    # at 8 kHz 216 samples become 432
    short8 = tmp_path / 'short8.wav'
    preprocess_data.write_pcm_wav(
        short8, preprocess_data.to_pcm(audio[0, :216]), 8000)
    with pytest.raises(RuntimeError, match='short8.wav'):
        preprocess.survey(files.FileBatch(None, [short8]))
    with pytest.raises(FileNotFoundError):
        preprocess.survey(files.FileBatch(
            None, [paths['pcm'], tmp_path / 'absent.wav']))
    # ... and `from_files_to_files` gets there before it needs a device
    out = tmp_path / 'out'
    with pytest.raises(RuntimeError, match='short.wav'):
        preprocess.from_files_to_files(
            [paths['pcm'], short], [out / 'a.pt', out / 'b.pt'])
    assert not out.exists()
    with pytest.raises(ValueError, match='as many'):
        preprocess.from_files_to_files([paths['pcm']], [])
    with pytest.raises(ValueError, match='no output'):
        preprocess.from_files_to_files([paths['pcm']])


def test_command_line_and_tracker_contract(tmp_path, monkeypatch):
    """The reference's `--datasets` and `--gpu` plus the new flags; 'pitch'
    with neither a tracker nor `penn` raises the text `Engine.features` has."""
    from emphases_amd import engine
    from emphases_amd.data.preprocess import __main__ as command
    parsed = command.parse_args(
        ['--datasets', 'libritts', 'buckeye', '--gpu', '3', '--cache_dir',
         str(tmp_path), '--features', 'mels', 'loudness',
         '--files_per_batch', '64'])
    assert parsed.datasets == ['libritts', 'buckeye'] and parsed.gpu == 3
    assert parsed.cache_dir == tmp_path
    assert parsed.features == ['mels', 'loudness']
    assert parsed.files_per_batch == 64
    default = command.parse_args(['--cache_dir', str(tmp_path)])
    assert default.datasets == ['libritts'] and default.gpu is None
    assert default.features is None and default.files_per_batch == 256
    with pytest.raises(SystemExit):
        command.parse_args(['--datasets', 'libritts'])      # no cache_dir
    with pytest.raises(SystemExit):
        command.parse_args(['--cache_dir', '.', '--features', 'energy'])

    monkeypatch.setitem(sys.modules, 'penn', None)          # import fails
    import emphases_amd
    with pytest.raises(NotImplementedError) as raised:
        emphases_amd.data.preprocess.datasets(
            ['libritts'], cache_dir=tmp_path, features=('pitch',))
    assert str(raised.value) == engine.TRACKS_NEEDED
    assert 'penn' in engine.TRACKS_NEEDED
    # without a tracker the default leaves pitch out; with one it is in
    assert preprocess._wanted(None, None, None) == (('mels', 'loudness'), None)
    features, tracker = preprocess._wanted(None, synth.pitch_tracks, None)
    assert features == ('mels', 'loudness', 'pitch')
    assert tracker is synth.pitch_tracks
    with pytest.raises(ValueError, match='energy'):
        preprocess._wanted(('energy',), None, None)
    # the reference's module names and argument order
    from emphases_amd.data.preprocess import loudness, mels
    for module in (mels, loudness):
        for name in ('from_file', 'from_file_to_file', 'from_files_to_files'):
            assert callable(getattr(module, name))


def test_abi_declares_the_new_entry_points():
    header = open(os.path.join(
        os.path.dirname(GOLDEN), '..', 'include', 'emphases_hip.h')).read()
    for name in ('emph_unpack_rows', 'emph_files_write_tensors',
                 'emph_files_write_tensors_error'):
        assert name in runtime.SIGNATURES and f'{name}(' in header
    lib = runtime.library()
    assert lib.emph_abi_version() == runtime.ABI_VERSION >= 33
    # what the host side of the launch can see is refused with a code
    assert lib.emph_unpack_rows(None, 64, None, 1, None, None) == -1
    assert lib.emph_unpack_rows(None, 64, None, -1, None, None) == -1
    assert lib.emph_unpack_rows(None, 64, None, 0, None, None) == 0
    table = np.zeros(5, dtype=np.int64)
    assert lib.emph_unpack_rows(
        table.ctypes.data, -5, table.ctypes.data, 1, table.ctypes.data,
        None) == -1
