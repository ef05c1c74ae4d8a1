"""`emphases/data/preprocess/core.py` on the device: `from_audio` (71-125)
and the feature cache of whole datasets (`datasets`, 13-68), a batch of files
at a time."""
import dataclasses
import functools
import os
import time

import numpy as np
import torch

from ... import batch
from ... import config as cfg
from ... import core
from ... import pipeline
from ... import runtime


def too_short(samples, name=None):
    """The RuntimeError of an audio the reflect padding cannot take."""
    # torch's reflect padding: "Padding size should be less than the
    # corresponding input dimension" (mels.py:31-36)
    return RuntimeError(
        ('' if name is None else f'{name}: ') +
        f'reflect padding of {cfg.PADDING} needs more than {cfg.PADDING} '
        f'samples, the audio has {samples}')


def batch_plan(lengths, names=None):
    """A `batch.Plan` with one segment per audio, each ALL of its audio of
    `lengths[i]` samples - what `mels.from_audio(audio)` of the reference sees
    - i.e. the slice [432, 432 + samples) of the zero-padded signal
    (`core.py:357-358`), F = 1 + (samples + 864 - 1024) // 160 frames, no
    words.  Audio i lies at offset sum(lengths[:i]) of the packed samples.
    An audio of 432 samples or fewer raises RuntimeError (with `names[i]`)."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    for index in np.nonzero(lengths <= cfg.PADDING)[0]:
        raise too_short(
            int(lengths[index]), None if names is None else names[index])
    count = len(lengths)
    frames = 1 + (lengths + 2 * cfg.PADDING - cfg.NUM_FFT) // cfg.HOPSIZE
    zeros = np.zeros(count, dtype=np.int64)
    return batch.Plan.from_columns(
        np.arange(count, dtype=np.int64), zeros,
        np.full(count, cfg.PADDING, dtype=np.int64), lengths, frames, zeros,
        np.zeros((2, 0), dtype=np.int64), np.cumsum(lengths) - lengths,
        lengths)


def whole_audio_plan(samples):
    """`batch_plan` of one audio of `samples` samples."""
    return batch_plan([int(samples)])


def _tracks(config, engine, plan, audio, pitch_tracker, gpu):
    """penn's pitch and periodicity of the whole audio on the packed frame
    axis (`data/preprocess/core.py:84-92,107-116`), or None."""
    if not (config.pitch_feature or config.periodicity_feature):
        return None
    tracker = pitch_tracker or core.penn_tracker(gpu)
    pitch, periodicity = tracker(
        batch.chunk_audio(audio.cpu(), plan.segments[0]))
    # penn's floating-point hopsize can yield one frame more than the integer
    # hopsize of the mels: the reference drops it (core.py:107-116)
    frames = int(plan.frames[0])
    if pitch.shape[-1] == frames + 1:
        pitch, periodicity = pitch[..., :-1], periodicity[..., :-1]
    pairs = [(pitch, periodicity)]
    packed = torch.from_numpy(batch.pack_tracks(plan, pairs))
    return packed.pin_memory().to(engine.device, non_blocking=True)


def features(audio, gpu=None, config=None, pitch_tracker=None):
    """(float32 [NUM_FEATURES, F] on the device - a fresh tensor, device)."""
    if audio.dim() == 2:
        audio = audio[0]                        # channel 0 only (mels.py:48)
    if audio.dim() != 1:
        raise ValueError('audio must be [1, samples] or [samples]')
    if gpu is None and audio.is_cuda:
        gpu = audio.device.index
    config = config or core.active_config()
    # (the front-end's constants live in an engine; which model it holds does
    # not matter here, and the default one always loads)
    engine = core.get_engine(None, gpu, cfg.DEFAULT)
    plan = whole_audio_plan(int(audio.shape[0]))
    if audio.dtype != torch.int16:              # (int16 = 16-bit PCM, as elsewhere)
        audio = audio.to(torch.float32)
    with torch.cuda.device(engine.device), engine.lock:
        resident = audio.to(engine.device).contiguous()
        meta = engine.upload(plan)
        tracks = _tracks(config, engine, plan, audio, pitch_tracker, gpu)
        out = engine.features(resident, plan, meta, tracks=tracks,
                              config=config)
        first = int(plan.frame_off[0])
        return out[:, first:first + int(plan.frames[0])].clone(), engine.device


def from_audio(audio, gpu=None, pitch_tracker=None):
    """Preprocess one audio file (`data/preprocess/core.py:71-125`): audio
    [1, S] at 16 kHz -> the active configuration's feature stack
    [1, NUM_FEATURES, F], F = S // 160 for S a multiple of 160 - mels, then
    log2 pitch and periodicity (from `pitch_tracker`, the stand-in for
    `penn.from_audio`, see `core.from_alignments_and_audios`), then loudness.
    Computed on GPU `gpu` (None: the current HIP device - there is no CPU
    path - and the result comes back on the host, where the reference would
    have computed it)."""
    result, _ = features(audio, gpu, core.active_config(), pitch_tracker)
    result = result[None]
    return result.cpu() if gpu is None and not audio.is_cuda else result


###############################################################################
# The feature cache (`data/preprocess/core.py:13-68`), a batch of files at a time
###############################################################################


FEATURES = ('mels', 'loudness', 'pitch')
# `from_files_to_files` appends (stage, batch, start, end) in perf_counter_ns
# here when it is a list (tools/preprocess_bench.py): where the stages run
TIMELINE = None
# destination blocks start on multiples of this many floats (64 bytes) of the
# result buffer (`emph_unpack_rows` itself takes any offset)
BLOCK_ALIGN = 16


def _stamp(stage, position, start):
    if TIMELINE is not None:
        TIMELINE.append((stage, position, start, time.perf_counter_ns()))


def unpack_table(plan, groups, align=BLOCK_ALIGN):
    """The table of `emph_unpack_rows` that takes the packed feature matrix
    of `plan` apart: for every segment (file), in order, one block per
    (first row, rows) of `groups` - int64 [segments * groups, 5] = (first
    column, frames, first row, rows, destination offset in floats), the
    blocks back to back in table order, each starting on a multiple of
    `align` floats.  Returns (table, floats of the destination)."""
    groups = np.asarray(groups, dtype=np.int64).reshape(-1, 2)
    count = len(plan)
    table = np.empty((count, len(groups), 5), dtype=np.int64)
    table[:, :, 0] = plan.frame_off[:, None]
    table[:, :, 1] = plan.frames[:, None]
    table[:, :, 2] = groups[None, :, 0]
    table[:, :, 3] = groups[None, :, 1]
    sizes = (table[:, :, 1] * table[:, :, 3]).ravel()
    sizes = (sizes + align - 1) // align * align
    table[:, :, 4] = (np.cumsum(sizes) - sizes).reshape(count, len(groups))
    return table.reshape(-1, 5), int(sizes.sum())


def unpack_rows(x, table, out, device_table=None):
    """`emph_unpack_rows` on the current stream: the blocks `table` (int64
    [n, 5] on the host, `unpack_table`) names of the float32 device matrix `x`
    [rows, ld] into the flat float32 device tensor `out`.  The kernel cannot
    refuse an entry (its table is device memory), so the host table is held
    against both shapes here.  `device_table`: the same table on the device
    when the caller has sent it along with other metadata."""
    table = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 5)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or \
            x.stride(1) != 1 or out.dtype != torch.float32 or \
            not out.is_cuda or not out.is_contiguous():
        raise ValueError('unpack_rows: float32 device tensors, x [rows, ld]')
    if not len(table):
        return out
    column, frames, row, rows, target = table.T
    if int(table.min()) < 0 or \
            int((column + frames).max()) > x.shape[1] or \
            int((row + rows).max()) > x.shape[0] or \
            int((rows * frames).max()) >= 1 << 31 or \
            int((target + rows * frames).max()) > out.numel():
        raise ValueError('unpack_rows: a block lies outside x or out')
    if device_table is None:
        device_table = torch.from_numpy(table).to(x.device)
    runtime.check(runtime.library().emph_unpack_rows(
        x.data_ptr(), x.stride(0), device_table.data_ptr(), len(table),
        out.data_ptr(), runtime.stream()), 'emph_unpack_rows')
    return out


@functools.lru_cache(maxsize=None)
def _session(device_index):
    """The lanes the feature cache runs through: a `Session` of its own on
    the engine `features` uses, so its batches in flight stay clear of an
    inference session's."""
    from ... import session
    return session.Session(
        core.get_engine(None, device_index, cfg.DEFAULT), depth=2)


def _feature_configs(active):
    """(mel-only, loudness-only) configurations: the ones `mels.from_audio`
    and `loudness.from_audio` featurise under."""
    mel = dataclasses.replace(
        active, mel_feature=True, pitch_feature=False,
        periodicity_feature=False, loudness_feature=False)
    loud = dataclasses.replace(
        active, mel_feature=False, pitch_feature=False,
        periodicity_feature=False, loudness_feature=True)
    return mel, loud


def survey(opened):
    """What the WAVE headers of a `files.FileBatch` say, before any GPU work:
    (lengths int64 [count] in samples at 16 kHz - after resampling for a file
    at another rate -, formats [count]: torch.int16 / torch.float32 for a file
    the fast path takes (mono, 16 kHz, 16-bit PCM or float32), None for one
    that goes through `load.audio`).  A missing or unreadable file raises what
    `load.wav_info` raises for it; a file of 432 samples or fewer raises the
    RuntimeError of `whole_audio_plan`, naming the file."""
    import math
    from ... import load
    lengths = np.zeros(opened.count, dtype=np.int64)
    formats = [None] * opened.count
    native = opened.native_audio()
    for index, row in enumerate(opened.sizes.tolist()):
        file = opened.audio_files[index]
        if row[0] & 2:
            rate, channels, samples = load.wav_info(file)       # raises
        else:
            channels, rate, bits, nbytes = row[6], row[7], row[8], row[10]
            samples = nbytes // (bits // 8 * channels)
        if rate != cfg.SAMPLE_RATE:
            gcd = math.gcd(int(rate), cfg.SAMPLE_RATE)
            samples = load.resampled_length(
                samples, rate // gcd, cfg.SAMPLE_RATE // gcd)
        elif native[index]:
            formats[index] = torch.int16 if row[5] == 1 else torch.float32
        lengths[index] = samples
        if samples <= cfg.PADDING:
            raise too_short(int(samples), file)
    return lengths, formats


def _room(lane, name, numel, dtype, pinned=False):
    """A buffer of the lane that only grows (`session.grown`), kept in the
    lane engine's workspace."""
    from ... import session
    store = lane.engine._workspace
    store[('preprocess', name)] = session.grown(
        store.get(('preprocess', name)), numel, dtype,
        None if pinned else lane.device)
    return store[('preprocess', name)]


def _per_file(audio_file, mel_file, loudness_file):
    """One file through `load.audio` and the seams (a file the fast path does
    not take: another rate, several channels, another sample format)."""
    from ... import files
    from ... import load
    from . import loudness, mels
    audio = load.audio(audio_file)
    for module, path in ((mels, mel_file), (loudness, loudness_file)):
        if path is None:
            continue
        tensor = module.from_audio(audio).cpu().contiguous()
        _raise_unwritten(files.write_tensors(
            [path], tensor.numpy().reshape(-1), [0], [tensor.shape[0]],
            [tensor.shape[1]], 1))


def _raise_unwritten(failed):
    if failed:
        raise OSError('; '.join(reason for _, reason in failed))


def from_files_to_files(audio_files, mel_files=None, loudness_files=None,
                        gpu=None, *, files_per_batch=256):
    """`mels.from_files_to_files` and `loudness.from_files_to_files`
    (`mels.py:79-86`, `loudness.py:44-51`) in one pass: `torch.save` of the
    float32 log-mel spectrogram [80, F] of `audio_files[i]` to `mel_files[i]`
    and of its A-weighted loudness [1, F] to `loudness_files[i]` (either list
    may be None), F = 1 + (S + 864 - 1024) // 160 for S samples at 16 kHz,
    under the active configuration's `normalize`; parent directories are
    created.  Every file is read and sent to the device once, whichever
    outputs are asked for.

    The reference runs one file at a time.  Here the mono 16 kHz files in
    16-bit PCM or float32 go in ragged batches of `files_per_batch`, two in
    flight, through the stages of `pipeline.run` (no `collect` here):

        opener   the samples of batches i + 1, i + 2 straight into pinned
                 memory (`files.FileBatch.read`), their plan (`batch_plan`),
                 its tables and the table of `emph_unpack_rows`
        caller   batch i: one H2D copy, `emph_logmel` for the mel rows,
                 `emph_frontend_peak` + `emph_logmel` for the loudness row -
                 the instantiations of `mels.from_audio` and
                 `loudness.from_audio`, whose bits the files hold -, one
                 `emph_unpack_rows`, one D2H copy into pinned memory
        writer   batch i - 1: `emph_files_write_tensors` on the file pool

    Any other file (another rate, several channels, 24-bit ...) goes through
    `load.audio` and the two seams on its own, after the batches.  Which way
    a file goes follows from its header alone, and what is written for it does
    not depend on `files_per_batch` or on the files around it.

    Every header is read before any GPU work: a missing file raises there,
    and a file of 432 samples or fewer raises `RuntimeError` naming it
    (`whole_audio_plan`), with nothing written."""
    from ... import engine as engine_module
    from ... import files
    from ... import load
    from ... import session as session_module
    audio_files = [os.fspath(file) for file in audio_files]
    count = len(audio_files)
    outputs = []
    for listed in (mel_files, loudness_files):
        if listed is not None:
            listed = [os.fspath(file) for file in listed]
            if len(listed) != count:
                raise ValueError('as many output files as audio files')
        outputs.append(listed)
    mel_files, loudness_files = outputs
    if mel_files is None and loudness_files is None:
        raise ValueError('no output files: mel_files, loudness_files or both')
    files_per_batch = int(files_per_batch)
    if files_per_batch < 1:
        raise ValueError('files_per_batch must be at least 1')
    if not count:
        return

    start = time.perf_counter_ns()
    # (the file pool's threads per stage: here the writer has the most to do -
    # a checksum and a copy of 324 KB per ten-second file against the opener's
    # read of 320 KB - so it gets the larger share of `files.stage_threads`)
    write_threads, open_threads = files.stage_threads(1)
    opened = files.FileBatch(None, audio_files, open_threads)
    lengths, formats = survey(opened)
    _stamp('headers', 0, start)

    index = runtime.device_index(gpu)
    session = _session(index)
    device = session.engine.device
    mel_config, loud_config = _feature_configs(core.active_config())
    # rows of the packed matrix: the mel rows, then the loudness row
    groups, configs, row = [], [], 0
    if mel_files is not None:
        groups.append((row, cfg.NUM_MELS))
        configs.append(mel_config)
        row += cfg.NUM_MELS
    if loudness_files is not None:
        groups.append((row, 1))
        configs.append(loud_config)
        row += 1
    matrix_rows = row

    # batches: consecutive fast files of one sample format
    batches = []
    for dtype in (torch.int16, torch.float32):
        chosen = [i for i in range(count) if formats[i] is dtype]
        batches += [(dtype, np.array(chosen[first:first + files_per_batch]))
                    for first in range(0, len(chosen), files_per_batch)]
    slow = [i for i in range(count) if formats[i] is None]

    def open_batch(position):
        begin = time.perf_counter_ns()
        dtype, chosen = batches[position]
        item = load.itemsize(dtype)
        samples = lengths[chosen]
        nbytes = samples * item
        where, total = files.aligned_placement(nbytes)
        with torch.cuda.device(device):
            staging = session.file_buffer(position, total)
        opened.read(chosen.astype(np.int32), where, nbytes,
                    staging.data_ptr())
        _stamp('open.read', position, begin)
        begin = time.perf_counter_ns()
        plan = batch_plan(samples)
        # (2-byte samples of an odd count leave a gap behind their file: the
        # segment table says where each file lies in the staged bytes)
        plan.table[:, runtime.SEG_AUDIO_OFF] = where // item
        host, offsets = plan.pack_metadata(
            [(runtime.AXIS_FRAMES, engine_module.FRONTEND_BLOCK)])
        table, floats = unpack_table(plan, groups)
        # one array for one small H2D copy: the plan's tables, then the
        # unpack table (int64: the plan's pieces end on 16-byte boundaries)
        host = np.concatenate([host, table.view(np.int32).ravel()])
        _stamp('open.plan', position, begin)
        return dict(dtype=dtype, chosen=chosen, staging=staging, total=total,
                    plan=plan, host=host, offsets=offsets, table=table,
                    floats=floats)

    def enqueue(position, job):
        begin = time.perf_counter_ns()
        lane = session.lanes[position % len(session.lanes)]
        engine, plan, dtype = lane.engine, job['plan'], job['dtype']
        with torch.cuda.device(lane.device), torch.cuda.stream(lane.stream):
            audio = _room(lane, 'audio', job['total'], torch.uint8)[
                :job['total']]
            audio.copy_(job['staging'][:job['total']], non_blocking=True)
            audio = audio.view(dtype)
            pinned = engine._pinned('preprocess', job['host'])
            tables = pinned.to(lane.device, non_blocking=True)
            meta = {name: (tables[first:first + size], size)
                    for name, (first, size) in job['offsets'].items()}
            cut = len(job['host']) - job['table'].size * 2
            device_table = tables[cut:].view(torch.int64)
            matrix = _room(
                lane, 'matrix', matrix_rows * plan.ld_frames, torch.float32)[
                    :matrix_rows * plan.ld_frames].view(
                        matrix_rows, plan.ld_frames)
            for (first, rows), config in zip(groups, configs):
                engine.features(audio, plan, meta, config=config,
                                out=matrix[first:first + rows])
            unpacked = _room(lane, 'unpacked', job['floats'], torch.float32)
            unpack_rows(matrix, job['table'], unpacked, device_table)
            result = _room(lane, 'result', job['floats'], torch.float32,
                           pinned=True)
            result[:job['floats']].copy_(
                unpacked[:job['floats']], non_blocking=True)
            lane.done.record(lane.stream)
        job['lane'], job['result'] = lane, result
        _stamp('submit', position, begin)
        return job

    def write(position, job):
        begin = time.perf_counter_ns()
        job['lane'].done.synchronize()
        _stamp('write.wait', position, begin)
        begin = time.perf_counter_ns()
        table = job['table'].reshape(len(job['chosen']), len(groups), 5)
        # (group by group, the order of `blocks` below)
        paths = [listed[i] for listed in (mel_files, loudness_files)
                 if listed is not None for i in job['chosen']]
        blocks = np.concatenate(
            [table[:, column] for column in range(len(groups))])
        failed = files.write_tensors(
            paths, job['result'], blocks[:, 4], blocks[:, 3], blocks[:, 1],
            write_threads)
        _stamp('write', position, begin)
        _raise_unwritten(failed)

    try:
        with pipeline.near_gpu(
                index, open_threads + write_threads + 2) as settle:
            # (the lane's pinned result buffer and the staging buffer that the
            # next opener takes are free once batch `position - 2` is written)
            pipeline.run(len(batches), open_batch, enqueue, write, openers=1,
                         ahead=session_module.FILE_BUFFERS - 2,
                         unwritten=len(session.lanes) - 1, initializer=settle)
    finally:
        for lane in session.lanes:
            lane.stream.synchronize()
        opened.close()
    begin = time.perf_counter_ns()
    for i in slow:
        _per_file(audio_files[i],
                  None if mel_files is None else mel_files[i],
                  None if loudness_files is None else loudness_files[i])
    _stamp('per_file', 0, begin)


def _wanted(features, pitch_tracker, gpu):
    """(features as a tuple, the tracker or None)."""
    if features is None:
        features = ['mels', 'loudness']
        if pitch_tracker is None:
            try:
                pitch_tracker = core.penn_tracker(gpu)
            except NotImplementedError:
                pass
        if pitch_tracker is not None:
            features.append('pitch')
    features = tuple(features)
    for feature in features:
        if feature not in FEATURES:
            raise ValueError(
                f'unknown feature {feature!r}: one of {", ".join(FEATURES)}')
    if 'pitch' in features and pitch_tracker is None:
        try:
            pitch_tracker = core.penn_tracker(gpu)
        except NotImplementedError:
            # (the text `Engine.features` has for a missing tracker)
            from ... import engine as engine_module
            raise NotImplementedError(engine_module.TRACKS_NEEDED) from None
    return features, pitch_tracker if 'pitch' in features else None


def _pitch_files(audio_files, prefixes, pitch_tracker):
    """`<prefix>-pitch.pt` and `<prefix>-periodicity.pt` [1, F]: the raw
    outputs of the tracker on the whole audio (`core.py:38-68`), without the
    last frame when it returns F + 1 of them."""
    from ... import files
    from ... import load
    for audio_file, prefix in zip(audio_files, prefixes):
        audio = load.audio(audio_file)[:1]
        audio = audio.to(torch.float32).cpu()
        samples = int(audio.shape[-1])
        frames = 1 + (samples + 2 * cfg.PADDING - cfg.NUM_FFT) // cfg.HOPSIZE
        pitch, periodicity = pitch_tracker(audio)
        tracks = []
        for track in (pitch, periodicity):
            track = torch.as_tensor(track).detach().to(
                'cpu', torch.float32).reshape(1, -1)
            if track.shape[1] == frames + 1:
                track = track[:, :-1]
            tracks.append(track.contiguous().numpy())
        data = np.concatenate([track.ravel() for track in tracks])
        _raise_unwritten(files.write_tensors(
            [f'{prefix}-pitch.pt', f'{prefix}-periodicity.pt'], data,
            [0, tracks[0].size], [1, 1],
            [tracks[0].shape[1], tracks[1].shape[1]], 1))


def datasets(datasets, gpu=None, *, cache_dir, features=None,
             pitch_tracker=None, files_per_batch=256):
    """Preprocess datasets (`data/preprocess/core.py:13-68`): for every
    `sorted((cache_dir / dataset).rglob('*.wav'))`, write
    `<cache_dir>/<dataset>/mels/<stem>.pt` [80, F] and `loudness/<stem>.pt`
    [1, F] (`from_files_to_files`, one pass) and - with a pitch tracker -
    `pitch/<stem>-pitch.pt` and `pitch/<stem>-periodicity.pt` [1, F].

    `features`: any of 'mels', 'loudness', 'pitch'; None: mels and loudness,
    and pitch when `pitch_tracker` is given or `penn` can be imported.
    `pitch_tracker`: the callable used everywhere else in the package, audio
    [1, S] at 16 kHz -> (pitch [1, F], periodicity [1, F]); its outputs are
    written as they are.  'pitch' with no tracker and no `penn` raises
    NotImplementedError."""
    from pathlib import Path
    if isinstance(datasets, str):
        datasets = [datasets]
    datasets = list(datasets)
    features, pitch_tracker = _wanted(features, pitch_tracker, gpu)
    listed = {}
    for dataset in datasets:
        directory = Path(cache_dir) / dataset
        if not directory.is_dir():
            raise FileNotFoundError(f'dataset {dataset}: {directory} not found')
        listed[dataset] = (directory, sorted(directory.rglob('*.wav')))
    for dataset in datasets:
        directory, audio_files = listed[dataset]
        if 'mels' in features or 'loudness' in features:
            from_files_to_files(
                audio_files,
                [directory / 'mels' / f'{file.stem}.pt'
                 for file in audio_files] if 'mels' in features else None,
                [directory / 'loudness' / f'{file.stem}.pt'
                 for file in audio_files] if 'loudness' in features else None,
                gpu, files_per_batch=files_per_batch)
        if 'pitch' in features:
            _pitch_files(
                audio_files,
                [directory / 'pitch' / file.stem for file in audio_files],
                pitch_tracker)
