"""Feature-cache preprocessing: the batched path against the per-file loop.

Throughput (default): `files` ten-second 16-bit WAVE files in /dev/shm under
`<cache>/corpus/audio`, warmed.  Laps alternate between

    batched  emphases_amd.data.preprocess.datasets() for mels + loudness
    loop     what a caller had to write before it: per file `load.audio` ->
             `mels.from_audio` + `loudness.from_audio` -> two `torch.save`
             (on the first `subset` files: the loop is slow)

and the tool reports files/s per lap, the medians and the lap-to-lap spread
((max - min) / median) of each side, then the stage timeline of the last
batched lap (`data.preprocess.core.TIMELINE`): busy time of every stage per
batch - the slowest stage is the bound of the pipeline.

Kernel rate (`--kernel`, meant to run under `rocprofv3 --kernel-trace
--stats`): one batch of `per_batch` ten-second files - `emph_unpack_rows` a
few times, then the `2 * per_batch` slice-and-clone copies it replaces - with
the bytes moved (read + written, from the shapes) and event-timed durations.

usage (GPU box):
    python tools/preprocess_bench.py [--files 4096] [--subset 256] [--laps 3]
    rocprofv3 --kernel-trace --stats -d DIR -- \\
        python tools/preprocess_bench.py --kernel
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import load, synth  # noqa: E402
from emphases_amd.data.preprocess import core as preprocess  # noqa: E402
from emphases_amd.data.preprocess import loudness, mels  # noqa: E402


def corpus(directory, count, frames=1000, distinct=32):
    """`count` WAVE files of `frames` frames (hard links of `distinct`
    different ones) under <directory>/corpus/audio."""
    audio = os.path.join(directory, 'corpus', 'audio')
    os.makedirs(audio)
    paths = []
    for index in range(count):
        path = os.path.join(audio, f'u{index:05d}.wav')
        if index < distinct:
            load.save_wav(path, synth.audio(index, frames))
        else:
            os.link(paths[index % distinct], path)
        paths.append(path)
    return paths


def loop(paths, directory):
    """The per-file loop over the one-audio seams."""
    os.makedirs(os.path.join(directory, 'mels'), exist_ok=True)
    os.makedirs(os.path.join(directory, 'loudness'), exist_ok=True)
    for path in paths:
        stem = os.path.basename(path)[:-4]
        audio = load.audio(path)
        torch.save(mels.from_audio(audio),
                   os.path.join(directory, 'mels', f'{stem}.pt'))
        torch.save(loudness.from_audio(audio),
                   os.path.join(directory, 'loudness', f'{stem}.pt'))


def stages(timeline):
    """{stage: (batches, total ms, mean ms per batch)} and the wall time."""
    table = {}
    for stage, _, start, end in timeline:
        table.setdefault(stage, []).append((end - start) / 1e6)
    wall = (max(t[3] for t in timeline) - min(t[2] for t in timeline)) / 1e6
    return {stage: (len(v), round(sum(v), 2), round(sum(v) / len(v), 3))
            for stage, v in table.items()}, round(wall, 2)


def throughput(arguments):
    directory = tempfile.mkdtemp(prefix='emph_preprocess_', dir='/dev/shm')
    try:
        paths = corpus(directory, arguments.files)
        subset = paths[:arguments.subset]
        scratch = os.path.join(directory, 'loop')

        def batched():
            emphases_amd.data.preprocess.datasets(
                ['corpus'], arguments.gpu, cache_dir=directory,
                features=['mels', 'loudness'],
                files_per_batch=arguments.per_batch)
        # warm: every pinned buffer, every output file, the page cache
        batched()
        loop(subset, scratch)
        torch.cuda.synchronize()
        laps = {'batched': [], 'loop': []}
        timeline = None
        for lap in range(arguments.laps):
            if lap == arguments.laps - 1:
                preprocess.TIMELINE = timeline = []
            start = time.perf_counter()
            batched()
            laps['batched'].append(
                len(paths) / (time.perf_counter() - start))
            preprocess.TIMELINE = None
            start = time.perf_counter()
            loop(subset, scratch)
            laps['loop'].append(len(subset) / (time.perf_counter() - start))
        # the two paths wrote the same bits
        for path in subset[:4]:
            stem = os.path.basename(path)[:-4]
            for kind in ('mels', 'loudness'):
                assert torch.equal(
                    torch.load(os.path.join(
                        directory, 'corpus', kind, f'{stem}.pt')),
                    torch.load(os.path.join(scratch, kind, f'{stem}.pt')))
        result = {'files': len(paths), 'subset': len(subset),
                  'per_batch': arguments.per_batch}
        for side, values in laps.items():
            median = statistics.median(values)
            result[side] = {
                'files_per_s': [round(v, 1) for v in values],
                'median': round(median, 1),
                'spread': round((max(values) - min(values)) / median, 4)}
        result['ratio'] = round(
            result['batched']['median'] / result['loop']['median'], 2)
        result['stages_ms'], result['wall_ms'] = stages(timeline)
        print(json.dumps(result))
        return result
    finally:
        shutil.rmtree(directory, ignore_errors=True)


def kernel(arguments):
    device = torch.device('cuda', arguments.gpu or 0)
    samples = [160000] * arguments.per_batch
    plan = preprocess.batch_plan(samples)
    table, floats = preprocess.unpack_table(plan, [(0, 80), (80, 1)])
    moved = 2 * 4 * int((table[:, 1] * table[:, 3]).sum())
    repeats = 10
    with torch.cuda.device(device):
        matrix = torch.randn(81, plan.ld_frames, device=device)
        out = torch.empty(floats, device=device)
        device_table = torch.from_numpy(table).to(device)
        begin = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        preprocess.unpack_rows(matrix, table, out, device_table)
        torch.cuda.synchronize()
        begin.record()
        for _ in range(repeats):
            preprocess.unpack_rows(matrix, table, out, device_table)
        end.record()
        torch.cuda.synchronize()
        unpack_us = begin.elapsed_time(end) * 1e3 / repeats

        def slices():
            return [matrix[row:row + rows, column:column + frames].clone()
                    for column, frames, row, rows, _ in table.tolist()]
        kept = slices()
        torch.cuda.synchronize()
        begin.record()
        for _ in range(repeats):
            kept = slices()
        end.record()
        torch.cuda.synchronize()
        slices_us = begin.elapsed_time(end) * 1e3 / repeats
        same = all(
            torch.equal(piece.reshape(-1),
                        out[target:target + piece.numel()])
            for piece, (_, _, _, _, target) in zip(kept, table.tolist()))
    print(json.dumps({
        'files': arguments.per_batch, 'entries': len(table),
        'bytes_read_plus_written': moved,
        'unpack_rows_us_events': round(unpack_us, 2),
        'unpack_rows_TBps_events': round(moved / unpack_us / 1e6, 3),
        'slice_copies': len(table),
        'slice_copies_us_events': round(slices_us, 1),
        'same_values': bool(same)}))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--files', type=int, default=4096)
    parser.add_argument('--subset', type=int, default=256)
    parser.add_argument('--laps', type=int, default=3)
    parser.add_argument('--per_batch', type=int, default=256)
    parser.add_argument('--gpu', type=int, default=0)
    parser.add_argument('--kernel', action='store_true')
    arguments = parser.parse_args()
    (kernel if arguments.kernel else throughput)(arguments)


if __name__ == '__main__':
    main()
