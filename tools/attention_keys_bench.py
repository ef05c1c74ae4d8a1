"""Launch times of `emph_attention_backward_keys`, by the library's own launch
timer (kernel begin -> end of each dispatch).

    python tools/attention_keys_bench.py --out profiles/attention_backward_keys_kernels.json \\
        [--parent <checkout of the parent commit, built>] [--laps 7]

1. The piece layout: the 75 x 1000 frames x 30 words of `train_bench`, every
   word a segment padded to the longest word of its utterance (what
   `batch.Pieces` builds), `key_counts` the words' real lengths.
   `emph_attention_backward_keys` against `emph_attention_backward` on the same
   layout without a mask - the work a caller without the table would do - in
   alternating laps.
2. No regression of the plain entry: `emph_attention_backward` on 75 segments
   of 1000 positions, this checkout against `--parent`, each in a child
   process of its own (this file's `--serve` on that checkout's package), in
   alternating laps.  A lap is the median over `--repeats` calls of the two
   launches' sum.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import train_bench  # noqa: E402  (puts the repository root on sys.path)

from emphases_amd import ops, runtime  # noqa: E402


class Buffers:
    """Random Q | K, V, dO and `out` of the forward on the segments `lengths`."""

    def __init__(self, lengths, keys=None):
        self.device = device = torch.device('cuda', 0)
        layout = ops._layout(device, np.asarray(lengths, dtype=np.int64))
        self.ld = ld = layout.plan.ld_frames
        self.tiles, self.n_tiles = layout.tiles(64)
        generator = torch.Generator(device='cuda').manual_seed(0)
        self.qk = torch.randn(160, ld, device=device, generator=generator)
        self.v = torch.randn(ld, 80, device=device, generator=generator)
        self.dout = torch.randn(80, ld, device=device, generator=generator)
        self.dqkv = torch.zeros(240, ld, device=device)
        self.lib = runtime.library()
        self.workspace = torch.empty(
            int(self.lib.emph_attention_backward_workspace(ld, 2)),
            device=device)
        self.table = None if keys is None else torch.tensor(
            keys, dtype=torch.int32, device=device)
        self.out = {None: self.forward(None)}
        if keys is not None:
            self.out['keys'] = self.forward(self.table)

    def forward(self, table):
        out = torch.zeros(80, self.ld, device=self.device)
        runtime.check(self.lib.emph_attention(
            self.qk.data_ptr(), self.v.data_ptr(), out.data_ptr(), self.ld,
            80, 2, self.tiles.data_ptr(), self.n_tiles, 64,
            None if table is None else table.data_ptr(), runtime.stream()),
            'emph_attention')
        return out

    def lap(self, keys, repeats):
        """Median microseconds of (query pass, key pass) over `repeats`."""
        head = (self.qk.data_ptr(), self.v.data_ptr(),
                self.out['keys' if keys else None].data_ptr(),
                self.dout.data_ptr(), self.dqkv.data_ptr(), self.ld, 80, 2,
                self.tiles.data_ptr(), self.n_tiles, 64)
        with runtime.LaunchTimer() as timer:
            for _ in range(repeats):
                if keys:
                    status = self.lib.emph_attention_backward_keys(
                        *head, self.table.data_ptr(),
                        self.workspace.data_ptr(), runtime.stream())
                else:
                    status = self.lib.emph_attention_backward(
                        *head, self.workspace.data_ptr(), runtime.stream())
                runtime.check(status, 'emph_attention_backward')
        times = np.asarray(timer.microseconds, dtype=np.float64)
        return [float(np.median(times[0::2])), float(np.median(times[1::2]))]


def piece_layout():
    """(padded lengths, real lengths) of every word of `train_bench`'s batch."""
    bounds = train_bench.make_batch(0)[2].numpy()
    lengths, keys = [], []
    for item in bounds:
        real = item[1] - item[0]
        lengths.extend([int(real.max())] * real.size)
        keys.extend(int(n) for n in real)
    return lengths, keys


def serve(repeats):
    """The child of the no-regression comparison: a line in, a lap out."""
    torch.cuda.set_device(0)
    buffers = Buffers([train_bench.FRAMES] * train_bench.ITEMS)
    buffers.lap(False, 2)
    for _ in sys.stdin:
        print(sum(buffers.lap(False, repeats)), flush=True)


class Child:
    def __init__(self, directory, repeats):
        directory = os.path.abspath(directory)
        self.process = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), '--serve',
             '--repeats', str(repeats)],
            cwd=directory, env=dict(os.environ, EMPHASES_BENCH_ROOT=directory),
            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def lap(self, seconds=120.):
        """A lap of the child, or RuntimeError when it does not answer in
        `seconds` (the caller then kills every child)."""
        import select
        self.process.stdin.write('1\n')
        self.process.stdin.flush()
        ready, _, _ = select.select([self.process.stdout], [], [], seconds)
        line = self.process.stdout.readline() if ready else ''
        if not line.strip():
            raise RuntimeError('a child of the comparison gave no lap')
        return float(line)

    def close(self):
        """Ends the child; killed if it does not leave by itself."""
        try:
            self.process.stdin.close()
            self.process.wait(timeout=30)
        except Exception:
            self.process.kill()
            self.process.wait()


def summary(laps):
    return {'us_median': float(np.median(laps)), 'us_min': float(min(laps)),
            'us_max': float(max(laps)), 'us_laps': laps}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    parser.add_argument('--parent', default=None)
    parser.add_argument('--laps', type=int, default=7)
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--serve', action='store_true')
    arguments = parser.parse_args()
    if arguments.serve:
        return serve(arguments.repeats)
    torch.cuda.set_device(0)
    lengths, keys = piece_layout()
    buffers = Buffers(lengths, keys)
    record = {
        'device': torch.cuda.get_device_name(0),
        'timer': "the library's launch timer: kernel begin -> end",
        'pieces': {
            'layout': {'segments': len(lengths), 'positions': int(sum(lengths)),
                       'real_positions': int(sum(keys)),
                       'longest': int(max(lengths))},
            'laps': arguments.laps, 'repeats': arguments.repeats}}
    laps = {name: {'queries': [], 'keys': [], 'both': []}
            for name in ('emph_attention_backward_keys',
                         'emph_attention_backward')}
    buffers.lap(True, 2)
    buffers.lap(False, 2)
    for _ in range(arguments.laps):
        for name, masked in (('emph_attention_backward_keys', True),
                             ('emph_attention_backward', False)):
            queries, key_pass = buffers.lap(masked, arguments.repeats)
            laps[name]['queries'].append(queries)
            laps[name]['keys'].append(key_pass)
            laps[name]['both'].append(queries + key_pass)
    for name, passes in laps.items():
        record['pieces'][name] = {
            which: summary(values) for which, values in passes.items()}
    record['pieces']['keys_over_unmasked'] = \
        record['pieces']['emph_attention_backward_keys']['both']['us_median'] / \
        record['pieces']['emph_attention_backward']['both']['us_median']
    if arguments.parent:
        root = os.path.dirname(HERE)
        children = {'this': Child(root, arguments.repeats),
                    'parent': Child(arguments.parent, arguments.repeats)}
        times = {name: [] for name in children}
        try:
            for child in children.values():
                child.lap()                               # (warms up)
            for _ in range(arguments.laps):
                for name, child in children.items():
                    times[name].append(child.lap())
        except BaseException:
            for child in children.values():
                child.process.kill()
            raise
        finally:
            for child in children.values():
                child.close()
        this, parent = summary(times['this']), summary(times['parent'])
        record['emph_attention_backward_75x1000'] = {
            'this': this, 'parent': parent,
            'this_over_parent': this['us_median'] / parent['us_median'],
            'median_within_the_parents_lap_range': bool(
                parent['us_min'] <= this['us_median'] <= parent['us_max']),
            'median_at_or_below_the_parents_slowest_lap': bool(
                this['us_median'] <= parent['us_max'])}
    print(json.dumps(record))
    if arguments.out:
        with open(arguments.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
