"""What a call through the `torch.ops.emphases_amd.*` seams costs against `Engine.forward`
on the same batch (BASELINE configs[1]: 64 x 10 s): the ops convert between the caller's
back-to-back layout and the library's packed one (one indexed copy each way); the plan of a
batch, its device tables and the copies' column indices come from a small cache keyed by the
`cu_*` / `bounds` values (`prominence_forward` alone builds its plan per call).

    python tools/ops_cost.py          -> one JSON object on stdout
    python tools/ops_cost.py --parent <checkout of the parent commit, built> [--laps 5] [--out FILE]

With `--parent` the forward of `conv1d_same_act` and of `segment_reduce` is also timed lap for
lap against the package of that checkout in a child process on the same GPU (`alternating`:
per-lap medians and their medians, parent and new).  A lap has two figures per op: `warm`, the
same arguments every call (the plan cache always hits), and `cold_plan`, 24 different `cu_frames`
in turn (more than the cache holds: every call builds its plan, as every call of the parent
does).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.environ.get('EMPHASES_BENCH_ROOT') or os.path.dirname(
    os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import emphases_amd  # noqa: E402
from emphases_amd import config as cfg  # noqa: E402

COLD_PLANS = 24


def clock(call, rounds=30):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    laps = []
    for _ in range(rounds):
        start = time.perf_counter()
        call()
        torch.cuda.synchronize()
        laps.append(time.perf_counter() - start)
    return float(np.median(laps)) * 1e3


class Seams:
    """The two differentiable ops' forward on the 64 x 10 s workload."""

    def __init__(self):
        device = torch.device('cuda', 0)
        audios, _, bounds = bench.workload(0)
        engine = emphases_amd.get_engine(None, 0)
        rng = np.random.default_rng(0)
        self.mel = torch.from_numpy(rng.standard_normal(
            (80, 1000 * len(audios))).astype(np.float32)).to(device)
        self.frames = torch.tensor([0] + [1000] * len(audios)).cumsum(0)
        # the same total, one frame moved between the first two segments
        self.cold = []
        for shift in range(COLD_PLANS):
            counts = [1000] * len(audios)
            counts[0], counts[1] = 1000 - shift, 1000 + shift
            self.cold.append(torch.tensor([0] + counts).cumsum(0))
        self.words = torch.tensor([0] + [b.shape[1] for b in bounds]).cumsum(0)
        self.bounds = torch.from_numpy(np.concatenate(bounds, axis=1))
        self.weight = torch.from_numpy(
            engine.state['input_layer.weight']).to(device)
        self.bias = torch.from_numpy(engine.state['input_layer.bias']).to(device)
        self.ops = torch.ops.emphases_amd
        self.hidden = self.ops.conv1d_same_act(
            self.mel, self.weight, self.bias, self.frames, 'relu')
        self.turn = 0

    def conv(self, frames=None):
        return self.ops.conv1d_same_act(
            self.mel, self.weight, self.bias,
            self.frames if frames is None else frames, 'relu')

    def reduce(self, frames=None):
        return self.ops.segment_reduce(
            self.hidden, self.bounds,
            self.frames if frames is None else frames, self.words, 'sum')

    def next_cold(self):
        self.turn = (self.turn + 1) % COLD_PLANS
        return self.cold[self.turn]

    def lap(self):
        return {
            'op_conv1d_same_act_ms': clock(self.conv),
            'op_segment_reduce_ms': clock(self.reduce),
            'op_conv1d_same_act_cold_plan_ms': clock(
                lambda: self.conv(self.next_cold()), rounds=2 * COLD_PLANS),
            'op_segment_reduce_cold_plan_ms': clock(
                lambda: self.reduce(self.next_cold()), rounds=2 * COLD_PLANS)}


def serve():
    """The child of `--parent`: a line on stdin -> one lap, as JSON."""
    seams = Seams()
    for _ in sys.stdin:
        print(json.dumps(seams.lap()), flush=True)


def alternate(directory, laps):
    directory = os.path.abspath(directory)
    child = subprocess.Popen(
        [sys.executable, os.path.abspath(__file__), '--serve'], cwd=directory,
        env=dict(os.environ, EMPHASES_BENCH_ROOT=directory),
        stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    seams = Seams()
    record = {'parent': [], 'new': []}
    try:
        for _ in range(laps):
            child.stdin.write('lap\n')
            child.stdin.flush()
            answer = child.stdout.readline()
            if not answer.strip():
                raise RuntimeError(
                    f"the parent checkout's process ended (exit status "
                    f'{child.wait()})')
            record['parent'].append(json.loads(answer))
            record['new'].append(seams.lap())
    finally:
        child.stdin.close()
        try:
            child.wait(timeout=60)
        except Exception:
            child.kill()
            child.wait()
    median = {side: {name: float(np.median([lap[name] for lap in rows]))
                     for name in rows[0]} for side, rows in record.items()}
    return {'laps': record, 'median': median,
            'new_over_parent': {name: median['new'][name] / median['parent'][name]
                                for name in median['new']}}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--parent', default=None)
    parser.add_argument('--laps', type=int, default=5)
    parser.add_argument('--out', default=None)
    parser.add_argument('--serve', action='store_true', help=argparse.SUPPRESS)
    arguments = parser.parse_args()
    if arguments.serve:
        return serve()
    device = torch.device('cuda', 0)
    audios, alignments, bounds = bench.workload(0)
    engine = emphases_amd.get_engine(None, 0)
    plan = bench.build_plan(audios, alignments)
    packed = torch.cat([torch.from_numpy(a).reshape(-1) for a in audios]).to(device)
    meta = engine.upload(plan)
    result = {'workload': '64 x 10 s, conv config, audio resident on the device'}
    result['engine_forward_eager_ms'] = clock(
        lambda: engine.forward(packed, plan, meta))
    replay, _, _ = engine.capture(packed, plan, meta)
    result['engine_graph_replay_ms'] = clock(replay)
    samples = torch.tensor([0] + [a.shape[1] for a in audios]).cumsum(0)
    words = torch.tensor([0] + [b.shape[1] for b in bounds]).cumsum(0)
    all_bounds = torch.from_numpy(np.concatenate(bounds, axis=1))
    ops = torch.ops.emphases_amd
    result['op_prominence_forward_ms'] = clock(
        lambda: ops.prominence_forward(packed, samples, all_bounds, words))
    result['op_logmel_ms'] = clock(lambda: ops.logmel(packed, samples))
    mel = ops.logmel(packed, samples)
    frames = torch.tensor([0] + [1000] * len(audios)).cumsum(0)
    weight = torch.from_numpy(engine.state['input_layer.weight']).to(device)
    bias = torch.from_numpy(engine.state['input_layer.bias']).to(device)
    result['op_conv1d_same_act_ms'] = clock(
        lambda: ops.conv1d_same_act(mel, weight, bias, frames, 'relu'))
    hidden = ops.conv1d_same_act(mel, weight, bias, frames, 'relu')
    result['op_segment_reduce_ms'] = clock(
        lambda: ops.segment_reduce(hidden, all_bounds, frames, words, 'sum'))
    # the layout conversion alone: one indexed copy in, one out
    from emphases_amd import ops as module
    layout = module._layout(device, np.asarray(plan.frames, dtype=np.int64))
    result['scatter_plus_gather_ms'] = clock(lambda: layout.scatter(
        mel, layout.frame_columns, layout.plan.ld_frames).index_select(
            1, layout.frame_columns))
    if arguments.parent:
        result['device'] = torch.cuda.get_device_name(0)
        result['alternating'] = alternate(arguments.parent, arguments.laps)
    print(json.dumps(result))
    if arguments.out:
        with open(arguments.out, 'w') as file:
            json.dump(result, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
