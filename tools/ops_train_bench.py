"""One training step through the differentiable operator seams, against
PyTorch and against the fused trainer.

    python tools/ops_train_bench.py [--laps 7] [--seconds 1.0] [--out profiles/ops_train_step.json]

The batch and the baselines are `tools/train_bench.py`'s: 75 utterances x
1 000 frames x 30 words, default configuration, weights of `emphases.Model()`
under seed 0.  Three contenders run in ALTERNATING laps of the same process on
the same GPU:

  ops         forward + backward + `torch.optim.Adam` step of
              `emphases_amd.train.TorchModel` (every layer a
              `torch.ops.emphases_amd` op, its backward the library's kernels)
  torch_fp32  the same model as torch.nn.Conv1d + ReLU modules and autograd
              (`train_bench.TorchModel`), float32
  trainer     `emphases_amd.train.Trainer.step` on a prepared batch

A lap of one contender is timed with a pair of device events around `steps`
steps, `steps` chosen so that a lap takes about `--seconds`; all are warmed up
first (the ops' second step is the first on device-packed weights).
Reported: median, minimum and maximum per-step time over the laps.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import train_bench  # noqa: E402  (puts the repository root on sys.path)

import emphases_amd  # noqa: E402
from emphases_amd import train  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--laps', type=int, default=7)
    parser.add_argument('--seconds', type=float, default=1.0)
    parser.add_argument('--steps', type=int, default=None)
    parser.add_argument('--out', default=None)
    arguments = parser.parse_args()
    torch.cuda.set_device(0)
    batch = train_bench.make_batch()
    features, _, bounds, _, targets = batch
    items, frames, words = \
        train_bench.ITEMS, train_bench.FRAMES, train_bench.WORDS
    state = train.initial_state(emphases_amd.DEFAULT, seed=0)

    # ---- ops: the batch back to back
    model = train.TorchModel(emphases_amd.DEFAULT, checkpoint=state).cuda()
    optimizer = torch.optim.Adam(model.parameters())
    flat = (features.permute(1, 0, 2).reshape(80, items * frames).cuda(),
            torch.arange(items + 1) * frames,
            bounds.permute(1, 0, 2).reshape(2, items * words),
            torch.arange(items + 1) * words)
    flat_targets = targets.reshape(items * words).cuda()

    def ops_step():
        optimizer.zero_grad(set_to_none=True)
        loss = train.loss_fn(model(*flat), flat_targets, 'bce')
        loss.backward()
        optimizer.step()
        return loss.detach()

    # ---- torch.nn.Conv1d + autograd, and the fused trainer
    device_features, device_bounds, device_targets = \
        features.cuda(), bounds.cuda(), targets.cuda()
    frame = torch.arange(frames, device='cuda')[None, :, None]
    membership = ((frame >= device_bounds[:, 0, None, :]) &
                  (frame < device_bounds[:, 1, None, :])).float()
    plain = train_bench.TorchModel(state).cuda()
    plain_optimizer = torch.optim.Adam(plain.parameters())
    fused = train.Trainer(checkpoint=state, gpu=0)
    prepared = fused.prepare(*batch)
    contenders = {
        'ops': ops_step,
        'torch_fp32': lambda: train_bench.torch_step(
            plain, plain_optimizer, None, device_features, membership,
            device_targets),
        'trainer': lambda: fused.step(prepared)}

    first = {}
    for name, function in contenders.items():
        first[name] = float(function())
        for _ in range(4):
            function()
    torch.cuda.synchronize()
    steps = {}
    for name, function in contenders.items():
        probe = train_bench.timed(function, 5)
        steps[name] = arguments.steps or max(
            5, int(arguments.seconds * 1e3 / probe))
    laps = {name: [] for name in contenders}
    for _ in range(arguments.laps):
        for name, function in contenders.items():
            laps[name].append(train_bench.timed(function, steps[name]))
    record = {
        'batch': {'utterances': items, 'frames': frames, 'words': words},
        'device': torch.cuda.get_device_name(0),
        'laps': arguments.laps, 'steps_per_lap': steps, 'first_loss': first,
        'ms_per_step': {
            name: {'median': float(np.median(values)),
                   'min': float(np.min(values)), 'max': float(np.max(values))}
            for name, values in laps.items()},
        'ms_per_step_laps': laps}
    median = {name: record['ms_per_step'][name]['median'] for name in laps}
    record['torch_fp32_over_ops'] = median['torch_fp32'] / median['ops']
    record['ops_over_trainer'] = median['ops'] / median['trainer']
    print(json.dumps(record))
    if arguments.out:
        with open(arguments.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
