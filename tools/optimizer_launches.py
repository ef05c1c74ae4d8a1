"""The optimizer part of a Transformer training step alone, to be counted
under a kernel trace:

    rocprofv3 --kernel-trace --stats -d <directory> -- \
        python tools/optimizer_launches.py --kind gathered [--updates 20]
    rocprofv3 --kernel-trace --stats -d <directory> -- \
        python tools/optimizer_launches.py --kind torch [--updates 20]

One forward and backward of the 6 + 6 layer model on a small batch leaves
the 148 gradients where autograd puts them; then `--updates` Adam updates
run and nothing else: `torch.optim.Adam.step()` over the model's parameters
('torch': what a step did before `TransformerTrainer`), or
`emph_adam_step_gathered` over the trainer's flat state ('gathered').  The
kernels of the updates divide by `--updates` in the trace's statistics; those
of the one forward and backward do not, which tells them apart.  Prints the
number of parameter tensors and of updates as one JSON line."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import runtime, train  # noqa: E402


def small_batch():
    """Two utterances of 200 frames and 10 words, collated."""
    rng = np.random.default_rng(0)
    items, frames, words = 2, 200, 10
    edges = np.linspace(0, frames, words + 1).astype(np.int64)
    bounds = torch.from_numpy(np.stack([edges[:-1], edges[1:]]))
    return (torch.from_numpy(
        rng.standard_normal((items, 80, frames)).astype(np.float32)),
        torch.full((items,), frames), bounds[None].repeat(items, 1, 1),
        torch.full((items,), words),
        torch.from_numpy(rng.uniform(0., 1., (items, 1, words)).astype(
            np.float32)))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--kind', choices=('torch', 'gathered'), required=True)
    parser.add_argument('--updates', type=int, default=20)
    arguments = parser.parse_args()
    torch.cuda.set_device(0)
    config = emphases_amd.Config(architecture='transformer', layers=6)
    trainer = train.TransformerTrainer(config, gpu=0)
    batch = trainer.prepare(*small_batch())
    trainer._loss_backward(batch)
    parameters = trainer._tensors
    assert all(p.grad is not None for p in parameters)
    if arguments.kind == 'torch':
        optimizer = torch.optim.Adam(parameters)
        for _ in range(arguments.updates):
            optimizer.step()
    else:
        addresses = np.array(
            [p.grad.data_ptr() for p in parameters], dtype=np.uint64)
        for step in range(1, arguments.updates + 1):
            runtime.check(trainer.lib.emph_adam_step_gathered(
                trainer.parameters.data_ptr(), addresses.ctypes.data,
                trainer._firsts.ctypes.data, trainer._sizes.ctypes.data,
                len(parameters), trainer.exp_avg.data_ptr(),
                trainer.exp_avg_sq.data_ptr(), 0.9, 0.999,
                1e-3 / (1. - 0.9 ** step), math.sqrt(1. - 0.999 ** step),
                1e-8, runtime.stream()), 'emph_adam_step_gathered')
    torch.cuda.synchronize()
    print(json.dumps({'kind': arguments.kind, 'updates': arguments.updates,
                      'parameter_tensors': len(parameters)}))


if __name__ == '__main__':
    main()
