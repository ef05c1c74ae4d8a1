"""Forward + backward of `ops.logmel` against the same function as torch ops
on the same GPU, float32, 64 x 10 s of audio by default.

    python tools/logmel_backward_bench.py                     # alternating laps
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- \\
        python tools/logmel_backward_bench.py --only ours --laps 1
    python tools/logmel_backward_bench.py --kernel-stats <dir>   # merge the kernels' times

The torch contender restates `mels.from_audio` of the reference
(data/preprocess/mels.py:16-109): F.pad(reflect), torch.stft(1024, hop 160,
periodic Hann), sqrt(re^2 + im^2 + 1e-6), matmul with the bundled basis, log
of the clamp - per utterance batched as [64, S], autograd's backward.

Laps alternate between the contenders in one process on one box; a lap is
`--steps` forward + backward passes between two device synchronisations, timed
on the host clock.  The two kernels' own times come from a separate
`rocprofv3 --kernel-trace --stats` run (tracing slows the host), merged with
`--kernel-stats`.

Launch A's bound is worked out by counting, from the shapes, what the kernel
moves and computes (`launch_a_model`): LDS bytes, HBM bytes and floating-point
operations, each over the rate MI355X sustains for it.  The largest of the
three times is the bound the kernel sits on; the achieved fraction is that
time over the kernel's measured one.

The result goes to profiles/logmel_backward.json (`--output`) and one JSON
line to stdout."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNELS = {'launch_a': 'logmel_backward_frames_kernel',
           'launch_b': 'logmel_backward_fold_kernel',
           'forward': 'frontend_kernel'}
# MI355X rates: LDS with every CU streaming (ds_read_b64 150 TB/s, ds_write_b64
# about 45 TB/s), HBM as a float4 copy measures it, FP32 vector peak
LDS_READ, LDS_WRITE, HBM, FP32 = 150e12, 45e12, 6.29e12, 157.3e12


def launch_a_model(frames, tiles):
    """What launch A needs, from the shapes: seconds on each bound."""
    # per frame: two transforms of five passes, each 256 threads x 4 complex
    # read and written; the frame in, the spectrum out and in again, the
    # windowed result accumulated (read + write), 513 magnitudes twice
    complex_bytes = 8
    passes = 2 * 5 * 256 * 4 * complex_bytes
    lds_read = passes + (513 + 1024) * complex_bytes + (1024 + 2 * 1001) * 4
    lds_write = passes + (1024 + 1024) * complex_bytes + (1024 + 513) * 4
    # a radix-4 butterfly: three complex multiplications (6 flop) and eight
    # complex additions (2 flop); the rest of a frame is a few thousand
    flops = 2 * 5 * 256 * (3 * 6 + 8 * 2) + 2 * 1001 * 2 + 513 * 12 + 2048
    # HBM: the tile's samples once, its cotangent columns, its slot
    hbm = tiles * ((7 * 160 + 1024) * 4 + 80 * 8 * 4 + 2144 * 4)
    return {
        'lds_seconds': frames * (lds_read / LDS_READ + lds_write / LDS_WRITE),
        'hbm_seconds': hbm / HBM,
        # (additions and multiplications that do not pair into fma: half of peak)
        'valu_seconds': frames * flops / (FP32 / 2),
        'lds_bytes_per_frame': lds_read + lds_write, 'flops_per_frame': flops,
        'hbm_bytes': hbm}


def torch_logmel(audio, window, basis):
    """[N, S] -> [N, 80, F]: the reference's ATen ops."""
    import torch
    padded = torch.nn.functional.pad(audio[:, None], (432, 432), mode='reflect')[:, 0]
    stft = torch.stft(padded, 1024, hop_length=160, window=window, center=False,
                      normalized=False, onesided=True, return_complex=True)
    stft = torch.view_as_real(stft)
    magnitude = torch.sqrt(stft.pow(2).sum(-1) + 1e-6)
    return torch.log(torch.clamp(torch.matmul(basis, magnitude), min=1e-5))


def contenders(utterances, seconds):
    import numpy as np
    import torch
    import emphases_amd  # noqa: F401
    from emphases_amd import ops
    from oracle import prominence as oracle
    device = torch.device('cuda', 0)
    samples = seconds * 16000
    generator = torch.Generator().manual_seed(0)
    audio = (0.1 * torch.randn((utterances, samples), generator=generator)).to(device)
    frames = samples // 160
    cotangent = torch.randn((utterances, 80, frames), generator=generator).to(device)
    packed = audio.reshape(-1)
    packed_cotangent = cotangent.permute(1, 0, 2).reshape(80, -1).contiguous()
    cu = torch.tensor(np.arange(utterances + 1) * samples, dtype=torch.int64)
    window = oracle.hann_window().to(device)
    basis = oracle.mel_basis().to(device)

    def ours():
        leaf = packed.detach().requires_grad_()
        out = ops.logmel(leaf, cu)
        return torch.autograd.grad((out * packed_cotangent).sum(), leaf)[0]

    def theirs():
        leaf = audio.detach().requires_grad_()
        out = torch_logmel(leaf, window, basis)
        return torch.autograd.grad((out * cotangent).sum(), leaf)[0]

    return {'ours': ours, 'torch': theirs}, frames * utterances


def lap(function, steps):
    import torch
    torch.cuda.synchronize()
    begin = time.perf_counter()
    for _ in range(steps):
        function()
    torch.cuda.synchronize()
    return (time.perf_counter() - begin) / steps


def kernel_stats(directory):
    """{role: (calls, average seconds)} from rocprofv3's kernel_stats csv."""
    found = {}
    for path in glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'),
                          recursive=True):
        for row in csv.DictReader(open(path)):
            for role, name in KERNELS.items():
                if name in row['Name'] and role not in found:
                    found[role] = (int(row['Calls']), float(row['AverageNs']) * 1e-9)
    return found


def main():
    parser = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    parser.add_argument('--utterances', type=int, default=64)
    parser.add_argument('--seconds', type=int, default=10)
    parser.add_argument('--laps', type=int, default=7)
    parser.add_argument('--steps', type=int, default=10)
    parser.add_argument('--warmup', type=int, default=3)
    parser.add_argument('--only', choices=('ours', 'torch'))
    parser.add_argument('--kernel-stats', help='directory of a rocprofv3 '
                        '--kernel-trace --stats run to merge into --output')
    parser.add_argument('--output', default=os.path.join(
        ROOT, 'profiles', 'logmel_backward.json'))
    arguments = parser.parse_args()

    if arguments.kernel_stats:
        result = json.load(open(arguments.output))
        stats = kernel_stats(arguments.kernel_stats)
        if 'launch_a' not in stats:
            raise SystemExit('no kernel_stats.csv with the backward kernels under '
                             + arguments.kernel_stats)
        frames = result['frames']
        tiles = result['utterances'] * ((frames // result['utterances'] + 7) // 8)
        model = launch_a_model(frames, tiles)
        runs = (tiles + 4093) // 4094         # launches of A and of B per backward
        seconds = {role: stats[role][1] for role in stats}
        bound = max(('lds', 'hbm', 'valu'), key=lambda name: model[name + '_seconds'])
        result['kernels'] = {
            'launch_a_microseconds_per_backward': seconds['launch_a'] * runs * 1e6,
            'launch_b_microseconds_per_backward': seconds['launch_b'] * runs * 1e6,
            'forward_microseconds': seconds.get('forward', float('nan')) * 1e6,
            'launches_per_backward': 2 * runs,
            'launch_a_model': model,
            'launch_a_bound': bound,
            'launch_a_fraction_of_bound':
                model[bound + '_seconds'] / (seconds['launch_a'] * runs)}
        json.dump(result, open(arguments.output, 'w'), indent=1)
        print(json.dumps(result['kernels']))
        return

    import torch
    if not torch.cuda.is_available():
        raise SystemExit('logmel_backward_bench needs an MI355X: nothing is '
                         'measured without one')
    functions, frames = contenders(arguments.utterances, arguments.seconds)
    names = [arguments.only] if arguments.only else ['ours', 'torch']
    for name in names:
        for _ in range(arguments.warmup):
            functions[name]()
    times = {name: [] for name in names}
    for _ in range(arguments.laps):
        for name in names:                      # alternating
            times[name].append(lap(functions[name], arguments.steps))
    result = {'utterances': arguments.utterances, 'seconds': arguments.seconds,
              'frames': frames, 'laps': arguments.laps, 'steps': arguments.steps,
              'milliseconds': {
                  name: {'median': sorted(values)[len(values) // 2] * 1e3,
                         'min': min(values) * 1e3, 'max': max(values) * 1e3}
                  for name, values in times.items()}}
    if len(names) == 2:
        difference = float((functions['ours']().reshape(-1) -
                            functions['torch']().reshape(-1)).abs().max())
        scale = float(functions['torch']().abs().max())
        result['max_difference_over_max'] = difference / scale
        result['ours_over_torch'] = (result['milliseconds']['ours']['median'] /
                                     result['milliseconds']['torch']['median'])
    if not arguments.only:
        json.dump(result, open(arguments.output, 'w'), indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
