"""The frame-rate head's launches at the training size, kernel by kernel,
against the composition the general entry points already allow.

    python tools/frame_head_bench.py [--repeats 20] [--out profiles/frame_head_kernels.json]

75 utterances x 1 000 frames x 30 words (tools/train_bench.py's batch), h
[80, ld_frames] random.  Timed with the library's launch timer
(`runtime.LaunchTimer`: the kernel's own begin -> end), median over
`--repeats` calls, every launch of a call added up:

  emph_frame_head            against  emph_conv1d with c_out = 1
  emph_frame_head_backward   against  emph_conv_weight_grad_any with c_out = 1
                                      + emph_conv1d on the flipped 1 -> 80 pack
  emph_frame_loss_grad, emph_upsample (C = 1): no substitute

and reported as microseconds and as the fraction of the 6.29 TB/s copy rate
(EXPERIMENTS.md) that the bytes each must move amount to: h once for the
forward, h once and dx once for the backward.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import train_bench  # noqa: E402

from emphases_amd import core as api  # noqa: E402
from emphases_amd import runtime  # noqa: E402

COPY_RATE = 6.29e12
CHANNELS = 80


def measure(function, repeats):
    """Median over `repeats` calls of the summed kernel time of a call (us),
    and the launches of a call."""
    function()
    torch.cuda.synchronize()
    totals, launches = [], 0
    for _ in range(repeats):
        with runtime.LaunchTimer() as timer:
            function()
        totals.append(float(timer.microseconds.sum()))
        launches = timer.launches
    return float(np.median(totals)), launches


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--out', default=None)
    arguments = parser.parse_args()
    torch.cuda.set_device(0)
    lib = runtime.library()
    _, frame_lengths, bounds, word_lengths, targets = train_bench.make_batch()
    frames = [int(n) for n in frame_lengths]
    words = [int(n) for n in word_lengths]
    plan = api._packed_plan(frames, bounds, words)
    host, offsets = plan.pack_metadata([(runtime.AXIS_FRAMES, 64)])
    meta = torch.from_numpy(host).cuda()
    view = lambda name: meta[  # noqa: E731
        offsets[name][0]:offsets[name][0] + offsets[name][1]]
    tiles = view(('tiles', runtime.AXIS_FRAMES, 64))
    n_tiles = tiles.numel() // runtime.TILE_FIELDS
    ld_f, ld_w = plan.ld_frames, plan.ld_words
    generator = torch.Generator().manual_seed(0)
    h = torch.randn(CHANNELS, ld_f, generator=generator).cuda()
    dlogit = torch.randn(1, ld_f, generator=generator).cuda()
    weight = (torch.randn(1, CHANNELS, 3, generator=generator) / 15.)
    bias = torch.zeros(1).cuda()
    packed_targets = torch.zeros(ld_w)
    for i, (off, count) in enumerate(zip(plan.word_off, words)):
        packed_targets[off:off + count] = targets[i, 0, :count]
    packed_targets = packed_targets.cuda()
    logits = torch.zeros(1, ld_f).cuda()
    dx = torch.zeros(CHANNELS, ld_f).cuda()
    dweight, dbias = torch.zeros(1, CHANNELS, 3).cuda(), torch.zeros(1).cuda()
    loss = torch.zeros(1).cuda()
    partials = torch.zeros(n_tiles, dtype=torch.float64).cuda()
    slabs = torch.zeros(
        int(lib.emph_frame_head_parts(n_tiles)) * (3 * CHANNELS + 1)).cuda()
    device_weight = weight.cuda()
    forward_pack = torch.from_numpy(runtime.conv_pack(weight.numpy())).cuda()
    flipped = np.ascontiguousarray(
        weight.numpy().transpose(1, 0, 2)[:, :, ::-1])
    backward_pack = torch.from_numpy(runtime.conv_pack(flipped)).cuda()
    any_workspace = torch.zeros(max(1, int(
        lib.emph_conv_weight_grad_any_workspace(
            CHANNELS, 1, 3, n_tiles)))).cuda()
    stream = runtime.stream()

    def head():
        runtime.check(lib.emph_frame_head(
            h.data_ptr(), ld_f, device_weight.data_ptr(), bias.data_ptr(),
            CHANNELS, 3, tiles.data_ptr(), n_tiles, logits.data_ptr(),
            stream), 'emph_frame_head')

    def head_composed():
        runtime.check(lib.emph_conv1d(
            h.data_ptr(), ld_f, logits.data_ptr(), ld_f,
            forward_pack.data_ptr(), bias.data_ptr(), CHANNELS, 1, 3, 0,
            tiles.data_ptr(), n_tiles, 64, 0, stream), 'emph_conv1d')

    def backward():
        runtime.check(lib.emph_frame_head_backward(
            dlogit.data_ptr(), h.data_ptr(), ld_f, device_weight.data_ptr(),
            CHANNELS, 3, tiles.data_ptr(), n_tiles, slabs.data_ptr(),
            dweight.data_ptr(), dbias.data_ptr(), dx.data_ptr(), ld_f,
            stream), 'emph_frame_head_backward')

    def backward_composed():
        runtime.check(lib.emph_conv_weight_grad_any(
            dlogit.data_ptr(), ld_f, h.data_ptr(), ld_f, CHANNELS, 1, 3,
            tiles.data_ptr(), n_tiles, 64, any_workspace.data_ptr(),
            dweight.data_ptr(), dbias.data_ptr(), stream),
            'emph_conv_weight_grad_any')
        runtime.check(lib.emph_conv1d(
            dlogit.data_ptr(), ld_f, dx.data_ptr(), ld_f,
            backward_pack.data_ptr(), None, 1, CHANNELS, 3, 0,
            tiles.data_ptr(), n_tiles, 64, 0, stream), 'emph_conv1d')

    def loss_grad():
        runtime.check(lib.emph_frame_loss_grad(
            logits.data_ptr(), packed_targets.data_ptr(),
            view('bounds').data_ptr(), ld_w, view('table').data_ptr(),
            tiles.data_ptr(), n_tiles, plan.total_frames, 0, 0,
            partials.data_ptr(), loss.data_ptr(), dlogit.data_ptr(), stream),
            'emph_frame_loss_grad')

    def upsample():
        runtime.check(lib.emph_upsample(
            packed_targets.data_ptr(), ld_w, view('bounds').data_ptr(),
            logits.data_ptr(), ld_f, 1, view('table').data_ptr(),
            tiles.data_ptr(), n_tiles, 0, stream), 'emph_upsample')

    h_bytes = 4 * CHANNELS * plan.total_frames
    moved = {'emph_frame_head': h_bytes, 'composed_forward': h_bytes,
             'emph_frame_head_backward': 2 * h_bytes,
             'composed_backward': 2 * h_bytes,
             'emph_frame_loss_grad': 8 * plan.total_frames,
             'emph_upsample': 4 * plan.total_frames}
    record = {'batch': {'utterances': len(frames), 'frames': frames[0],
                        'words': words[0]},
              'device': torch.cuda.get_device_name(0), 'tiles': n_tiles,
              'copy_rate_bytes_per_second': COPY_RATE, 'kernels': {}}
    # (the composition first: the dedicated kernels' results are what is left
    # in the buffers that loss_grad then reads)
    for name, function in (
            ('composed_forward', head_composed), ('emph_frame_head', head),
            ('composed_backward', backward_composed),
            ('emph_frame_head_backward', backward),
            ('emph_upsample', upsample), ('emph_frame_loss_grad', loss_grad)):
        microseconds, launches = measure(function, arguments.repeats)
        record['kernels'][name] = {
            'microseconds': microseconds, 'launches': launches,
            'bytes': moved[name],
            'fraction_of_copy_rate':
                moved[name] / (microseconds * 1e-6) / COPY_RATE}
    print(json.dumps(record))
    if arguments.out:
        with open(arguments.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
