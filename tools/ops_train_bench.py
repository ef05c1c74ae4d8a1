"""One training step through the differentiable operator seams, against
PyTorch and against the fused trainer.

    python tools/ops_train_bench.py [--laps 7] [--seconds 1.0] [--out profiles/ops_train_step.json]
    python tools/ops_train_bench.py --architecture transformer \
        [--out profiles/ops_transformer_train_step.json] \
        [--kernels-out profiles/attention_backward_kernels.json]
    python tools/ops_train_bench.py --architecture transformer --precision bf16x3 \
        [--parent <checkout of the parent commit, built>] \
        [--out profiles/ops_transformer_train_step_bf16x3.json] \
        [--kernels-out profiles/attention_backward_split_kernels.json]

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

`--architecture transformer`: the same batch through
`emphases_amd.train.TransformerModel` (6 layers, 'intermediate': `ops`)
against the same model as `torch.nn.TransformerEncoder(dropout=0.)` +
autograd + Adam in float32 (`torch_fp32`), laps alternating.  `--kernels-out`
adds the launch timer's per-kernel times of `emph_attention` and
`emph_attention_backward` on one layer's shapes (75 x 1 000 positions, 2
heads of 40), the MFMA flops they execute over the 157.3 TFLOP/s fp32 peak,
and torch's own `scaled_dot_product_attention` forward and backward on the
same shapes with the backend torch picked.

`--reference_dropout` (with `--architecture transformer`): three contenders
in the same alternation - `ops_dropout`, the step of
`TransformerModel(reference_dropout=True)` (the reference's five dropouts as
specified masks, `steps` advanced per update), `ops`, the default model
without dropout (the code path every earlier figure was taken on), and
`torch_fp32_dropout`, `torch.nn.TransformerEncoder(dropout=0.1)` plus the
positional dropout of 0.1 under autograd and Adam in float32.  `--kernels-out`
then also times `emph_attention_dropout` and the two passes of
`emph_attention_dropout_backward` (p = 0.1) beside the plain kernels.

`--precision bf16x3` (with `--architecture transformer`): `ops_bf16x3`, the
step of `TransformerModel(precision='bf16x3')`, in the same alternation as
`ops` (the f32 model of this checkout) and `torch_fp32`.  `--parent
DIRECTORY` (with `--architecture transformer`, at either precision) adds
`ops_parent`, the f32 step of the package of that checkout in a child process
(this file's `--serve`), lap for lap between the others.
`--kernels-out` then times the split launches - `emph_split_kv` +
`emph_attention_split` and the three launches of
`emph_attention_backward_split` - beside `emph_attention` and
`emph_attention_backward` in the same run, with the MFMA flops they execute
over the bf16 peak.

`--trainer` (with `--architecture transformer`, at either precision):
`trainer`, `emphases_amd.train.TransformerTrainer.step` on the prepared batch,
against `ops`, the step of `TransformerModel` + `torch.optim.Adam` of this
checkout at the same precision, and - `--parent DIRECTORY` - `ops_parent`,
the same of that checkout.  `ops` and `ops_parent` each run in a child
process (this file's `--serve`), lap for lap between the trainer's: two sets
of 148 parameters stepping in one process outgrow the 256 entries of the ops'
weight caches, and each would evict the other's on every step.  The record
says whether the trainer's median lap is above the `ops` median by more than
the laps' own spread.

    python tools/ops_train_bench.py --architecture transformer --trainer \
        [--precision bf16x3] [--parent <checkout, built>] \
        [--out profiles/transformer_trainer_step.json]
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


PEAK_FP32_MFMA = 157.3e12
PEAK_BF16_MFMA = 16 * PEAK_FP32_MFMA      # the bf16 matrix rate


class TorchTransformer(torch.nn.Module):
    """`emphases.Model` under ARCHITECTURE 'transformer', 'intermediate' +
    'sum', on a batch of equal lengths (no padding mask); `dropout` is the
    probability of the layers' dropouts and of the positional one (the
    reference's 0.1), 0 for none."""

    def __init__(self, config, state, dropout=0.):
        super().__init__()
        from emphases_amd import weights
        self.dropout = dropout
        stack = lambda: torch.nn.TransformerEncoder(  # noqa: E731
            torch.nn.TransformerEncoderLayer(
                80, 2, dim_feedforward=80, dropout=dropout), config.layers,
            enable_nested_tensor=False)
        self.input_layer = torch.nn.Conv1d(80, 80, 3, padding='same')
        self.frame_encoder = stack()
        self.word_decoder = stack()
        self.output_layer = torch.nn.Conv1d(80, 1, 3, padding='same')
        self.register_buffer('encoding', torch.from_numpy(
            weights.positional_encoding(1000, 80))[:, None], persistent=False)
        self.load_state_dict(
            {name.replace('.model.', '.'): torch.from_numpy(value)
             for name, value in state.items()})

    def positioned(self, x):
        return torch.nn.functional.dropout(
            x + self.encoding[:x.shape[0]], self.dropout, self.training)

    def forward(self, features, membership):
        x = self.input_layer(features).permute(2, 0, 1)            # [T, B, C]
        x = self.frame_encoder(self.positioned(x))
        words = torch.bmm(x.permute(1, 2, 0), membership)           # [B, C, W]
        words = words.permute(2, 0, 1)
        words = self.word_decoder(self.positioned(words))
        return self.output_layer(words.permute(1, 2, 0))


class TorchLocations(torch.nn.Module):
    """`emphases.Model` under ARCHITECTURE 'transformer' at 'input' (the
    pieces [P, 80, L] padded to the BATCH's longest word, as the reference's
    own training batch pads them, behind `src_key_padding_mask`; 'sum' over
    the padded axis; the word decoder) or at 'inference' in training (the
    frame-rate head); no dropout."""

    def __init__(self, config, state):
        super().__init__()
        from emphases_amd import weights
        self.location = config.downsample_location
        stack = lambda: torch.nn.TransformerEncoder(  # noqa: E731
            torch.nn.TransformerEncoderLayer(
                80, 2, dim_feedforward=80, dropout=0.), config.layers,
            enable_nested_tensor=False)
        self.input_layer = torch.nn.Conv1d(80, 80, 3, padding='same')
        self.frame_encoder = stack()
        if config.has_decoder:
            self.word_decoder = stack()
        self.output_layer = torch.nn.Conv1d(80, 1, 3, padding='same')
        self.register_buffer('encoding', torch.from_numpy(
            weights.positional_encoding(1000, 80))[:, None], persistent=False)
        self.load_state_dict(
            {name.replace('.model.', '.'): torch.from_numpy(value)
             for name, value in state.items()})

    def forward(self, x, mask=None, items=0):
        x = self.input_layer(x).permute(2, 0, 1)                   # [L, P, C]
        x = self.frame_encoder(x + self.encoding[:x.shape[0]],
                               src_key_padding_mask=mask)
        if self.location == 'inference':
            return self.output_layer(x.permute(1, 2, 0))            # [B, 1, T]
        words = x.sum(0).reshape(items, -1, x.shape[2]).permute(1, 0, 2)
        words = self.word_decoder(words + self.encoding[:words.shape[0]])
        return self.output_layer(words.permute(1, 2, 0))            # [B, 1, W]


def locations_main(arguments):
    """`--trainer --downsample_location {input,inference}`:
    `TransformerLocationsTrainer.step` against the same model as
    `torch.nn.TransformerEncoder(dropout=0.)` + `torch.optim.Adam` in fp32,
    alternating laps; per step and per column (at 'input' torch needs ONE
    length for its batch, the batch's longest word, where the trainer pads a
    word to its utterance's longest)."""
    torch.cuda.set_device(0)
    location = arguments.downsample_location
    items, frames, words = \
        train_bench.ITEMS, train_bench.FRAMES, train_bench.WORDS
    config = emphases_amd.Config(
        architecture='transformer', layers=6, downsample_location=location)
    trainer = train.TransformerLocationsTrainer(config, gpu=0)
    state = {name: value.numpy() for name, value in
             trainer.state_dict().items()}
    batch = train_bench.make_batch()
    features, frame_lengths, bounds, word_lengths, targets = batch
    prepared = trainer.prepare(*batch)
    plain = TorchLocations(config, state).cuda().train()
    optimizer = torch.optim.Adam(plain.parameters())
    loss_fn = torch.nn.functional.binary_cross_entropy_with_logits
    if location == 'input':
        lengths = (bounds[:, 1] - bounds[:, 0]).reshape(-1)          # [P]
        longest = int(lengths.max())
        position = torch.arange(longest)[None]
        mask = (position >= lengths[:, None]).cuda()                 # [P, L]
        item = torch.arange(items).repeat_interleave(words)
        source = (item * frames + bounds[:, 0].reshape(-1))[:, None] + position
        flat = torch.cat([features.permute(1, 0, 2).reshape(80, -1),
                          torch.zeros(80, 1)], dim=1)
        source = torch.where(mask.cpu(), torch.tensor(items * frames), source)
        pieces = flat[:, source].permute(1, 0, 2).contiguous().cuda()
        wanted = targets.cuda()
        torch_columns = int(pieces.shape[0] * longest)
        ours = np.repeat((bounds[:, 1] - bounds[:, 0]).max(dim=1).values
                         .numpy(), words)
        columns = int(sum((int(n) + 15) // 16 * 16 for n in ours))
        forward = lambda: plain(pieces, mask, items)  # noqa: E731
    else:
        spread = emphases_amd.upsample(
            targets.cuda(), bounds, word_lengths, frame_lengths, config)
        wanted = spread.clamp(0., 1.)
        device_features = features.cuda()
        torch_columns = columns = items * frames
        forward = lambda: plain(device_features)  # noqa: E731

    def torch_step():
        optimizer.zero_grad(set_to_none=True)
        loss = loss_fn(forward(), wanted)
        loss.backward()
        optimizer.step()
        return loss.detach()

    contenders = {'trainer': lambda: trainer.step(prepared),
                  'torch_fp32': torch_step}
    first, steps = {}, {}
    for name, function in contenders.items():
        first[name] = float(function())
        for _ in range(2):
            function()
    torch.cuda.synchronize()
    for name, function in contenders.items():
        probe = train_bench.run_lap(function, 2)
        steps[name] = arguments.steps or max(
            2, int(arguments.seconds * 1e3 / probe))
    laps = {name: [] for name in contenders}
    for _ in range(arguments.laps):
        for name, function in contenders.items():
            laps[name].append(train_bench.run_lap(function, steps[name]))
    median = {name: float(np.median(values)) for name, values in laps.items()}
    record = {
        'architecture': 'transformer', 'layers': config.layers,
        'downsample_location': location,
        'batch': {'utterances': items, 'frames': frames, 'words': words},
        'device': torch.cuda.get_device_name(0), 'laps': arguments.laps,
        'steps_per_lap': steps, 'first_loss': first,
        'ms_per_step': {
            name: {'median': median[name], 'min': float(np.min(values)),
                   'max': float(np.max(values))}
            for name, values in laps.items()},
        'ms_per_step_laps': laps,
        'columns': {'trainer': columns, 'torch_fp32': torch_columns},
        'ns_per_column': {
            'trainer': median['trainer'] * 1e6 / columns,
            'torch_fp32': median['torch_fp32'] * 1e6 / torch_columns},
        'torch_fp32_over_trainer': median['torch_fp32'] / median['trainer'],
        'torch_is_faster_per_step': bool(
            median['torch_fp32'] < median['trainer'])}
    record['torch_is_faster_per_column'] = bool(
        record['ns_per_column']['torch_fp32'] <
        record['ns_per_column']['trainer'])
    print(json.dumps(record))
    if arguments.out:
        with open(arguments.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


def sdpa_backend(query, key, value):
    """Which backend torch's dispatcher may pick for these tensors."""
    try:
        from torch.backends import cuda
        parameters = cuda.SDPAParams(query, key, value, None, 0., False, False)
        if cuda.flash_sdp_enabled() and cuda.can_use_flash_attention(parameters):
            return 'flash'
        if cuda.mem_efficient_sdp_enabled() and \
                cuda.can_use_efficient_attention(parameters):
            return 'mem_efficient'
        return 'math'
    except Exception as error:      # (the probe's signature moves between versions)
        return f'unknown ({type(error).__name__})'


def attention_kernels(path, items, frames, dropout=False):
    """Per-kernel times of the attention forward and backward of one layer
    (`dropout`: of the masked kernels at p = 0.1 as well)."""
    from emphases_amd import ops, runtime
    device = torch.device('cuda', 0)
    layout = ops._layout(device, np.full(items, frames, dtype=np.int64))
    ld = layout.plan.ld_frames
    tiles, n_tiles = layout.tiles(64)
    generator = torch.Generator(device='cuda').manual_seed(0)
    qk = torch.randn(160, ld, device=device, generator=generator)
    v = torch.randn(ld, 80, device=device, generator=generator)
    dout = torch.randn(80, ld, device=device, generator=generator)
    out = torch.zeros(80, ld, device=device)
    dqkv = torch.zeros(240, ld, device=device)
    lib = runtime.library()
    workspace = torch.empty(
        int(lib.emph_attention_dropout_backward_workspace(ld, 2)),
        device=device)
    times = {'emph_attention': [], 'backward_queries': [], 'backward_keys': []}
    if dropout:
        times.update({'emph_attention_dropout': [],
                      'dropout_backward_queries': [],
                      'dropout_backward_keys': []})
    for lap in range(8):
        with runtime.LaunchTimer() as timer:
            runtime.check(lib.emph_attention(
                qk.data_ptr(), v.data_ptr(), out.data_ptr(), ld, 80, 2,
                tiles.data_ptr(), n_tiles, 64, None, runtime.stream()),
                'emph_attention')
            runtime.check(lib.emph_attention_backward(
                qk.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(),
                dqkv.data_ptr(), ld, 80, 2, tiles.data_ptr(), n_tiles, 64,
                workspace.data_ptr(), runtime.stream()),
                'emph_attention_backward')
            if dropout:
                runtime.check(lib.emph_attention_dropout(
                    qk.data_ptr(), v.data_ptr(), out.data_ptr(), ld, 80, 2,
                    tiles.data_ptr(), n_tiles, 64, 0.1, 0, 1, lap,
                    runtime.stream()), 'emph_attention_dropout')
                runtime.check(lib.emph_attention_dropout_backward(
                    qk.data_ptr(), v.data_ptr(), out.data_ptr(),
                    dout.data_ptr(), dqkv.data_ptr(), ld, 80, 2,
                    tiles.data_ptr(), n_tiles, 64, workspace.data_ptr(), 0.1,
                    0, 1, lap, runtime.stream()),
                    'emph_attention_dropout_backward')
        if lap:                                     # (the first lap warms up)
            for name, value in zip(times, timer.microseconds):
                times[name].append(float(value))
    blocks = items * 2 * ((frames + 15) // 16) ** 2  # 16 x 16 score blocks
    mfma = 2 * 16 * 16 * 4                           # flops of one 16x16x4
    flops = {'emph_attention': blocks * 22 * mfma,
             'backward_queries': blocks * (10 + 20 + 12) * mfma,
             'backward_keys': blocks * (20 + 24) * mfma}
    # (the masked kernels execute the same products; the forward the query
    # pass's two score loops and its 12 product tiles)
    flops.update({'emph_attention_dropout': blocks * (10 + 10 + 12) * mfma,
                  'dropout_backward_queries': flops['backward_queries'],
                  'dropout_backward_keys': flops['backward_keys']})
    record = {'shape': {'utterances': items, 'positions': frames, 'heads': 2,
                        'head_dimension': 40},
              'device': torch.cuda.get_device_name(0), 'kernels': {}}
    for name, values in times.items():
        median = float(np.median(values))
        record['kernels'][name] = {
            'us_median': median, 'us_laps': values,
            'executed_mfma_flops': flops[name],
            'fraction_of_fp32_mfma_peak':
                flops[name] / (median * 1e-6) / PEAK_FP32_MFMA}
    record['kernels']['emph_attention_backward'] = {
        'us_median': record['kernels']['backward_queries']['us_median'] +
        record['kernels']['backward_keys']['us_median'],
        'executed_mfma_flops':
            flops['backward_queries'] + flops['backward_keys']}
    total = record['kernels']['emph_attention_backward']
    total['fraction_of_fp32_mfma_peak'] = total['executed_mfma_flops'] / (
        total['us_median'] * 1e-6) / PEAK_FP32_MFMA
    if dropout:
        kernels = record['kernels']
        kernels['emph_attention_dropout_backward'] = {
            'us_median': kernels['dropout_backward_queries']['us_median'] +
            kernels['dropout_backward_keys']['us_median']}
    # torch's own attention on the same shapes: [B, heads, T, d] float32
    query, key, value = (torch.randn(
        items, 2, frames, 40, device=device, generator=generator
    ).requires_grad_(True) for _ in range(3))
    upstream = torch.randn(items, 2, frames, 40, device=device,
                           generator=generator)
    attention = torch.nn.functional.scaled_dot_product_attention
    forward, backward = [], []
    for lap in range(8):
        events = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        events[0].record()
        result = attention(query, key, value)
        events[1].record()
        result.backward(upstream)
        events[2].record()
        events[2].synchronize()
        query.grad = key.grad = value.grad = None
        if lap:
            forward.append(events[0].elapsed_time(events[1]) * 1e3)
            backward.append(events[1].elapsed_time(events[2]) * 1e3)
    record['torch_sdpa'] = {
        'backend': sdpa_backend(query, key, value),
        'forward_us_median': float(np.median(forward)),
        'backward_us_median': float(np.median(backward)),
        'forward_us_laps': forward, 'backward_us_laps': backward,
        'note': 'device events around the call: launches included'}
    print(json.dumps(record))
    with open(path, 'w') as file:
        json.dump(record, file, indent=1)
        file.write('\n')


def split_kernels(path, items, frames):
    """Per-kernel times of the split forward and of the three launches of
    `emph_attention_backward_split` on one layer's shapes, beside
    `emph_attention` and `emph_attention_backward` in the same run."""
    from emphases_amd import engine, ops, runtime
    device = torch.device('cuda', 0)
    layout = ops._layout(device, np.full(items, frames, dtype=np.int64))
    ld = layout.plan.ld_frames
    tiles, n_tiles = layout.tiles(64)
    stages, n_stages = layout.tiles(64, engine.LONG)
    groups, n_groups = layout.tiles(256, engine.LONG)
    generator = torch.Generator(device='cuda').manual_seed(0)
    qk = torch.randn(160, ld, device=device, generator=generator)
    v = torch.randn(ld, 80, device=device, generator=generator)
    dout = torch.randn(80, ld, device=device, generator=generator)
    out = torch.zeros(80, ld, device=device)
    dqkv = torch.zeros(240, ld, device=device)
    lib = runtime.library()
    workspace = torch.empty(
        int(lib.emph_attention_backward_workspace(ld, 2)), device=device)
    forward_images = torch.empty(
        int(lib.emph_split_kv_bytes(ld, items, 80, 2, 32)),
        dtype=torch.uint8, device=device)
    images = torch.empty(
        int(lib.emph_attention_backward_split_bytes(ld, items, 80, 2)),
        dtype=torch.uint8, device=device)
    names = ('emph_attention', 'backward_queries', 'backward_keys',
             'emph_split_kv', 'emph_attention_split', 'split_backward_images',
             'split_backward_queries', 'split_backward_keys')
    times = {name: [] for name in names}
    for lap in range(8):
        with runtime.LaunchTimer() as timer:
            runtime.check(lib.emph_attention(
                qk.data_ptr(), v.data_ptr(), out.data_ptr(), ld, 80, 2,
                tiles.data_ptr(), n_tiles, 64, None, runtime.stream()),
                'emph_attention')
            runtime.check(lib.emph_attention_backward(
                qk.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(),
                dqkv.data_ptr(), ld, 80, 2, tiles.data_ptr(), n_tiles, 64,
                workspace.data_ptr(), runtime.stream()),
                'emph_attention_backward')
            runtime.check(lib.emph_split_kv(
                qk.data_ptr(), v.data_ptr(), ld, 80, 2, stages.data_ptr(),
                n_stages, 64, 32, forward_images.data_ptr(),
                runtime.stream()), 'emph_split_kv')
            runtime.check(lib.emph_attention_split(
                qk.data_ptr(), forward_images.data_ptr(), out.data_ptr(), ld,
                80, 2, groups.data_ptr(), n_groups, 256, None, 32,
                runtime.stream()), 'emph_attention_split')
            runtime.check(lib.emph_attention_backward_split(
                qk.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(),
                dqkv.data_ptr(), ld, 80, 2, groups.data_ptr(), n_groups, 256,
                images.data_ptr(), workspace.data_ptr(), runtime.stream()),
                'emph_attention_backward_split')
        assert timer.launches == len(names), timer.launches
        if lap:                                     # (the first lap warms up)
            for name, value in zip(names, timer.microseconds):
                times[name].append(float(value))
    # executed flops.  fp32: 16 x 16 score blocks of 16x16x4 instructions
    # (attention_kernels); bf16: 32 x 32 score blocks of 32x32x16 ones - the
    # query pass 18 (scores) + 18 + 9 + 12 (scores, dP, dQ in two m-tiles of
    # which the second holds 8 rows of 32), the key pass 18 + 9 + 12 + 12
    small = items * 2 * ((frames + 15) // 16) ** 2
    large = items * 2 * ((frames + 31) // 32) ** 2
    mfma4, mfma16 = 2 * 16 * 16 * 4, 2 * 32 * 32 * 16
    flops = {'emph_attention': small * 22 * mfma4,
             'backward_queries': small * (10 + 20 + 12) * mfma4,
             'backward_keys': small * (20 + 24) * mfma4,
             'split_backward_queries': large * (18 + 18 + 9 + 12) * mfma16,
             'split_backward_keys': large * (18 + 9 + 12 + 12) * mfma16}
    record = {'shape': {'utterances': items, 'positions': frames, 'heads': 2,
                        'head_dimension': 40},
              'device': torch.cuda.get_device_name(0), 'kernels': {}}
    kernels = record['kernels']
    for name, values in times.items():
        kernels[name] = {'us_median': float(np.median(values)),
                         'us_laps': values}
        if name in flops:
            bf16 = name.startswith('split_')
            kernels[name]['executed_mfma_flops'] = flops[name]
            kernels[name]['fraction_of_bf16_mfma_peak' if bf16 else
                          'fraction_of_fp32_mfma_peak'] = \
                flops[name] / (kernels[name]['us_median'] * 1e-6) / (
                    PEAK_BF16_MFMA if bf16 else PEAK_FP32_MFMA)

    def together(parts, peak, label):
        total = {'us_median': sum(kernels[p]['us_median'] for p in parts)}
        if all(p in flops for p in parts if 'images' not in p):
            total['executed_mfma_flops'] = sum(flops.get(p, 0) for p in parts)
            total[label] = total['executed_mfma_flops'] / (
                total['us_median'] * 1e-6) / peak
        return total
    kernels['emph_attention_backward'] = together(
        ('backward_queries', 'backward_keys'), PEAK_FP32_MFMA,
        'fraction_of_fp32_mfma_peak')
    kernels['emph_attention_backward_split'] = together(
        ('split_backward_images', 'split_backward_queries',
         'split_backward_keys'), PEAK_BF16_MFMA, 'fraction_of_bf16_mfma_peak')
    kernels['split_forward'] = {'us_median': sum(
        kernels[p]['us_median']
        for p in ('emph_split_kv', 'emph_attention_split'))}
    record['backward_split_over_backward'] = \
        kernels['emph_attention_backward_split']['us_median'] / \
        kernels['emph_attention_backward']['us_median']
    print(json.dumps(record))
    with open(path, 'w') as file:
        json.dump(record, file, indent=1)
        file.write('\n')


def transformer_step(config, state, precision=None):
    """(the model, its step on the bench batch): forward + backward + Adam."""
    batch = train_bench.make_batch()
    features, _, bounds, _, targets = batch
    items, frames, words = \
        train_bench.ITEMS, train_bench.FRAMES, train_bench.WORDS
    keywords = {} if precision is None else {'precision': precision}
    model = train.TransformerModel(config, checkpoint=state, **keywords).cuda()
    optimizer = torch.optim.Adam(model.parameters())
    flat = (features.permute(1, 0, 2).reshape(80, items * frames).cuda(),
            torch.arange(items + 1) * frames,
            bounds.permute(1, 0, 2).reshape(2, items * words),
            torch.arange(items + 1) * words)
    flat_targets = targets.reshape(items * words).cuda()

    def step():
        optimizer.zero_grad(set_to_none=True)
        loss = train.loss_fn(model(*flat), flat_targets, 'bce')
        loss.backward()
        optimizer.step()
        return loss.detach()
    return model, step


class Parent(train_bench.Parent):
    """The f32 Transformer step of another checkout of this package in a
    child process: this file's `--serve` on that checkout's package."""

    def __init__(self, directory, precision='f32'):
        import subprocess
        directory = os.path.abspath(directory)
        self.process = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), '--serve',
             '--precision', precision],
            cwd=directory, env=dict(os.environ, EMPHASES_BENCH_ROOT=directory),
            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)


def serve(precision='f32'):
    """The child of `Parent`: 0 -> one step, its loss; n -> a timed lap.
    (No `precision=` at 'f32': the package may be older than the keyword.)"""
    torch.cuda.set_device(0)
    config = emphases_amd.Config(architecture='transformer', layers=6)
    state = train.initial_transformer_state(config, seed=0)
    _, step = transformer_step(
        config, state, None if precision == 'f32' else precision)
    for line in sys.stdin:
        steps = int(line)
        if steps == 0:
            print(float(step()), flush=True)
        else:
            print(train_bench.timed(step, steps), flush=True)


def trainer_main(arguments):
    """`--trainer`: see the module docstring."""
    torch.cuda.set_device(0)
    items, frames, words = \
        train_bench.ITEMS, train_bench.FRAMES, train_bench.WORDS
    config = emphases_amd.Config(architecture='transformer', layers=6)
    state = train.initial_transformer_state(config, seed=0)
    trainer = train.TransformerTrainer(
        config, checkpoint=state, gpu=0, precision=arguments.precision)
    prepared = trainer.prepare(*train_bench.make_batch())
    contenders = {'trainer': lambda: trainer.step(prepared),
                  'ops': Parent(train_bench.ROOT, arguments.precision)}
    if arguments.parent:
        contenders['ops_parent'] = Parent(arguments.parent, arguments.precision)
    first = {}
    for name, function in contenders.items():
        first[name] = float(function())
        for _ in range(2):
            function()
    torch.cuda.synchronize()
    steps = {}
    for name, function in contenders.items():
        probe = train_bench.run_lap(function, 2)
        steps[name] = arguments.steps or max(
            2, int(arguments.seconds * 1e3 / probe))
    laps = {name: [] for name in contenders}
    for _ in range(arguments.laps):
        for name, function in contenders.items():
            laps[name].append(train_bench.run_lap(function, steps[name]))
    for function in contenders.values():
        if isinstance(function, train_bench.Parent):
            function.close()
    record = {
        'architecture': 'transformer', 'layers': config.layers,
        'downsample_location': config.downsample_location,
        'precision': arguments.precision,
        'batch': {'utterances': items, 'frames': frames, 'words': words},
        'device': torch.cuda.get_device_name(0),
        'parameter_tensors': len(trainer.offsets),
        'laps': arguments.laps, 'steps_per_lap': steps, 'first_loss': first,
        'ms_per_step': {
            name: {'median': float(np.median(values)),
                   'min': float(np.min(values)), 'max': float(np.max(values))}
            for name, values in laps.items()},
        'ms_per_step_laps': laps}
    median = {name: record['ms_per_step'][name]['median'] for name in laps}
    spread = max(max(values) - min(values) for values in laps.values())
    record['trainer_over_ops'] = median['trainer'] / median['ops']
    record['laps_spread_ms'] = spread
    # (no regression: the trainer's median lap is not above the model +
    # torch.optim.Adam median by more than the laps' own spread)
    record['trainer_within_the_spread_of_ops'] = bool(
        median['trainer'] <= median['ops'] + spread)
    if 'ops_parent' in laps:
        record['trainer_over_ops_parent'] = \
            median['trainer'] / median['ops_parent']
        record['ops_over_ops_parent'] = median['ops'] / median['ops_parent']
        record['trainer_within_the_spread_of_ops_parent'] = bool(
            median['trainer'] <= median['ops_parent'] + spread)
    print(json.dumps(record))
    if arguments.out:
        with open(arguments.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


def transformer_main(arguments):
    torch.cuda.set_device(0)
    batch = train_bench.make_batch()
    features, _, bounds, _, targets = batch
    items, frames, words = \
        train_bench.ITEMS, train_bench.FRAMES, train_bench.WORDS
    config = emphases_amd.Config(architecture='transformer', layers=6)
    state = train.initial_transformer_state(config, seed=0)
    model = train.TransformerModel(config, checkpoint=state).cuda()
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

    device_features, device_bounds, device_targets = \
        features.cuda(), bounds.cuda(), targets.cuda()
    frame = torch.arange(frames, device='cuda')[None, :, None]
    membership = ((frame >= device_bounds[:, 0, None, :]) &
                  (frame < device_bounds[:, 1, None, :])).float()
    plain = TorchTransformer(config, state).cuda()
    plain.train()
    plain_optimizer = torch.optim.Adam(plain.parameters())
    contenders = {
        'ops': ops_step,
        'torch_fp32': lambda: train_bench.torch_step(
            plain, plain_optimizer, None, device_features, membership,
            device_targets)}
    if arguments.precision != 'f32':
        _, split_step = transformer_step(config, state, arguments.precision)
        contenders = {f'ops_{arguments.precision}': split_step, **contenders}
    if arguments.parent:
        contenders['ops_parent'] = Parent(arguments.parent)
    if arguments.reference_dropout:
        dropping = train.TransformerModel(
            config, checkpoint=state, reference_dropout=True).cuda()
        dropping.train()
        dropping_optimizer = torch.optim.Adam(dropping.parameters())

        def ops_dropout_step():
            dropping_optimizer.zero_grad(set_to_none=True)
            loss = train.loss_fn(dropping(*flat), flat_targets, 'bce')
            loss.backward()
            dropping_optimizer.step()
            dropping.steps += 1
            return loss.detach()

        noisy = TorchTransformer(config, state, dropout=0.1).cuda()
        noisy.train()
        noisy_optimizer = torch.optim.Adam(noisy.parameters())
        contenders = {
            'ops_dropout': ops_dropout_step,
            'ops': ops_step,
            'torch_fp32_dropout': lambda: train_bench.torch_step(
                noisy, noisy_optimizer, None, device_features, membership,
                device_targets)}
    first = {}
    for name, function in contenders.items():
        loss = function()
        first[name] = float(loss.detach() if torch.is_tensor(loss) else loss)
        for _ in range(2):
            function()
    torch.cuda.synchronize()
    steps = {}
    for name, function in contenders.items():
        probe = train_bench.run_lap(function, 2)
        steps[name] = arguments.steps or max(
            2, int(arguments.seconds * 1e3 / probe))
    laps = {name: [] for name in contenders}
    for _ in range(arguments.laps):
        for name, function in contenders.items():
            laps[name].append(train_bench.run_lap(function, steps[name]))
    for function in contenders.values():
        if isinstance(function, train_bench.Parent):
            function.close()
    record = {
        'architecture': 'transformer', 'layers': config.layers,
        'downsample_location': config.downsample_location,
        'batch': {'utterances': items, 'frames': frames, 'words': words},
        'device': torch.cuda.get_device_name(0),
        'laps': arguments.laps, 'steps_per_lap': steps, 'first_loss': first,
        'ms_per_step': {
            name: {'median': float(np.median(values)),
                   'min': float(np.min(values)), 'max': float(np.max(values))}
            for name, values in laps.items()},
        'ms_per_step_laps': laps}
    median = {name: record['ms_per_step'][name]['median'] for name in laps}
    if arguments.reference_dropout:
        record['ops_dropout_over_ops'] = median['ops_dropout'] / median['ops']
        record['torch_fp32_dropout_over_ops_dropout'] = \
            median['torch_fp32_dropout'] / median['ops_dropout']
    else:
        record['torch_fp32_over_ops'] = median['torch_fp32'] / median['ops']
    if arguments.precision != 'f32':
        name = f'ops_{arguments.precision}'
        record['precision'] = arguments.precision
        record[f'ops_over_{name}'] = median['ops'] / median[name]
        record[f'slowest_{name}_lap_below_fastest_ops_lap'] = bool(
            max(laps[name]) < min(laps['ops']))
    if 'ops_parent' in laps:
        # (no regression: the f32 step of this checkout is not above the
        # parent's laps; below them is no regression either)
        record['ops_over_ops_parent'] = median['ops'] / median['ops_parent']
        record['ops_at_or_below_the_parents_slowest_lap'] = bool(
            median['ops'] <= max(laps['ops_parent']))
    print(json.dumps(record))
    if arguments.out:
        with open(arguments.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')
    if arguments.kernels_out and arguments.precision != 'f32':
        split_kernels(arguments.kernels_out, items, frames)
    elif arguments.kernels_out:
        attention_kernels(arguments.kernels_out, items, frames,
                          arguments.reference_dropout)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--architecture', default='convolution',
                        choices=('convolution', 'transformer'))
    parser.add_argument('--kernels-out', default=None)
    parser.add_argument('--reference_dropout', action='store_true')
    parser.add_argument('--precision', default='f32',
                        choices=('f32', 'bf16x3'))
    parser.add_argument('--parent', default=None)
    parser.add_argument('--trainer', action='store_true')
    parser.add_argument('--downsample_location', default='intermediate',
                        choices=('input', 'intermediate', 'inference', 'loss'))
    parser.add_argument('--serve', action='store_true')
    parser.add_argument('--laps', type=int, default=7)
    parser.add_argument('--seconds', type=float, default=1.0)
    parser.add_argument('--steps', type=int, default=None)
    parser.add_argument('--out', default=None)
    arguments = parser.parse_args()
    if arguments.serve:
        return serve(arguments.precision)
    if arguments.trainer:
        if arguments.architecture != 'transformer' or \
                arguments.reference_dropout or arguments.kernels_out:
            parser.error('--trainer goes with --architecture transformer, '
                         'without --reference_dropout and --kernels-out')
        if arguments.downsample_location in ('input', 'inference'):
            return locations_main(arguments)
        if arguments.downsample_location != 'intermediate':
            parser.error("--downsample_location 'input', 'inference' or the "
                         "default 'intermediate'")
        return trainer_main(arguments)
    if arguments.downsample_location != 'intermediate':
        parser.error('--downsample_location goes with --trainer')
    if arguments.precision != 'f32' and (
            arguments.architecture != 'transformer' or
            arguments.reference_dropout):
        parser.error('--precision bf16x3 goes with --architecture '
                     'transformer, without --reference_dropout '
                     '(tools/train_bench.py --precision times the conv step)')
    if arguments.parent and (arguments.architecture != 'transformer' or
                             arguments.reference_dropout):
        parser.error('--parent goes with --architecture transformer, '
                     'without --reference_dropout (tools/train_bench.py '
                     '--parent times the conv steps of a parent checkout)')
    if arguments.architecture == 'transformer':
        return transformer_main(arguments)
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
