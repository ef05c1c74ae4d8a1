"""One training step at the reference's training size, against PyTorch.

    python tools/train_bench.py [--laps 7] [--seconds 1.0] [--out profiles/train_step.json]
    python tools/train_bench.py --precision bf16x3 --parent <checkout of the parent commit>
    python tools/train_bench.py --dropout 0.1 --parent <checkout of the parent commit>
    python tools/train_bench.py --downsample_location inference loss --laps 3 --parent <checkout of the parent commit> --out profiles/train_step_locations.json
    python tools/train_bench.py --downsample_location input --laps 3 --parent <checkout of the parent commit> --out profiles/train_step_input.json
    python tools/train_bench.py --activation gelu --laps 3 --parent <checkout of the parent commit> --out profiles/train_step_grid.json
    python tools/train_bench.py --channels 64 --encoder_kernel_size 5 --decoder_kernel_size 1 --laps 3 --parent <checkout> --out profiles/train_step_grid.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/train_bench.py --only ours --steps 20
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/train_bench.py --only ours --downsample_location inference --steps 20

The batch is what the reference's sampler fills up to (`MAX_TRAINING_FRAMES =
75 000`, `config/defaults.py`): 75 utterances x 1 000 frames x 30 words,
default configuration, weights of `emphases.Model()` under seed 0.

Three contenders run in ALTERNATING laps of the same process on the same GPU:

  ours            `emphases_amd.train.Trainer.step` on a prepared batch
  torch_fp32      the same model as torch.nn.Conv1d + ReLU modules, the word
                  sums as one batched matmul with a 0/1 frame-to-word matrix
                  (the reference's per-word Python loop would only measure the
                  interpreter), `binary_cross_entropy_with_logits`, autograd,
                  `torch.optim.Adam` - in float32
  torch_autocast  the same under `torch.autocast` + `GradScaler`, as the
                  reference trains (`train/core.py:78,111,136-142`)

With `--precision bf16x3` a fourth contender, `ours_bf16x3`, is the same
trainer at that precision; with `--parent DIRECTORY` a child process runs the
f32 step of the package in that checkout (built there) on the same batch,
lap for lap between the others: `ours_parent`.

With `--dropout P` one more contender, `ours_dropout`, is the same trainer
under `Config(dropout=P)` (Philox masks, `emph_dropout`), and both torch
models gain `torch.nn.Dropout(P)` after each activation, as the reference
builds them under DROPOUT; `ours` stays the step without dropout.

With `--downsample_location inference` and / or `loss` the contenders are the
decoder-less models instead: `ours_<location>` is
`emphases_amd.train.EncoderTrainer.step` there, `torch_fp32_<location>` the
same model (input layer, frame encoder, output layer; the word sums as the
batched matmul at 'loss', the frame targets of `emphases_amd.upsample`, made
once outside the timed region and clamped, at 'inference') with autograd and
`torch.optim.Adam` in float32, and `ours_parent` (with `--parent`) the
'intermediate' step of the parent checkout on the same batch.

With `--downsample_location input` the contenders are `ours_input`,
`emphases_amd.train.PieceTrainer.step` (every word a zero-padded sequence of
its own, padded to the longest word of ITS utterance), and `torch_fp32_input`:
the same layers as torch.nn.Conv1d + ReLU over the padded pieces
[2 250, 80, L], the pooling as a sum over the padded axis, autograd and
`torch.optim.Adam` in float32.  torch needs one L for its batch, so its pieces
are padded to the longest word of the BATCH, as the reference's own training
batch is (`core.py:552-586`).  The
record carries both column counts and the per-column times, whose ratio is
the one that compares like with like, and the per-batch host time of the piece
layout (plan, pieces, metadata upload); with `--parent`, also the time the
parent checkout's own `Plan.pieces` takes on the same plan.

With any of `--activation`, `--channels`, `--encoder_kernel_size`,
`--decoder_kernel_size` and `--downsample_method` the contenders are those of
the reference's hyperparameter grid at 'intermediate' under that
configuration: `ours_grid`, `emphases_amd.train.GridTrainer.step`;
`torch_fp32_grid`, the same model as torch.nn.Conv1d + activation modules
built from the same settings (the word reduction as the batched matmul for
'sum' and 'average', `torch.segment_reduce` for 'max', a gather of the middle
frame for 'center'), autograd and `torch.optim.Adam` in float32; `seams`,
`emphases_amd.train.TorchModel` + `torch.optim.Adam` on the differentiable
operator seams; and with `--parent`, `seams_parent`, the same on the package
of the parent checkout, and `ours_parent`, that checkout's `Trainer.step` at
the default configuration.  `--out` then holds one record per configuration:
a run adds its own to the file, under the name made of its settings, and
the record carries the launch timer's times of the three kernels of
csrc/grid.hip on the batch's buffers with the bytes they move.

Every utterance has the same lengths, so the padded batch of the torch model
and the ragged batch of this package compute the same function.  A lap of one
contender is timed with a pair of device events around `steps` steps, `steps`
chosen so that a lap takes about `--seconds`; both sides are warmed up first.
Reported: median, minimum and maximum per-step time over the laps.
"""
import argparse
import json
import os
import sys

ROOT = os.environ.get('EMPHASES_BENCH_ROOT') or os.path.dirname(
    os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import train  # noqa: E402

ITEMS, FRAMES, WORDS = 75, 1000, 30
PEAK_FP32_MATRIX = 157.3e12


def make_batch(seed=0):
    rng = np.random.default_rng(seed)
    features = torch.from_numpy(
        rng.standard_normal((ITEMS, 80, FRAMES)).astype(np.float32))
    bounds = torch.zeros(ITEMS, 2, WORDS, dtype=torch.long)
    for item in range(ITEMS):
        cuts = np.sort(rng.choice(
            np.arange(1, FRAMES), size=WORDS - 1, replace=False))
        edges = np.concatenate([[0], cuts, [FRAMES]])
        bounds[item, 0] = torch.from_numpy(edges[:-1])
        bounds[item, 1] = torch.from_numpy(edges[1:])
    targets = torch.from_numpy(
        rng.uniform(0., 1., (ITEMS, 1, WORDS)).astype(np.float32))
    return (features, torch.full((ITEMS,), FRAMES), bounds,
            torch.full((ITEMS,), WORDS), targets)


class TorchModel(torch.nn.Module):
    """`emphases.Model` of the default configuration (`model/core.py`)."""

    def __init__(self, state, dropout=None):
        super().__init__()
        conv = lambda c_in, c_out: torch.nn.Conv1d(  # noqa: E731
            c_in, c_out, kernel_size=3, padding='same')
        # (`model/layers/convolution.py:25-33`: layer i is module 3 i under
        # DROPOUT, 2 i without)
        extra = [] if dropout is None else [torch.nn.Dropout(dropout)]
        stack = lambda: torch.nn.Sequential(*[  # noqa: E731
            module for _ in range(6)
            for module in [conv(80, 80), torch.nn.ReLU()] + extra])
        if dropout is not None:
            saved = train.checkpoint_names(emphases_amd.Config(dropout=dropout))
            state = {saved[name]: value for name, value in state.items()}
        self.input_layer = conv(80, 80)
        self.frame_encoder = stack()
        self.word_decoder = stack()
        self.output_layer = conv(80, 1)
        self.load_state_dict(
            {name: torch.from_numpy(value) for name, value in state.items()})

    def forward(self, features, membership):
        frames = self.frame_encoder(self.input_layer(features))
        words = torch.bmm(frames, membership.to(frames.dtype))
        return self.output_layer(self.word_decoder(words))


class TorchEncoderModel(torch.nn.Module):
    """`emphases.Model` without a word decoder (`model/core.py:28-30`) in
    train mode: frame logits at 'inference', word logits at 'loss'."""

    def __init__(self, state, location):
        super().__init__()
        conv = lambda c_in, c_out: torch.nn.Conv1d(  # noqa: E731
            c_in, c_out, kernel_size=3, padding='same')
        self.location = location
        self.input_layer = conv(80, 80)
        self.frame_encoder = torch.nn.Sequential(*[
            module for _ in range(6)
            for module in [conv(80, 80), torch.nn.ReLU()]])
        self.output_layer = conv(80, 1)
        self.load_state_dict(
            {name: torch.from_numpy(value) for name, value in state.items()})

    def forward(self, features, membership):
        frames = self.frame_encoder(self.input_layer(features))
        if self.location == 'loss':
            frames = torch.bmm(frames, membership.to(frames.dtype))
        return self.output_layer(frames)


class TorchPieceModel(torch.nn.Module):
    """`emphases.Model` at DOWNSAMPLE_LOCATION = 'input', 'sum'
    (`model/core.py:41-87`): pieces [P, 80, L] -> word logits [B, 1, W]."""

    def __init__(self, state, items, words):
        super().__init__()
        conv = lambda c_in, c_out: torch.nn.Conv1d(  # noqa: E731
            c_in, c_out, kernel_size=3, padding='same')
        stack = lambda: torch.nn.Sequential(*[  # noqa: E731
            module for _ in range(6)
            for module in [conv(80, 80), torch.nn.ReLU()]])
        self.items, self.words = items, words
        self.input_layer = conv(80, 80)
        self.frame_encoder = stack()
        self.word_decoder = stack()
        self.output_layer = conv(80, 1)
        self.load_state_dict(
            {name: torch.from_numpy(value) for name, value in state.items()})

    def forward(self, pieces, membership=None):
        pooled = self.frame_encoder(self.input_layer(pieces)).sum(dim=2)
        words = pooled.reshape(self.items, self.words, -1).transpose(1, 2)
        return self.output_layer(self.word_decoder(words))


ACTIVATION_MODULES = {
    'relu': torch.nn.ReLU, 'gelu': torch.nn.GELU, 'silu': torch.nn.SiLU,
    'leaky_relu': torch.nn.LeakyReLU}
GRID_FLAGS = ('activation', 'channels', 'encoder_kernel_size',
              'decoder_kernel_size', 'downsample_method')
COPY_RATE = 6.29e12      # bytes/s of a device copy on this part (README)


class TorchGridModel(torch.nn.Module):
    """`emphases.Model` at 'intermediate' under any configuration of the
    hyperparameter grid (`model/core.py`, `model/layers/convolution.py`)."""

    def __init__(self, config, state):
        super().__init__()
        conv = lambda c_in, c_out, k: torch.nn.Conv1d(  # noqa: E731
            c_in, c_out, kernel_size=k, padding='same')
        channels = config.channels
        stack = lambda k: torch.nn.Sequential(*[  # noqa: E731
            module for _ in range(config.layers)
            for module in [conv(channels, channels, k),
                           ACTIVATION_MODULES[config.activation]()]])
        self.method = config.downsample_method
        self.input_layer = conv(
            config.num_features, channels, config.encoder_kernel_size)
        self.frame_encoder = stack(config.encoder_kernel_size)
        self.word_decoder = stack(config.decoder_kernel_size)
        self.output_layer = conv(channels, 1, config.decoder_kernel_size)
        self.load_state_dict(
            {name: torch.from_numpy(value) for name, value in state.items()})

    def forward(self, features, membership):
        """membership: the 0/1 matrix [B, T, W] for 'sum'; (matrix, word
        lengths [B, 1, W]) for 'average'; the word lengths [B W] of words
        that tile every utterance for 'max'; the middle frames [B, 1, W] for
        'center'."""
        frames = self.frame_encoder(self.input_layer(features))
        if self.method == 'sum':
            words = torch.bmm(frames, membership)
        elif self.method == 'average':
            words = torch.bmm(frames, membership[0]) / membership[1]
        elif self.method == 'max':
            items, channels, count = frames.shape
            flat = frames.permute(0, 2, 1).reshape(items * count, channels)
            words = torch.segment_reduce(
                flat, 'max', lengths=membership, axis=0).reshape(
                    items, -1, channels).permute(0, 2, 1)
        else:
            words = torch.gather(
                frames, 2, membership.expand(-1, frames.shape[1], -1))
        return self.output_layer(self.word_decoder(words))


def grid_membership(method, bounds):
    """What `TorchGridModel.forward` takes for `method`, on the device."""
    bounds = bounds.cuda()
    lengths = (bounds[:, 1] - bounds[:, 0])
    if method == 'max':
        assert int(lengths.sum()) == ITEMS * FRAMES     # the words tile
        return lengths.reshape(-1)
    if method == 'center':
        return (bounds[:, 0] + lengths // 2)[:, None, :]
    frame = torch.arange(FRAMES, device='cuda')[None, :, None]
    matrix = ((frame >= bounds[:, 0, None, :]) &
              (frame < bounds[:, 1, None, :])).float()
    if method == 'sum':
        return matrix
    return matrix, lengths[:, None, :].float()


def seams_step(config, state, batch):
    """One step of `train.TorchModel` + Adam on the batch back to back."""
    features, _, bounds, _, targets = batch
    model = train.TorchModel(config, checkpoint=state).cuda()
    optimizer = torch.optim.Adam(model.parameters())
    flat = (features.permute(1, 0, 2).reshape(
                features.shape[1], ITEMS * FRAMES).cuda(),
            torch.arange(ITEMS + 1) * FRAMES,
            bounds.permute(1, 0, 2).reshape(2, ITEMS * WORDS),
            torch.arange(ITEMS + 1) * WORDS)
    flat_targets = targets.reshape(ITEMS * WORDS).cuda()

    def step():
        optimizer.zero_grad(set_to_none=True)
        loss = train.loss_fn(model(*flat), flat_targets, config.loss)
        loss.backward()
        optimizer.step()
        return loss.detach()
    return step


def grid_kernels(trainer, prepared, repeats=9):
    """Median microseconds of the three kernels of csrc/grid.hip alone on the
    step's own buffers (the launch timer: the kernel's begin -> end), and
    the bytes each reads and writes over `COPY_RATE`."""
    from emphases_amd import runtime
    lib, config = runtime.library(), trainer.config
    buffers = trainer._buffers(prepared.plan)
    frames, grads = buffers['frames'][1], buffers['frame_grad'][0].clone()
    source = buffers.get('pre_frames', buffers['frames'])[0]
    words, meta = buffers['words'], prepared.meta
    ld_w, channels = prepared.plan.ld_words, config.channels
    activation = runtime.ACTIVATIONS[config.activation]
    scratch = torch.zeros_like(frames)
    dweight = torch.zeros(channels * config.decoder_kernel_size + 1,
                          device=frames.device)
    launches = {
        'emph_activation_dropout': lambda p: lib.emph_activation_dropout(
            source.data_ptr(), scratch.data_ptr(), source.numel(), activation,
            p, 1, 1, 0, runtime.stream()),
        'emph_activation_dropout_gradient':
            lambda p: lib.emph_activation_dropout_gradient(
                source.data_ptr(), grads.data_ptr(), grads.numel(),
                activation, p, 1, 1, 0, runtime.stream()),
        'emph_output_layer_backward_any':
            lambda p: lib.emph_output_layer_backward_any(
                buffers['dlogit'].data_ptr(), words[-1].data_ptr(), ld_w,
                trainer._parameter('output_layer.weight'),
                meta['word_segment'].data_ptr(), channels,
                config.decoder_kernel_size, ld_w, dweight.data_ptr(),
                dweight[-1:].data_ptr(), buffers['word_grad'][0].data_ptr(),
                ld_w, runtime.stream())}
    elements = source.numel()
    moved = {'emph_activation_dropout': 8 * elements,
             'emph_activation_dropout_gradient': 12 * elements,
             'emph_output_layer_backward_any':
                 4 * (2 * channels * ld_w + 3 * ld_w)}
    record = {'elements': elements, 'copy_rate': COPY_RATE}
    for name, launch in launches.items():
        for p in (0., 0.1):
            if name == 'emph_output_layer_backward_any' and p:
                continue
            times = []
            for lap in range(repeats + 1):
                with runtime.LaunchTimer() as timer:
                    runtime.check(launch(p), name)
                if lap:                             # (the first lap warms up)
                    times.append(float(sum(timer.microseconds)))
            median = float(np.median(times))
            record[name + ('' if not p else f'_p{p}')] = {
                'us_median': median, 'us_min': min(times), 'us_max': max(times),
                'bytes': moved[name],
                'rate_over_copy': moved[name] / (median * 1e-6) / COPY_RATE}
    return record


def grid(arguments, batch, settings):
    """The contenders of a configuration of the hyperparameter grid."""
    config = emphases_amd.Config(**settings)
    state = train.initial_state(config, seed=0)
    ours = train.GridTrainer(config, checkpoint=state, gpu=0)
    prepared = ours.prepare(*batch)
    arguments.keep = (ours, prepared)
    contenders = {'ours_grid': lambda: ours.step(prepared)}
    arguments.extra = {'config': settings}
    if not arguments.only:
        arguments.extra['kernels'] = grid_kernels(ours, prepared)
    if arguments.no_torch or arguments.only:
        return contenders
    features, _, bounds, _, targets = batch
    model = TorchGridModel(config, state).cuda()
    optimizer = torch.optim.Adam(model.parameters())
    membership = grid_membership(config.downsample_method, bounds)
    contenders['torch_fp32_grid'] = (
        lambda m=model, o=optimizer, f=features.cuda(), t=targets.cuda():
        torch_step(m, o, None, f, membership, t))
    contenders['seams'] = seams_step(config, state, batch)
    if arguments.parent:
        flags = [item for name, value in settings.items()
                 for item in (f'--{name}', str(value))]
        contenders['seams_parent'] = Parent(
            arguments.parent, ['seams'] + flags)
    return contenders


def padded_pieces(batch):
    """[B W, 80, L] of a batch, L the longest word of the batch."""
    features, _, bounds, _, _ = batch
    lengths = bounds[:, 1] - bounds[:, 0]
    longest = int(lengths.max())
    pieces = torch.zeros(ITEMS * WORDS, 80, longest)
    for item in range(ITEMS):
        for word in range(WORDS):
            start, end = int(bounds[item, 0, word]), int(bounds[item, 1, word])
            pieces[item * WORDS + word, :, :end - start] = \
                features[item, :, start:end]
    return pieces


def piece_builder_ms(batch, repeats=20):
    """Median ms of `Plan.pieces('sum')` of this checkout's package on the
    batch's plan (a fresh plan each time: the pieces are cached per plan)."""
    import time
    from emphases_amd import core as api
    _, frame_lengths, bounds, word_lengths, _ = batch
    frames = [int(n) for n in frame_lengths]
    words = [int(n) for n in word_lengths]
    laps = []
    for _ in range(repeats):
        plan = api._packed_plan(frames, bounds, words)
        start = time.perf_counter()
        plan.pieces('sum')
        laps.append(time.perf_counter() - start)
    return 1e3 * float(np.median(laps))


def host_times(trainer, batch, repeats=20):
    """Median ms per batch of the host work of the piece layout: the plan,
    the pieces, the metadata (one upload)."""
    import time
    from emphases_amd import core as api
    _, frame_lengths, bounds, word_lengths, _ = batch
    frames = [int(n) for n in frame_lengths]
    words = [int(n) for n in word_lengths]
    laps = {'plan': [], 'pieces': [], 'metadata': []}
    for _ in range(repeats):
        torch.cuda.synchronize()
        start = time.perf_counter()
        plan = api._packed_plan(frames, bounds, words)
        planned = time.perf_counter()
        plan.pieces('sum')
        built = time.perf_counter()
        trainer.metadata(plan)
        torch.cuda.synchronize()
        uploaded = time.perf_counter()
        laps['plan'].append(planned - start)
        laps['pieces'].append(built - planned)
        laps['metadata'].append(uploaded - built)
    record = {name: 1e3 * float(np.median(values))
              for name, values in laps.items()}
    record['total'] = record['plan'] + record['pieces'] + record['metadata']
    return record


def torch_step(model, optimizer, scaler, features, membership, targets):
    with torch.autocast('cuda', enabled=scaler is not None):
        loss = torch.nn.functional.binary_cross_entropy_with_logits(
            model(features, membership), targets)
    optimizer.zero_grad()
    if scaler is None:
        loss.backward()
        optimizer.step()
    else:
        scaler.scale(loss).backward()
        scaler.step(optimizer)
        scaler.update()
    return loss


def timed(function, steps):
    begin = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    begin.record()
    for _ in range(steps):
        function()
    end.record()
    end.synchronize()
    return begin.elapsed_time(end) / steps


class Parent:
    """The f32 step of another checkout of this package in a child process
    (`--serve` of that checkout's copy of this batch and trainer, driven by
    this file): a lap is a line to its stdin, the answer its ms per step."""

    def __init__(self, directory, serve=()):
        import subprocess
        directory = os.path.abspath(directory)
        self.process = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), '--serve',
             *serve],
            cwd=directory, env=dict(os.environ, EMPHASES_BENCH_ROOT=directory),
            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, steps):
        self.process.stdin.write(f'{steps}\n')
        self.process.stdin.flush()
        answer = self.process.stdout.readline()
        if not answer.strip():
            raise RuntimeError(
                f'the parent checkout\'s process ended (exit status '
                f'{self.process.wait()})')
        return float(answer)

    def __call__(self):
        return self.ask(0)

    def piece_builder_ms(self):
        """The parent checkout's own `Plan.pieces('sum')` on this batch."""
        return self.ask(-1)

    def close(self):
        self.process.stdin.close()
        try:
            self.process.wait(timeout=60)
        except Exception:
            self.process.kill()
            self.process.wait()


def run_lap(function, steps):
    if isinstance(function, Parent):
        return function.ask(steps)
    return timed(function, steps)


def locations(arguments, batch):
    """The contenders of `--downsample_location`."""
    contenders, keep = {}, []
    for location in arguments.downsample_location:
        config = emphases_amd.Config(downsample_location=location)
        state = train.initial_state(config, seed=0)
        ours = train.trainer_for(config, checkpoint=state, gpu=0)
        prepared = ours.prepare(*batch)
        keep.append((ours, prepared))
        contenders[f'ours_{location}'] = \
            lambda o=ours, p=prepared: o.step(p)
        if location == 'input':
            pieces = prepared.meta['pieces']['plan']
            arguments.extra = {
                'pieces': len(pieces), 'piece_columns': pieces.ld_frames,
                'frame_columns': prepared.plan.ld_frames,
                'host_ms': host_times(ours, batch)}
        if arguments.no_torch or arguments.only:
            continue
        features, frame_lengths, bounds, word_lengths, targets = batch
        if location == 'input':
            pieces = padded_pieces(batch).cuda()
            arguments.extra['torch_piece_columns'] = \
                pieces.shape[0] * pieces.shape[2]
            model = TorchPieceModel(state, ITEMS, WORDS).cuda()
            optimizer = torch.optim.Adam(model.parameters())
            contenders['torch_fp32_input'] = (
                lambda m=model, o=optimizer, f=pieces, t=targets.cuda():
                torch_step(m, o, None, f, None, t))
            continue
        if location == 'inference':
            targets = torch.clamp(emphases_amd.upsample(
                targets.cuda(), bounds, word_lengths, frame_lengths, config),
                0., 1.)
        features, bounds, targets = features.cuda(), bounds.cuda(), targets.cuda()
        frame = torch.arange(FRAMES, device='cuda')[None, :, None]
        membership = ((frame >= bounds[:, 0, None, :]) &
                      (frame < bounds[:, 1, None, :])).float()
        model = TorchEncoderModel(state, location).cuda()
        optimizer = torch.optim.Adam(model.parameters())
        contenders[f'torch_fp32_{location}'] = (
            lambda m=model, o=optimizer, f=features, b=membership, t=targets:
            torch_step(m, o, None, f, b, t))
    return contenders


def serve(what, settings):
    """The child of `Parent`: 0 -> one step, its loss; n -> a timed lap.
    what: 'trainer', `Trainer.step` at the default configuration, or 'seams',
    `TorchModel` + Adam under `settings`."""
    torch.cuda.set_device(0)
    if what == 'seams':
        config = emphases_amd.Config(**settings)
        # (the state as arrays: a checkout older than the grid step builds
        # only the default configuration's state itself)
        model = train.TorchModel(config, seed=0)
        state = {name: value.detach().numpy()
                 for name, value in model.state_dict().items()}
        step = seams_step(config, state, make_batch())
    else:
        state = train.initial_state(emphases_amd.DEFAULT, seed=0)
        ours = train.Trainer(checkpoint=state, gpu=0)
        prepared = ours.prepare(*make_batch())
        step = lambda: ours.step(prepared)  # noqa: E731
    for line in sys.stdin:
        steps = int(line)
        if steps < 0:
            print(piece_builder_ms(make_batch()), flush=True)
        elif steps == 0:
            print(float(step()), flush=True)
        else:
            print(timed(step, steps), flush=True)


def compare(arguments, contenders):
    """Alternating laps of the `--downsample_location` contenders."""
    parent = None
    if arguments.only is None and arguments.parent:
        parent = contenders['ours_parent'] = Parent(arguments.parent)
    children = [c for c in contenders.values() if isinstance(c, Parent)]
    try:
        if parent is not None and 'host_ms' in getattr(arguments, 'extra', {}):
            arguments.extra['host_ms']['pieces_parent'] = \
                parent.piece_builder_ms()
        first = {}
        for name, function in contenders.items():
            first[name] = float(function())
            for _ in range(4):
                function()
        torch.cuda.synchronize()
        steps = {}
        for name, function in contenders.items():
            probe = run_lap(function, 5)
            steps[name] = arguments.steps or max(
                5, int(arguments.seconds * 1e3 / probe))
        if arguments.only:
            name = next(iter(contenders))
            timed(contenders[name], steps[name])
            print(json.dumps({f'{name}_steps': steps[name]}))
            return
        laps = {name: [] for name in contenders}
        for _ in range(arguments.laps):
            for name, function in contenders.items():
                laps[name].append(run_lap(function, steps[name]))
    finally:
        for child in children:
            child.close()
    record = {
        'batch': {'utterances': ITEMS, 'frames': FRAMES, 'words': WORDS},
        'device': torch.cuda.get_device_name(0),
        'laps': arguments.laps, 'steps_per_lap': steps, 'first_loss': first,
        'ms_per_step': {
            name: {'median': float(np.median(values)),
                   'min': float(np.min(values)), 'max': float(np.max(values))}
            for name, values in laps.items()},
        'ms_per_step_laps': laps}
    record.update(getattr(arguments, 'extra', {}))
    if 'torch_piece_columns' in record:
        # torch pads to the batch's longest word and so computes more
        # columns: the ratio that compares like with like is per column
        median = {name: entry['median']
                  for name, entry in record['ms_per_step'].items()}
        record['ns_per_column'] = {
            'ours_input': 1e6 * median['ours_input'] / record['piece_columns'],
            'torch_fp32_input': 1e6 * median['torch_fp32_input'] /
            record['torch_piece_columns']}
        record['torch_over_ours_per_column'] = \
            record['ns_per_column']['torch_fp32_input'] / \
            record['ns_per_column']['ours_input']
    if 'ours_grid' in record['ms_per_step']:
        median = {name: entry['median']
                  for name, entry in record['ms_per_step'].items()}
        record['over_ours_grid'] = {
            name: value / median['ours_grid']
            for name, value in median.items() if name != 'ours_grid'}
        # one record per configuration in the same file
        name = '_'.join(f'{key}={value}' for key, value in
                        record['config'].items())
        records = {}
        if arguments.out and os.path.exists(arguments.out):
            with open(arguments.out) as file:
                records = json.load(file)
        records[name] = record
        record = records
    print(json.dumps(record))
    if arguments.out:
        with open(arguments.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--laps', type=int, default=7)
    parser.add_argument('--seconds', type=float, default=1.0)
    parser.add_argument('--steps', type=int, default=None)
    parser.add_argument('--only', choices=('ours',), default=None)
    parser.add_argument('--out', default=None)
    # (`--serve` also runs against the parent's package, which has no PRECISIONS)
    parser.add_argument(
        '--precision', default='f32',
        choices=getattr(train, 'PRECISIONS', ('f32',)))
    parser.add_argument('--parent', default=None)
    parser.add_argument('--dropout', type=float, default=None)
    parser.add_argument(
        '--downsample_location', nargs='+', default=None,
        choices=('inference', 'loss', 'input'))
    parser.add_argument('--no-torch', action='store_true')
    parser.add_argument('--activation', choices=sorted(ACTIVATION_MODULES))
    parser.add_argument('--channels', type=int)
    parser.add_argument('--encoder_kernel_size', type=int)
    parser.add_argument('--decoder_kernel_size', type=int)
    parser.add_argument(
        '--downsample_method', choices=('sum', 'average', 'max', 'center'))
    parser.add_argument('--serve', nargs='?', const='trainer', default=None,
                        choices=('trainer', 'seams'), help=argparse.SUPPRESS)
    arguments = parser.parse_args()
    settings = {name: getattr(arguments, name) for name in GRID_FLAGS
                if getattr(arguments, name) is not None}
    if arguments.serve:
        return serve(arguments.serve, settings)
    torch.cuda.set_device(0)
    batch = make_batch()
    if settings:
        if arguments.downsample_location:
            parser.error('the grid flags train at the default location')
        return compare(arguments, grid(arguments, batch, settings))
    if arguments.downsample_location:
        return compare(arguments, locations(arguments, batch))
    state = train.initial_state(emphases_amd.DEFAULT, seed=0)
    dropped = None if arguments.dropout is None else \
        emphases_amd.Config(dropout=arguments.dropout)
    if arguments.only:
        ours = train.Trainer(
            dropped, checkpoint=state, gpu=0, precision=arguments.precision)
    else:
        ours = train.Trainer(checkpoint=state, gpu=0)
    prepared = ours.prepare(*batch)
    contenders = {'ours': lambda: ours.step(prepared)}
    if arguments.only is None and arguments.precision != 'f32':
        split = train.Trainer(
            checkpoint=state, gpu=0, precision=arguments.precision)
        split_batch = split.prepare(*batch)
        contenders[f'ours_{arguments.precision}'] = \
            lambda: split.step(split_batch)
    if arguments.only is None and dropped is not None:
        masked = train.Trainer(
            dropped, checkpoint=state, gpu=0, precision=arguments.precision)
        masked_batch = masked.prepare(*batch)
        contenders['ours_dropout'] = lambda: masked.step(masked_batch)
    parent = None
    if arguments.only is None and arguments.parent:
        parent = Parent(arguments.parent)
        contenders['ours_parent'] = parent
    if arguments.only is None and not arguments.no_torch:
        features, _, bounds, _, targets = (item.cuda() for item in batch)
        frame = torch.arange(FRAMES, device='cuda')[None, :, None]
        membership = ((frame >= bounds[:, 0, None, :]) &
                      (frame < bounds[:, 1, None, :])).float()
        for name, mixed in (('torch_fp32', False), ('torch_autocast', True)):
            model = TorchModel(state, arguments.dropout).cuda()
            optimizer = torch.optim.Adam(model.parameters())
            scaler = torch.amp.GradScaler('cuda') if mixed else None
            contenders[name] = (
                lambda m=model, o=optimizer, s=scaler: torch_step(
                    m, o, s, features, membership, targets))
    try:
        first = {}
        for name, function in contenders.items():
            first[name] = float(function())
            for _ in range(4):
                function()
        torch.cuda.synchronize()
        steps = {}
        for name, function in contenders.items():
            probe = run_lap(function, 5)
            steps[name] = arguments.steps or max(
                5, int(arguments.seconds * 1e3 / probe))
        if arguments.only:
            timed(contenders['ours'], steps['ours'])
            print(json.dumps({'ours_steps': steps['ours'],
                              'precision': arguments.precision,
                              'dropout': arguments.dropout}))
            return
        laps = {name: [] for name in contenders}
        for _ in range(arguments.laps):
            for name, function in contenders.items():
                laps[name].append(run_lap(function, steps[name]))
    finally:
        if parent is not None:
            parent.close()
    record = {
        'batch': {'utterances': ITEMS, 'frames': FRAMES, 'words': WORDS},
        'device': torch.cuda.get_device_name(0),
        'laps': arguments.laps, 'steps_per_lap': steps,
        'dropout': arguments.dropout, 'precision': arguments.precision,
        'first_loss': first,
        'ms_per_step': {
            name: {'median': float(np.median(values)),
                   'min': float(np.min(values)), 'max': float(np.max(values))}
            for name, values in laps.items()}}
    median = {name: record['ms_per_step'][name]['median'] for name in laps}
    record['ms_per_step_laps'] = laps
    if 'ours_dropout' in median:
        record['ours_dropout_over_ours'] = \
            median['ours_dropout'] / median['ours']
        if 'torch_fp32' in median:
            record['torch_fp32_over_ours_dropout'] = \
                median['torch_fp32'] / median['ours_dropout']
            record['torch_autocast_over_ours_dropout'] = \
                median['torch_autocast'] / median['ours_dropout']
        # emph_dropout and emph_activation_dropout_backward per step: bytes
        # read + written, and the 32 x 32 -> 64 integer multiplies of
        # Philox-4x32-10 (2 a round, 10 rounds, per quad of elements)
        # over the packed buffers [80, ld] of the 6 + 6 layers
        elements = 6 * 80 * (
            masked_batch.plan.ld_frames + masked_batch.plan.ld_words)
        record['dropout_forward_bytes'] = 8 * elements
        record['dropout_backward_bytes'] = 12 * elements
        record['dropout_integer_multiplies'] = 20 * (elements // 4)
    if 'torch_fp32' in median:
        record['torch_fp32_over_ours'] = median['torch_fp32'] / median['ours']
        record['torch_autocast_over_ours'] = \
            median['torch_autocast'] / median['ours']
    # executed MFMA flops of emph_conv_weight_grad per step: 64-position
    # tiles, 5 m-tiles x (3 x 5 + 1) n-tiles of 16 x 16 per k-step of 4
    tiles = ITEMS * -(-FRAMES // 64), ITEMS * -(-WORDS // 64)
    record['weight_grad_executed_flops'] = float(
        2 * 16 * 16 * 64 * 5 * 16 * (7 * tiles[0] + 6 * tiles[1]))
    record['fp32_matrix_peak_flops'] = PEAK_FP32_MATRIX
    print(json.dumps(record))
    if arguments.out:
        with open(arguments.out, 'w') as file:
            json.dump(record, file, indent=1)
            file.write('\n')


if __name__ == '__main__':
    main()
