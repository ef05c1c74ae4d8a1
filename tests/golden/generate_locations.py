"""Capture golden vectors of the reference's training step for the models
without a word decoder - DOWNSAMPLE_LOCATION 'inference' and 'loss', which
`emphases_amd.train.EncoderTrainer` trains - and of `emphases.upsample`.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_locations.py

Imports the UNMODIFIED reference `emphases` with the stand-ins of
`tests/golden/stubs/` (through `generate_grid.py`, whose helpers it shares)
and runs, on the CPU with one thread and without autocast, its `Model` in
train mode, its loss and autograd with LAYERS = 2 from the reference's own
initialisation under `torch.manual_seed(seed)`, on the stored `ragged` inputs
of tests/golden/train.npz, one utterance at a time.  The loss is
sum_i w_i loss_i with w_i = T_i / sum T (frames) at 'inference', whose loss is
a mean over frames, and n_i / N (words) at 'loss'; the backward calls
accumulate.

Variants (everything else as `config/defaults.py`), one file
tests/golden/locations_<variant>.npz each:

  sum_inference              'inference', UPSAMPLE_METHOD 'linear', bce; also
                             `clamped_frames`, the number of frames whose
                             target the clamp of `train/core.py:335-336`
                             changed (asserted non-zero), and `eval/<method>`:
                             the word logits of the same model in eval mode
                             (float64) under each DOWNSAMPLE_METHOD.  The seed
                             is the first at which 'max' has no near tie
                             (generate_grid.py's rule, margin 1e-4)
  sum_inference_nearest_mse  'inference', 'nearest', LOSS 'mse'
  sum_loss                   'loss'
  max_loss                   'loss', DOWNSAMPLE_METHOD 'max' (near-tie rule)
  sum_inference_dropout10    'inference', DROPOUT 0.1 with the masks of
                             `emphases_amd/train/dropout.py` injected as
                             generate_dropout.py injects them (its seed, which
                             is the model's seed here too, step 0)

Per file: the seed, the loss (float64), the float64 gradients under the
package's internal names STORED rounded to float32, the `init/` sums (sum and
sum of squares of every initial tensor) and `ref32_error`, the worst over
tensors of max|g32 - g64| / max|g64| of the same run in float32.

tests/golden/upsample.npz: the reference's `emphases.upsample` in float64,
every utterance alone, for 'linear' (C = 1) and 'nearest' (C = 3) on five
utterances (`CASES`), with `<method>/ref32_error`: the worst over the
utterances of max|u32 - u64| / max|u64| of its float32 run.

The GPU box never runs this script; it only reads the .npz files.
"""
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import generate_grid as base  # noqa: E402  (paths, stubs, the reference)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases  # noqa: E402  (the reference)
import generate_dropout as masks  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import train  # noqa: E402

LAYERS = 2
DEFAULTS = dict(
    base.DEFAULTS, UPSAMPLE_METHOD='linear', DROPOUT=None)
VARIANTS = {
    'sum_inference': dict(DOWNSAMPLE_LOCATION='inference'),
    'sum_inference_nearest_mse': dict(
        DOWNSAMPLE_LOCATION='inference', UPSAMPLE_METHOD='nearest',
        LOSS='mse'),
    'sum_loss': dict(DOWNSAMPLE_LOCATION='loss'),
    'max_loss': dict(DOWNSAMPLE_LOCATION='loss', DOWNSAMPLE_METHOD='max'),
    'sum_inference_dropout10': dict(
        DOWNSAMPLE_LOCATION='inference', DROPOUT=0.1),
}
METHODS = ('sum', 'average', 'max', 'center')

# (frames, word starts, word ends) of upsample.npz
CASES = (
    (1, [0], [1]),
    (7, [0, 3], [3, 7]),
    # gaps between the words, the first one starts after frame 0
    (64, [3, 12, 25, 41, 55], [10, 20, 40, 50, 64]),
    # two one-frame words and odd lengths: frame centres that equal a centre
    (65, [0, 1, 4, 5, 12, 20, 33, 40, 52], [1, 4, 5, 12, 20, 33, 40, 52, 65]),
    (200, list(range(0, 200, 5)), list(range(5, 205, 5))),
)


def package_config(settings):
    return emphases_amd.Config(
        layers=LAYERS,
        downsample_location=settings['DOWNSAMPLE_LOCATION'],
        downsample_method=settings.get('DOWNSAMPLE_METHOD', 'sum'),
        upsample_method=settings.get('UPSAMPLE_METHOD', 'linear'),
        loss=settings.get('LOSS', 'bce'), dropout=settings.get('DROPOUT'))


def build(seed, dtype, settings, plan):
    """The reference's model from its own initialisation; under DROPOUT with
    every `torch.nn.Dropout` replaced by the package's mask of step 0."""
    net = base.model(seed, dtype)
    p = settings.get('DROPOUT')
    if p is not None:
        assert seed == masks.SEED
        config = package_config(settings)
        stack = net.frame_encoder
        assert len(stack) == 3 * LAYERS and not hasattr(net, 'word_decoder')
        for i in range(LAYERS):
            assert isinstance(stack[3 * i + 2], torch.nn.Dropout)
            stack[3 * i + 2] = masks.FixedMask(masks.layer_masks(
                config, plan, f'frame_encoder.{2 * i}', p, 0), p)
        assert not any(isinstance(module, torch.nn.Dropout)
                       for module in net.modules())
    return net


def accumulate(net, items, dtype, loss_fn, location, watch=None):
    """Every utterance alone, weighted by its share of the loss's mean: the
    loss and the number of frames whose target the clamp changed; the
    gradients are left in `.grad`."""
    net.zero_grad()
    axis = 0 if location == 'inference' else 1
    total_count = sum(item[axis].shape[1] for item in items)
    total, clamped = 0., 0
    for index, (features, bounds, targets) in enumerate(items):
        masks.FixedMask.CURRENT[0] = index
        seen = []
        hook = net.frame_encoder.register_forward_hook(
            lambda module, inputs, output: seen.append(output.detach()))
        frame_lengths = torch.tensor([features.shape[1]])
        word_bounds = torch.from_numpy(bounds)[None]
        word_lengths = torch.tensor([bounds.shape[1]])
        scores = net(torch.from_numpy(features)[None].to(dtype), frame_lengths,
                     word_bounds, word_lengths)
        hook.remove()
        if watch is not None:
            watch(seen[0][0], bounds)
        wide_targets = torch.from_numpy(targets)[None, None].to(dtype)
        if location == 'inference':
            assert scores.shape == (1, 1, features.shape[1])
            if emphases.UPSAMPLE_METHOD == 'linear':
                spread = emphases.upsample(
                    wide_targets, word_bounds, word_lengths, frame_lengths)
                clamped += int(((spread < 0) | (spread > 1)).sum())
        else:
            assert scores.shape == (1, 1, bounds.shape[1])
        value = sys.modules['emphases.train.core'].loss(
            scores, wide_targets, frame_lengths, word_bounds, word_lengths,
            training=True, loss_fn=loss_fn) * (
                items[index][axis].shape[1] / total_count)
        value.backward()
        total += float(value.detach().double())
    return total, clamped


def internal(config, gradients):
    """The reference's names (`3 i` under DROPOUT) back to the package's."""
    saved = train.checkpoint_names(config)
    assert set(saved.values()) == set(gradients), (saved, list(gradients))
    return {name: gradients[saved[name]] for name in saved}


def eval_logits(net, items, method, watch=None):
    """Word logits of the model in eval mode under DOWNSAMPLE_METHOD
    `method`, the utterances one after the other."""
    emphases.DOWNSAMPLE_METHOD = method
    net.eval()
    out = []
    with torch.no_grad():
        for features, bounds, _ in items:
            seen = []
            hook = net.frame_encoder.register_forward_hook(
                lambda module, inputs, output: seen.append(output.detach()))
            scores = net(
                torch.from_numpy(features)[None].to(
                    next(net.parameters()).dtype),
                torch.tensor([features.shape[1]]),
                torch.from_numpy(bounds)[None],
                torch.tensor([bounds.shape[1]]))
            hook.remove()
            if watch is not None:
                watch(seen[0][0], bounds)
            assert scores.shape == (1, 1, bounds.shape[1])
            out.append(scores[0, 0].double().numpy())
    net.train()
    return np.concatenate(out)


def capture(variant, settings, items, plan):
    for name, value in {**DEFAULTS, **settings}.items():
        if name != 'LOSS':
            setattr(emphases, name, value)
    emphases.LAYERS = LAYERS
    loss_fn = settings.get('LOSS', 'bce')
    location = settings['DOWNSAMPLE_LOCATION']
    method = settings.get('DOWNSAMPLE_METHOD', 'sum')
    config = package_config(settings)
    seeds = [masks.SEED] if settings.get('DROPOUT') is not None else range(100)
    evaluated = {}
    for seed in seeds:
        try:
            wide = build(seed, torch.float64, settings, plan)
            loss, clamped = accumulate(
                wide, items, torch.float64, loss_fn, location,
                base.no_near_ties if method == 'max' else None)
            if variant == 'sum_inference':
                evaluated = {
                    name: eval_logits(
                        wide, items, name,
                        base.no_near_ties if name == 'max' else None)
                    for name in METHODS}
                emphases.DOWNSAMPLE_METHOD = method
            break
        except ArithmeticError:
            print(variant, 'seed', seed, 'has a near tie; next')
    else:
        raise ArithmeticError(f'{variant}: every seed has a near tie')
    exact = internal(config, base.gradients(wide))
    narrow = build(seed, torch.float32, settings, plan)
    accumulate(narrow, items, torch.float32, loss_fn, location)
    rounded = internal(config, base.gradients(narrow))
    for name, value in exact.items():
        assert np.abs(value).max() > 0, f'{variant} {name}: zero gradient'
    error = max(
        np.abs(rounded[name] - exact[name]).max() / np.abs(exact[name]).max()
        for name in exact)
    out = {'seed': np.int64(seed), 'loss': np.float64(loss),
           'ref32_error': np.float64(error)}
    saved = train.checkpoint_names(config)
    initial = dict(build(seed, torch.float32, settings, plan).named_parameters())
    for name in saved:
        value = initial[saved[name]].detach().double().numpy()
        out[f'init/{name}'] = np.array([value.sum(), (value ** 2).sum()])
    for name, value in exact.items():
        out[f'grad/{name}'] = value.astype(np.float32)
    if variant == 'sum_inference':
        assert clamped > 0, 'the clamp changes no target'
        out['clamped_frames'] = np.int64(clamped)
        for name, value in evaluated.items():
            out[f'eval/{name}'] = value
    if settings.get('DROPOUT') is not None:
        out['p'] = np.float64(settings['DROPOUT'])
    path = os.path.join(HERE, f'locations_{variant}.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(variant, 'seed', seed, 'loss', loss, 'ref32', error, 'clamped',
          clamped, size, 'bytes')
    assert size < 1 << 20


def capture_upsample():
    rng = np.random.default_rng(20261019)
    frames = np.array([case[0] for case in CASES], dtype=np.int64)
    words = np.array([len(case[1]) for case in CASES], dtype=np.int64)
    bounds = np.concatenate(
        [np.array([case[1], case[2]], dtype=np.int64) for case in CASES],
        axis=1)
    out = {'frames': frames, 'words': words, 'bounds': bounds}
    for method, channels in (('linear', 1), ('nearest', 3)):
        emphases.UPSAMPLE_METHOD = method
        x = rng.random((channels, int(words.sum()))).astype(np.float32)
        wide, worst, first = [], 0., 0
        for count, starts, ends in CASES:
            arguments = (
                torch.tensor([[starts, ends]]), torch.tensor([len(starts)]),
                torch.tensor([count]))
            piece = torch.from_numpy(x[None, :, first:first + len(starts)])
            exact = emphases.upsample(piece.double(), *arguments)[0].numpy()
            rounded = emphases.upsample(piece, *arguments)[0].double().numpy()
            assert exact.shape == (channels, count)
            worst = max(worst, np.abs(rounded - exact).max() /
                        np.abs(exact).max())
            wide.append(exact)
            first += len(starts)
        out[f'{method}/x'] = x
        out[f'{method}/y'] = np.concatenate(wide, axis=1)
        out[f'{method}/ref32_error'] = np.float64(worst)
        print('upsample', method, 'ref32', worst)
    emphases.UPSAMPLE_METHOD = 'linear'
    path = os.path.join(HERE, 'upsample.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20


def main():
    assert emphases.DROPOUT is None and emphases.LOSS == 'bce'
    assert emphases.UPSAMPLE_METHOD == 'linear'
    items = base.ragged()
    plan = masks.packed_plan()
    assert list(plan.frames) == [item[0].shape[1] for item in items]
    for variant, settings in VARIANTS.items():
        capture(variant, settings, items, plan)
    for name, value in DEFAULTS.items():
        setattr(emphases, name, value)
    capture_upsample()
    leaked = [
        root for root, dirs, _ in os.walk(base.REFERENCE)
        if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
