"""Dropout of the training step on the MI355X: `emph_dropout` and
`emph_activation_dropout_backward` alone, bitwise against the host
specification (`emphases_amd/train/dropout.py`); the step's loss and gradients
against the unmodified reference under DROPOUT with the same masks
(tests/golden/dropout*.npz, written by tests/golden/generate_dropout.py);
identity, determinism and resume.

The bound of the gradient comparison is 4 x the reference's own float32 error
(`ref32_error`), the project's standing allowance; at precision='bf16x3' the
recorded error of the two-piece arithmetic (`ragged/emulated_error` of
train_split.npz) is added, as in test_gpu_train_precision.py: dropping a share
of the terms and scaling the rest leaves the relative rounding of a split
product as it is.  Each figure is printed before it is asserted.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import dropout_data  # noqa: E402
import loop_data  # noqa: E402
import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import runtime, synth, train, weights  # noqa: E402
from emphases_amd.train import dropout  # noqa: E402

pytestmark = pytest.mark.gpu

RELU = runtime.ACTIVATIONS['relu']
# 80 x 1040 = 20 800 quads: 82 blocks of 256 threads, the last one partial
SHAPES = [(4, 0), (80 * 16, 0), (80 * 1040, 0), (80 * 1040, (1 << 34) - 8)]


def values(count, seed):
    """randn with exact zeros of both signs among it."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(count).astype(np.float32)
    x[rng.random(count) < 0.1] = 0.
    x[rng.random(count) < 0.05] = -0.
    x[:4] = [0., -1.5, 2.5, -0.]
    assert (x < 0).any() and (x == 0).any() and (x > 0).any()
    return x


def dropped(x, p, seed, stream_id, step, origin=0):
    out = torch.from_numpy(x).cuda()
    runtime.check(runtime.library().emph_dropout(
        out.data_ptr(), out.numel(), origin, p, seed, stream_id, step,
        runtime.stream()), 'emph_dropout')
    return out.cpu().numpy()


def bits(array):
    return np.ascontiguousarray(array).view(np.uint32)


@pytest.mark.parametrize('count,origin', SHAPES)
def test_dropout_is_bitwise_the_specification(count, origin):
    seed = 0xfedcba9876543210
    x = values(count, count)
    for p in (0.1, 0.5):
        got = dropped(x, p, seed, 5, 3, origin)
        keep = dropout.keep_mask(seed, 5, 3, count, p, origin)
        want = np.where(keep, x * dropout.scale(p), np.float32(0))
        assert want.dtype == np.float32
        assert np.array_equal(bits(got), bits(want))
        assert not bits(got)[~keep].any()           # +0.0, never -0.0
        if count > 4:
            assert 0 < keep.sum() < count
        # the same call again: the same bits
        assert np.array_equal(bits(dropped(x, p, seed, 5, 3, origin)), bits(got))
    # p = 0 is the identity, bit for bit
    assert np.array_equal(bits(dropped(x, 0., seed, 5, 3, origin)), bits(x))


def test_dropout_masks_depend_on_stream_step_and_seed():
    count = 80 * 1040
    x = np.ones(count, dtype=np.float32)
    base = dropped(x, 0.5, 11, 2, 7) != 0
    assert np.array_equal(base, dropout.keep_mask(11, 2, 7, count, 0.5))
    for name, arguments in (('stream', (11, 3, 7)), ('step', (11, 2, 8)),
                            ('seed', (12, 2, 7)),
                            ('seed_hi', (11 + (1 << 32), 2, 7))):
        other = dropped(x, 0.5, *arguments) != 0
        assert np.array_equal(
            other, dropout.keep_mask(*arguments, count, 0.5)), name
        assert 0.4 < np.mean(other != base) < 0.6, name
    # what lies in a dropped place never matters: a select, not a product
    noise = x.copy()
    noise[~base] = np.array([np.nan, np.inf, -np.inf, -1.])[
        np.arange((~base).sum()) % 4]
    assert np.array_equal(bits(dropped(noise, 0.5, 11, 2, 7)),
                          bits(dropped(x, 0.5, 11, 2, 7)))


def test_activation_dropout_backward_alone():
    count = 80 * 1040
    y = np.maximum(values(count, 1), np.float32(0))       # after ReLU + dropout
    y[:4] = [0., -0., 2.5, -1.]                           # (padding may hold < 0)
    gradient = values(count, 2)
    lib = runtime.library()
    y_device = torch.from_numpy(y).cuda()

    def backward(p):
        out = torch.from_numpy(gradient).cuda()
        if p is None:
            runtime.check(lib.emph_activation_backward(
                y_device.data_ptr(), out.data_ptr(), count, RELU,
                runtime.stream()), 'emph_activation_backward')
        else:
            runtime.check(lib.emph_activation_dropout_backward(
                y_device.data_ptr(), out.data_ptr(), count, RELU, p,
                runtime.stream()), 'emph_activation_dropout_backward')
        return out.cpu().numpy()

    for p in (0.1, 0.5):
        want = np.where(y > 0, gradient * dropout.scale(p), np.float32(0))
        assert np.array_equal(bits(backward(p)), bits(want))
    assert np.array_equal(bits(backward(0.)), bits(backward(None)))
    assert torch.equal(y_device.cpu(), torch.from_numpy(y))


def reference_trainer(case, precision='f32'):
    p, seed, step = dropout_data.settings(case)
    model = train.Trainer(
        emphases_amd.Config(dropout=p), checkpoint=weights.DEFAULT_CHECKPOINT,
        gpu=0, seed=seed, precision=precision)
    model.steps = step
    return model


@pytest.mark.parametrize('case,precision', [
    ('p10', 'f32'), ('p50', 'f32'), ('p10', 'bf16x3')])
def test_gradients_match_the_reference(case, precision):
    golden = dropout_data.golden()
    bound = float(golden[f'{case}/ref32_error'])
    if precision == 'bf16x3':
        with np.load(os.path.join(HERE, 'golden', 'train_split.npz')) as split:
            bound += float(split['ragged/emulated_error'])
    bound *= 4.
    loss, gradients = reference_trainer(case, precision).loss_and_gradients(
        *train_data.collated('ragged'))
    want_loss = float(golden[f'{case}/loss'])
    loss_error = abs(float(loss) - want_loss) / abs(want_loss)
    print(f'{case} {precision}: loss {float(loss):.9g} (reference '
          f'{want_loss:.9g}), error {loss_error:.3g}, bound {bound:.3g} '
          f'({loss_error / bound:.2f} of the bound)')
    wanted = dropout_data.gradients(case)
    assert wanted and set(wanted) <= set(gradients)
    if case == 'p10':
        assert set(wanted) == set(gradients)
    worst = {}
    for name, want in wanted.items():
        got = gradients[name].cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        worst[name] = np.abs(got - want).max() / np.abs(want).max()
        print(f'{case} {precision}: {name} error {worst[name]:.3g} '
              f'({worst[name] / bound:.2f} of the bound)')
    assert loss_error <= bound
    missed = {name: error for name, error in worst.items() if not error <= bound}
    assert not missed, (missed, bound)


def same(first, second):
    return all(torch.equal(first[name].view(torch.int32),
                           second[name].view(torch.int32)) for name in first)


def test_identity_and_determinism():
    batch = train_data.collated('ragged')
    build = lambda value: train.Trainer(  # noqa: E731
        emphases_amd.Config(dropout=value),
        checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0, seed=3)
    plain, zero, half = build(None), build(0.0), build(0.5)
    # 0.0 is the identity (torch.nn.Dropout(0.)), bit for bit
    loss, gradients = plain.loss_and_gradients(*batch)
    zero_loss, zero_gradients = zero.loss_and_gradients(*batch)
    assert torch.equal(loss, zero_loss) and same(gradients, zero_gradients)
    # validation never drops
    prepared = half.prepare(*batch)
    assert torch.equal(half.logits(prepared), plain.logits(prepared))
    # the same batch at the same step: the same bits; at another step, another
    # mask (the parameters are the same)
    first_loss, first = half.loss_and_gradients(prepared)
    again_loss, again = half.loss_and_gradients(prepared)
    assert torch.equal(first_loss, again_loss) and same(first, again)
    assert not torch.equal(first_loss, loss)
    half.steps = 1
    moved_loss, moved = half.loss_and_gradients(prepared)
    assert not torch.equal(moved_loss, first_loss)
    assert not torch.equal(moved['input_layer.weight'],
                           first['input_layer.weight'])
    half.steps = 0
    back_loss, back = half.loss_and_gradients(prepared)
    assert torch.equal(back_loss, first_loss) and same(back, first)
    # another seed, another mask
    other = train.Trainer(
        emphases_amd.Config(dropout=0.5),
        checkpoint=weights.DEFAULT_CHECKPOINT, gpu=0, seed=4)
    assert not torch.equal(other.loss_and_gradients(prepared)[0], first_loss)
    # after one update the gradients of the same batch differ
    half.step(prepared)
    assert half.steps == 1
    assert not torch.equal(
        half.loss_and_gradients(prepared)[1]['output_layer.weight'],
        first['output_layer.weight'])


def test_resume_continues_the_mask_stream(tmp_path):
    """One epoch of the synthetic cache at 600 frames a batch, then a resumed
    run to the end of the second, against the two epochs uninterrupted: a
    resumed run restarts its file's epoch, so the stop lies on an epoch's
    end.  The seed is not the default, so the resumed trainer must be handed
    it."""
    from emphases_amd import data
    partition_dir, cache_dir = loop_data.build_cache(str(tmp_path / 'data'))
    config = emphases_amd.Config(dropout=0.1)
    sampler = data.Sampler(data.Dataset(
        loop_data.DATASET, 'train', partition_dir=partition_dir,
        cache_dir=cache_dir, config=config, gpu=0, upload=False), 600, 7)
    stop = len(sampler)
    sampler.set_epoch(1)
    end = stop + len(sampler)
    assert stop >= 2 and end >= stop + 2

    def run(directory, num_steps):
        return train.train(
            loop_data.DATASET, tmp_path / directory, 0,
            partition_dir=partition_dir, cache_dir=cache_dir, config=config,
            max_training_frames=600, num_steps=num_steps, seed=7)

    load = lambda path: torch.load(  # noqa: E731
        path, map_location='cpu', weights_only=False)
    first = load(run('resumed', stop))
    assert first['step'] == stop and first['epoch'] == 1
    resumed = load(run('resumed', end))
    whole_path = run('whole', end)
    whole = load(whole_path)
    assert resumed['step'] == whole['step'] == end
    names = list(train.checkpoint_names(config).values())
    assert 'frame_encoder.15.weight' in names and \
        'word_decoder.3.bias' in names and 'frame_encoder.2.weight' not in names
    assert list(whole['model']) == names == list(resumed['model'])
    for name in names:
        assert torch.equal(resumed['model'][name].view(torch.int32),
                           whole['model'][name].view(torch.int32)), name
    for index, entry in whole['optimizer']['state'].items():
        for moment in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(
                resumed['optimizer']['state'][index][moment], entry[moment])
    # the masks were in play: the same run without dropout ends elsewhere
    assert not torch.equal(first['model']['output_layer.weight'], load(
        train.train(
            loop_data.DATASET, tmp_path / 'plain', 0,
            partition_dir=partition_dir, cache_dir=cache_dir,
            config=emphases_amd.DEFAULT, max_training_frames=600,
            num_steps=stop, seed=7))['model']['output_layer.weight'])
    # inference reads the file, whatever its configuration says of dropout
    audio = torch.from_numpy(synth.audio(3, 211))
    alignment = emphases_amd.Alignment.from_frames(
        synth.word_frames(3, 211, 3, 40))
    scores = emphases_amd.from_alignment_and_audio(
        alignment, audio, emphases_amd.SAMPLE_RATE, checkpoint=whole_path,
        gpu=0)
    assert scores.shape[-1] == len(alignment) and torch.isfinite(scores).all()
    trainer = train.Trainer(config, checkpoint=whole_path, gpu=0, seed=7)
    assert trainer.steps == end
    assert list(trainer.state_dict()) == names
    state = weights.load(whole_path, emphases_amd.DEFAULT)
    assert np.array_equal(
        state['frame_encoder.10.weight'],
        whole['model']['frame_encoder.15.weight'].numpy())
