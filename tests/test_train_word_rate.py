"""What tests/test_gpu_train_word_rate.py stands on, checked without a device:
the float64 restatement of `word_rate_data` against the reference's recorded
loss and gradients, the properties of the `HARD` layout, and the distance of
every ReLU input from zero under the recorded seed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import train_data  # noqa: E402
import word_rate_data  # noqa: E402

from emphases_amd import runtime, weights  # noqa: E402


@pytest.mark.parametrize('case', ['ragged', 'mse', 'average'])
def test_the_restatement_reproduces_the_reference(case):
    """The stored gradients are float64 rounded to float32 (6e-8 of a value);
    2e-7 of max |want| leaves room for that and nothing else."""
    golden = train_data.golden()
    overrides = train_data.VARIANTS.get(case, {})
    loss, gradients, _ = word_rate_data.restatement(
        weights.load(weights.DEFAULT_CHECKPOINT), train_data.collated(case),
        overrides.get('downsample_method', 'sum'),
        overrides.get('loss', 'bce'))
    want_loss = float(golden[f'{case}/loss'])
    print(f'{case}: loss {loss:.17g}, reference {want_loss:.17g}')
    assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
    wanted = train_data.gradients(case)
    assert wanted and set(wanted) <= set(gradients)
    if case == 'ragged':
        assert set(wanted) == set(gradients)
    worst = 0.
    for name, want in wanted.items():
        got = gradients[name].numpy()
        assert got.shape == want.shape
        worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print(f'{case}: worst gradient error {worst:.3g}')
    assert worst <= 2e-7


def test_the_hard_layout_has_the_properties_the_tests_rely_on():
    plan = word_rate_data.plan_of(word_rate_data.HARD)
    other = word_rate_data.plan_of(word_rate_data.REVERSED)
    assert plan.ld_words > 512
    segment = plan.word_segment
    abutting = [c for c in range(plan.ld_words - 1)
                if segment[c] >= 0 and segment[c + 1] >= 0 and
                segment[c] != segment[c + 1]]
    assert len(abutting) >= 2, abutting
    # valid words on both sides of column 256: a second trip of a 256-thread
    # walk meets them, and a third (padding alone) follows
    columns = plan.word_columns()
    assert columns.min() < 256 < columns.max() and len(columns) == 354
    assert (plan.words == 0).any()
    assert (plan.frames == 1).any()
    uncovered = 0
    for utterance in word_rate_data.HARD:
        covered = np.zeros(utterance.frames, dtype=bool)
        for start, end in utterance.bounds.T:
            assert not covered[start:end].any()
            covered[start:end] = True
        if utterance.bounds.shape[1]:
            uncovered += int((~covered).sum())
            if not covered.all():
                # a head, a gap and a tail
                assert not covered[0] and not covered[-1]
                assert (~covered[utterance.bounds[0, 0]:
                                 utterance.bounds[1, -1]]).any()
    assert uncovered > 0
    frames, tile = runtime.AXIS_FRAMES, 64
    for first, second in (
            (plan, other),
            (word_rate_data.plan_of(word_rate_data.HARD_WORDED),
             word_rate_data.plan_of(word_rate_data.REVERSED_WORDED))):
        assert first.ld_frames == second.ld_frames
        assert first.ld_words == second.ld_words
        assert len(first.tiles(frames, tile)) == len(second.tiles(frames, tile))
        assert first.total_words == second.total_words
        assert not np.array_equal(first.word_off, second.word_off)
        assert not np.array_equal(first.frame_off, second.frame_off)
    assert plan.ld_frames <= 16 + 580 + 6 * 15 + 128 and plan.ld_words == 528


def test_no_relu_input_is_near_zero_under_the_recorded_seed():
    """1e-6 of the layer's largest value is ten times what a 240-term float32
    dot product is off by; the recorded seed is the first that keeps it."""
    for seed in range(word_rate_data.SEED):
        assert word_rate_data.relu_margin(seed) < word_rate_data.MARGIN, seed
    margin = word_rate_data.relu_margin(word_rate_data.SEED)
    print(f'seed {word_rate_data.SEED}: smallest relative ReLU input '
          f'{margin:.3g}')
    assert margin >= word_rate_data.MARGIN
