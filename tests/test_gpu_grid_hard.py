"""`GridTrainer` on the MI355X across its grid and on hard layouts: six
configurations that each cross several fields no golden covers (tests/
grid_data.py: channels 16 .. 128, kernel sizes 1 .. 7 on either axis, every
activation and reduction, dropout, `mse`, layers 0, 1 and 3) on the `HARD`
layout of tests/word_rate_data.py, three of them on `ABUT` (segments that abut
on both axes, one word past the 32- and the 64-wide tile), against the float64
restatement that tests/test_grid_data.py anchors to the reference; and one
trainer's buffers under two layouts with the same leading dimensions.

A bound is 4 x `ref32`: the restatement in float32 against itself in float64,
worst tensor, over max |want| (the project's standing allowance).  The masks
are those of step 3.  The oracle is torch on the CPU, never the library.  Each
figure is printed before it is asserted.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import grid_data  # noqa: E402
import word_rate_data  # noqa: E402

from emphases_amd import train, weights  # noqa: E402

pytestmark = pytest.mark.gpu


def assert_initial(trainer, config, seed):
    """The trainer's parameters are bitwise `initial_state(config, seed)`."""
    state = train.initial_state(config, seed)
    saved = train.checkpoint_names(config)
    held = trainer.state_dict()
    assert set(held) == {saved[name] for name in state}
    for name, value in state.items():
        assert np.array_equal(held[saved[name]].numpy(), value), name


@pytest.mark.parametrize('case,layout', grid_data.PAIRS)
def test_the_step_matches_the_restatement(case, layout):
    config, seed, _, want, ref32 = grid_data.reference(case, layout)
    trainer = train.GridTrainer(config, gpu=0, seed=seed)
    assert_initial(trainer, config, seed)
    trainer.steps = grid_data.STEP
    got_loss, gradients = trainer.loss_and_gradients(
        *grid_data.collate(grid_data.LAYOUTS[layout], seed, num_features=80))
    assert trainer.steps == grid_data.STEP
    bound = 4. * ref32
    label = f'grid {case} {layout}'
    loss_error = abs(float(got_loss) - want.loss) / abs(want.loss)
    print(f'{label}: loss {float(got_loss):.9g} (float64 {want.loss:.9g}), '
          f'error {loss_error:.3g}, bound {bound:.3g}, ratio '
          f'{loss_error / bound:.2f}')
    assert set(gradients) == set(want.gradients) == \
        set(weights.parameter_shapes(config))
    worst = {}
    for name, value in want.gradients.items():
        got = gradients[name].cpu().double()
        assert got.shape == value.shape
        worst[name] = float((got - value).abs().max() / value.abs().max())
        print(f'{label} {name}: error {worst[name]:.3g}, bound {bound:.3g}, '
              f'ratio {worst[name] / bound:.2f}')
    assert loss_error <= bound
    missed = {name: error for name, error in worst.items()
              if not error <= bound}
    assert not missed, (missed, bound)


@pytest.mark.parametrize('case', ['A', 'D'])
def test_a_new_layout_in_reused_buffers_changes_nothing(case):
    """One trainer runs HARD, then REVERSED in the same buffers, which hold
    HARD's values in REVERSED's padding columns; a fresh trainer runs REVERSED
    alone.  Case A keeps the pre-activations ('pre_frames', 'pre_words'),
    case D has dropout and `max`."""
    config, seed = grid_data.config_of(case), grid_data.SEEDS[case, 'hard']
    plans = [word_rate_data.plan_of(layout)
             for layout in (grid_data.HARD, grid_data.REVERSED)]
    assert plans[0].ld_frames == plans[1].ld_frames
    assert plans[0].ld_words == plans[1].ld_words
    assert not np.array_equal(plans[0].word_off, plans[1].word_off)
    used = train.GridTrainer(config, gpu=0, seed=seed)
    fresh = train.GridTrainer(config, gpu=0, seed=seed)
    used.steps = fresh.steps = grid_data.STEP
    used.loss_and_gradients(*grid_data.collate(grid_data.HARD, seed))
    buffers = dict(used._workspace)
    (kept,) = buffers.values()
    assert ('pre_frames' in kept) == ('pre_words' in kept) == (case == 'A')
    # ... which now hold the first layout's values between the second's
    # utterances, on both axes
    for axis, offsets, counts, ld in (
            ('frames', plans[1].frame_off, plans[1].frames,
             plans[1].ld_frames),
            ('words', plans[1].word_off, plans[1].words, plans[1].ld_words)):
        outside = torch.ones(ld, dtype=torch.bool)
        for off, count in zip(offsets, counts):
            outside[off:off + count] = False
        outside = outside.cuda()
        assert kept[axis][:, :, outside].any(), axis
        if case == 'A':
            assert kept[f'pre_{axis}'][:, :, outside].any(), axis
    batch = grid_data.collate(grid_data.REVERSED, seed)
    got_loss, got = used.loss_and_gradients(*batch)
    # the cached buffers really were reused
    assert len(used._workspace) == 1 and all(
        used._workspace[key] is value for key, value in buffers.items())
    want_loss, want = fresh.loss_and_gradients(*batch)
    assert float(want_loss) > 0. and np.isfinite(float(want_loss))
    assert torch.equal(got_loss, want_loss), (got_loss, want_loss)
    assert set(got) == set(want) == set(weights.parameter_shapes(config))
    for name in want:
        assert torch.isfinite(want[name]).all() and want[name].any(), name
        assert torch.equal(got[name], want[name]), name
    assert torch.equal(used.step(*batch), fresh.step(*batch))
    assert used.steps == fresh.steps == grid_data.STEP + 1
    for name in ('parameters', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(getattr(used, name), getattr(fresh, name)), name
    assert not torch.equal(fresh.exp_avg, torch.zeros_like(fresh.exp_avg))


@pytest.mark.parametrize('case', list(grid_data.CASES))
def test_select_trainer_picks_the_grid_step(case):
    config = grid_data.config_of(case)
    trainer = train.select_trainer(config, gpu=0, seed=1)
    assert type(trainer) is train.GridTrainer
    assert trainer.config == config and trainer.seed == 1
    assert_initial(trainer, config, 1)
