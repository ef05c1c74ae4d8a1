"""What tests/test_gpu_grid_hard.py stands on, checked without a device: the
float64 restatement of `grid_data` against the reference's recorded loss and
gradients of the eight grid goldens, the properties of the `ABUT` layout, the
margins of every recorded seed, that every gradient is alive, and that the
bound of the GPU test tells three deliberate defects from a correct step."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import grid_data  # noqa: E402
import test_gpu_grid_train  # noqa: E402  (its GOLDENS; nothing there runs)
import train_data  # noqa: E402
import word_rate_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import runtime, train  # noqa: E402
from emphases_amd.train import core as train_core  # noqa: E402

GOLDENS = test_gpu_grid_train.GOLDENS


###############################################################################
# Anchor
###############################################################################


@pytest.mark.parametrize('name', list(GOLDENS))
def test_the_restatement_reproduces_the_reference(name):
    """The stored gradients are float64 rounded to float32 (6e-8 of a value);
    2e-7 of max |want| leaves room for that and nothing else."""
    with np.load(os.path.join(train_data.GOLDEN, f'{name}.npz')) as file:
        golden = {key: file[key] for key in file.files}
    config = emphases_amd.Config(layers=2, **GOLDENS[name])
    seed = int(golden['seed'])
    step = int(golden['step']) if 'step' in golden else 0
    if 'p' in golden:
        assert float(golden['p']) == config.dropout
    found = grid_data.restatement(
        config, train.initial_state(config, seed),
        train_data.collated('ragged'), seed, step)
    want_loss = float(golden['loss'])
    print(f'{name}: loss {found.loss:.17g}, reference {want_loss:.17g}')
    assert abs(found.loss - want_loss) <= 1e-12 * abs(want_loss)
    wanted = {key[len('grad/'):]: value.astype(np.float64)
              for key, value in golden.items() if key.startswith('grad/')}
    assert wanted and set(wanted) <= set(found.gradients)
    if name != 'grid_c128_k7':
        assert set(wanted) == set(found.gradients)
    worst = 0.
    for key, want in wanted.items():
        got = found.gradients[key].numpy()
        assert got.shape == want.shape
        worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print(f'{name}: worst gradient error {worst:.3g}')
    assert worst <= 2e-7


###############################################################################
# ABUT
###############################################################################


def test_the_abut_layout_has_the_properties_the_tests_rely_on():
    plan = word_rate_data.plan_of(grid_data.ABUT)
    other = word_rate_data.plan_of(grid_data.ABUT_REVERSED)
    assert list(plan.frames) == [64, 128, 16, 1, 48, 192]
    assert list(plan.words) == [33, 64, 1, 1, 16, 65]
    # frame segments with no padding column between them
    frame_segment = np.full(plan.ld_frames, -1)
    for index, (off, count) in enumerate(zip(plan.frame_off, plan.frames)):
        assert (frame_segment[off:off + count] == -1).all()
        frame_segment[off:off + count] = index

    def abutting(segment):
        return [(int(segment[c]), int(segment[c + 1]))
                for c in range(len(segment) - 1)
                if segment[c] >= 0 and segment[c + 1] >= 0 and
                segment[c] != segment[c + 1]]
    assert abutting(frame_segment) == [(0, 1), (1, 2), (2, 3), (4, 5)]
    # word segments likewise: after the 64- and the 16-word utterance
    words = abutting(plan.word_segment)
    assert len(words) >= 2, words
    assert [int(plan.words[i]) for i in range(5)
            if plan.word_off[i] + plan.words[i] == plan.word_off[i + 1]] == \
        [64, 16]
    # one word past the 32-wide conv tile and the 64-wide gradient tile: a
    # second tile of one column
    for count, tile in ((33, train_core.WORD_TILE), (65, train_core.GRAD_TILE)):
        assert count == tile + 1 and count in list(plan.words)
    assert train_core.WORD_TILE == 32 and train_core.GRAD_TILE == 64
    assert (plan.frames == 1).any()
    assert ((plan.words == 1) & (plan.frames > 1)).any()
    # every worded utterance is tiled by its words
    for utterance in grid_data.ABUT:
        assert utterance.bounds[0, 0] == 0
        assert utterance.bounds[1, -1] == utterance.frames
        assert (utterance.bounds[0, 1:] == utterance.bounds[1, :-1]).all()
        assert (utterance.bounds[1] > utterance.bounds[0]).all()
    assert plan.total_words == 180 and plan.total_frames == 449
    # the reverse: the same buffers, other offsets
    assert plan.ld_frames == other.ld_frames
    assert plan.ld_words == other.ld_words
    for axis, tile in ((runtime.AXIS_FRAMES, 64), (runtime.AXIS_WORDS, 32),
                       (runtime.AXIS_WORDS, 64)):
        assert len(plan.tiles(axis, tile)) == len(other.tiles(axis, tile))
    assert not np.array_equal(plan.word_off, other.word_off)
    assert not np.array_equal(plan.frame_off, other.frame_off)


def test_every_case_is_one_the_grid_step_accepts_and_no_other():
    for case in grid_data.CASES:
        config = grid_data.config_of(case)
        assert train_core.refusal('GridTrainer', config) is None, case
        assert train_core.refusal('Trainer', config) is not None, case
        assert train_core.step_class(config, 'f32') is train.GridTrainer
    assert set(grid_data.PAIRS) == \
        {(case, 'hard') for case in 'ABCDEF'} | \
        {(case, 'abut') for case in 'BDF'}
    assert grid_data.STEP == 3


###############################################################################
# Margins and liveness
###############################################################################


@pytest.mark.parametrize('case,layout', grid_data.PAIRS)
def test_the_recorded_seed_is_the_first_that_meets_both_margins(case, layout):
    """1e-6 of the layer's largest value is ten times what a float32 dot
    product of a few hundred terms is off by; see `word_rate_data`."""
    recorded = grid_data.SEEDS[case, layout]
    for seed in range(recorded):
        kink, gap = grid_data.margins(case, layout, seed)
        assert min(kink, gap) < grid_data.MARGIN, seed
    kink, gap = grid_data.margins(case, layout, recorded)
    print(f'{case} {layout} seed {recorded}: kink margin {kink:.3g}, '
          f'max gap {gap:.3g}')
    assert kink >= grid_data.MARGIN and gap >= grid_data.MARGIN
    config = grid_data.config_of(case)
    assert np.isfinite(kink) == (config.activation in grid_data.KINKED and
                                 config.layers > 0)
    assert np.isfinite(gap) == (config.downsample_method == 'max')


@pytest.mark.parametrize('case,layout', grid_data.PAIRS)
def test_every_gradient_is_alive(case, layout):
    config, _, state, want, ref32 = grid_data.reference(case, layout)
    assert np.isfinite(want.loss) and want.loss > 0
    assert set(want.gradients) == set(state)
    for name, value in want.gradients.items():
        assert value.shape == state[name].shape
        assert bool(value.isfinite().all()) and bool(value.any()), name
    print(f'{case} {layout}: loss {want.loss:.9g}, ref32 {ref32:.3g}')
    # float32 against float64 with no flipped kink and no moved argmax
    assert 0 < ref32 < 1e-5


###############################################################################
# The bound discriminates
###############################################################################

# (defect, case, layout): what the GPU test must not let pass
DEFECTS = [
    # (a) the encoder runs utterances 0 -> 1 -> 2 of ABUT as one sequence
    ('halo', 'B', 'abut'), ('halo', 'F', 'abut'),
    # (b) the masks of the next step
    ('step', 'D', 'hard'), ('step', 'D', 'abut'),
    # (c) `center` at (n - 1) // 2
    ('center', 'B', 'hard'), ('center', 'B', 'abut'),
]


@pytest.mark.parametrize('defect,case,layout', DEFECTS)
def test_the_bound_tells_a_defect_from_a_correct_step(defect, case, layout):
    _, seed, _, want, ref32 = grid_data.reference(case, layout)
    bound = 4. * ref32
    if defect == 'step':
        broken = grid_data.exact(case, layout, seed, grid_data.STEP + 1)
    else:
        broken = grid_data.exact(
            case, layout, seed, grid_data.STEP,
            {'halo': grid_data.HALO, 'center': grid_data.CENTER}[defect])
    error = grid_data.worst_error(broken.gradients, want.gradients)
    loss_error = abs(broken.loss - want.loss) / abs(want.loss)
    print(f'{defect} {case} {layout}: worst gradient error {error:.3g} '
          f'({error / bound:.3g} of the bound {bound:.3g}), loss error '
          f'{loss_error:.3g}')
    assert error >= 10. * bound
