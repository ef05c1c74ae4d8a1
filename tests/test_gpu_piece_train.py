"""`train.PieceTrainer` on the MI355X: the step at DOWNSAMPLE_LOCATION =
'input' against the reference's goldens (tests/golden/input_*.npz) and, on
hard layouts, against the float64 restatement of tests/input_reference.py;
`emph_piece_pool_backward` alone against numpy; determinism, the engine's
logits, `precision='bf16x3'`, and the loop end to end.

Every bound is 4 x the float32 error of the float64 computation it is
compared with (`ref32_error` of a golden; the restatement's own float32 run
elsewhere), plus, at 'bf16x3', what the three-product arithmetic costs with
exact accumulation (tests/split_emulation.py).  Each figure is printed before
it is asserted.
"""
import dataclasses
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import input_reference  # noqa: E402
import loop_data  # noqa: E402
import piece_layouts  # noqa: E402
import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import engine as engine_module  # noqa: E402
from emphases_amd import runtime, synth, train  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, 'golden')
VARIANTS = {
    'sum': ('sum', 'bce'), 'average': ('average', 'bce'),
    'max': ('max', 'bce'), 'center': ('center', 'bce'),
    'average_mse': ('average', 'mse')}
INPUT = emphases_amd.Config(downsample_location='input', layers=2)


def bits(tensor):
    return tensor.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def golden(variant):
    with np.load(os.path.join(GOLDEN, f'input_{variant}.npz')) as archive:
        return {name: archive[name] for name in archive.files}


def config_of(variant):
    method, loss = VARIANTS[variant]
    return dataclasses.replace(INPUT, downsample_method=method, loss=loss)


def report(what, loss, want_loss, gradients, wanted, bound):
    """Print every ratio, then return what missed the bound."""
    loss_error = abs(float(loss) - want_loss) / abs(want_loss)
    print(f'{what}: loss {float(loss):.9g} (reference {want_loss:.9g}), '
          f'error {loss_error:.3g}, bound {bound:.3g}')
    assert set(wanted) == set(gradients)
    missed = {} if loss_error <= bound else {'loss': loss_error}
    for name, want in wanted.items():
        got = gradients[name].cpu().numpy().astype(np.float64)
        error = np.abs(got - want).max() / np.abs(want).max()
        print(f'{what}: {name} error {error:.3g} '
              f'({error / bound:.2f} of the bound)')
        if not error <= bound:
            missed[name] = error
    return missed


###############################################################################
# Against the reference
###############################################################################


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_gradients_match_the_reference(variant):
    data = golden(variant)
    bound = 4. * float(data['ref32_error'])
    model = train.PieceTrainer(
        config_of(variant), gpu=0, seed=int(data['seed']))
    loss, gradients = model.loss_and_gradients(
        *train_data.collated('ragged'))
    wanted = {name[5:]: value.astype(np.float64)
              for name, value in data.items() if name.startswith('grad/')}
    missed = report(f'input_{variant}', loss, float(data['loss']), gradients,
                    wanted, bound)
    assert not missed, (missed, bound)


###############################################################################
# Hard layouts against the float64 restatement
###############################################################################


@functools.lru_cache(maxsize=None)
def oracle(layout, method, loss='bce'):
    """(config, items, float64 step, its float32 error, float32 step) of a
    layout; under 'max' at the first seed of the features at which a float32
    evaluation cannot choose another column than float64: no two candidates
    of a piece closer than 8 x the float32 error of the restatement's own
    embeddings there (`input_reference.no_reachable_ties`; with 360 pieces
    some pair always lies within the generator's fixed 1e-4)."""
    config = dataclasses.replace(INPUT, downsample_method=method, loss=loss)
    state = train.initial_state(config, 0)
    for seed in range(20):
        items = piece_layouts.items_of(piece_layouts.layouts()[layout], seed)
        seen = {torch.float64: [], torch.float32: []}
        steps = {
            dtype: input_reference.step(
                state, items, config.layers, method, loss, dtype=dtype,
                watch=lambda x, bounds, layers, kept=kept: kept.append(x))
            for dtype, kept in seen.items()}
        try:
            if method == 'max':
                for wide, narrow, item in zip(
                        seen[torch.float64], seen[torch.float32], items):
                    input_reference.no_reachable_ties(
                        wide, narrow, item[1], config.layers)
            break
        except ArithmeticError:
            print(f'{layout} {method}: seed {seed} has a tie within reach; '
                  'next')
    else:
        raise ArithmeticError(f'{layout} {method}: every seed has such a tie')
    exact, narrow = steps[torch.float64], steps[torch.float32]
    error = input_reference.worst_error(narrow[1], exact[1])
    return config, items, exact, error, narrow


@pytest.mark.parametrize('layout,method', piece_layouts.cases())
def test_hard_layouts_match_the_restatement(layout, method):
    config, items, exact, error, _ = oracle(layout, method)
    bound = 4. * error
    model = train.PieceTrainer(config, gpu=0, seed=0)
    batch = model.prepare(*input_reference.collate(items))
    pieces = batch.meta['pieces']['plan']
    print(f'{layout} {method}: {len(pieces)} pieces on {pieces.ld_frames} '
          f'columns, float32 error of the restatement {error:.3g}')
    loss, gradients = model.loss_and_gradients(batch)
    missed = report(f'{layout} {method}', loss, exact[0], gradients, exact[1],
                    bound)
    assert not missed, (missed, bound)
    if layout == 'many_words':
        tiles = len(pieces.tiles(runtime.AXIS_FRAMES, 64))
        assert runtime.library().emph_conv_weight_grad_parts(tiles) > 1


###############################################################################
# emph_piece_pool_backward alone
###############################################################################


def pool_backward_numpy(pieces, dword, x, y, method):
    """{piece: dx [C, L]} by the header's table."""
    out = {}
    for piece, (_, length, first, padded) in enumerate(pieces.gather):
        g = dword[:, pieces.piece_column[piece]]
        dx = np.zeros((dword.shape[0], padded), dtype=np.float32)
        if method == 'sum':
            dx[:] = g[:, None]
        elif method == 'average':
            dx[:] = (g * (np.float32(1) / np.float32(padded)))[:, None]
        elif method == 'center':
            dx[:, length // 2] = g
        else:
            values = x[:, first:first + padded]
            top = y[:, pieces.piece_column[piece]]
            hit = values == top[:, None]
            chosen = hit.argmax(axis=1)
            rows = np.nonzero(hit.any(axis=1))[0]
            dx[rows, chosen[rows]] = g[rows]
        out[piece] = dx
    return out


@pytest.mark.parametrize('method', piece_layouts.METHODS)
@pytest.mark.parametrize('layout', list(piece_layouts.layouts()))
def test_piece_pool_backward_alone(layout, method):
    lib = runtime.library()
    plan = piece_layouts.plan_of(piece_layouts.layouts()[layout])
    pieces = plan.pieces(method)
    ld_p, ld_w, channels = pieces.plan.ld_frames, plan.ld_words, 80
    rng = np.random.default_rng(7)
    # few distinct values: ties inside a piece on every channel, across tiles
    # for the pieces longer than 64 columns
    x = rng.integers(0, 4, (channels, ld_p)).astype(np.float32)
    dword = rng.standard_normal((channels, ld_w)).astype(np.float32)
    y = np.full((channels, ld_w), np.float32('nan'))
    for piece, (_, _, first, padded) in enumerate(pieces.gather):
        y[:, pieces.piece_column[piece]] = \
            x[:, first:first + padded].max(axis=1)
    tiles = pieces.plan.tiles(runtime.AXIS_FRAMES, 64)
    device = lambda array: torch.from_numpy(array).cuda()  # noqa: E731
    tables = [device(pieces.gather), device(pieces.piece_column),
              device(tiles)]
    x_device, y_device, dword_device = device(x), device(y), device(dword)
    poison = np.float32(-123456.75)
    results = []
    for launch in range(2):
        dx = torch.full((channels, ld_p), float(poison), device='cuda:0')
        runtime.check(lib.emph_piece_pool_backward(
            dword_device.data_ptr(), ld_w, tables[0].data_ptr(),
            tables[1].data_ptr(), len(pieces.plan), x_device.data_ptr(), ld_p,
            y_device.data_ptr(), dx.data_ptr(), ld_p, channels,
            tables[2].data_ptr(), len(tiles),
            runtime.REDUCTIONS[method], runtime.stream()),
            'emph_piece_pool_backward')
        results.append(dx)
    assert same(results[0], results[1])
    got = results[0].cpu().numpy()
    written = np.zeros(ld_p, dtype=bool)
    wanted = pool_backward_numpy(pieces, dword, x, y, method)
    for piece, (_, _, first, padded) in enumerate(pieces.gather):
        written[first:first + padded] = True
        assert np.array_equal(
            got[:, first:first + padded].view(np.int32),
            wanted[piece].view(np.int32)), (layout, method, piece)
    # the alignment gaps (and lead and tail) are untouched
    assert (got[:, ~written] == poison).all()
    assert written.sum() == pieces.plan.total_frames
    if method == 'max':
        # one column per (piece, channel) took the gradient, ties or not
        for piece, (_, _, first, padded) in enumerate(pieces.gather):
            taken = got[:, first:first + padded] != 0
            assert (taken.sum(axis=1) <= 1).all()


###############################################################################
# Determinism and parity
###############################################################################


def _one_utterance(words, seed):
    lengths = np.array(words, dtype=np.int64)
    ends = np.cumsum(lengths)
    layout = [(int(ends[-1]), np.stack([ends - lengths, ends]))]
    return input_reference.collate(piece_layouts.items_of(layout, seed))


def test_same_batch_twice_is_bitwise_the_same():
    """Also behind another batch whose buffers have the SAME widths and
    another piece layout - the workspace is kept then, and the alignment gaps
    of the piece layout, which no kernel writes, hold the other batch's
    columns - and behind finite garbage in every frame-rate buffer."""
    for method in ('sum', 'max'):
        model = train.PieceTrainer(
            dataclasses.replace(INPUT, downsample_method=method), gpu=0)
        # pieces of 5 columns and pieces of 4: two pieces of 16 aligned
        # columns either way, where [5, 16) or [4, 16) is the gap
        batch = model.prepare(*_one_utterance([5, 3], 0))
        other = model.prepare(*_one_utterance([2, 4], 1))
        plans = [b.meta['pieces']['plan'] for b in (batch, other)]
        assert plans[0].ld_frames == plans[1].ld_frames
        assert batch.plan.ld_words == other.plan.ld_words
        assert list(plans[0].frames) == [5, 5] and \
            list(plans[1].frames) == [4, 4]
        first_loss, first = model.loss_and_gradients(batch)
        workspace = model._buffers(batch.plan)
        other_loss, other_first = model.loss_and_gradients(other)
        assert model._buffers(other.plan) is workspace      # kept, not rebuilt
        second_loss, second = model.loss_and_gradients(batch)
        generator = torch.Generator(device='cuda:0').manual_seed(5)
        for name in ('piece_features', 'frames', 'frame_grad'):
            workspace[name].normal_(generator=generator).mul_(1e3)
        third_loss, third = model.loss_and_gradients(batch)
        assert model._buffers(batch.plan) is workspace
        fresh = train.PieceTrainer(model.config, gpu=0)
        fresh_loss, fresh_other = fresh.loss_and_gradients(other)
        assert same(first_loss, second_loss) and same(first_loss, third_loss)
        assert same(other_loss, fresh_loss)
        for name in first:
            assert same(first[name], second[name]), (method, name)
            assert same(first[name], third[name]), (method, name)
            assert same(other_first[name], fresh_other[name]), (method, name)
        assert float(first['input_layer.weight'].abs().max()) > 0
        # and the ragged batch behind a batch of other widths
        ragged = train_data.collated('ragged')
        ragged_loss, ragged_first = model.loss_and_gradients(*ragged)
        model.loss_and_gradients(batch)
        again_loss, again = model.loss_and_gradients(*ragged)
        assert same(ragged_loss, again_loss)
        for name in ragged_first:
            assert same(ragged_first[name], again[name]), (method, name)


@pytest.mark.parametrize('method', piece_layouts.METHODS)
def test_eval_logits_agree_with_the_engine(method):
    """The engine runs Winograd kernels: two float32 evaluations of one
    function, each within the restatement's own float32 error of float64."""
    config = dataclasses.replace(INPUT, downsample_method=method)
    items = input_reference.ragged_items()
    state = train.initial_state(config, 0)
    exact = input_reference.logits_of(
        {k: torch.from_numpy(v).double() for k, v in state.items()},
        [(torch.from_numpy(f).double(), b, t) for f, b, t in items],
        config.layers, method).numpy()
    narrow = input_reference.logits_of(
        {k: torch.from_numpy(v) for k, v in state.items()},
        [(torch.from_numpy(f), b, t) for f, b, t in items],
        config.layers, method).double().numpy()
    scale = np.abs(exact).max()
    bound = 4. * float(np.abs(narrow - exact).max() / scale)
    model = train.PieceTrainer(config, gpu=0, seed=0)
    batch = train_data.collated('ragged')
    logits = model.logits(model.prepare(*batch)).cpu().double().numpy()
    features, frame_lengths, word_bounds, word_lengths, _ = batch
    engine = emphases_amd.Model(gpu=0, config=config)
    engine.engine = engine_module.Engine(config, model.state_dict(), 0)
    padded = engine(features.cuda(), frame_lengths, word_bounds, word_lengths)
    from_engine = torch.cat([
        padded[i, 0, :int(n)] for i, n in enumerate(word_lengths)]
    ).cpu().double().numpy()
    errors = {
        'trainer against float64': np.abs(logits - exact).max() / scale,
        'engine against float64': np.abs(from_engine - exact).max() / scale,
        'trainer against engine': np.abs(logits - from_engine).max() / scale}
    for what, error in errors.items():
        print(f'{method}: {what} {error:.3g}, bound {bound:.3g}')
    assert errors['trainer against float64'] <= bound
    assert errors['trainer against engine'] <= bound


SPLIT_LAYOUTS = {
    'gaps': piece_layouts.layouts()['gaps'],
    'tile_edge': piece_layouts.layouts()['tile_edge'],
    # pieces of 300 columns: more than one span of `emph_conv1d_split`
    'two_spans': [(305, np.array([[0, 300], [300, 305]], dtype=np.int64))]}
# three k = 3 layers of three-product arithmetic: every product drops the
# low x low term, 2^-16 of it; ten of those is far above what they add up to
# and far below what one flipped ReLU costs (per cent)
ARITHMETIC_GRADE = 10 * 2. ** -16


@functools.lru_cache(maxsize=None)
def split_oracle(layout, method):
    """(config, items, float64 step, emulated error, float32 error) of a
    layout at the first seed of its features at which the comparison measures
    the ARITHMETIC of 'bf16x3': no ReLU of the frame encoder within reach
    (8 x the emulation's, and the float32 run's, own distance from float64)
    of changing its mask, and under 'max' no second candidate within reach of
    the maximum (`input_reference.unreachable_masks`, `no_reachable_ties`).
    One flipped mask moves a weight gradient of such a batch by per cent and
    would be all that the bound then holds."""
    config = dataclasses.replace(INPUT, downsample_method=method)
    state = train.initial_state(config, 0)
    for seed in range(20):
        items = piece_layouts.items_of(SPLIT_LAYOUTS[layout], seed)
        runs = {}
        for name, arguments in (('exact', {}), ('split', {'split': True}),
                                ('narrow', {'dtype': torch.float32})):
            seen, pre = [], []
            runs[name] = (input_reference.step(
                state, items, config.layers, method, config.loss,
                watch=lambda x, bounds, layers, kept=seen: kept.append(x),
                probe=pre, **arguments), seen, pre)
        try:
            for rough in ('split', 'narrow'):
                if not input_reference.unreachable_masks(
                        runs['exact'][2], runs[rough][2]):
                    raise ArithmeticError('a ReLU within reach of zero')
                if method == 'max':
                    for wide, other, item in zip(
                            runs['exact'][1], runs[rough][1], items):
                        input_reference.no_reachable_ties(
                            wide, other, item[1], config.layers)
            break
        except ArithmeticError as error:
            print(f'{layout} {method}: seed {seed}: {error}; next')
    else:
        raise ArithmeticError(f'{layout} {method}: no seed is out of reach')
    exact = runs['exact'][0]
    return (config, items, exact,
            input_reference.worst_error(runs['split'][0][1], exact[1]),
            input_reference.worst_error(runs['narrow'][0][1], exact[1]))


@pytest.mark.parametrize('method', ['sum', 'max'])
@pytest.mark.parametrize('layout', list(SPLIT_LAYOUTS))
def test_bf16x3_matches_the_restatement(layout, method):
    """4 x (emulated error + float32 error) where both are what the
    arithmetic costs, some 1e-5: a defect of a span table at a piece's edge
    or of a split pack is orders of magnitude above it."""
    config, items, exact, emulated_error, narrow_error = \
        split_oracle(layout, method)
    bound = 4. * (emulated_error + narrow_error)
    print(f'{layout} {method} bf16x3: emulated error {emulated_error:.3g}, '
          f'float32 error {narrow_error:.3g}, bound {bound:.3g}')
    assert 0 < emulated_error < ARITHMETIC_GRADE
    model = train.PieceTrainer(config, gpu=0, seed=0, precision='bf16x3')
    batch = model.prepare(*input_reference.collate(items))
    spans = batch.meta['pieces']['conv_spans'].numel() // 8
    print(f'{layout} {method} bf16x3: {len(batch.meta["pieces"]["plan"])} '
          f'pieces, {spans} spans')
    if layout == 'two_spans':
        assert spans > len(batch.meta['pieces']['plan'])
    loss, gradients = model.loss_and_gradients(batch)
    missed = report(f'{layout} {method} bf16x3', loss, exact[0], gradients,
                    exact[1], bound)
    assert not missed, (missed, bound)
    # the split path ran: not the f32 trainer's bits
    _, f32 = train.PieceTrainer(config, gpu=0, seed=0).loss_and_gradients(
        *input_reference.collate(items))
    assert not same(gradients['frame_encoder.0.weight'],
                    f32['frame_encoder.0.weight'])


@pytest.mark.parametrize('variant', ['sum', 'max'])
def test_bf16x3_on_the_reference_batch(variant):
    """`ragged` against the reference's golden under the bound of
    tests/test_gpu_train_precision.py, 4 x (emulated error + ref32_error).
    On this batch that bound holds LITTLE and is kept for the record only:
    with 283 000 ReLUs in the frame encoder every seed has one within reach
    of the split arithmetic, the emulation flips one at either golden's seed
    (frame_encoder.0, a pre-activation of -1e-6), and that one column moves
    frame_encoder.0.weight by 2.3 % ('sum') and 2.7 % ('max'): the emulated
    error is the flip, not the arithmetic, and the bound is some 10 %.  What
    the arithmetic costs is held by `test_bf16x3_matches_the_restatement`."""
    data = golden(variant)
    config = config_of(variant)
    seed = int(data['seed'])
    state = train.initial_state(config, seed)
    items = input_reference.ragged_items()
    pre = {False: [], True: []}
    steps = {split: input_reference.step(
        state, items, config.layers, config.downsample_method, config.loss,
        split=split, probe=pre[split]) for split in pre}
    flips = sum(int(((a > 0) != (b > 0)).sum())
                for a, b in zip(pre[False], pre[True]))
    emulated_error = input_reference.worst_error(steps[True][1], steps[False][1])
    bound = 4. * (emulated_error + float(data['ref32_error']))
    print(f'input_{variant} bf16x3: emulated error {emulated_error:.3g} with '
          f'{flips} flipped ReLU(s) in the emulation, ref32_error '
          f"{float(data['ref32_error']):.3g}, bound {bound:.3g}")
    assert emulated_error > 0
    model = train.PieceTrainer(config, gpu=0, seed=seed, precision='bf16x3')
    batch = model.prepare(*train_data.collated('ragged'))
    assert 'conv_spans' in batch.meta['pieces']
    loss, gradients = model.loss_and_gradients(batch)
    wanted = {name[5:]: value.astype(np.float64)
              for name, value in data.items() if name.startswith('grad/')}
    missed = report(f'input_{variant} bf16x3', loss, float(data['loss']),
                    gradients, wanted, bound)
    assert not missed, (missed, bound)
    # the split path ran: not the f32 trainer's bits; and an f32 batch, which
    # carries no span table, is refused by name
    plain = train.PieceTrainer(config, gpu=0, seed=seed)
    _, f32 = plain.loss_and_gradients(*train_data.collated('ragged'))
    assert not same(gradients['frame_encoder.0.weight'],
                    f32['frame_encoder.0.weight'])
    with pytest.raises(ValueError, match="precision='f32'"):
        model.loss_and_gradients(
            plain.prepare(*train_data.collated('ragged')))
    with pytest.raises(ValueError, match='piece tables'):
        plain.loss_and_gradients(train.Trainer(gpu=0).prepare(
            *train_data.collated('ragged')))


def test_five_adam_steps_lower_the_loss_and_the_checkpoint_loads(tmp_path):
    config = dataclasses.replace(INPUT, downsample_method='max')
    model = train.PieceTrainer(config, gpu=0, seed=1)
    batch = model.prepare(*train_data.collated('ragged'))
    losses = [float(model.step(batch)) for _ in range(5)]
    losses.append(float(model.loss_and_gradients(batch)[0]))
    print('losses', losses)
    assert model.steps == 5 and np.all(np.diff(losses) < 0), losses
    path = tmp_path / '00000005.pt'
    model.save(path)
    saved = torch.load(path, map_location='cpu', weights_only=False)
    assert list(saved['model']) == list(train.checkpoint_names(config).values())
    assert 'word_decoder.2.weight' in saved['model']
    resumed = train.trainer_for(config, checkpoint=str(path), gpu=0, seed=1)
    assert isinstance(resumed, train.PieceTrainer) and resumed.steps == 5
    assert same(resumed.parameters, model.parameters)
    assert same(resumed.exp_avg_sq, model.exp_avg_sq)
    assert same(resumed.step(batch), model.step(batch))
    assert same(resumed.parameters, model.parameters)


###############################################################################
# End to end
###############################################################################


def test_loop_at_input_resumes_bitwise_and_the_checkpoint_scores(tmp_path):
    partition_dir, cache_dir = loop_data.build_cache(str(tmp_path / 'cache'))
    config = INPUT

    def run(directory, num_steps):
        return train.train(
            loop_data.DATASET, directory, 0, partition_dir=partition_dir,
            cache_dir=cache_dir, config=config, num_steps=num_steps,
            log_interval=4, save_after=100)
    whole = run(tmp_path / 'whole', 8)
    assert whole == str(tmp_path / 'whole' / '00000008.pt')
    with open(tmp_path / 'whole' / 'scalars.jsonl') as file:
        scalars = [json.loads(line) for line in file]
    assert [line['step'] for line in scalars] == [0, 4]
    for line in scalars:
        assert all(np.isfinite(value) for value in line.values())
    load = lambda path: torch.load(  # noqa: E731
        path, map_location='cpu', weights_only=False)
    stopped = run(tmp_path / 'parts', 4)
    assert stopped == str(tmp_path / 'parts' / '00000004.pt')
    # (two batches an epoch: the file stops on an epoch's edge, where a
    # resumed run, which restarts the file's epoch, is the run itself)
    assert load(stopped)['epoch'] == 2
    resumed = run(tmp_path / 'parts', 8)
    first, second = load(whole), load(resumed)
    assert first['step'] == second['step'] == 8
    assert list(first['model']) == list(second['model'])
    for name, value in first['model'].items():
        assert same(value, second['model'][name]), name
    for index, entry in first['optimizer']['state'].items():
        for moment in ('exp_avg', 'exp_avg_sq'):
            assert same(entry[moment],
                        second['optimizer']['state'][index][moment])
    audio = torch.from_numpy(synth.audio(3, 211))
    alignment = emphases_amd.Alignment.from_frames(
        synth.word_frames(3, 211, 3, 40))
    before = emphases_amd.core.active_config()
    try:
        emphases_amd.configure(config)
        scores = emphases_amd.from_alignment_and_audio(
            alignment, audio, emphases_amd.SAMPLE_RATE, checkpoint=whole,
            gpu=0)
    finally:
        emphases_amd.configure(before)
    assert scores.shape[-1] == len(alignment)
    assert torch.isfinite(scores).all()
