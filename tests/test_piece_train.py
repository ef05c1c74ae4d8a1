"""Training at DOWNSAMPLE_LOCATION = 'input' without a GPU: the array piece
builder against its per-word restatement, the float64 restatement of the step
against the reference's goldens, the dispatcher and its refusals, `--config`,
and the contract of `emph_piece_pool_backward`."""
import dataclasses
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import input_reference  # noqa: E402
import piece_layouts  # noqa: E402
import pieces_reference  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import batch, runtime, train  # noqa: E402
from emphases_amd.train import __main__ as cli  # noqa: E402
from emphases_amd.train import core as train_core  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden')
VARIANTS = {
    'sum': ('sum', 'bce'), 'average': ('average', 'bce'),
    'max': ('max', 'bce'), 'center': ('center', 'bce'),
    'average_mse': ('average', 'mse')}
INPUT = emphases_amd.Config(downsample_location='input', layers=2)


###############################################################################
# The piece builder
###############################################################################


def random_plan(seed):
    """1..8 utterances, 0..30 words each (one word may be empty, words may
    leave gaps, an utterance may have no word at all)."""
    rng = np.random.default_rng(seed)
    layout = []
    for _ in range(int(rng.integers(1, 9))):
        count = int(rng.integers(0, 31))
        lengths = rng.integers(1, 40, count)
        if count > 1 and rng.random() < .3:
            lengths[rng.integers(0, count)] = 0
        gaps = rng.integers(0, 4, count + 1) * (rng.random() < .5)
        starts = np.cumsum(gaps[:-1] + np.concatenate([[0], lengths[:-1]]))
        bounds = np.stack([starts, starts + lengths]).astype(np.int64)
        frames = int(max((starts + lengths).max() if count else 0, 0)
                     + gaps[-1] + 1)
        layout.append((frames, bounds.reshape(2, count)))
    if not any(b.shape[1] for _, b in layout):
        layout.append((3, np.array([[0], [3]], dtype=np.int64)))
    return piece_layouts.plan_of(layout)


@pytest.mark.parametrize('method', piece_layouts.METHODS)
def test_array_builder_equals_the_per_word_builder(method):
    plans = [random_plan(seed) for seed in range(200)]
    plans += [piece_layouts.plan_of(layout)
              for layout in piece_layouts.layouts().values()]
    for plan in plans:
        pieces_reference.assert_same(
            batch.Pieces(plan, method), pieces_reference.Pieces(plan, method))
    pieces = plans[-1].pieces(method)
    assert pieces is plans[-1].pieces(method)               # cached per method
    columns = plans[-1].word_columns()
    assert pieces.piece_column.dtype == np.int32
    assert np.array_equal(pieces.piece_column, columns)
    assert np.array_equal(
        pieces.word_piece[columns], np.arange(len(columns)))


def test_builder_of_a_columns_plan_and_of_no_word():
    plan = piece_layouts.plan_of(piece_layouts.layouts()['gaps'])
    columns = batch.Plan.from_columns(
        plan.utterance, plan.start_word, np.zeros(2, dtype=np.int64),
        np.zeros(2, dtype=np.int64), plan.frames, plan.words,
        plan.segment_bounds, [0, 0], [0, 0])
    pieces_reference.assert_same(
        batch.Pieces(columns, 'max'), pieces_reference.Pieces(plan, 'max'))
    empty = piece_layouts.plan_of([(7, np.zeros((2, 0), dtype=np.int64))])
    pieces_reference.assert_same(
        batch.Pieces(empty, 'sum'), pieces_reference.Pieces(empty, 'sum'))
    assert len(batch.Pieces(empty, 'sum').plan) == 0


@pytest.mark.parametrize('layout,message', [
    ([(10, np.array([[0, 4], [4, 11]]))], 'outside the chunk'),
    ([(10, np.array([[-1, 4], [4, 9]]))], 'outside the chunk'),
    ([(10, np.array([[0, 6], [4, 5]]))], 'outside the chunk'),
    ([(10, np.array([[2, 4], [2, 4]]))], 'no word of the chunk covers'),
    # the first refused chunk speaks, by its first reason
    ([(5, np.array([[0], [5]])), (10, np.array([[3], [3]])),
      (10, np.array([[0], [11]]))], 'no word of the chunk covers'),
    ([(5, np.array([[0], [5]])), (10, np.array([[3, 3], [3, 12]]))],
     'outside the chunk'),
])
def test_builder_refusals_are_the_same(layout, message):
    plan = piece_layouts.plan_of(
        [(f, b.astype(np.int64)) for f, b in layout])
    raised = []
    for builder in (batch.Pieces, pieces_reference.Pieces):
        with pytest.raises(ValueError, match=message) as info:
            builder(plan, 'sum')
        raised.append(str(info.value))
    assert raised[0] == raised[1]


###############################################################################
# The float64 restatement against the reference
###############################################################################


def golden(variant):
    with np.load(os.path.join(GOLDEN, f'input_{variant}.npz')) as archive:
        return {name: archive[name] for name in archive.files}


def golden_state(variant):
    """The reference's initialisation under the golden's seed, checked
    against the sums the golden recorded."""
    data = golden(variant)
    method, loss = VARIANTS[variant]
    config = dataclasses.replace(
        INPUT, downsample_method=method, loss=loss)
    state = train.initial_state(config, int(data['seed']))
    for name, value in state.items():
        want = data[f'init/{name}']
        wide = value.astype(np.float64)
        assert np.allclose([wide.sum(), (wide ** 2).sum()], want,
                           rtol=1e-12, atol=1e-12), name
    return config, state, data


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_restatement_reproduces_the_reference(variant):
    config, state, data = golden_state(variant)
    assert 0 < float(data['ref32_error']) < 1e-5
    loss, gradients, _ = input_reference.step(
        state, input_reference.ragged_items(), config.layers,
        config.downsample_method, config.loss)
    assert abs(loss - float(data['loss'])) <= 1e-12 * abs(float(data['loss']))
    names = [name[5:] for name in data if name.startswith('grad/')]
    assert sorted(names) == sorted(gradients)
    for name in names:
        want = data[f'grad/{name}'].astype(np.float64)     # float32 roundings
        got = gradients[name]
        assert np.abs(want).max() > 0
        # a float32 holds a float64 to 2^-24 relative (2^-23: headroom of
        # one unit for the float64 noise of two different orders of addition)
        allowed = 2. ** -23 * np.abs(got) + 1e-12 * np.abs(got).max()
        assert (np.abs(got - want) <= allowed).all(), name


###############################################################################
# Dispatch and refusals
###############################################################################


def test_trainer_for_dispatches_before_a_gpu_is_needed(monkeypatch):
    built = []
    for name in ('Trainer', 'EncoderTrainer', 'PieceTrainer'):
        monkeypatch.setattr(
            train_core, name,
            lambda config, _name=name, **arguments: built.append(
                (_name, config, arguments)) or _name)
    wanted = {'intermediate': 'Trainer', 'inference': 'EncoderTrainer',
              'loss': 'EncoderTrainer', 'input': 'PieceTrainer'}
    for location, name in wanted.items():
        config = emphases_amd.Config(downsample_location=location)
        assert train.trainer_for(config, precision='bf16x3', seed=3) == name
        assert built[-1] == (name, config,
                             {'precision': 'bf16x3', 'seed': 3})
    # make_trainer keeps refusing 'input'; so do the two other classes
    with pytest.raises(NotImplementedError, match='downsample_location'):
        train.make_trainer(emphases_amd.Config(downsample_location='input'))
    count = len(built)
    with pytest.raises(NotImplementedError, match='dropout'):
        train.trainer_for(emphases_amd.Config(
            downsample_location='input', dropout=0.1))
    with pytest.raises(NotImplementedError, match='architecture'):
        train.trainer_for(emphases_amd.Config(
            downsample_location='input', architecture='transformer'))
    with pytest.raises(NotImplementedError, match='downsample_method'):
        train.trainer_for(emphases_amd.Config(downsample_method='max'))
    with pytest.raises(NotImplementedError, match='precision'):
        train.trainer_for(emphases_amd.Config(downsample_location='input'),
                          precision='bf16x6')
    assert len(built) == count


@pytest.mark.parametrize('field,value', [
    ('architecture', 'transformer'), ('downsample_location', 'intermediate'),
    ('downsample_location', 'loss'), ('activation', 'gelu'),
    ('channels', 64), ('encoder_kernel_size', 5), ('decoder_kernel_size', 1),
    ('layers', 17), ('mel_feature', False), ('method', 'pitch-variance'),
    ('dropout', 0.), ('dropout', 0.1)])
def test_check_pieces_supported_names_the_field(field, value):
    config = dataclasses.replace(INPUT, **{field: value})
    with pytest.raises(NotImplementedError, match=field):
        train.check_pieces_supported(config)
    with pytest.raises(NotImplementedError, match=field):
        train.PieceTrainer(config=config)
    if field != 'downsample_location':
        with pytest.raises(NotImplementedError, match=field):
            train.train('none', 'none', partition_dir='none', config=config)


def test_check_pieces_supported_passes():
    for overrides in ({}, {'loss': 'mse'}, {'layers': 0}, {'layers': 16},
                      {'loudness_feature': True, 'pitch_feature': True},
                      *({'downsample_method': m}
                        for m in piece_layouts.METHODS)):
        config = dataclasses.replace(INPUT, **overrides)
        train.check_pieces_supported(config)
        state = train.initial_state(config, 0)
        assert list(state) == list(train.parameter_offsets(config)[0])
        assert 'word_decoder.0.weight' in state or config.layers == 0
    assert set(train.gather_tables(INPUT)['forward']) == \
        set(train.layer_names(INPUT))


###############################################################################
# --config
###############################################################################


FLAGS = ['--directory', 'run', '--partition_dir', 'parts']


def test_config_file_is_read(tmp_path):
    path = tmp_path / 'max-input.py'
    path.write_text(
        '"""An experiment."""\n'
        "MODULE = 'emphases'\n\n# Configuration name\nCONFIG = 'max-input'\n"
        "DOWNSAMPLE_LOCATION = 'input'\nDOWNSAMPLE_METHOD = 'max'\n"
        'ACTIVATION_FUNCTION = torch.nn.ReLU\nLAYERS = 4\nDROPOUT = None\n'
        'NUM_STEPS = 120\nMAX_TRAINING_FRAMES = 60000\nLOUDNESS_FEATURE = True\n')
    overrides, arguments = cli.settings(FLAGS + ['--config', str(path)])
    assert overrides == {
        'downsample_location': 'input', 'downsample_method': 'max',
        'activation': 'relu', 'layers': 4, 'dropout': None,
        'loudness_feature': True}
    assert arguments['num_steps'] == 120
    assert arguments['max_training_frames'] == 60000
    assert 'config' not in arguments
    config = emphases_amd.Config(**overrides)
    train.check_pieces_supported(config)
    # explicit flags override the file
    overrides, arguments = cli.settings(FLAGS + [
        '--config', str(path), '--downsample_method', 'sum', '--num_steps',
        '7', '--loss', 'mse'])
    assert overrides['downsample_method'] == 'sum'
    assert overrides['loss'] == 'mse' and overrides['layers'] == 4
    assert arguments['num_steps'] == 7
    assert arguments['max_training_frames'] == 60000
    # without a file: the reference's defaults
    overrides, arguments = cli.settings(FLAGS)
    assert overrides == {}
    assert arguments['num_steps'] == train.loop.NUM_STEPS
    assert arguments['max_training_frames'] == train.loop.MAX_TRAINING_FRAMES


def test_config_file_reaches_train(tmp_path, monkeypatch):
    path = tmp_path / 'sum-input.py'
    path.write_text("DOWNSAMPLE_LOCATION = 'input'\nNUM_STEPS = 3\n")
    calls = []
    monkeypatch.setattr(
        emphases_amd.train, 'train',
        lambda *args, **kwargs: calls.append(
            (args, kwargs, emphases_amd.core.active_config())))
    before = emphases_amd.core.active_config()
    try:
        cli.main(FLAGS + ['--config', str(path)])
    finally:
        emphases_amd.configure(before)
    (args, kwargs, config), = calls
    assert config.downsample_location == 'input'
    assert kwargs['num_steps'] == 3 and 'config' not in kwargs


@pytest.mark.parametrize('text,message', [
    ('BUCKETS = 2\n', 'BUCKETS'),
    ('FROBNICATE = 1\n', 'FROBNICATE'),
    ('layers = 2\n', 'layers'),
    ('LAYERS = 1 + 1\n', 'LAYERS'),
    ('LAYERS = {[]: 1}\n', 'LAYERS'),
    ('LAYERS = ' + '[' * 3000 + ']' * 3000 + '\n', 'bad.py is not'),
    ('LAYERS = (\n', 'bad.py is not'),
    ('ACTIVATION_FUNCTION = torch.nn.Tanh\n', 'ACTIVATION_FUNCTION'),
    ('ACTIVATION_FUNCTION = other.nn.ReLU\n', 'ACTIVATION_FUNCTION'),
    ('import os\n', 'only assignments'),
    ('A, B = 1, 2\n', 'only assignments'),
], ids=lambda value: value[:24].strip() if '=' in value or ' ' in value
    else None)
def test_config_file_errors_name_the_setting(tmp_path, text, message):
    path = tmp_path / 'bad.py'
    path.write_text("DOWNSAMPLE_LOCATION = 'input'\n" + text)
    with pytest.raises(ValueError, match=message):
        cli.read_config(path)


def test_config_file_is_never_executed(tmp_path):
    witness = tmp_path / 'witness'
    path = tmp_path / 'evil.py'
    path.write_text(
        f"LAYERS = open({str(witness)!r}, 'w').write('x')\n")
    with pytest.raises(ValueError, match='LAYERS'):
        cli.read_config(path)
    path.write_text(
        f"import pathlib\npathlib.Path({str(witness)!r}).touch()\n")
    with pytest.raises(ValueError):
        cli.read_config(path)
    path.write_text(
        f"LOSS = 'mse'\n__import__('pathlib').Path({str(witness)!r}).touch()\n")
    with pytest.raises(ValueError):
        cli.read_config(path)
    assert not witness.exists()


###############################################################################
# emph_piece_pool_backward: the contract
###############################################################################


def test_abi_declares_the_piece_pool_backward():
    header = open(os.path.join(
        os.path.dirname(HERE), 'include', 'emphases_hip.h')).read()
    assert 'int emph_piece_pool_backward(' in header
    assert 'emph_piece_pool_backward' in runtime.SIGNATURES
    assert runtime.ABI_VERSION >= 44
    assert runtime.library().emph_abi_version() == runtime.ABI_VERSION


def test_piece_pool_backward_contract_violations_launch_nothing():
    lib = runtime.library()
    one = np.zeros(64, dtype=np.int64).ctypes.data     # any non-null address

    def call(dword=one, pieces=one, column=one, n_pieces=1, x=one, ldx=64,
             y=one, dx=one, ld_dx=64, channels=80, tiles=one, n_tiles=1,
             mode=0, ldw=64):
        return lib.emph_piece_pool_backward(
            dword, ldw, pieces, column, n_pieces, x, ldx, y, dx, ld_dx,
            channels, tiles, n_tiles, mode, None)
    for arguments, message in (
            (dict(dword=None), b'null pointer'),
            (dict(pieces=None), b'null pointer'),
            (dict(column=None), b'null pointer'),
            (dict(dx=None), b'null pointer'),
            (dict(tiles=None), b'null pointer'),
            (dict(mode=4), b'unknown mode 4'),
            (dict(mode=-1), b'unknown mode -1'),
            (dict(mode=2, x=None), b'max needs'),
            (dict(mode=2, y=None), b'max needs'),
            (dict(channels=0), b'bad shape'),
            (dict(ldw=0), b'bad shape'),
            (dict(ld_dx=0), b'bad shape'),
            (dict(mode=2, ldx=0), b'bad shape'),
            (dict(n_tiles=0), b'0 tiles for 1 pieces'),
            (dict(n_pieces=3, n_tiles=2), b'2 tiles for 3 pieces'),
            (dict(n_tiles=-1), b'-1 tiles')):
        status = call(**arguments)
        assert status != 0, arguments
        assert message in lib.emph_last_error(), (
            arguments, lib.emph_last_error())
    # nothing to do is not an error, whatever the pointers
    assert call(n_pieces=0, n_tiles=0, dword=None, dx=None) == 0
