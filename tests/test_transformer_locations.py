"""The key-padded attention backward and `encoder_layer_padded` without a
GPU: the new C entry is declared, bound and exported and checks its arguments
before it looks at a pointer; the op is registered with its schema; the
Transformer classes keep refusing `'input'` and `'inference'`;
`TransformerLocationsModel` / `TransformerLocationsTrainer` accept the four
locations and refuse by field name, the CLI routes to them, and their
parameter layout is `weights.parameter_shapes`'s."""
import os

import pytest
import torch

import emphases_amd
from emphases_amd import ops, runtime, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    name = 'emph_attention_backward_keys'
    assert f'int {name}(' in header
    # emph_attention_backward's arguments with the table before the workspace
    plain = runtime.SIGNATURES['emph_attention_backward']
    result, arguments = runtime.SIGNATURES[name]
    assert result is plain[0] and len(arguments) == 14
    assert arguments == plain[1][:11] + [plain[1][8]] + plain[1][11:]
    library = runtime.library()
    assert getattr(library, name).argtypes == arguments


def test_argument_checks_before_any_pointer():
    """Return codes of calls that launch nothing (no GPU here)."""
    library = runtime.library()

    def call(channels, heads, n_tiles=1, tile_n=64, table=None):
        return library.emph_attention_backward_keys(
            None, None, None, None, None, 64, channels, heads, None, n_tiles,
            tile_n, table, None, None)
    table = (runtime._c.c_int32 * 1)(1)
    for keys in (None, table):
        for channels, heads in ((64, 2), (80, 4), (128, 2), (80, 1), (80, 0)):
            assert call(channels, heads, table=keys) == -2
        assert call(80, 2, table=keys) == -1
        assert b'null pointer' in library.emph_last_error()
        assert call(80, 2, tile_n=32, table=keys) == -1
        assert call(80, 2, n_tiles=0, table=keys) == 0
    assert call(64, 2, table=table) == -2
    assert b'emph_attention_backward_keys' in library.emph_last_error()


def test_the_op_is_registered():
    assert 'encoder_layer_padded' in ops.__all__
    schema = str(torch.ops.emphases_amd.encoder_layer_padded.default._schema)
    arguments = schema[schema.index('(') + 1:schema.index(') ->')].split(', ')
    assert len(arguments) == 16
    assert arguments[0] == 'Tensor x'
    assert arguments[13:] == ['Tensor cu_T', 'Tensor key_counts',
                              'SymInt heads']


def test_the_op_has_no_cpu_implementation():
    x = torch.zeros(80, 4)
    tensors = [torch.zeros(1)] * 12
    with pytest.raises(runtime.LibraryError, match='HIP device only'):
        torch.ops.emphases_amd.encoder_layer_padded(
            x, *tensors, torch.tensor([0, 4]), torch.tensor([2]), 2)


def test_key_counts_are_checked_against_the_layout():
    import numpy as np
    plan = ops._frame_plan(np.array([3, 7], dtype=np.int64), None, None)

    class Layout:
        def key_counts(self, counts, check):
            check(counts)
            return counts
    layout = Layout()
    layout.plan = plan
    assert ops._key_counts(torch.tensor([3, 1]), layout).tolist() == [3, 1]
    for bad in ([0, 7], [3, 8], [3], [3, 7, 1], [-1, 2]):
        with pytest.raises(ValueError, match='key_counts'):
            ops._key_counts(torch.tensor(bad), layout)
    with pytest.raises(TypeError, match='key_counts'):
        ops._key_counts(torch.tensor([3., 7.]), layout)


@pytest.mark.parametrize('location', ['input', 'inference'])
def test_the_transformer_classes_still_refuse(location):
    config = emphases_amd.Config(
        architecture='transformer', layers=2, downsample_location=location)
    for refuse in (train.TransformerModel, train.initial_transformer_state,
                   train.TransformerTrainer, train.TransformerTrainer.check,
                   train.check_transformer_supported):
        with pytest.raises(NotImplementedError, match='downsample_location'):
            refuse(config)


###############################################################################
# TransformerLocationsModel / TransformerLocationsTrainer, host side
###############################################################################

LOCATIONS = ('input', 'intermediate', 'inference', 'loss')


def located(location, **more):
    return emphases_amd.Config(
        architecture='transformer', layers=2, downsample_location=location,
        **more)


def test_check_accepts_the_four_locations():
    check = train.TransformerLocationsTrainer.check
    for location in LOCATIONS:
        for method in ('sum', 'average', 'max', 'center'):
            assert check(located(location, downsample_method=method)) == 'f32'
    for location in ('intermediate', 'inference', 'loss'):
        assert check(located(location), 'bf16x3') == 'bf16x3'
        assert check(located(location), 'f32', True) == 'f32'


@pytest.mark.parametrize('keywords, overrides, field', [
    ({'precision': 'bf16x3'}, {}, 'precision'),
    ({'reference_dropout': True}, {}, 'reference_dropout'),
    ({}, {'dropout': 0.1}, 'dropout'),
])
def test_check_refuses_at_input_by_field_name(keywords, overrides, field):
    config = located('input', **overrides)
    with pytest.raises(NotImplementedError, match=field):
        train.TransformerLocationsTrainer.check(config, **keywords)
    with pytest.raises(NotImplementedError, match=field):
        train.TransformerLocationsModel(config, **keywords)
    # (before a GPU is needed: there is none here)
    with pytest.raises(NotImplementedError, match=field):
        train.TransformerLocationsTrainer(config, **keywords)


@pytest.mark.parametrize('overrides, keywords, field', [
    ({'channels': 64}, {}, 'channels'), ({'heads': 4}, {}, 'heads'),
    ({'dropout': 0.1}, {}, 'dropout'),
    ({'architecture': 'convolution'}, {}, 'architecture'),
    ({}, {'precision': 'bf16x3', 'reference_dropout': True}, 'precision'),
])
def test_check_refuses_everywhere_what_the_parent_refuses(
        overrides, keywords, field):
    settings = dict(architecture='transformer', layers=2,
                    downsample_location='inference')
    settings.update(overrides)
    with pytest.raises(NotImplementedError, match=field):
        train.TransformerLocationsTrainer.check(
            emphases_amd.Config(**settings), **keywords)


@pytest.mark.parametrize('location', ['input', 'inference'])
def test_parameter_offsets_agree_with_parameter_shapes(location):
    import numpy as np
    from emphases_amd import weights
    from emphases_amd.train import core
    config = located(location)
    shapes = weights.parameter_shapes(config)
    offsets, count = core.parameter_offsets(config)
    assert list(offsets) == list(shapes)
    first = 0
    for name, (offset, shape) in offsets.items():
        assert tuple(shape) == tuple(shapes[name]) and offset >= first, name
        first = offset + int(np.prod(shape))
    assert first <= count
    model = train.TransformerLocationsModel(config, seed=2)
    assert [(k, tuple(p.shape)) for k, p in model.named_parameters()] == \
        [(k, tuple(s)) for k, s in shapes.items()]
    assert ('word_decoder.model.layers.0.norm1.weight' in shapes) == \
        (location == 'input')
    # the reference's initialisation for that configuration: the draws of the
    # parent's at the location with the same modules, in the same order
    twin = located('intermediate' if location == 'input' else 'loss')
    want = train.initial_transformer_state(twin, 2)
    for key, parameter in model.named_parameters():
        assert np.array_equal(parameter.detach().numpy(), want[key]), key


def test_the_piece_tables_pad_to_the_utterances_longest_word():
    import numpy as np
    from emphases_amd.train import transformer_model
    as_bytes = lambda values: np.asarray(  # noqa: E731
        values, dtype=np.int64).tobytes()
    index, cu_pieces, keys, pool, cu_one = transformer_model._piece_tables(
        as_bytes([0, 10, 13]), as_bytes([[0, 3, 0], [3, 8, 2]]),
        as_bytes([0, 2, 3]), False)
    assert cu_pieces.tolist() == [0, 5, 10, 12]
    assert keys.tolist() == [3, 5, 2]
    # (13 is the zero column behind the features)
    assert index.tolist() == [0, 1, 2, 13, 13, 3, 4, 5, 6, 7, 10, 11]
    assert pool.tolist() == [[0, 0, 0], [5, 5, 2]]
    assert cu_one.tolist() == [0, 1, 2, 3]
    centre = transformer_model._piece_tables(
        as_bytes([0, 10, 13]), as_bytes([[0, 3, 0], [3, 8, 2]]),
        as_bytes([0, 2, 3]), True)[3]
    assert centre.tolist() == [[0, 0, 0], [3, 5, 2]]
    with pytest.raises(ValueError, match='input'):
        transformer_model._piece_tables(
            as_bytes([0, 10]), as_bytes([[0], [11]]), as_bytes([0, 1]), False)


def faked_main(monkeypatch, arguments):
    from emphases_amd.train import __main__ as cli
    calls = []
    monkeypatch.setattr(
        emphases_amd.train, 'train',
        lambda *args, **kwargs: calls.append(
            (kwargs, emphases_amd.core.active_config())))
    before = emphases_amd.core.active_config()
    try:
        cli.main(arguments)
    finally:
        emphases_amd.configure(before)
    (kwargs, config), = calls
    return kwargs, config


FLAGS = ['--directory', 'run', '--partition_dir', 'parts']


@pytest.mark.parametrize('location, trainer', [
    ('input', 'TransformerLocationsTrainer'),
    ('inference', 'TransformerLocationsTrainer'),
    ('intermediate', 'TransformerTrainer'), ('loss', 'TransformerTrainer')])
def test_cli_routing(tmp_path, monkeypatch, location, trainer):
    kwargs, config = faked_main(monkeypatch, FLAGS + [
        '--architecture', 'transformer', '--downsample_location', location])
    assert kwargs['trainer'] is getattr(train, trainer)
    assert 'trainer_arguments' not in kwargs
    assert config.downsample_location == location
    path = tmp_path / 'file.py'
    path.write_text(f"ARCHITECTURE = 'transformer'\n"
                    f"DOWNSAMPLE_LOCATION = '{location}'\n")
    kwargs, config = faked_main(monkeypatch, FLAGS + ['--config', str(path)])
    assert kwargs['trainer'] is getattr(train, trainer)
    assert config.architecture == 'transformer'
    assert config.downsample_location == location


def test_cli_input_without_the_transformer_stays_a_usage_error():
    from emphases_amd.train import __main__ as cli
    with pytest.raises(SystemExit):
        cli.parse_args(FLAGS + ['--downsample_location', 'input'])
    assert cli.parse_args(FLAGS + [
        '--architecture', 'transformer', '--downsample_location',
        'input']).downsample_location == 'input'


def test_dispatch_without_the_opt_in_still_refuses():
    for location in LOCATIONS:
        with pytest.raises(NotImplementedError, match='architecture'):
            train.make_trainer(located(location))
