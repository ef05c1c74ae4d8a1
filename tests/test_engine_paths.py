"""CPU: `engine.decide` - the one place an engine's kernels are chosen - says,
without a device, what `tests/test_gpu_paths.py` asserts of a live engine: for
every row of its `ROWS` at every precision the row's path, for every entry of
its `REFUSED` the ValueError.  No kernel is launched here."""
import pytest

from emphases_amd import config as cfg, engine as engine_module, weights
from test_gpu_paths import PRECISIONS, REFUSED, ROWS, SPLIT


def decision(row, precision, monkeypatch):
    for key, value in row['env'].items():
        monkeypatch.setenv(key, value)
    config = cfg.Config(**row['overrides'])
    return config, engine_module.decide(
        config, weights.random_state(config, seed=17), precision)


def stack_forms(paths, name):
    """The layer forms of a Transformer stack under the tile tables
    `Engine._pack` requests: tiles of 32 positions always, tiles of
    `split_tile` positions on the frame axis where `paths.split_tables`."""
    return paths.forms(getattr(paths, name), True,
                       name == 'frame_encoder' and paths.split_tables)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('row', ROWS, ids=[row['name'] for row in ROWS])
def test_decision_is_the_rows_path(row, precision, monkeypatch):
    """The facts of `test_gpu_paths.assert_path`, on the decision."""
    config, paths = decision(row, precision, monkeypatch)
    path, opt_in = row['path'], precision != 'f32'
    assert (paths.split_pieces, paths.attention_pieces,
            paths.linear_pieces) == engine_module.PRECISIONS[precision]
    assert paths.quad == path['quad']
    if config.architecture == 'convolution':
        assert paths.stack == path['stack']
        assert paths.fold == path['fold']
        assert paths.split_conv == (path['stack'] and precision in SPLIT)
        assert paths.frame_encoder == () and paths.word_decoder == ()
        assert not paths.word_transformer
        return
    assert not paths.stack and not paths.fold and not paths.split_conv
    assert not paths.model and not paths.compose and not paths.mel_plan
    assert paths.word_transformer == path['words']
    assert len(paths.frame_encoder) == config.layers
    assert [packs.block for packs in paths.frame_encoder] == \
        [path['block']] * config.layers
    assert [packs.split for packs in paths.frame_encoder] == \
        [path['split'] and opt_in] * config.layers
    assert (paths.attention_pieces != 0 and
            config.channels // config.heads == 40) == \
        (path['attention'] and opt_in)
    assert paths.split_tile == int(row['env'].get('EMPHASES_SPLIT_TILE', 16))
    assert paths.fuse_qkv == (row['env'].get('EMPHASES_FUSE_QKV') != '0')


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('row', ROWS, ids=[row['name'] for row in ROWS])
def test_decision_names_the_launches(row, precision, monkeypatch):
    """What follows from the path: the route of a batch, the forms of the
    Transformer's layers, the limit of the packed axis."""
    config, paths = decision(row, precision, monkeypatch)
    path, opt_in = row['path'], precision != 'f32'
    if config.architecture == 'convolution':
        tile = paths.frame_tile(None) if paths.quad else 32
        assert tile == (64 if path['quad'] else 32)
        route = paths.route(tile)
        assert route.stack == path['stack'] and route.fold == path['fold']
        # one C call: the default feature rows, F(2,3) packs, fp32 kernels
        assert route.one_call == (
            paths.model and not (path['stack'] and precision in SPLIT))
        assert not paths.model or (
            config.downsample_location != 'input' and
            config.encoder_kernel_size == 3)
        if row['name'] == 'conv':
            assert paths.model and paths.mel_plan
            assert paths.compose == (precision not in SPLIT)
        # taps, a nested layout and narrower tiles leave the fast routes
        assert paths.route(tile, stages=True) == (False, False, False)
        assert paths.route(tile, nested=True)[1:] == (False, False)
        assert paths.route(16) == (False, False, False)
        for tap in ('features', 'timers'):
            assert paths.route(tile, **{tap: True}) == (False,) + route[1:]
        assert paths.max_columns == engine_module.KERNEL_COLUMNS
        return
    assert paths.route(64) == (False, False, False)
    split = path['split'] and opt_in
    assert paths.max_columns == (
        engine_module.SPLIT16_COLUMNS if opt_in and paths.split_tile == 16
        else engine_module.KERNEL_COLUMNS)
    assert paths.transformer and paths.split_tables == opt_in
    forms = stack_forms(paths, 'frame_encoder')
    kind = 'split' if split else 'fused' if path['block'] else 'convs'
    assert [form.block for form in forms] == [kind] * config.layers
    fused_projection = config.channels in (64, 80)
    assert [form.project for form in forms] == [
        'split' if split else 'fused' if fused_projection else 'convs'
    ] * config.layers
    # every block but the last makes the next layer's projections, unless
    # EMPHASES_FUSE_QKV=0 or the per-layer form runs
    assert [form.ahead for form in forms] == [
        kind != 'convs' and paths.fuse_qkv and index + 1 < config.layers
        for index in range(config.layers)]
    # the split forms are frame-axis kernels; without tiles of 32: per layer
    assert all(form.block != 'split'
               for form in stack_forms(paths, 'word_decoder'))
    assert all(form == ('convs', 'convs', False)
               for form in paths.forms(paths.frame_encoder, fused=False))
    # a shortened stack: its last block has no next layer to project for
    assert not paths.forms(paths.frame_encoder[:1], True, split)[0].ahead


@pytest.mark.parametrize('overrides,message', REFUSED)
def test_decision_refuses(overrides, message):
    config = cfg.Config(**overrides)
    with pytest.raises(ValueError, match=message):
        engine_module.decide(config, weights.random_state(config))


def test_decision_refuses_switches_and_precisions(monkeypatch):
    state = weights.random_state(cfg.DEFAULT)
    with pytest.raises(ValueError, match="precision 'bf16' is not one of"):
        engine_module.decide(cfg.DEFAULT, state, 'bf16')
    with pytest.raises(ValueError, match='EMPHASES_SPLIT_TILE must be 16 or 32'):
        engine_module.decide(cfg.DEFAULT, state,
                             environ={'EMPHASES_SPLIT_TILE': '8'})
    # the switches come from `environ` alone when it is given
    monkeypatch.setenv('EMPHASES_CONV_STACK', '0')
    assert engine_module.decide(cfg.DEFAULT, state, environ={}).stack
    assert not engine_module.decide(cfg.DEFAULT, state).stack
