"""`TransformerTrainer` and the loop's `trainer=` opt-in, host side (no
device): every refusal before a GPU is needed and before the run directory
exists, the CLI's two flags and its dispatch, the C ABI of
`emph_adam_step_gathered` with its argument checks, and the optimizer state's
layout."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import emphases_amd  # noqa: E402
from emphases_amd import runtime, train, weights  # noqa: E402
from emphases_amd.train import __main__ as cli  # noqa: E402

EINVAL, ERANGE = -1, -2          # include/emphases_hip.h
FLAGS = ['--directory', 'run', '--partition_dir', 'parts']
TRANSFORMER = emphases_amd.Config(architecture='transformer', layers=2)


@pytest.fixture
def no_gpu(monkeypatch):
    """Every refusal comes before a device is asked for."""
    def fail(*_):
        raise AssertionError('a GPU was required')
    monkeypatch.setattr(runtime, 'require_gpu', fail)


def run(tmp_path, **arguments):
    return train.train('nothing', tmp_path / 'run', partition_dir='nowhere',
                       cache_dir='nowhere', **arguments)


###############################################################################
# Refusals
###############################################################################


def test_without_the_opt_in_every_dispatch_still_refuses(no_gpu, tmp_path):
    for config in (TRANSFORMER, emphases_amd.Config(architecture='transformer')):
        with pytest.raises(NotImplementedError, match='architecture'):
            run(tmp_path, config=config)
        for dispatch in (train.select_trainer, train.trainer_for,
                         train.make_trainer, train.step_class):
            with pytest.raises(NotImplementedError, match='architecture'):
                dispatch(config)
    with pytest.raises(ValueError, match='trainer_arguments'):
        run(tmp_path, trainer_arguments={'reference_dropout': True})
    assert not (tmp_path / 'run').exists()


REFUSED = [
    ({'architecture': 'convolution'}, {}, 'architecture'),
    ({'downsample_location': 'inference'}, {}, 'downsample_location'),
    ({'downsample_location': 'input'}, {}, 'downsample_location'),
    ({'channels': 64}, {}, 'channels'),
    ({'heads': 4}, {}, 'heads'),
    ({'dropout': 0.1}, {}, 'dropout'),
    ({}, {'precision': 'bf16x6'}, 'precision'),
    ({}, {'precision': 'bf16x3',
          'trainer_arguments': {'reference_dropout': True}},
     'reference_dropout'),
]


@pytest.mark.parametrize(
    'fields,arguments,named', REFUSED, ids=[named + '-' + '-'.join(
        str(value) for value in fields.values()) for fields, _, named in REFUSED])
def test_the_opt_in_refuses_by_field_before_anything_exists(
        no_gpu, tmp_path, fields, arguments, named):
    config = emphases_amd.Config(
        **{'architecture': 'transformer', 'layers': 2, **fields})
    with pytest.raises(NotImplementedError, match=named):
        run(tmp_path, config=config, trainer=train.TransformerTrainer,
            **arguments)
    assert not (tmp_path / 'run').exists()
    # the class makes the same refusal, and its constructor with it
    keywords = {'precision': arguments.get('precision', 'f32'),
                **arguments.get('trainer_arguments', {})}
    with pytest.raises(NotImplementedError, match=named):
        train.TransformerTrainer.check(config, **keywords)
    with pytest.raises(NotImplementedError, match=named):
        train.TransformerTrainer(config, **keywords)


def test_what_is_covered_gets_as_far_as_the_device(no_gpu, tmp_path):
    for fields, keywords in (
            ({}, {}), ({'downsample_location': 'loss',
                        'downsample_method': 'max'}, {}),
            ({'loss': 'mse'}, {'precision': 'bf16x3'}),
            ({}, {'reference_dropout': True})):
        config = emphases_amd.Config(
            architecture='transformer', layers=2, **fields)
        assert train.TransformerTrainer.check(config, **keywords) == \
            keywords.get('precision', 'f32')
        with pytest.raises(AssertionError, match='a GPU was required'):
            train.TransformerTrainer(config, **keywords)
    with pytest.raises(ValueError, match='precision'):
        train.TransformerTrainer.check(TRANSFORMER, 'fp16')
    # the loop gets past its refusals to the first file it reads
    with pytest.raises(AssertionError, match='a GPU was required'):
        run(tmp_path, config=TRANSFORMER, trainer=train.TransformerTrainer,
            trainer_arguments={'reference_dropout': True})


###############################################################################
# CLI
###############################################################################


def faked_main(monkeypatch, arguments):
    """The keyword arguments and the active configuration `train.train` sees
    from `main(arguments)`."""
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


def test_architecture_flag_becomes_an_override():
    overrides, arguments = cli.settings(FLAGS + ['--architecture', 'transformer'])
    assert overrides == {'architecture': 'transformer'}
    assert cli.settings(FLAGS)[0] == {}
    assert cli.settings(FLAGS + ['--architecture', 'convolution'])[0] == \
        {'architecture': 'convolution'}
    with pytest.raises(SystemExit):
        cli.settings(FLAGS + ['--architecture', 'recurrent'])


def test_transformer_config_reaches_train_with_the_trainer(
        tmp_path, monkeypatch):
    path = tmp_path / 'transformer.py'
    path.write_text("ARCHITECTURE = 'transformer'\nLAYERS = 2\nNUM_STEPS = 3\n")
    kwargs, config = faked_main(monkeypatch, FLAGS + ['--config', str(path)])
    assert kwargs['trainer'] is train.TransformerTrainer
    assert 'trainer_arguments' not in kwargs and kwargs['num_steps'] == 3
    assert 'reference_dropout' not in kwargs
    assert config.architecture == 'transformer' and config.layers == 2
    # the flag does what the file does; --reference_dropout goes along
    kwargs, config = faked_main(monkeypatch, FLAGS + [
        '--architecture', 'transformer', '--reference_dropout',
        '--downsample_location', 'loss'])
    assert kwargs['trainer'] is train.TransformerTrainer
    assert kwargs['trainer_arguments'] == {'reference_dropout': True}
    assert config.architecture == 'transformer'
    assert config.downsample_location == 'loss'
    # an explicit flag overrides the file
    kwargs, config = faked_main(monkeypatch, FLAGS + [
        '--config', str(path), '--architecture', 'convolution'])
    assert 'trainer' not in kwargs and config.architecture == 'convolution'


def test_without_the_transformer_train_gets_what_it_always_got(monkeypatch):
    kwargs, config = faked_main(monkeypatch, FLAGS + ['--loss', 'mse'])
    assert sorted(kwargs) == [
        'cache_dir', 'gpu', 'log_interval', 'max_training_frames',
        'num_steps', 'partition_dir', 'precision']
    assert config.architecture == 'convolution'
    kwargs, _ = faked_main(monkeypatch, FLAGS)
    assert 'trainer' not in kwargs and 'trainer_arguments' not in kwargs
    assert 'reference_dropout' not in kwargs


def test_reference_dropout_alone_is_a_usage_error(monkeypatch):
    with pytest.raises(SystemExit, match='reference_dropout'):
        faked_main(monkeypatch, FLAGS + ['--reference_dropout'])


def test_reference_dropout_at_bf16x3_reaches_the_trainers_refusal(
        no_gpu, tmp_path):
    """Through the real `train.train`."""
    with pytest.raises(NotImplementedError, match='reference_dropout'):
        before = emphases_amd.core.active_config()
        try:
            cli.main(['--directory', str(tmp_path / 'run'), '--partition_dir',
                      'nowhere', '--architecture', 'transformer',
                      '--precision', 'bf16x3', '--reference_dropout'])
        finally:
            emphases_amd.configure(before)
    assert not (tmp_path / 'run').exists()


###############################################################################
# emph_adam_step_gathered: the contract
###############################################################################


def test_gathered_adam_is_declared_bound_and_exported():
    """The ABI number itself stays: tests/test_grid_train.py,
    tests/test_transformer_dropout.py and tests/test_transformer_precision.py
    pin it to 45, as they did when the last symbols were added.  A library
    built before this symbol fails to load by the missing export instead
    (`runtime.library`)."""
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    version = int(re.search(r'#define EMPH_ABI_VERSION (\d+)', header).group(1))
    assert version == runtime.ABI_VERSION
    capacity = int(re.search(r'#define EMPH_ADAM_TABLE (\d+)', header).group(1))
    assert capacity == runtime.ADAM_TABLE
    # the table travels in the launch's arguments: two pointers' worth and two
    # ints per tensor, well inside the 4 KB a launch may pass
    assert capacity * (8 + 8 + 4 + 4) + 64 <= 3072
    stripped = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'\bint emph_adam_step_gathered\s*\(', stripped)
    library = runtime.library()
    assert library.emph_abi_version() == runtime.ABI_VERSION
    function = library.emph_adam_step_gathered
    assert function.argtypes == \
        runtime.SIGNATURES['emph_adam_step_gathered'][1]
    source = open(os.path.join(
        ROOT, 'emphases_amd', 'csrc', 'train.hip')).read()
    # one element update, called by both kernels
    assert len(re.findall(r'\badam_update\(', source)) == 3


def gathered(pointers, offsets, counts, tensors=None, flat=16):
    """`emph_adam_step_gathered` on host tables; the flat buffers are host
    addresses too, which is as far as a refused call gets."""
    pointers = np.array(pointers, dtype=np.uint64)
    offsets = np.array(offsets, dtype=np.int64)
    counts = np.array(counts, dtype=np.int64)
    return runtime.library().emph_adam_step_gathered(
        flat, pointers.ctypes.data, offsets.ctypes.data, counts.ctypes.data,
        len(counts) if tensors is None else tensors, flat, flat, 0.9, 0.999,
        1e-3, 1., 1e-8, None)


def test_gathered_adam_refuses_bad_tables_and_launches_nothing():
    """Checked before the first launch, so host memory (never read) will do."""
    library = runtime.library()
    assert gathered([], [], [], tensors=0) == 0
    assert library.emph_adam_step_gathered(
        None, None, None, None, 0, None, None, 0.9, 0.999, 1e-3, 1., 1e-8,
        None) == 0
    # nothing but empty tensors: nothing to launch, whatever their pointers
    assert gathered([0, 18], [0, 5], [0, 0]) == 0
    assert gathered([16], [0], [4], tensors=-1) == EINVAL
    assert b'-1 tensors' in library.emph_last_error()
    assert gathered([16], [0], [4], flat=None) == EINVAL
    assert b'null pointer' in library.emph_last_error()
    # a null gradient of a non-empty tensor, behind good ones
    assert gathered([16, 16, 0], [0, 4, 8], [4, 0, 4]) == EINVAL
    assert b'tensor 2: null gradient' in library.emph_last_error()
    assert gathered([16, 16], [0, 4], [4, -1]) == EINVAL
    assert gathered([16, 16], [0, -4], [4, 4]) == EINVAL
    assert b'tensor 1' in library.emph_last_error()
    assert gathered([16, 18], [0, 4], [4, 4]) == EINVAL
    assert b'4-byte' in library.emph_last_error()
    assert gathered([16], [0], [1 << 30]) == ERANGE
    assert gathered([16], [1 << 39], [4]) == ERANGE


###############################################################################
# Optimizer state
###############################################################################


@pytest.mark.parametrize('location', ['intermediate', 'loss'])
def test_optimizer_state_loads_into_adam_over_the_model(location):
    config = emphases_amd.Config(
        architecture='transformer', layers=2, downsample_location=location)
    shapes = weights.parameter_shapes(config)
    offsets, count = train.parameter_offsets(config)
    assert list(offsets) == list(shapes)
    exp_avg = torch.arange(count, dtype=torch.float32)
    exp_avg_sq = exp_avg + 0.5
    model = train.TransformerModel(config)
    assert [name for name, _ in model.named_parameters()] == list(shapes)
    state = train.adam_state_dict(
        config, 3, exp_avg, exp_avg_sq, lr=2e-3, betas=(0.8, 0.9), eps=1e-6)
    optimizer = torch.optim.Adam(model.parameters())
    optimizer.load_state_dict(state)
    group = optimizer.param_groups[0]
    assert (group['lr'], group['betas'], group['eps']) == \
        (2e-3, (0.8, 0.9), 1e-6)
    assert len(state['state']) == len(shapes)
    for index, (name, shape) in enumerate(shapes.items()):
        entry = state['state'][index]
        first = offsets[name][0]
        assert tuple(entry['exp_avg'].shape) == tuple(shape), name
        assert tuple(entry['exp_avg_sq'].shape) == tuple(shape), name
        assert float(entry['step']) == 3.
        assert float(entry['exp_avg'].ravel()[0]) == first
        assert float(entry['exp_avg_sq'].ravel()[-1]) == \
            first + int(np.prod(shape)) - 0.5
        loaded = optimizer.state[dict(model.named_parameters())[name]]
        assert torch.equal(loaded['exp_avg'], entry['exp_avg'])
    fresh = train.adam_state_dict(config, 0, exp_avg, exp_avg_sq)
    assert fresh['state'] == {}
    torch.optim.Adam(model.parameters()).load_state_dict(fresh)
    assert train.TransformerTrainer.optimizer_state_dict is \
        train.Trainer.optimizer_state_dict


###############################################################################
# ops.mark_trained: the resume rule's contract
###############################################################################


def test_mark_trained_makes_restored_weights_count_as_trained():
    from emphases_amd import ops
    flat = torch.zeros(12)
    views = [torch.nn.Parameter(flat[:6].view(2, 3)),
             torch.nn.Parameter(flat[6:])]
    version = flat._version
    ops.mark_trained(views, base=flat)
    assert flat._version == version + 1
    assert all(view._version == version + 1 for view in views)
    assert all(ops._weight_changes(view) for view in views)
    # without a base every tensor's own counter moves
    alone = [torch.zeros(3), torch.zeros(4)]
    ops.mark_trained(alone)
    assert all(ops._weight_changes(tensor) for tensor in alone)
    assert [tensor._version for tensor in alone] == [1, 1]
    # a weight the ops see first by themselves is not in training ...
    other = torch.zeros(5)
    assert not ops._weight_changes(other)
    # ... and one that does not share the base's counter is reported
    with pytest.raises(RuntimeError, match='mark_trained'):
        ops.mark_trained([torch.zeros(2)], base=flat)
