"""`precision=` of the training step, host side (no device): the refusals,
the CLI flag, the C ABI of the two new entry points, their argument checks,
the table of the device pack, and the float64 emulation of the bf16x3
arithmetic (tests/split_emulation.py) with the split switched off."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import split_emulation  # noqa: E402
import train_data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import runtime, train  # noqa: E402
from emphases_amd.train import __main__ as cli  # noqa: E402

SYMBOLS = ('emph_conv_weight_grad_split', 'emph_conv_split_pack_device')
EINVAL, ERANGE = -1, -2          # include/emphases_hip.h


@pytest.fixture
def no_gpu(monkeypatch):
    """A precision is judged before a device is asked for."""
    def fail(*_):
        raise AssertionError('a GPU was required')
    monkeypatch.setattr(runtime, 'require_gpu', fail)


@pytest.mark.parametrize('precision', ['bf16x3_fast', 'bf16x6'])
def test_inference_only_precisions_are_refused_by_name(no_gpu, precision):
    with pytest.raises(NotImplementedError, match='precision'):
        train.Trainer(precision=precision)
    with pytest.raises(NotImplementedError, match='precision'):
        train.train('nowhere', os.devnull, partition_dir='nowhere',
                    precision=precision)


@pytest.mark.parametrize(
    'precision', ['fp16', 'BF16X3', None, 3, ['bf16x3'], {'bf16x3': 1}])
def test_unknown_precisions_are_value_errors(no_gpu, precision):
    with pytest.raises(ValueError, match='precision'):
        train.Trainer(precision=precision)


@pytest.mark.parametrize('precision', ['f32', 'bf16x3'])
def test_supported_precisions_get_as_far_as_the_device(precision):
    assert train.check_precision(precision) == precision
    assert precision in train.PRECISIONS
    if not torch.cuda.is_available():
        with pytest.raises(runtime.LibraryError):
            train.Trainer(precision=precision)


def test_cli_flag_reaches_train(monkeypatch, tmp_path):
    arguments = ['--directory', str(tmp_path), '--partition_dir', 'p']
    assert cli.parse_args(arguments).precision == 'f32'
    parsed = cli.parse_args(arguments + ['--precision', 'bf16x3'])
    assert parsed.precision == 'bf16x3'
    for refused in ('bf16x6', 'bf16x3_fast', 'fp16'):
        with pytest.raises(SystemExit):
            cli.parse_args(arguments + ['--precision', refused])
    seen = {}
    monkeypatch.setattr(
        emphases_amd.train, 'train',
        lambda dataset, directory, **kwargs: seen.update(
            kwargs, dataset=dataset, directory=directory))
    cli.main(arguments + ['--precision', 'bf16x3'])
    assert seen['precision'] == 'bf16x3' and seen['directory'] == tmp_path
    cli.main(arguments)
    assert seen['precision'] == 'f32'


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    version = int(re.search(r'#define EMPH_ABI_VERSION (\d+)', header).group(1))
    assert version == runtime.ABI_VERSION >= 36
    stripped = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    library = runtime.library()
    for name in SYMBOLS:
        assert re.search(rf'\bint {name}\s*\(', stripped), name
        assert name in runtime.SIGNATURES
        function = getattr(library, name)
        assert function.argtypes == runtime.SIGNATURES[name][1]
    source = open(os.path.join(
        ROOT, 'emphases_amd', 'csrc', 'conv_grad_split.hip')).read()
    assert 'mfma_f32_16x16x32_bf16' in source
    assert 'conv_grad_split.hip' in open(os.path.join(
        ROOT, 'emphases_amd', 'csrc', 'Makefile')).read()


def test_bad_arguments_are_refused_and_never_launched():
    """Checked before the launch, so host memory (never read) will do."""
    library = runtime.library()
    buffer = np.zeros(64, dtype=np.float32)
    pointer = buffer.ctypes.data

    def weight_grad(c_in=80, c_out=80, kernel_size=3, n_tiles=1, tile=64,
                    **null):
        names = ('dy', 'x', 'tiles', 'workspace', 'dweight', 'dbias')
        p = {name: None if null.get(name) else pointer for name in names}
        return library.emph_conv_weight_grad_split(
            p['dy'], 128, p['x'], 128, c_in, c_out, kernel_size, p['tiles'],
            n_tiles, tile, p['workspace'], p['dweight'], p['dbias'], None)

    for name in ('dy', 'x', 'tiles', 'workspace', 'dweight', 'dbias'):
        assert weight_grad(**{name: True}) == EINVAL, name
        assert b'null' in library.emph_last_error()
    for shape in ({'c_in': 83}, {'c_in': 79}, {'c_out': 64},
                  {'kernel_size': 5}, {'c_in': 1, 'c_out': 1}, {'tile': 32}):
        assert weight_grad(**shape) == ERANGE, shape
        assert b'emph_conv_weight_grad_split' in library.emph_last_error()
    assert weight_grad(n_tiles=0) == EINVAL
    pack = library.emph_conv_split_pack_device
    assert pack(None, pointer, pointer, 1, None) == EINVAL
    assert pack(pointer, None, pointer, 1, None) == EINVAL
    assert pack(pointer, pointer, None, 1, None) == EINVAL
    assert pack(pointer, pointer, pointer, -1, None) == ERANGE
    assert pack(pointer, pointer, pointer + 4, 1, None) == EINVAL
    assert pack(None, None, None, 0, None) == 0


@pytest.mark.parametrize('features', [80, 83])
def test_split_pack_table_is_the_host_pack_layout(features):
    """Gathering bf16-exact weights through the table equals the high pieces
    of `emph_conv_split_pack`, forward and flipped; 83 feature rows leave the
    input layer to the fp32 kernels."""
    config = emphases_amd.Config(
        layers=2, pitch_feature=features > 80,
        periodicity_feature=features > 81, loudness_feature=features > 82)
    offsets, count = train.parameter_offsets(config)
    tables = train.split_pack_tables(config)
    names = train.split_layer_names(config)
    assert names == (['input_layer'] if features == 80 else []) + \
        ['frame_encoder.0', 'frame_encoder.2']
    assert list(tables['forward']) == names
    assert list(tables['backward']) == ['frame_encoder.0', 'frame_encoder.2']
    index = tables['index']
    size = int(runtime.library().emph_conv_split_pack_size())
    assert index.dtype == np.int32 and index.shape == (
        len(names) + 2, size // 4) and index.max() < count
    # values exact in bf16: -64 .. 63.5 by halves
    rng = np.random.default_rng(features)
    flat = (rng.permutation(count) % 256 - 128).astype(np.float32) * 0.5
    for direction in ('forward', 'backward'):
        for name, number in tables[direction].items():
            first, shape = offsets[f'{name}.weight']
            weight = flat[first:first + 80 * 80 * 3].reshape(shape)
            if direction == 'backward':
                weight = np.ascontiguousarray(
                    weight.transpose(1, 0, 2)[:, :, ::-1])
            want = runtime.conv_split_pack(weight).view(np.uint16).reshape(
                -1, 2, 512)
            taken = np.where(index[number] < 0, np.float32(0),
                             flat[np.maximum(index[number], 0)])
            high = (taken.view(np.uint32) >> 16).astype(np.uint16)
            assert np.array_equal(high.reshape(-1, 512), want[:, 0])
            assert not want[:, 1].any()
            inside = index[number][index[number] >= 0]
            assert np.array_equal(
                np.sort(inside), np.arange(first, first + 80 * 80 * 3))


def test_emulation_without_the_split_is_plain_float64_autograd():
    """The custom autograd.Function of the layers in scope, split switched
    off, against `torch.nn.functional.conv1d` under autograd; and the whole
    model against the reference's float64 gradients on `uniform`."""
    generator = torch.Generator().manual_seed(5)
    x = torch.randn(1, 80, 37, dtype=torch.float64, generator=generator,
                    ).requires_grad_()
    weight = torch.randn(80, 80, 3, dtype=torch.float64, generator=generator,
                         ).requires_grad_()
    bias = torch.randn(80, dtype=torch.float64, generator=generator,
                       ).requires_grad_()
    dy = torch.randn(1, 80, 37, dtype=torch.float64, generator=generator)
    results = []
    for split in (None, False, True):
        for leaf in (x, weight, bias):
            leaf.grad = None
        if split is None:
            y = torch.nn.functional.conv1d(x, weight, bias, padding=1)
        else:
            y = split_emulation.SplitConv.apply(x, weight, bias, split)
        y.backward(dy)
        results.append([y.detach()] + [leaf.grad for leaf in (x, weight, bias)])
    plain, exact, emulated = results
    for name, want, got, rough in zip(
            ('y', 'dx', 'dweight', 'dbias'), plain, exact, emulated):
        scale = float(want.abs().max())
        error = float((got - want).abs().max()) / scale
        split_error = float((rough - want).abs().max()) / scale
        print(f'{name}: split off {error:.3g}, split on {split_error:.3g}')
        assert error < 1e-14, name
        # two pieces hold 16 bits of an operand: the dropped lo.lo and the
        # rounding of lo leave about 2^-16 per product, far less after a sum
        assert (split_error == 0) if name == 'dbias' else \
            (1e-9 < split_error < 2. ** -14), name
    # pieces: hi + lo within 2^-17 of the float32 value, both exact in bf16
    value = torch.randn(1000, dtype=torch.float64, generator=generator)
    high, low = split_emulation.pieces(value)
    for piece in (high, low):
        assert torch.equal(piece.float().bfloat16().double(), piece)
    assert float(((high + low) - value.float().double()).abs().max() /
                 value.abs().max()) <= 2. ** -17
    golden = train_data.golden()
    state = split_emulation.load_state()
    loss, gradients = split_emulation.loss_and_gradients(
        state, split_emulation.items_of(golden, 'uniform'), split=False)
    assert loss == pytest.approx(float(golden['uniform/loss']), rel=1e-12)
    for name, want in train_data.gradients('uniform').items():
        error = np.abs(gradients[name] - want).max() / np.abs(want).max()
        assert error < 2e-7, (name, error)     # (stored as float32)


def test_recorded_emulation_errors():
    """tests/golden/train_split.npz: the errors are those of two-piece
    arithmetic (1e-6 .. 1e-4 of the largest gradient), the Adam trajectory
    under the emulation decreases and starts at the emulated loss."""
    with np.load(os.path.join(HERE, 'golden', 'train_split.npz')) as archive:
        split = {name: archive[name] for name in archive.files}
    golden = train_data.golden()
    for case in ('ragged', 'uniform'):
        assert 1e-6 < float(split[f'{case}/emulated_error']) < 1e-4
        assert float(split[f'{case}/emulated_loss_error']) < 1e-6
        assert float(split[f'{case}/exact_error']) < 2e-7
    losses = split['adam/emulated']
    assert losses.shape == (6,) and np.all(np.diff(losses) < 0)
    assert abs(losses[0] - float(golden['ragged/loss'])) <= \
        float(split['ragged/emulated_loss_error']) * losses[0] * 1.000001
