"""The backward of the log-mel front-end without a GPU: the specification
(tests/logmel_grad_reference.py) against torch autograd of the float64 oracle,
the new C ABI and its refusals, the workspace cap, and the refusal of
`mels.from_audio` under `normalize=True`."""
import os
import re

import numpy as np
import pytest
import torch

import logmel_grad_reference as reference
from emphases_amd import core, runtime
from emphases_amd.data.preprocess import mels
from oracle import prominence as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('emph_logmel_backward_workspace', 'emph_logmel_backward')
# csrc/frontend_grad.hip: kRunSlots tiles of (8 - 1) * 160 + 1024 floats
WORKSPACE_CAP = 4096 * 2144
EINVAL = -1          # EMPH_EINVAL


def autograd(audio, cotangent):
    """d sum(cotangent * oracle.logmel(audio)) / d audio, in audio's dtype."""
    leaf = audio.clone()[None].requires_grad_()
    out = oracle.logmel(leaf)
    gradient, = torch.autograd.grad((out * cotangent.to(out.dtype)).sum(), leaf)
    return gradient[0]


@pytest.mark.parametrize('samples', [433, 864, 865, 5920, 16077])
def test_the_specification_is_torch_autograd_of_the_oracle(samples):
    rng = np.random.default_rng(samples)
    audio = 0.1 * rng.standard_normal(samples)
    cotangent = rng.standard_normal((80, reference.frames_of(samples)))
    want = autograd(torch.from_numpy(audio), torch.from_numpy(cotangent))
    got = reference.backward(audio, cotangent)
    assert got['dx'].shape == (samples,)
    scale = float(want.abs().max())
    error = float(np.abs(got['dx'] - want.numpy()).max()) / scale
    print(f'S={samples}: helper against autograd {error:.2e}')
    assert error < 1e-12
    # ... and the forward it differentiates is the oracle's
    assert np.abs(got['y'] - oracle.logmel(
        torch.from_numpy(audio)[None]).numpy()).max() < 1e-12
    assert got['q'].shape == cotangent.shape
    assert got['G'].shape == (513, cotangent.shape[1])
    assert got['t'].shape == (cotangent.shape[1], 1024)
    assert got['P'].shape == (samples + 864,)


def test_the_clamp_stops_the_gradient_in_the_specification():
    """A basis scaled down until some rows clamp: the helper follows torch's
    rule for clamp(min=) there too."""
    rng = np.random.default_rng(5)
    audio = 1e-3 * rng.standard_normal(1600)
    cotangent = rng.standard_normal((80, 10))
    basis = 0.01 * oracle.mel_basis().double()
    leaf = torch.from_numpy(audio)[None].requires_grad_()
    out = oracle.log_of_mel(oracle.mel(leaf, basis))
    want, = torch.autograd.grad((out * torch.from_numpy(cotangent)).sum(), leaf)
    got = reference.backward(audio, cotangent, basis.numpy())
    clamped = got['m'] < 1e-5
    assert 0 < clamped.sum() < clamped.size
    assert np.abs(got['dx'] - want[0].numpy()).max() < \
        1e-12 * float(want.abs().max())


def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, 'include', 'emphases_hip.h')).read()
    version = int(re.search(r'#define EMPH_ABI_VERSION (\d+)', header).group(1))
    assert version == runtime.ABI_VERSION >= 43
    library = runtime.library()
    for name in SYMBOLS:
        assert f'{name}(' in header
        assert name in runtime.SIGNATURES
        assert getattr(library, name).argtypes == runtime.SIGNATURES[name][1]
    makefile = open(os.path.join(
        ROOT, 'emphases_amd', 'csrc', 'Makefile')).read()
    assert 'frontend_grad.hip' in makefile


def test_null_negative_and_misaligned_arguments_are_refused():
    """Host checks only: nothing is launched (there is no GPU here)."""
    library = runtime.library()
    room = np.zeros(64, dtype=np.int64)
    good = (room.ctypes.data + 15) // 16 * 16     # 16-byte aligned, inside `room`
    #       audio seg tiles n table start count offset values nnz dmel ld row
    base = [good, good, good, 1, good, good, good, good, good, 1001, good, 64,
            0, good, good, None]
    pointers = (0, 1, 2, 4, 5, 6, 7, 8, 10, 13, 14)
    for at in pointers:
        arguments = list(base)
        arguments[at] = None
        assert library.emph_logmel_backward(*arguments) == EINVAL, at
    for at in pointers:
        arguments = list(base)
        arguments[at] = good + 2
        assert library.emph_logmel_backward(*arguments) == EINVAL, at
    arguments = list(base)
    arguments[2] = good + 8                       # the tile table: 16 bytes
    assert library.emph_logmel_backward(*arguments) == EINVAL
    arguments = list(base)
    arguments[3] = -1
    assert library.emph_logmel_backward(*arguments) == EINVAL
    assert b'n_tiles' in library.emph_last_error()
    # no tiles: nothing to do, whatever the device
    arguments = list(base)
    arguments[3] = 0
    assert library.emph_logmel_backward(*arguments) == 0


def test_the_workspace_is_positive_and_capped():
    library = runtime.library()
    sizes = [int(library.emph_logmel_backward_workspace(n))
             for n in (0, 1, 2, 100, 4095, 4096, 4097, 1 << 16, 1 << 20)]
    assert all(size > 0 for size in sizes)
    assert sizes == sorted(sizes)
    assert sizes[1] == 2144 and sizes[3] == 100 * 2144
    assert max(sizes) == sizes[-1] == WORKSPACE_CAP
    assert int(library.emph_logmel_backward_workspace(-3)) > 0
    assert WORKSPACE_CAP * 4 < 34 * (1 << 20)


def test_from_audio_refuses_normalize_with_grad_before_any_gpu(monkeypatch):
    def no_gpu(*args, **kwargs):
        raise AssertionError('a GPU was asked for')
    monkeypatch.setattr(runtime, 'require_gpu', no_gpu)
    monkeypatch.setattr(core, 'get_engine', no_gpu)
    before = core.active_config()
    try:
        core.configure(normalize=True)
        audio = torch.zeros(1, 1600, requires_grad=True)
        with pytest.raises(NotImplementedError, match='normalize'):
            mels.from_audio(audio)
    finally:
        core.configure(before)
