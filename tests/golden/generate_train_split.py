"""Measure what the bf16x3 arithmetic of the training step costs.

    python tests/golden/generate_train_split.py

Runs tests/split_emulation.py (float64, three products of bf16 pieces in the
frame-rate convolutions, exact accumulation) on the `ragged` and `uniform`
inputs stored in tests/golden/train.npz and compares with the reference's
float64 gradients of train_grads_<k>.npz.  Needs neither the reference nor a
GPU.  Output (committed): tests/golden/train_split.npz -

  <case>/emulated_error       worst over tensors of max|g_emu - g64| / max|g64|
  <case>/emulated_loss_error  |loss_emu - loss64| / |loss64|
  <case>/exact_error          the same as emulated_error with the split switched
                              off: how far this restatement of the model is from
                              the stored reference (stored as float32: ~6e-8)
  adam/emulated               the losses of steps 0..5 of five Adam updates on
                              `ragged` under the emulation

The tests' bound is 4 x (emulated_error + ref32_error of train.npz).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import split_emulation  # noqa: E402
import train_data  # noqa: E402

torch.set_num_threads(1)


def worst(got, want):
    return max(np.abs(got[name] - want[name]).max() / np.abs(want[name]).max()
               for name in want)


def main():
    golden = train_data.golden()
    out = {}
    for case in ('ragged', 'uniform'):
        items = split_emulation.items_of(golden, case)
        want = train_data.gradients(case)
        want_loss = float(golden[f'{case}/loss'])
        state = split_emulation.load_state()
        assert set(want) == set(state)
        loss, exact = split_emulation.loss_and_gradients(
            state, items, split=False)
        out[f'{case}/exact_error'] = worst(exact, want)
        assert out[f'{case}/exact_error'] < 2e-7, out[f'{case}/exact_error']
        assert abs(loss - want_loss) <= 1e-12 * want_loss, (loss, want_loss)
        loss, emulated = split_emulation.loss_and_gradients(state, items)
        out[f'{case}/emulated_error'] = worst(emulated, want)
        out[f'{case}/emulated_loss_error'] = \
            abs(loss - want_loss) / abs(want_loss)
        print(case, {name: float(value) for name, value in out.items()
                     if name.startswith(case)},
              'ref32', float(golden[f'{case}/ref32_error']))
    ragged = split_emulation.items_of(golden, 'ragged')
    plain = split_emulation.adam_losses(ragged, split=False)
    assert np.abs(plain - golden['adam/float64']).max() < 1e-9, plain
    out['adam/emulated'] = split_emulation.adam_losses(ragged)
    print('adam', out['adam/emulated'], 'float64', golden['adam/float64'])
    path = os.path.join(HERE, 'train_split.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
