"""The golden vectors of the training step under dropout
(tests/golden/dropout.npz and dropout_grads_<k>.npz, written by
tests/golden/generate_dropout.py).  The inputs are the `ragged` case of
tests/train_data.py."""
import functools
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ('p10', 'p50')


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLDEN, 'dropout.npz')) as archive:
        return {name: archive[name] for name in archive.files}


def settings(case):
    """(p, seed, step) of a case."""
    data = golden()
    return (float(data[f'{case}/p']), int(data[f'{case}/seed']),
            int(data[f'{case}/step']))


@functools.lru_cache(maxsize=None)
def gradients(case):
    """{internal parameter name: the reference's float64 gradient (stored as
    float32)}: every tensor of `p10`, the VARIANT_TENSORS of `p50`."""
    prefix = f'{case}/grad/'
    found = {name[len(prefix):]: value.astype(np.float64)
             for name, value in golden().items() if name.startswith(prefix)}
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'dropout_grads_*.npz'))):
        with np.load(path) as archive:
            for name in archive.files:
                if name.startswith(case + '/'):
                    found[name[len(case) + 1:]] = \
                        archive[name].astype(np.float64)
    return found
