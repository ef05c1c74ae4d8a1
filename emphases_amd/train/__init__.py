"""Training the convolution model on the GPU (`emphases.train`): the step -
forward with every layer kept, masked loss, backward and Adam
(`emphases/train/core.py:91-142`) - and the loop around it - resume, train,
validate, save (`train/core.py:13-307`) - fed by `emphases_amd.data`."""
from .core import (  # noqa: F401
    PRECISIONS, Batch, Trainer, adam_state_dict, check_batch,
    check_precision, check_supported, checkpoint_names, gather_tables,
    initial_state,
    layer_names, parameter_offsets, split_layer_names, split_pack_tables,
    write_checkpoint)
from . import dropout  # noqa: F401
from .loop import evaluate, latest_path, train  # noqa: F401
