"""One training step of the convolution model on the GPU: forward with every
layer kept, masked loss, backward and Adam (`emphases/train/core.py:91-142`
without the loader, the loop, validation and logging around it)."""
from .core import (  # noqa: F401
    Batch, Trainer, adam_state_dict, check_batch, check_supported,
    gather_tables, initial_state, layer_names, parameter_offsets,
    write_checkpoint)
