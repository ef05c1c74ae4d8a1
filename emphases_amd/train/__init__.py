"""Training on the GPU (`emphases.train`): the step of the convolution model -
forward with every layer kept, masked loss, backward and Adam
(`emphases/train/core.py:91-142`) - and the loop around it - resume, train,
validate, save (`train/core.py:13-307`) - fed by `emphases_amd.data`; and
`TorchModel`, the same architecture as a `torch.nn.Module` on the
differentiable operator seams for the configurations the fused steps refuse.
`TransformerModel` is the Transformer architecture on the same seams, and
`TransformerTrainer` the step around it with the fused steps' interface: the
fused steps and their dispatch (`step_class` ... `make_trainer`) refuse the
architecture, and so does `train` unless it is given
`trainer=TransformerTrainer`.  `TransformerLocationsModel` and
`TransformerLocationsTrainer` are the same pair at all four locations
('input' through `ops.encoder_layer_padded`, 'inference' with the frame-rate
head and upsampled targets), a second opt-in: the first pair keeps refusing
those two.

The fused steps, one class per `downsample_location` and one behind them:
`Trainer` ('intermediate'), `EncoderTrainer` ('inference' and 'loss', no word
decoder), `PieceTrainer` ('input', every word a padded sequence of its own)
and `GridTrainer` (the rest of the reference's hyperparameter grid at
'intermediate').  `step_class` is the one dispatch, with every check made and
nothing constructed; `select_trainer` builds what it names, `trainer_for` the
same without the grid step, `make_trainer` without the piece step either."""
from .core import (  # noqa: F401
    PRECISIONS, Batch, EncoderTrainer, GridTrainer, PieceTrainer, Trainer,
    adam_state_dict, check_batch, check_encoder_supported,
    check_grid_supported, check_pieces_supported, check_precision,
    check_supported, checkpoint_names, gather_tables, initial_state,
    layer_names, make_trainer, parameter_offsets, select_trainer,
    split_layer_names, split_pack_tables, step_class, trainer_for,
    write_checkpoint)
from . import dropout  # noqa: F401
from .model import (  # noqa: F401
    TorchModel, check_model_supported, initial_model_state, loss_fn)
from .transformer_model import (  # noqa: F401
    TransformerLocationsModel, TransformerModel, check_locations_supported,
    check_transformer_supported, initial_transformer_state)
from .transformer_step import (  # noqa: F401
    TransformerLocationsTrainer, TransformerTrainer)
from .loop import evaluate, latest_path, train  # noqa: F401
