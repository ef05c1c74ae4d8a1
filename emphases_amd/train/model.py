"""The reference's `emphases.Model` for the convolution architecture
(`emphases/model/core.py:11-138`, `model/layers/convolution.py:13-37`) as a
`torch.nn.Module` on the two differentiable operator seams
(`torch.ops.emphases_amd.conv1d_same_act` / `segment_reduce`): the general
training path next to the fused `train.Trainer`, which stays specialised to
Conv1d(., 80, 3) + ReLU + 'intermediate' + 'sum' / 'average'.

Every layer, the output layer included, is the op: every utterance runs alone
with its own zero halo, exactly as inference runs it, and the same batch gives
the same bits.  `Config.dropout` inserts `torch.nn.Dropout` modules, which draw
from torch's own generator - not from the trainer's Philox specification
(`train/dropout.py`).
"""
import collections

import torch

from .. import config as cfg
from .. import core as api
from .. import ops  # noqa: F401  (registers torch.ops.emphases_amd)
from .. import weights as weights_module

MAX_CHANNELS = 128   # emph_conv_weight_grad_any, emph_segment_reduce


def check_model_supported(config):
    """NotImplementedError, naming the field, for a configuration `TorchModel`
    does not cover."""
    def refuse(field, supported):
        raise NotImplementedError(
            f'TorchModel supports {field} {supported} only, not '
            f'{field}={getattr(config, field)!r}')
    if config.method != 'neural':
        refuse('method', "'neural'")
    if config.architecture != 'convolution':
        refuse('architecture', "'convolution'")
    if config.downsample_location not in ('intermediate', 'loss'):
        # 'inference' needs `upsample` of the targets; the padded-axis pooling
        # of 'input' depends on the batch's longest word
        refuse('downsample_location', "'intermediate' or 'loss'")
    if config.loss not in ('bce', 'mse'):
        refuse('loss', "'bce' or 'mse'")
    if config.channels % 16 or not 16 <= config.channels <= MAX_CHANNELS:
        refuse('channels', f'a multiple of 16 up to {MAX_CHANNELS}')
    if not 0 <= config.layers <= 16:
        refuse('layers', '0..16')
    if not config.mel_feature:
        refuse('mel_feature', 'True (80..83 input features)')


def initial_model_state(config=cfg.DEFAULT, seed=0):
    """`train.initial_state` for every configuration of `TorchModel`: bitwise
    the parameters of the reference's `emphases.Model()` after
    `torch.manual_seed(seed)` (`torch.nn.Conv1d` modules built on the CPU in
    the reference's construction order).  The caller's generator is left as
    it was."""
    check_model_supported(config)
    state = collections.OrderedDict()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)

        def conv(name, c_in, c_out, kernel_size):
            module = torch.nn.Conv1d(
                c_in, c_out, kernel_size=kernel_size, padding='same')
            state[f'{name}.weight'] = module.weight.detach().numpy().copy()
            state[f'{name}.bias'] = module.bias.detach().numpy().copy()
        conv('input_layer', config.num_features, config.channels,
             config.encoder_kernel_size)
        stacks = [('frame_encoder', config.encoder_kernel_size)]
        if config.has_decoder:
            stacks.append(('word_decoder', config.decoder_kernel_size))
        for prefix, kernel_size in stacks:
            for i in range(config.layers):
                conv(f'{prefix}.{2 * i}', config.channels, config.channels,
                     kernel_size)
        conv('output_layer', config.channels, 1, config.decoder_kernel_size)
    assert list(state) == list(weights_module.parameter_shapes(config))
    return state


def loss_fn(logits, targets, form='bce'):
    """The reference's loss over the valid words (`train/core.py:315-353`) as
    plain torch: the mean of binary_cross_entropy_with_logits ('bce') or of
    the squared error ('mse')."""
    if form == 'bce':
        return torch.nn.functional.binary_cross_entropy_with_logits(
            logits, targets)
    if form == 'mse':
        return torch.nn.functional.mse_loss(logits, targets)
    raise ValueError(f'Loss {form} is not defined')


class _Conv(torch.nn.Module):
    """The parameters of one `torch.nn.Conv1d(c_in, c_out, k, 'same')`."""

    def __init__(self, weight, bias):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.from_numpy(weight.copy()))
        self.bias = torch.nn.Parameter(torch.from_numpy(bias.copy()))


class _Stack(torch.nn.Module):
    """`Convolution` (`convolution.py:13-37`): layer i is module 2 i (3 i under
    `Config.dropout`, followed by its `torch.nn.Dropout` at 3 i + 2)."""

    def __init__(self, config, prefix, state):
        super().__init__()
        self.activation = config.activation
        self.stride = 2 if config.dropout is None else 3
        self.layers = config.layers
        for i in range(config.layers):
            self.add_module(str(i * self.stride), _Conv(
                state[f'{prefix}.{2 * i}.weight'],
                state[f'{prefix}.{2 * i}.bias']))
            if config.dropout is not None:
                self.add_module(str(i * self.stride + 2),
                                torch.nn.Dropout(float(config.dropout)))

    def forward(self, x, cu):
        for i in range(self.layers):
            conv = getattr(self, str(i * self.stride))
            x = torch.ops.emphases_amd.conv1d_same_act(
                x, conv.weight, conv.bias, cu, self.activation)
            if self.stride == 3:
                x = getattr(self, str(i * self.stride + 2))(x)
        return x


class TorchModel(torch.nn.Module):
    """`TorchModel(config, checkpoint=None, seed=0)`; `forward(features [C_in,
    sum T], cu_frames, bounds [2, sum W], cu_words) -> logits [sum W]`, the
    utterances back to back (`cu_*`: N + 1 prefix sums, on the host).

    The parameters carry the reference's names and order
    (`weights.parameter_shapes`; the `3 i` numbering under `Config.dropout`):
    `state_dict()` is read by `weights.load` and by every inference entry
    point's `checkpoint=`.  Without a checkpoint they are bitwise
    `initial_model_state(config, seed)`.  checkpoint: a state dict or a file
    `weights.load` reads."""

    def __init__(self, config=None, checkpoint=None, seed=0):
        super().__init__()
        self.config = config = config or api.active_config()
        check_model_supported(config)
        if checkpoint is None:
            state = initial_model_state(config, seed)
        else:
            state = weights_module.load(checkpoint, config)
        self.input_layer = _Conv(
            state['input_layer.weight'], state['input_layer.bias'])
        self.frame_encoder = _Stack(config, 'frame_encoder', state)
        if config.has_decoder:
            self.word_decoder = _Stack(config, 'word_decoder', state)
        self.output_layer = _Conv(
            state['output_layer.weight'], state['output_layer.bias'])

    def forward(self, features, cu_frames, bounds, cu_words):
        conv = torch.ops.emphases_amd.conv1d_same_act
        x = conv(features, self.input_layer.weight, self.input_layer.bias,
                 cu_frames, 'none')
        x = self.frame_encoder(x, cu_frames)
        x = torch.ops.emphases_amd.segment_reduce(
            x, bounds, cu_frames, cu_words, self.config.downsample_method)
        if self.config.has_decoder:
            x = self.word_decoder(x, cu_words)
        x = conv(x, self.output_layer.weight, self.output_layer.bias,
                 cu_words, 'none')
        return x[0]

