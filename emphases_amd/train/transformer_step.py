"""The training step of the Transformer architecture behind the loop's
interface: `TransformerTrainer` is to `TransformerModel` what `Trainer` is to
the convolution model for `loop.train`, `loop.evaluate` and `data.Loader`.

The gradient path is `TransformerModel` under autograd, exactly as it stands
(`train/transformer_model.py`: the differentiable operator seams, HIP forward
and backward).  The trainer owns what the loop needs around it:

* the state, as the fused steps keep it (`core._State`): parameters, both
  Adam moments and the step count in flat device buffers in
  `weights.parameter_shapes` order; the model's `nn.Parameter`s are views of
  the flat parameter buffer;
* the batch: the packed `train.Batch` of `Loader` and `prepare` becomes the
  model's back-to-back layout by one gather per tensor, through column
  indices that `metadata(plan)` uploads once per batch;
* the optimizer: `emph_adam_step_gathered` reads every gradient where
  autograd left it and updates the flat buffers - two launches for the 148
  tensors of 6 + 6 layers, no copy into a flat gradient, nothing uploaded;
* the checkpoint of `_State.save`, which every inference entry point reads and
  from which the same class resumes, moments and step count included.

The version counter.  The optimizer kernel writes the parameters through raw
addresses, which does not advance a tensor's `_version` - and the ops tell a
weight that is being trained from one that is not, and a stale device pack
from a current one, by `_version` alone (`ops/packs.py`).  The parameters are
views of one buffer and share its counter, so after every update the trainer
advances it once (`torch.autograd.graph.increment_version`, which launches
nothing).  Without it step 2 would run on the packs of step 1.

The same rule makes a resumed run continue the uninterrupted one bit for bit:
weights that were never updated take the ops' inference path (host packs, the
fused layer), updated ones the unfused path on device packs, and the two
round differently.  A trainer restored at a step count above zero therefore
hands its parameters to `ops.mark_trained` before the first forward: they
are weights in training, as they were when they were saved.
"""
import collections
import math

import numpy as np
import torch

from .. import core as api
from .. import packed
from .. import runtime
from ..ops import packs
from . import core
from .model import loss_fn
from .transformer_model import (
    ALL_LOCATIONS, TransformerLocationsModel, TransformerModel,
    check_locations_supported, check_reference_dropout,
    check_transformer_supported, initial_transformer_state)


class TransformerTrainer(core._State):
    """`TransformerTrainer(...).step(*batch[:5])` is one iteration of the
    reference's loop (`train/core.py:105-142`) for ARCHITECTURE =
    'transformer': `TransformerModel` in training mode, `loss_fn`, `backward`
    and one Adam update.  `Trainer`'s interface (`device`, `config`, `steps`,
    `metadata`, `prepare`, `logits`, `loss_and_gradients`, `step`,
    `state_dict`, `optimizer_state_dict`, `save`) on `_State`, the state,
    batch preparation and checkpoint it shares with the fused steps.

    What it covers is what `TransformerModel` covers (`check`):
    downsample_location 'intermediate' or 'loss', every downsample_method, 80
    channels, 2 heads, precision 'f32' or 'bf16x3', and
    `reference_dropout=True` (the reference's five dropouts as specified
    masks of (`seed`, site, `steps`)) at 'f32'.  `steps` counts the updates
    and is the step of the dropout stream: a step can be repeated, and a
    resumed run continues the same masks."""

    _model_class = TransformerModel
    _initial_state = staticmethod(initial_transformer_state)

    @staticmethod
    def check(config, precision='f32', reference_dropout=False):
        """Every refusal, before a GPU is needed: `check_transformer_supported`
        by field name, `check_precision`, and `TransformerModel`'s refusal of
        `reference_dropout=True` off 'f32'.  Returns the precision."""
        check_transformer_supported(config)
        precision = core.check_precision(precision)
        check_reference_dropout(precision, reference_dropout)
        return precision

    def __init__(self, config=None, checkpoint=None, gpu=None, lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, seed=0, precision='f32',
                 reference_dropout=False):
        """checkpoint: None (`initial_transformer_state(config, seed)`), a
        state dict, or a file `weights.load` reads; a file written by `save`
        also restores the Adam moments and the step count.  `seed`: of the
        initialisation and of the dropout masks.  `precision` and
        `reference_dropout` are not part of the checkpoint."""
        self.config = config = config or api.active_config()
        self.precision = self.check(config, precision, reference_dropout)
        self.reference_dropout = bool(reference_dropout)
        self._settings(lr, betas, eps, seed)
        state, optimizer = self._read(checkpoint, self._initial_state)
        self.offsets, self.count = core.parameter_offsets(config)
        self.device = runtime.require_gpu(gpu)
        self.lib = runtime.library()
        with torch.cuda.device(self.device):
            self._allocate(state, optimizer)
            self.model = self._model_class(
                config, state, seed, self.reference_dropout,
                self.precision).to(self.device)
        self._tensors = self._adopt_parameters()
        # the table of emph_adam_step_gathered but for the gradients' addresses
        sizes = [int(np.prod(shape)) for _, shape in self.offsets.values()]
        self._firsts = np.array(
            [first for first, _ in self.offsets.values()], dtype=np.int64)
        self._sizes = np.array(sizes, dtype=np.int64)
        self._addresses = np.zeros(len(sizes), dtype=np.uint64)
        self._counts = np.zeros(len(sizes), dtype=np.int64)
        if self.steps:
            # (module docstring: restored weights are weights in training)
            packs.mark_trained(self._tensors, base=self.parameters)

    def _adopt_parameters(self):
        """Replaces every parameter of the model by a view of the flat buffer
        (a `Parameter` made of a view shares the buffer's version counter);
        returns them in `weights.parameter_shapes` order."""
        named = dict(self.model.named_parameters())
        if list(named) != list(self.offsets):
            raise RuntimeError(
                'TransformerModel does not hold its parameters in '
                'weights.parameter_shapes order')
        tensors = []
        for name in self.offsets:
            owner, _, leaf = name.rpartition('.')
            parameter = torch.nn.Parameter(self._view(self.parameters, name))
            setattr(self.model.get_submodule(owner), leaf, parameter)
            tensors.append(parameter)
        before = tensors[-1]._version
        torch.autograd.graph.increment_version(self.parameters)
        if tensors[-1]._version != before + 1 or \
                tensors[0].data_ptr() != self.parameters.data_ptr():
            raise RuntimeError(
                "this torch does not advance a view's version with its "
                "base's: the ops would run on stale weight packs")
        return tensors

    ###########################################################################
    # State
    ###########################################################################

    def state_dict(self):
        """The parameters under the reference's names and shapes (CPU)."""
        flat = self.parameters.cpu()
        return collections.OrderedDict(
            (name, self._view(flat, name).clone()) for name in self.offsets)

    ###########################################################################
    # Batches
    ###########################################################################

    def metadata(self, plan):
        """What turns the packed layout of `plan` into the model's
        back-to-back one (`Batch.meta`): the prefix sums `cu_frames` and
        `cu_words` and the utterance-relative `bounds` [2, sum W] on the host,
        where the ops read them, and the packed column of every frame and of
        every word (`frame_columns`, `word_columns`) on the device, in one
        copy."""
        prefix = lambda counts: torch.from_numpy(np.concatenate(  # noqa: E731
            [[0], np.cumsum(counts)]).astype(np.int64))
        host = np.concatenate([
            packed.column_index(plan.frame_off, plan.frames),
            plan.word_columns()]).astype(np.int64)
        with torch.cuda.device(self.device):
            columns = torch.from_numpy(host).to(self.device)
        return {
            'cu_frames': prefix(plan.frames), 'cu_words': prefix(plan.words),
            'bounds': torch.from_numpy(np.ascontiguousarray(
                plan.segment_bounds, dtype=np.int64)),
            'frame_columns': columns[:plan.total_frames],
            'word_columns': columns[plan.total_frames:], '_buffer': columns}

    def _batch(self, arguments):
        if len(arguments) == 1 and isinstance(arguments[0], core.Batch):
            if 'frame_columns' not in arguments[0].meta:
                raise ValueError(
                    'the batch carries no column indices: prepare it with '
                    "this trainer (architecture='transformer')")
            return arguments[0]
        return self.prepare(*arguments)

    def _inputs(self, batch):
        """(the model's arguments, the targets [sum W]) of a prepared batch:
        one gather each off the packed axes."""
        meta = batch.meta
        features = batch.features.index_select(1, meta['frame_columns'])
        targets = batch.targets.index_select(0, meta['word_columns'])
        return (features, meta['cu_frames'], meta['bounds'],
                meta['cu_words']), targets

    ###########################################################################
    # API
    ###########################################################################

    def logits(self, batch):
        """The model's logits of a prepared `Batch` in eval mode (nothing is
        dropped, no gradient, no update): float32 [total_words] on the
        device, the words of the items in order."""
        batch = self._batch((batch,))
        with torch.cuda.device(self.device), torch.no_grad():
            self.model.eval()
            return self.model(*self._inputs(batch)[0])

    def _loss_backward(self, batch):
        """The training forward at the dropout stream's step `steps`, the loss
        and `backward`: the loss (detached); the gradients are the
        parameters' `.grad`."""
        inputs, targets = self._inputs(batch)
        self.model.train()
        self.model.steps = self.steps
        for parameter in self._tensors:
            parameter.grad = None
        loss = loss_fn(self.model(*inputs), targets, self.config.loss)
        loss.backward()
        return loss.detach()

    def loss_and_gradients(self, *batch):
        """(loss, {name: gradient}) of a collated batch (or a prepared
        `Batch`), device tensors; the parameters are left as they are."""
        batch = self._batch(batch)
        with torch.cuda.device(self.device):
            loss = self._loss_backward(batch)
        gradients = collections.OrderedDict()
        for name, parameter in zip(self.offsets, self._tensors):
            gradients[name], parameter.grad = parameter.grad, None
        return loss, gradients

    def step(self, *batch):
        """Forward, loss, backward and Adam on the current stream; returns the
        loss (before the update) as a 0-dim device tensor without
        synchronising."""
        batch = self._batch(batch)
        with torch.cuda.device(self.device):
            loss = self._loss_backward(batch)
            # (a parameter the loss does not reach has no gradient and, as in
            # torch.optim.Adam, no update: a tensor of zero elements)
            kept = []
            for index, parameter in enumerate(self._tensors):
                gradient = parameter.grad
                if gradient is None:
                    self._addresses[index] = self._counts[index] = 0
                    continue
                if gradient.dtype != torch.float32 or \
                        not gradient.is_contiguous():
                    gradient = gradient.to(torch.float32).contiguous()
                kept.append(gradient)
                self._addresses[index] = gradient.data_ptr()
                self._counts[index] = self._sizes[index]
            self.steps += 1
            beta1, beta2 = self.betas
            correction1 = 1. - beta1 ** self.steps
            correction2 = 1. - beta2 ** self.steps
            runtime.check(self.lib.emph_adam_step_gathered(
                self.parameters.data_ptr(), self._addresses.ctypes.data,
                self._firsts.ctypes.data, self._counts.ctypes.data,
                len(self._tensors), self.exp_avg.data_ptr(),
                self.exp_avg_sq.data_ptr(), beta1, beta2,
                self.lr / correction1, math.sqrt(correction2), self.eps,
                runtime.stream()), 'emph_adam_step_gathered')
            torch.autograd.graph.increment_version(self.parameters)
            for parameter in self._tensors:
                parameter.grad = None
        return loss


def _initial_locations_state(config, seed=0):
    return initial_transformer_state(config, seed, ALL_LOCATIONS)


class TransformerLocationsTrainer(TransformerTrainer):
    """`TransformerTrainer` around `TransformerLocationsModel`: all four
    DOWNSAMPLE_LOCATIONs behind the same interface, state, checkpoints and
    resume.  At 'inference' the training logits are at frame rate, and the
    batch carries the frame targets: `emph_upsample` of the word targets on
    the packed layout (`config.upsample_method`; clamped to [0, 1] under
    'linear', as the reference's loss clamps them), formed once per batch
    and kept with it; every utterance needs a word.  `loss_fn` serves
    unchanged.  `logits` is the eval-mode model, word rate at every
    location."""

    _model_class = TransformerLocationsModel
    _initial_state = staticmethod(_initial_locations_state)

    @staticmethod
    def check(config, precision='f32', reference_dropout=False):
        """Every refusal, before a GPU is needed, by field name: the
        parent's but for the location, and at 'input' `precision='bf16x3'`,
        `reference_dropout=True` and `Config.dropout`."""
        precision = core.check_precision(precision)
        check_locations_supported(config, precision, reference_dropout)
        return precision

    def metadata(self, plan):
        meta = super().metadata(plan)
        if self.config.downsample_location == 'inference':
            if any(int(count) < 1 for count in plan.words):
                raise ValueError(
                    "downsample_location 'inference' upsamples the targets: "
                    'every utterance needs a word')
            request = (runtime.AXIS_FRAMES, 64)
            with torch.cuda.device(self.device):
                meta['_padded'] = packed.Padded(plan, self.device, [request])
            meta['_plan'] = plan
        return meta

    def _frame_targets(self, batch):
        """[sum T]: the word targets spread over the frames, once per batch."""
        meta = batch.meta
        if '_frame_targets' not in meta:
            plan, view = meta['_plan'], meta['_padded'].view
            tiles = view(('tiles', runtime.AXIS_FRAMES, 64))
            out = torch.zeros((1, plan.ld_frames), dtype=torch.float32,
                              device=self.device)
            method = self.config.upsample_method
            runtime.check(self.lib.emph_upsample(
                batch.targets.data_ptr(), plan.ld_words,
                view('bounds').data_ptr(), out.data_ptr(), plan.ld_frames, 1,
                view('table').data_ptr(), tiles.data_ptr(),
                tiles.numel() // runtime.TILE_FIELDS,
                runtime.UPSAMPLE_METHODS[method], runtime.stream()),
                'emph_upsample')
            if method == 'linear':
                out = out.clamp_(0., 1.)
            meta['_frame_targets'] = out[0].index_select(
                0, meta['frame_columns'])
        return meta['_frame_targets']

    def _loss_backward(self, batch):
        self.model.train()                  # (`_inputs` asks which targets)
        return super()._loss_backward(batch)

    def _inputs(self, batch):
        inputs, targets = super()._inputs(batch)
        if self.config.downsample_location == 'inference' and \
                self.model.training:
            targets = self._frame_targets(batch)
        return inputs, targets
