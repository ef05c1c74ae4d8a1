"""The Transformer under the reference's dropout, restated in plain torch (any
dtype; the tests use float64 for the oracle and float32 for the bound): the
masked attention, one encoder layer and the whole model, with the five kinds
of mask of `emphases_amd/train/dropout.py` cut per utterance from the packed
plan.  Nothing here calls the library: `ops._frame_plan` is host arithmetic
(where each segment starts on the packed axis, and the leading dimension).

`tests/test_transformer_dropout.py` anchors it on the CPU: without masks it
reproduces `tests/golden/transformer_train*.npz`, with masks
`tests/golden/transformer_dropout*.npz` (the reference's modules with fixed
masks).
"""
import math

import numpy as np
import torch

from emphases_amd import config as cfg
from emphases_amd import ops
from emphases_amd import weights as weights_module
from emphases_amd.train import dropout as spec

CHANNELS, HEADS, DIM = 80, 2, 40
EPS = 1e-5
LAYER_NAMES = ('self_attn.in_proj_weight', 'self_attn.in_proj_bias',
               'self_attn.out_proj.weight', 'self_attn.out_proj.bias',
               'norm1.weight', 'norm1.bias', 'linear1.weight', 'linear1.bias',
               'linear2.weight', 'linear2.bias', 'norm2.weight', 'norm2.bias')


def packed_plan(counts):
    """(first packed column of every segment, ld) of segments back to back."""
    plan = ops._frame_plan(np.asarray(counts, dtype=np.int64))
    return [int(offset) for offset in plan.frame_off], int(plan.ld_frames)


class LayerMasks:
    """The four masks of one layer call over segments of `counts` positions,
    under (p, seed, stream_base, step): `attention(i)` bool [heads, T_i, T_i]
    (head, query, key) and `element(site, rows, i)` bool [rows, T_i], cut from
    the packed buffer [rows, ld]."""

    def __init__(self, counts, p, seed, stream_base, step):
        self.counts = [int(count) for count in counts]
        self.offsets, self.ld = packed_plan(self.counts)
        self.p, self.seed, self.base, self.step = p, seed, stream_base, step
        self.scale = float(spec.scale(p))
        self.whole = {}

    def attention(self, i):
        return torch.from_numpy(spec.attention_segment_mask(
            self.seed, self.base, self.step, self.p, self.ld, HEADS,
            self.offsets[i], self.counts[i]))

    def element(self, site, rows, i):
        key = (site, rows)
        if key not in self.whole:
            self.whole[key] = spec.keep_mask(
                self.seed, self.base + site, self.step, rows * self.ld,
                self.p).reshape(rows, self.ld)
        first = self.offsets[i]
        return torch.from_numpy(
            self.whole[key][:, first:first + self.counts[i]].copy())


def attention(q, k, v, keep=None, scale=1., wrong=None):
    """[80, T] of one segment: softmax attention per head with the weights
    multiplied by `keep` [heads, T, T] (query, key) and `scale`.  `wrong`
    restates a MISTAKE, for the tests that show the bound can fail:
    'transposed' takes the mask with query and key exchanged, 'dv' leaves the
    mask out of the gradient of V alone (the forward value is the right one).
    """
    outs = []
    for head in range(HEADS):
        rows = slice(head * DIM, (head + 1) * DIM)
        scores = q[rows].t() @ k[rows] / math.sqrt(DIM)
        weights = torch.softmax(scores, dim=1)
        values = v[rows].t()
        if keep is None:
            outs.append((weights @ values).t())
            continue
        mask = keep[head].t() if wrong == 'transposed' else keep[head]
        kept = weights * mask.to(weights.dtype) * scale
        if wrong == 'dv':
            plain = weights.detach() @ values
            outs.append((kept @ values.detach() + plain - plain.detach()).t())
        else:
            outs.append((kept @ values).t())
    return torch.cat(outs)


def _drop(x, masks, site, i):
    if masks is None:
        return x
    keep = masks.element(site, x.shape[0], i)
    return x * keep.to(x.dtype) * masks.scale


def _norm(x, weight, bias):
    return torch.nn.functional.layer_norm(
        x.t(), (x.shape[0],), weight, bias, EPS).t()


def layer(x, parameters, counts, masks=None, wrong=None):
    """One post-LN encoder layer (`LAYER_NAMES` order) over segments back to
    back, x [80, sum T] -> [80, sum T], each segment alone."""
    (in_w, in_b, out_w, out_b, norm1_w, norm1_b, ff1_w, ff1_b, ff2_w, ff2_b,
     norm2_w, norm2_b) = parameters
    outs, first = [], 0
    for i, count in enumerate(counts):
        part = x[:, first:first + count]
        first += count
        q, k, v = (in_w @ part + in_b[:, None]).split(CHANNELS)
        if masks is None:
            attended = attention(q, k, v)
        else:
            attended = attention(q, k, v, masks.attention(i), masks.scale,
                                 wrong)
        projected = _drop(out_w @ attended + out_b[:, None], masks, 1, i)
        normed1 = _norm(part + projected, norm1_w, norm1_b)
        hidden = _drop(torch.relu(ff1_w @ normed1 + ff1_b[:, None]), masks, 2,
                       i)
        fed = _drop(ff2_w @ hidden + ff2_b[:, None], masks, 3, i)
        outs.append(_norm(normed1 + fed, norm2_w, norm2_b))
    return torch.cat(outs, dim=1)


def _stack(x, state, prefix, config, counts, dropout):
    """`Transformer` (`transformer.py:13-30`) over segments back to back."""
    table = torch.from_numpy(weights_module.positional_encoding(
        cfg.MAX_POSITIONS, config.channels)).to(x.dtype).t()
    x = x + torch.cat([table[:, :count] for count in counts], dim=1)
    if dropout is not None:
        seed, step = dropout
        p = spec.TRANSFORMER_POSITION_DROPOUT
        keep = spec.keep_mask(
            seed, spec.transformer_stream(config, prefix), step, x.numel(),
            p).reshape(x.shape)
        x = x * torch.from_numpy(keep).to(x.dtype) * float(spec.scale(p))
    for index in range(config.layers):
        masks = None
        if dropout is not None:
            masks = LayerMasks(
                counts, spec.TRANSFORMER_LAYER_DROPOUT, seed,
                spec.transformer_stream(config, prefix, index, 'attention'),
                step)
        x = layer(x, [state[f'{prefix}.model.layers.{index}.{name}']
                      for name in LAYER_NAMES], counts, masks)
    return x


def _conv(x, weight, bias, counts):
    outs, first = [], 0
    for count in counts:
        outs.append(torch.nn.functional.conv1d(
            x[None, :, first:first + count], weight, bias, padding='same')[0])
        first += count
    return torch.cat(outs, dim=1)


def model(state, config, features, frames, bounds, words, targets, dtype,
          dropout=None):
    """(loss, logits [sum W], name -> gradient) of the model of `state` (name
    -> array) on utterances back to back, every utterance alone; `dropout` =
    (seed, steps) draws the reference's dropouts as specified masks."""
    frames = [int(count) for count in frames]
    words = [int(count) for count in words]
    leaves = {name: torch.from_numpy(np.asarray(value)).to(dtype)
              .requires_grad_(True) for name, value in state.items()}
    x = _conv(torch.from_numpy(np.asarray(features)).to(dtype),
              leaves['input_layer.weight'], leaves['input_layer.bias'], frames)
    x = _stack(x, leaves, 'frame_encoder', config, frames, dropout)
    pooled, first_frame, first_word = [], 0, 0
    for count, own in zip(frames, words):
        for start, end in np.asarray(bounds)[:, first_word:first_word + own].T:
            span = x[:, first_frame + int(start):first_frame + int(end)]
            if config.downsample_method == 'sum':
                pooled.append(span.sum(dim=1))
            else:
                assert config.downsample_method == 'max'
                pooled.append(span.max(dim=1).values)
        first_frame += count
        first_word += own
    x = torch.stack(pooled, dim=1)
    if config.has_decoder:
        x = _stack(x, leaves, 'word_decoder', config, words, dropout)
    logits = _conv(x, leaves['output_layer.weight'],
                   leaves['output_layer.bias'], words)[0]
    loss = torch.nn.functional.binary_cross_entropy_with_logits(
        logits, torch.from_numpy(np.asarray(targets)).to(dtype))
    loss.backward()
    return (float(loss.detach().double()), logits.detach().double().numpy(),
            {name: leaf.grad.double().numpy() for name, leaf in leaves.items()})
