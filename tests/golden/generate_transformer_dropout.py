"""Capture golden vectors of the reference's Transformer in TRAINING mode, its
five dropouts drawn as the package's specified masks, for
`emphases_amd.train.TransformerModel(reference_dropout=True)`.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_transformer_dropout.py

Imports the UNMODIFIED reference `emphases` through `generate_transformer.py`
(whose batch, configs and helpers it shares) and builds its `Model` under
ARCHITECTURE = 'transformer', LAYERS = 2 in `.train()` mode from the
reference's own initialisation under `torch.manual_seed(seed)`.  On the
INSTANCE, per stack,

  * `position.dropout` and each layer's `dropout`, `dropout1`, `dropout2` are
    replaced by a module that multiplies by a fixed mask and by
    float32(1 / (1 - p)) (`FixedMask`);
  * each layer's `self_attn` is replaced by a module over the SAME parameters
    (same names) that evaluates multi-head attention in plain torch with the
    mask on the softmax weights (`MaskedAttention`).

The masks are the package's specification (`emphases_amd/train/dropout.py`,
numpy) under (seed, `transformer_stream`, step = STEP): the element-wise ones
`keep_mask` over the layer's packed buffer [rows, ld] cut at the utterance's
columns, the positional one `keep_mask` over [C, sum T] back to back, the
attention's `attention_keep_mask` of (head, packed query column); the packed
plan (where each utterance starts, ld) is `ops._frame_plan`'s host arithmetic.
p is 0.1 everywhere (`transformer.py:17` and torch's default at
`transformer.py:19-22`).

Every utterance runs ALONE, weighted n_i / N, in float64 and in float32.  With
keep-everything masks the patched instance in float64 must equal the
unpatched `.eval()` instance to 1e-12 (asserted; `keep_all_error` stored).
'loss' + 'max' runs under `generate_transformer.py`'s `no_near_ties` and
moves to the next seed otherwise.

tests/golden/transformer_dropout.npz: per config the seed, the step, the loss
and the logits (float64), `ref32_error` and `keep_all_error`.
tests/golden/transformer_dropout_grads_<config>.npz: the float64 gradients,
stored rounded to float32.  The GPU box never runs this script.
"""
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]

import generate_transformer as base  # noqa: E402  (paths, stubs, the reference)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases  # noqa: E402  (the reference)

import emphases_amd  # noqa: E402
from emphases_amd import ops  # noqa: E402
from emphases_amd.train import dropout as spec  # noqa: E402

STEP = 3
CHANNELS, HEADS, DIM = 80, 2, 40
CURRENT = [None]            # the utterance that is running


def scale_of(p):
    return float(spec.scale(p)) if p else 1.


class FixedMask(torch.nn.Module):
    """In place of a `torch.nn.Dropout` on [T, 1, C]: x * mask * scale, with
    `masks[u]` bool [C, T_u]."""

    def __init__(self, masks, p):
        super().__init__()
        self.masks, self.scale = masks, scale_of(p)

    def forward(self, x):
        mask = torch.from_numpy(self.masks[CURRENT[0]]).to(x.dtype)
        return x * mask.t()[:, None, :] * self.scale


class MaskedAttention(torch.nn.Module):
    """In place of an `nn.MultiheadAttention` (sequence first, one utterance,
    no padding), over its parameters: softmax(Q K^T / sqrt(d)) o mask * scale
    per head, `masks[u]` bool [heads, T_u, T_u] (head, query, key)."""
    batch_first = False
    _qkv_same_embed_dim = True

    def __init__(self, inner, masks, p):
        super().__init__()
        self.in_proj_weight, self.in_proj_bias = \
            inner.in_proj_weight, inner.in_proj_bias
        self.out_proj = inner.out_proj
        self.num_heads, self.embed_dim = inner.num_heads, inner.embed_dim
        assert (self.num_heads, self.embed_dim) == (HEADS, CHANNELS)
        self.masks, self.scale = masks, scale_of(p)

    def forward(self, query, key, value, attn_mask=None,
                key_padding_mask=None, need_weights=False, is_causal=False):
        assert query is key and key is value and attn_mask is None
        assert key_padding_mask is None or not bool(key_padding_mask.any())
        x = query[:, 0]                                             # [T, C]
        q, k, v = torch.nn.functional.linear(
            x, self.in_proj_weight, self.in_proj_bias).split(CHANNELS, dim=1)
        mask = torch.from_numpy(self.masks[CURRENT[0]]).to(x.dtype)
        outs = []
        for head in range(HEADS):
            columns = slice(head * DIM, (head + 1) * DIM)
            weights = torch.softmax(
                q[:, columns] @ k[:, columns].t() / DIM ** 0.5, dim=1)
            outs.append((weights * mask[head] * self.scale) @ v[:, columns])
        return self.out_proj(torch.cat(outs, dim=1))[:, None], None


def patch(net, config, counts_of, seed, keep_all=False):
    """Replaces the dropouts of both stacks of `net`; `counts_of[stack]` the
    segment lengths of the batch on that stack's axis."""
    for stack in spec.TRANSFORMER_STACKS:
        if not hasattr(net, stack):
            continue
        counts = [int(count) for count in counts_of[stack]]
        plan = ops._frame_plan(np.asarray(counts, dtype=np.int64))
        offsets, ld = [int(o) for o in plan.frame_off], int(plan.ld_frames)
        starts = np.concatenate([[0], np.cumsum(counts)])
        module = getattr(net, stack)
        p = 0. if keep_all else spec.TRANSFORMER_POSITION_DROPOUT
        whole = spec.keep_mask(
            seed, spec.transformer_stream(config, stack), STEP,
            CHANNELS * int(starts[-1]), p).reshape(CHANNELS, -1)
        module.position.dropout = FixedMask(
            [whole[:, starts[u]:starts[u + 1]].copy()
             for u in range(len(counts))], p)
        p = 0. if keep_all else spec.TRANSFORMER_LAYER_DROPOUT
        for index, layer in enumerate(module.model.layers):
            first = spec.transformer_stream(config, stack, index, 'attention')
            assert first + 3 == spec.transformer_stream(
                config, stack, index, 'residual2')
            layer.self_attn = MaskedAttention(layer.self_attn, [
                spec.attention_segment_mask(
                    seed, first, STEP, p, ld, HEADS, offsets[u], counts[u])
                for u in range(len(counts))], p)
            for site, name in ((1, 'dropout1'), (2, 'dropout'),
                               (3, 'dropout2')):
                whole = spec.keep_mask(
                    seed, first + site, STEP, CHANNELS * ld, p).reshape(
                        CHANNELS, ld)
                setattr(layer, name, FixedMask(
                    [whole[:, offsets[u]:offsets[u] + counts[u]].copy()
                     for u in range(len(counts))], p))


def accumulate(net, items, dtype, watch=None):
    """`generate_transformer.accumulate`, telling the masks which utterance
    runs."""
    net.zero_grad()
    total_words = sum(item[1].shape[1] for item in items)
    total, logits = 0., []
    for index, (features, bounds, targets) in enumerate(items):
        CURRENT[0] = index
        seen = []
        hook = net.frame_encoder.register_forward_hook(
            lambda module, inputs, output: seen.append(output.detach()))
        frame_lengths = torch.tensor([features.shape[1]])
        word_bounds = torch.from_numpy(bounds)[None]
        word_lengths = torch.tensor([bounds.shape[1]])
        scores = net(torch.from_numpy(features)[None].to(dtype), frame_lengths,
                     word_bounds, word_lengths)
        hook.remove()
        if watch is not None:
            watch(seen[0][0], bounds)
        value = sys.modules['emphases.train.core'].loss(
            scores, torch.from_numpy(targets)[None, None].to(dtype),
            frame_lengths, word_bounds, word_lengths, training=True,
            loss_fn='bce') * (bounds.shape[1] / total_words)
        value.backward()
        total += float(value.detach().double())
        logits.append(scores.detach().double().numpy().reshape(-1))
    return total, np.concatenate(logits)


def built(seed, dtype, config, counts_of, keep_all=False):
    torch.manual_seed(seed)
    net = emphases.Model()
    net.train()
    patch(net, config, counts_of, seed, keep_all)
    return net.to(dtype)


def capture(name, settings, items, out):
    emphases.ARCHITECTURE = 'transformer'
    emphases.LAYERS = base.LAYERS
    for key, value in settings.items():
        setattr(emphases, key, value)
    transformer = sys.modules['emphases.model.layers.transformer'].Transformer
    transformer.__init__.__defaults__ = (base.LAYERS, emphases.CHANNELS)
    config = emphases_amd.Config(
        architecture='transformer', layers=base.LAYERS,
        downsample_location=settings['DOWNSAMPLE_LOCATION'],
        downsample_method=settings['DOWNSAMPLE_METHOD'])
    counts_of = {'frame_encoder': base.FRAMES, 'word_decoder': base.WORDS}
    is_max = settings['DOWNSAMPLE_METHOD'] == 'max'
    for seed in range(100):
        try:
            wide = built(seed, torch.float64, config, counts_of)
            loss, logits = accumulate(
                wide, items, torch.float64,
                base.no_near_ties if is_max else None)
            break
        except ArithmeticError:
            print(name, 'seed', seed, 'has a near tie; next')
    else:
        raise ArithmeticError(f'{name}: every seed has a near tie')
    assert len(wide.frame_encoder.model.layers) == base.LAYERS
    exact = base.gradients(wide)
    narrow = built(seed, torch.float32, config, counts_of)
    loss32, logits32 = accumulate(narrow, items, torch.float32)
    rounded = base.gradients(narrow)
    for key, value in exact.items():
        assert np.abs(value).max() > 0, f'{name} {key}: zero gradient'
    error = max([base.relative(rounded[key], exact[key]) for key in exact] +
                [base.relative(logits32, logits), abs(loss32 - loss) / abs(loss)])

    # the patch itself: keep-everything masks against the unpatched eval model
    plain = base.model(seed, torch.float64)
    plain_loss, plain_logits = base.accumulate(plain, items, torch.float64)
    plain_grads = base.gradients(plain)
    kept = built(seed, torch.float64, config, counts_of, keep_all=True)
    kept_loss, kept_logits = accumulate(kept, items, torch.float64)
    kept_grads = base.gradients(kept)
    assert set(kept_grads) == set(plain_grads) == set(exact)
    keep_all_error = max(
        [base.relative(kept_grads[key], plain_grads[key]) for key in exact] +
        [base.relative(kept_logits, plain_logits),
         abs(kept_loss - plain_loss) / abs(plain_loss)])
    assert keep_all_error <= 1e-12, keep_all_error
    assert abs(loss - plain_loss) > 1e-6 * abs(plain_loss)   # the masks bite

    out[f'{name}/seed'] = np.int64(seed)
    out[f'{name}/step'] = np.int64(STEP)
    out[f'{name}/loss'] = np.float64(loss)
    out[f'{name}/logits'] = logits
    out[f'{name}/ref32_error'] = np.float64(error)
    out[f'{name}/keep_all_error'] = np.float64(keep_all_error)
    grads = {key: value.astype(np.float32) for key, value in exact.items()}
    path = os.path.join(HERE, f'transformer_dropout_grads_{name}.npz')
    np.savez_compressed(path, **grads)
    size = os.path.getsize(path)
    print(name, 'seed', seed, 'loss', loss, 'without dropout', plain_loss,
          'ref32', error, 'keep-all', keep_all_error, size, 'bytes')
    assert size < 1 << 20


def main():
    assert emphases.DROPOUT is None and emphases.LOSS == 'bce'
    assert emphases.CHANNELS == CHANNELS
    items = base.make_batch()
    out = {'configs': np.array(list(base.CONFIGS))}
    for name, settings in base.CONFIGS.items():
        capture(name, settings, items, out)
    path = os.path.join(HERE, 'transformer_dropout.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    leaked = [root for root, dirs, _ in os.walk(base.REFERENCE)
              if '__pycache__' in dirs]
    assert not leaked, leaked


if __name__ == '__main__':
    main()
