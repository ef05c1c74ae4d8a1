"""The training step at DOWNSAMPLE_LOCATION = 'input' as plain torch on the
CPU (`emphases/model/core.py:41-87,138`, `core.py:552-586`,
`train/core.py:315-353`): every word of an utterance cut out of the features,
zero-padded to the longest word of ITS utterance, `conv1d` over the padded
pieces as a batch, pooled over the padded axis, then the word decoder, the
output layer and the loss over all words of the batch.  The oracle of
`train.PieceTrainer` on layouts no golden file covers, in float64; in float32
it measures its own rounding; with `split=True` the Conv1d(80, 80, 3) layers
on the frame axis multiply as `precision='bf16x3'` does, with exact
accumulation (tests/split_emulation.py)."""
import collections

import numpy as np
import torch


TIE_MARGIN = 1e-4


def _conv(x, state, name, split=False):
    weight, bias = state[f'{name}.weight'], state[f'{name}.bias']
    if split and tuple(weight.shape) == (80, 80, 3):
        import split_emulation
        return split_emulation.SplitConv.apply(x, weight, bias, True)
    return torch.nn.functional.conv1d(x, weight, bias, padding='same')


def _stack(x, state, prefix, layers, split=False, probe=None):
    for i in range(layers):
        x = _conv(x, state, f'{prefix}.{2 * i}', split)
        if probe is not None:
            probe.append(x.detach())
        x = torch.relu(x)
    return x


def unreachable_masks(exact, rough, factor=8.):
    """Whether no ReLU of the frame encoder can open or close between two
    evaluations of one batch: `exact` and `rough` are their pre-activations
    (`probe` of `step`), and every exact one lies further from zero than
    `factor` x its distance from the rough one.  One mask that flips moves a
    weight gradient of a small batch by per cent, whatever the arithmetic
    costs elsewhere: a comparison across it measures the flip alone."""
    return all(
        bool((a.abs() > factor * (b.double() - a).abs()).all())
        for a, b in zip(exact, rough))


def no_near_ties(embeddings, bounds, layers):
    """ArithmeticError when float32 might choose another column than float64
    under 'max': two candidates of a piece within 1e-4 (relative) of each
    other on a channel with a positive maximum.  The columns
    [n + layers + 1, L - layers) of a piece see nothing but zeros, hold one
    value and carry one gradient: ONE candidate
    (tests/golden/generate_input.py)."""
    padded = embeddings.shape[2]
    for piece, (start, end) in zip(embeddings, np.asarray(bounds).T):
        length = int(end - start)
        flat = list(range(min(length + layers + 1, padded),
                          max(padded - layers, 0)))
        columns = [t for t in range(padded) if t not in flat] + flat[:1]
        if len(columns) < 2:
            continue
        top = torch.topk(piece[:, columns], 2, dim=1).values
        close = (top[:, 0] > 0) & \
            (top[:, 0] - top[:, 1] <= TIE_MARGIN * top[:, 0].abs())
        if bool(close.any()):
            raise ArithmeticError('two maxima of a piece within the margin')


def no_reachable_ties(wide, narrow, bounds, layers, factor=8., floor=1e-6):
    """`no_near_ties` with the margin measured, not fixed, for layouts with
    so many pieces that some pair of candidates always lies within 1e-4:
    `wide` and `narrow` are the float64 and the float32 embeddings of the same
    pieces, and two candidates are too close when their gap is within
    `factor` x the float32 error of that channel of that piece (or `floor` x
    its maximum): only then can a float32 evaluation prefer the other."""
    padded = wide.shape[2]
    for piece, rough, (start, end) in zip(wide, narrow, np.asarray(bounds).T):
        length = int(end - start)
        flat = list(range(min(length + layers + 1, padded),
                          max(padded - layers, 0)))
        columns = [t for t in range(padded) if t not in flat] + flat[:1]
        if len(columns) < 2:
            continue
        top = torch.topk(piece[:, columns], 2, dim=1).values
        error = (rough.double() - piece).abs().max(dim=1).values
        margin = torch.maximum(factor * error, floor * top[:, 0].abs())
        close = (top[:, 0] > 0) & (top[:, 0] - top[:, 1] <= margin)
        if bool(close.any()):
            raise ArithmeticError('two maxima of a piece within reach')


def pieces_of(features, bounds):
    """[W, C, L]: the words of one utterance as zero-padded pieces."""
    starts, ends = bounds[0], bounds[1]
    longest = int((ends - starts).max())
    out = features.new_zeros(len(starts), features.shape[0], longest)
    for j, (start, end) in enumerate(zip(starts.tolist(), ends.tolist())):
        out[j, :, :end - start] = features[:, start:end]
    return out


def pool(embeddings, bounds, method):
    """[W, C, L] -> [C, W] (`model/core.py:54-71`)."""
    if method == 'sum':
        pooled = embeddings.sum(dim=2)
    elif method == 'average':
        pooled = embeddings.mean(dim=2)
    elif method == 'max':
        pooled = embeddings.max(dim=2).values
    elif method == 'center':
        center = torch.as_tensor((bounds[1] - bounds[0]) // 2)
        pooled = embeddings[torch.arange(len(center)), :, center]
    else:
        raise ValueError(method)
    return pooled.transpose(0, 1)


def logits_of(state, items, layers, method, split=False, watch=None,
              probe=None):
    """The logits of every utterance, back to back: [sum W].
    `watch(piece embeddings [W, C, L], bounds, layers)` sees what the pooling
    reads; `probe`: a list that takes the pre-activations of the frame
    encoder's ReLUs, layer by layer, utterance by utterance."""
    out = []
    for features, bounds, _ in items:
        pieces = pieces_of(features, np.asarray(bounds))
        x = _conv(pieces, state, 'input_layer', split)
        x = _stack(x, state, 'frame_encoder', layers, split, probe)
        if watch is not None:
            watch(x.detach(), bounds, layers)
        words = pool(x, np.asarray(bounds), method)[None]
        words = _stack(words, state, 'word_decoder', layers)
        out.append(torch.nn.functional.conv1d(
            words, state['output_layer.weight'], state['output_layer.bias'],
            padding='same')[0, 0])
    return torch.cat(out)


def step(state, items, layers, method='sum', loss='bce',
         dtype=torch.float64, split=False, watch=None, probe=None):
    """(loss, {name: gradient}, logits) of a batch.  state: {name: numpy};
    items: per utterance (features [C, T], bounds int [2, W], targets [W]),
    numpy.  Everything is returned as float64 numpy."""
    parameters = collections.OrderedDict(
        (name, torch.tensor(np.asarray(value), dtype=dtype,
                            requires_grad=True))
        for name, value in state.items())
    items = [(torch.tensor(np.asarray(f), dtype=dtype), np.asarray(b),
              torch.tensor(np.asarray(t), dtype=dtype)) for f, b, t in items]
    logits = logits_of(parameters, items, layers, method, split, watch,
                       probe)
    targets = torch.cat([item[2] for item in items])
    if loss == 'bce':
        value = torch.nn.functional.binary_cross_entropy_with_logits(
            logits, targets)
    else:
        value = torch.nn.functional.mse_loss(logits, targets)
    value.backward()
    return (float(value.detach().double()),
            {name: parameter.grad.double().numpy()
             for name, parameter in parameters.items()},
            logits.detach().double().numpy())


def ragged_items():
    """The `ragged` utterances of tests/golden/train.npz."""
    import train_data
    data = train_data.golden()
    frames, words = data['ragged/frames'], data['ragged/words']
    items, f0, w0 = [], 0, 0
    for f, w in zip(frames, words):
        items.append((data['ragged/features'][:, f0:f0 + f],
                      data['ragged/bounds'][:, w0:w0 + w],
                      data['ragged/targets'][w0:w0 + w]))
        f0, w0 = f0 + f, w0 + w
    return items


def collate(items):
    """What `emphases.data.collate` makes of the utterances: (features
    [B, C, Tmax], frame_lengths, word_bounds [B, 2, Wmax], word_lengths,
    targets [B, 1, Wmax])."""
    frames = [item[0].shape[1] for item in items]
    words = [np.asarray(item[1]).shape[1] for item in items]
    features = torch.zeros(len(items), items[0][0].shape[0], max(frames))
    bounds = torch.zeros(len(items), 2, max(words), dtype=torch.long)
    targets = torch.zeros(len(items), 1, max(words))
    for i, (f, b, t) in enumerate(items):
        features[i, :, :frames[i]] = torch.as_tensor(np.asarray(f))
        bounds[i, :, :words[i]] = torch.as_tensor(np.asarray(b))
        targets[i, 0, :words[i]] = torch.as_tensor(np.asarray(t))
    return (features, torch.tensor(frames), bounds, torch.tensor(words),
            targets)


def worst_error(got, want):
    """The worst over tensors of max|got - want| / max|want|."""
    return max(
        float(np.abs(np.asarray(got[name], dtype=np.float64) - want[name]).max()
              / np.abs(want[name]).max()) for name in want)
