"""The dropout masks of the training step, as a specification (numpy only).

`torch.nn.Dropout` after every activation of the conv stacks
(`model/layers/convolution.py:29-30`) draws its mask from torch's generator;
here the mask is a pure function of (seed, layer, step, element), so that a
step can be repeated, resumed and checked bit for bit.  `emph_dropout`
(`csrc/dropout.hip`), the golden generator and the tests all follow this file.

* Philox-4x32 with 10 rounds (Salmon et al., "Parallel random numbers: as easy
  as 1, 2, 3", SC'11; the Random123 known answers are held by the tests).
* An activation buffer [channels, ld] is a flat array.  Quad
  q = (origin + flat index) // 4 (64-bit) has the counter
  (q_lo, q_hi, stream, step) and the key (seed_lo, seed_hi); its four output
  words belong to elements 4 q .. 4 q + 3, in order.
* `stream` is the layer's position in `train.layer_names(config)`:
  `frame_encoder.2i` is 1 + i, `word_decoder.2i` is 1 + layers + i (the input
  layer, 0, has no dropout).  `step` is the number of updates already done.
* An element is kept iff its word >= `threshold(p)`; kept values are scaled by
  `scale(p)`.  The probability is what the C ABI carries, float32(p): both
  are functions of that value alone, so that the library and this file agree
  for every p.
* The Transformer's five dropouts (`TransformerModel(reference_dropout=True)`,
  `emph_attention_dropout` in `csrc/transformer_grad.hip`): the streams of
  `transformer_stream`, `keep_mask` for the element-wise sites and
  `attention_keep_mask` for the softmax weights, at the end of this file.
"""
import numpy as np

MULTIPLIERS = (0xD2511F53, 0xCD9E8D57)
WEYL = (0x9E3779B9, 0xBB67AE85)
ROUNDS = 10
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox-4x32-10 over arrays: `counter` four and `key` two uint32 arrays
    (or scalars) that broadcast; returns the four output words as uint32
    arrays."""
    c = [np.asarray(word, dtype=np.uint64) & _MASK for word in counter]
    k = [np.asarray(word, dtype=np.uint64) & _MASK for word in key]
    assert len(c) == 4 and len(k) == 2
    for _ in range(ROUNDS):
        # (a 32 x 32 product fits uint64)
        first = c[0] * np.uint64(MULTIPLIERS[0])
        second = c[2] * np.uint64(MULTIPLIERS[1])
        c = [(second >> np.uint64(32)) ^ c[1] ^ k[0], second & _MASK,
             (first >> np.uint64(32)) ^ c[3] ^ k[1], first & _MASK]
        k = [(k[0] + np.uint64(WEYL[0])) & _MASK,
             (k[1] + np.uint64(WEYL[1])) & _MASK]
    return tuple(word.astype(np.uint32) for word in c)


def probability(p):
    """The probability as `emph_dropout` receives it: float32(p), as float."""
    return float(np.float32(p))


def threshold(p):
    """Words below it are dropped: min(round(p 2^32), 2^32 - 1) of the float32
    probability (round half to even; p 2^32 is exact in float64)."""
    return min(int(np.rint(probability(p) * 4294967296.)), _MASK)


def scale(p):
    """float32(1 / (1 - p)), formed in float64 and rounded once."""
    return np.float32(1. / (1. - probability(p)))


def stream_of(config, name):
    """The mask stream of a layer: its position in `train.layer_names`."""
    prefix, index = name.rsplit('.', 1)
    first = {'frame_encoder': 1, 'word_decoder': 1 + config.layers}[prefix]
    return first + int(index) // 2


def keep_mask(seed, stream, step, count, p, origin=0):
    """bool [count]: which of the elements origin .. origin + count - 1 of the
    layer `stream` are kept at `step` under `seed` (any integer, taken modulo
    2^64)."""
    seed, origin, count = int(seed) & (1 << 64) - 1, int(origin), int(count)
    assert origin >= 0 and count >= 0
    first, last = origin // 4, (origin + count + 3) // 4
    quads = first + np.arange(last - first, dtype=np.uint64)
    words = philox4x32_10(
        (quads & _MASK, quads >> np.uint64(32), int(stream) & _MASK,
         int(step) & _MASK), (seed & _MASK, seed >> 32))
    words = np.stack(np.broadcast_arrays(*words), axis=1).ravel()
    skip = origin - 4 * first
    return words[skip:skip + count] >= np.uint32(threshold(p))


# ---- the Transformer (`TransformerModel(reference_dropout=True)`)
#
# The reference's Transformer hard-codes its dropouts; they are constants of
# the architecture, not of the configuration (`Config.dropout` is the conv
# stacks' switch and stays refused for the Transformer).

# model/layers/transformer.py:18-23: `torch.nn.TransformerEncoderLayer(
# channels, 2, dim_feedforward=CHANNELS)` keeps torch's default dropout=0.1 on
# the attention weights, on both residual branches and on the hidden layer
TRANSFORMER_LAYER_DROPOUT = 0.1
# model/layers/transformer.py:17: `PositionalEncoding(channels, .1)`
TRANSFORMER_POSITION_DROPOUT = 0.1

TRANSFORMER_STACKS = ('frame_encoder', 'word_decoder')
# the four masks of a layer, in the order of their stream ids
TRANSFORMER_SITES = ('attention', 'residual1', 'hidden', 'residual2')


def transformer_stream(config, stack, layer=None, site='position'):
    """The mask stream of one dropout of the Transformer: stack s of
    `TRANSFORMER_STACKS` owns the ids s (1 + 4 layers) + ..., first its
    positional site (`layer` None), then four per layer in the order of
    `TRANSFORMER_SITES`.  `encoder_layer_dropout` takes the id of a layer's
    'attention' site as its `stream_base`."""
    first = TRANSFORMER_STACKS.index(stack) * (1 + 4 * config.layers)
    if layer is None:
        assert site == 'position'
        return first
    assert 0 <= int(layer) < config.layers
    return first + 1 + 4 * int(layer) + TRANSFORMER_SITES.index(site)


def attention_keep_mask(seed, stream, step, p, ld, head, query_column, keys):
    """bool [keys]: which attention weights of one query are kept.  The query
    is (head, its column in the packed buffer [., ld]); the keys are counted
    from the first position of its segment.  Key quad k // 4 has the counter
    (k // 4, head ld + query_column, stream, step) and the key (seed_lo,
    seed_hi); its four words belong to keys 4 (k // 4) .. + 3, in order.
    ld < 2^28 and 2 heads keep word 1 inside 32 bits.  The three element-wise
    sites of a layer use `keep_mask` over the packed buffer [rows, ld], the
    positional site `keep_mask` over the caller's [C, sum T]."""
    seed, keys = int(seed) & (1 << 64) - 1, int(keys)
    row = int(head) * int(ld) + int(query_column)
    assert 0 <= row <= _MASK and keys >= 0
    quads = np.arange((keys + 3) // 4, dtype=np.uint64)
    words = philox4x32_10(
        (quads, row, int(stream) & _MASK, int(step) & _MASK),
        (seed & _MASK, seed >> 32))
    words = np.stack(np.broadcast_arrays(*words), axis=1).ravel()
    return words[:keys] >= np.uint32(threshold(p))


def attention_segment_mask(seed, stream, step, p, ld, heads, offset, count):
    """bool [heads, count, count] (head, query, key): `attention_keep_mask` of
    every query of the segment whose first packed column is `offset`."""
    seed, count = int(seed) & (1 << 64) - 1, int(count)
    rows = (np.arange(int(heads), dtype=np.uint64)[:, None] * np.uint64(ld)
            + np.uint64(offset) + np.arange(count, dtype=np.uint64)[None, :])
    assert not rows.size or int(rows.max()) <= _MASK
    quads = np.arange((count + 3) // 4, dtype=np.uint64)
    words = philox4x32_10(
        (quads[None, None, :], rows[:, :, None], int(stream) & _MASK,
         int(step) & _MASK), (seed & _MASK, seed >> 32))
    words = np.stack(np.broadcast_arrays(*words), axis=3).reshape(
        int(heads), count, -1)
    return words[:, :, :count] >= np.uint32(threshold(p))
