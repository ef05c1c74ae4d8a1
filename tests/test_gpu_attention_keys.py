"""`emph_attention_backward_keys` on the MI355X: the backward of
`emph_attention(..., key_counts, ...)`, the attention behind
`src_key_padding_mask` over zero-padded word pieces.

One batch of segments (n positions, k real keys), back to back with the packed
layout's gaps.  The reference is torch autograd of the masked per-segment,
per-head attention in float64 on the CPU; the bound is the project's (the
convention of `test_gpu_ops_transformer`, restated here): error <= 4 x the
error of the same autograd in float32, both over max |want|, per dQ, dK, dV.
Each figure is printed before it is asserted.
"""
import functools
import math

import numpy as np
import pytest
import torch

from emphases_amd import ops, runtime

pytestmark = pytest.mark.gpu

CHANNELS, HEADS, DIM = 80, 2, 40
SENTINEL = 12345.
# a single real key; k off the 4- and 16-key steps; k and n on either side of
# the 32-key wave share and of the 64-wide tile; several tiles
SEGMENTS = [(1, 1), (2, 1), (17, 1), (16, 5), (17, 16), (33, 17), (64, 31),
            (65, 33), (65, 64), (65, 65), (129, 63), (130, 65), (257, 256),
            (300, 100)]
LENGTHS = [n for n, _ in SEGMENTS]
KEYS = [k for _, k in SEGMENTS]
KINDS = ['normal', 'peaked', 'uniform']


def device():
    return torch.device('cuda', 0)


def check(name, got, want, narrow):
    """error <= 4 x the float32 CPU error, both over max |want|."""
    want = want.double()
    scale = float(want.abs().max())
    allowed = 4. * float((narrow.double() - want).abs().max()) / scale
    error = float((got.detach().cpu().double() - want).abs().max()) / scale
    print(f'{name}: error {error:.3g}, bound {allowed:.3g}, ratio '
          f'{error / allowed if allowed else float("inf"):.2f}')
    assert error <= allowed, (name, error, allowed)


def attention_inputs(kind):
    """(q, k, v, dout) [80, sum n] on the CPU, float32, made as
    `test_gpu_ops_transformer.attention_inputs` makes them."""
    generator = torch.Generator().manual_seed(
        {'normal': 1, 'peaked': 2, 'uniform': 3}[kind])
    total = sum(LENGTHS)
    q, k, v, dout = (torch.randn(CHANNELS, total, generator=generator)
                     for _ in range(4))
    if kind == 'peaked':
        # logits q.k / sqrt(40) of unit-normal rows have a standard deviation
        # of 1; sqrt(8) on either side makes it 8
        q, k = q * math.sqrt(8.), k * math.sqrt(8.)
    if kind == 'uniform':
        first = 0
        for count in LENGTHS:
            k[:, first:first + count] = k[:, first:first + 1]
            first += count
    return q, k, v, dout


def attention_autograd(q, k, v, dout, dtype):
    """(dq, dk, dv) [80, sum n] of the per-segment, per-head softmax attention
    over the keys j < k alone (every position a query), by torch autograd in
    `dtype`.  A padded key is never touched: its gradient is zero."""
    leaves = [t.detach().clone().to(dtype).requires_grad_(True)
              for t in (q, k, v)]
    first = 0
    for count, keys in SEGMENTS:
        for head in range(HEADS):
            rows = slice(head * DIM, (head + 1) * DIM)
            queries = leaves[0][rows, first:first + count]
            key_part = leaves[1][rows, first:first + keys]
            value_part = leaves[2][rows, first:first + keys]
            scores = queries.t() @ key_part / math.sqrt(DIM)
            out = torch.softmax(scores, dim=1) @ value_part.t()      # [n, d]
            out.backward(dout[rows, first:first + count].t().to(dtype))
        first += count
    return [leaf.grad.double() for leaf in leaves]


@functools.lru_cache(maxsize=None)
def attention_want(kind):
    inputs = attention_inputs(kind)
    return (attention_autograd(*inputs, torch.float64),
            attention_autograd(*inputs, torch.float32))


def padded_columns():
    """Indices into the back-to-back axis [sum n] of every padded position."""
    index, first = [], 0
    for count, keys in SEGMENTS:
        index.extend(range(first + keys, first + count))
        first += count
    return torch.tensor(index, dtype=torch.int64)


class Batch:
    """The packed device buffers of (q, k, v, dout) [80, sum of `lengths`]
    and the forward / backward calls on them."""

    def __init__(self, q, k, v, dout, lengths=LENGTHS, lead=()):
        # `lead`: segments in front, which only move the offsets
        self.layout = ops._layout(
            device(), np.array(list(lead) + list(lengths), dtype=np.int64))
        self.ld = ld = self.layout.plan.ld_frames
        skip = sum(lead)
        self.columns = self.layout.frame_columns[skip:]
        self.tiles, self.n_tiles = self.layout.tiles(64)
        self.lib = runtime.library()

        def scatter(value, fill=0.):
            packed = torch.full((value.shape[0], ld), fill, device=device())
            packed[:, self.columns] = value.to(device())
            return packed
        self.qk = scatter(torch.cat([q, k]))
        self.v = scatter(v).t().contiguous()
        self.dout = scatter(dout)
        self.lead = len(lead)
        self.workspace = torch.empty(
            int(self.lib.emph_attention_backward_workspace(ld, HEADS)),
            device=device())

    def table(self, keys, lead_value=1):
        return torch.tensor([lead_value] * self.lead + list(keys),
                            dtype=torch.int32, device=device())

    def forward(self, table):
        out = torch.zeros((CHANNELS, self.ld), device=device())
        runtime.check(self.lib.emph_attention(
            self.qk.data_ptr(), self.v.data_ptr(), out.data_ptr(), self.ld,
            CHANNELS, HEADS, self.tiles.data_ptr(), self.n_tiles, 64,
            None if table is None else table.data_ptr(), runtime.stream()),
            'emph_attention')
        return out

    def backward(self, out, table, entry='keys'):
        dqkv = torch.full((3 * CHANNELS, self.ld), SENTINEL, device=device())
        head = (self.qk.data_ptr(), self.v.data_ptr(), out.data_ptr(),
                self.dout.data_ptr(), dqkv.data_ptr(), self.ld, CHANNELS,
                HEADS, self.tiles.data_ptr(), self.n_tiles, 64)
        if entry == 'keys':
            status = self.lib.emph_attention_backward_keys(
                *head, None if table is None else table.data_ptr(),
                self.workspace.data_ptr(), runtime.stream())
        else:
            status = self.lib.emph_attention_backward(
                *head, self.workspace.data_ptr(), runtime.stream())
        runtime.check(status, 'emph_attention_backward' + '_' + entry)
        return dqkv


@functools.lru_cache(maxsize=None)
def batch_result(kind):
    """(the batch, its table, `out`, `dqkv`) of `kind`, computed once."""
    batch = Batch(*attention_inputs(kind))
    table = batch.table(KEYS)
    out = batch.forward(table)
    return batch, table, out, batch.backward(out, table)


@pytest.mark.parametrize('kind', KINDS)
def test_against_float64_autograd(kind):
    batch, table, out, dqkv = batch_result(kind)
    assert batch.n_tiles == sum((n + 63) // 64 for n in LENGTHS)
    # the same inputs give the same bits
    assert torch.equal(dqkv, batch.backward(out, table))
    inside = torch.zeros(batch.ld, dtype=torch.bool, device=device())
    inside[batch.columns] = True
    assert int(inside.sum()) == sum(LENGTHS) < batch.ld
    # every column inside a segment was written; the gaps keep the sentinel
    assert not bool((dqkv[:, inside] == SENTINEL).any())
    assert bool((dqkv[:, ~inside] == SENTINEL).all())
    assert bool(torch.isfinite(dqkv[:, inside]).all())
    got = dqkv.index_select(1, batch.columns)
    # dK and dV at padded keys are exactly 0
    padded = padded_columns().to(device())
    assert padded.numel() == sum(LENGTHS) - sum(KEYS)
    assert not bool(got[CHANNELS:].index_select(1, padded).any())
    exact, narrow = attention_want(kind)
    for index, name in enumerate(('dQ', 'dK', 'dV')):
        check(f'attention backward keys ({kind}) {name}',
              got[index * CHANNELS:(index + 1) * CHANNELS], exact[index],
              narrow[index])


@pytest.mark.parametrize('kind', KINDS)
def test_one_real_key_in_front_of_padding_has_no_score_gradient(kind):
    """The softmax over a single key is the constant 1: dQ of every query and
    dK of the key are exactly 0, as autograd's softmax backward gives them
    (float32 rounding of dP - D, two sums of size 10, would leave 4e-6
    there, above the bound wherever nothing else sets the scale)."""
    batch, _, _, dqkv = batch_result(kind)
    got = dqkv.index_select(1, batch.columns)
    exact, _ = attention_want(kind)
    first = 0
    for count, keys in SEGMENTS:
        if keys == 1 and count > 1:
            columns = slice(first, first + count)
            assert not bool(exact[0][:, columns].any())
            assert not bool(exact[1][:, columns].any())
            assert not bool(got[:2 * CHANNELS, columns].any())
            assert bool(got[2 * CHANNELS:, first].any())         # dV of the key
        first += count


@pytest.mark.parametrize('kind', KINDS)
def test_padded_keys_and_values_reach_nothing(kind):
    """NaN in the K rows and V rows at every padded position, before the
    forward and the backward: bitwise the `dqkv` of finite values there."""
    _, _, _, want = batch_result(kind)
    q, k, v, dout = attention_inputs(kind)
    padded = padded_columns()
    k, v = k.clone(), v.clone()
    k[:, padded] = float('nan')
    v[:, padded] = float('nan')
    batch = Batch(q, k, v, dout)
    table = batch.table(KEYS)
    out = batch.forward(table)
    assert bool(torch.isfinite(out[:, batch.columns]).all())
    assert torch.equal(batch.backward(out, table), want)


def test_full_key_counts_and_null_are_the_plain_backward():
    batch = Batch(*attention_inputs('normal'))
    out = batch.forward(None)
    want = batch.backward(out, None, entry='plain')
    assert torch.equal(batch.forward(batch.table(LENGTHS)), out)
    assert torch.equal(batch.backward(out, batch.table(LENGTHS)), want)
    assert torch.equal(batch.backward(out, None), want)


@pytest.mark.parametrize('which', [6, 11, 13])
def test_a_segment_alone_at_another_offset(which):
    """(64, 31), (130, 65) and (300, 100) alone behind a 5-position segment
    are bitwise their columns in the batch."""
    batch, _, _, dqkv = batch_result('peaked')
    first = sum(LENGTHS[:which])
    count, keys = SEGMENTS[which]
    part = [t[:, first:first + count] for t in attention_inputs('peaked')]
    alone = Batch(*part, lengths=[count], lead=[5])
    assert int(alone.columns[0]) != int(batch.columns[first])
    table = alone.table([keys])
    got = alone.backward(alone.forward(table), table)
    assert torch.equal(
        got.index_select(1, alone.columns),
        dqkv.index_select(1, batch.columns[first:first + count]))


def test_a_table_out_of_range_is_clamped():
    """0 behaves as 1 and n + 5 as n (`out` is the forward's at 1 and n: the
    forward of an empty key set is NaN, as in torch)."""
    batch = Batch(*attention_inputs('normal'))
    clamped = [1 if index % 2 else n for index, n in enumerate(LENGTHS)]
    wild = [0 if index % 2 else n + 5 for index, n in enumerate(LENGTHS)]
    out = batch.forward(batch.table(clamped))
    want = batch.backward(out, batch.table(clamped))
    got = batch.backward(out, batch.table(wild))
    assert torch.equal(got, want)
    inside = torch.zeros(batch.ld, dtype=torch.bool, device=device())
    inside[batch.columns] = True
    assert bool((got[:, ~inside] == SENTINEL).all())


def test_other_shapes_are_refused():
    """Return codes of calls that launch nothing."""
    lib = runtime.library()
    layout = ops._layout(device(), np.array([64], dtype=np.int64))
    tiles, n_tiles = layout.tiles(64)
    buffer = torch.zeros(1 << 16, device=device())
    table = torch.ones(1, dtype=torch.int32, device=device())
    pointer = buffer.data_ptr()
    for channels, heads in ((64, 2), (80, 4), (128, 2), (80, 1)):
        assert lib.emph_attention_backward_keys(
            pointer, pointer, pointer, pointer, pointer, 64, channels, heads,
            tiles.data_ptr(), n_tiles, 64, table.data_ptr(), pointer,
            runtime.stream()) == -2
    torch.cuda.synchronize()
    assert not bool(buffer.any())
