"""The reference's dropout of the Transformer on the MI355X:
`emph_attention_dropout` and `emph_attention_dropout_backward` through the C
ABI against float64 autograd with the specified mask, the ops
`encoder_layer_dropout` and `dropout`, and
`train.TransformerModel(reference_dropout=True)` against the reference's
float64 run with fixed masks (tests/golden/transformer_dropout*.npz).

Every oracle is torch on the CPU (`transformer_dropout_data`, anchored by
tests/test_transformer_dropout.py) or the reference's recorded run.  Every
bound is 4 x the error of the same computation in float32 on the CPU against
float64, per tensor, over max |want| (the reference's own `ref32_error` for
the goldens); each figure is printed before it is asserted.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import transformer_dropout_data as data  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import engine as engine_module  # noqa: E402
from emphases_amd import ops, runtime, session, synth, train, weights  # noqa: E402
from emphases_amd.train import dropout as spec  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, 'golden')
CHANNELS, HEADS, DIM = 80, 2, 40
SENTINEL = 12345.
ATTENTION_SEGMENTS = [1, 2, 15, 16, 17, 63, 64, 65, 130, 257, 300]
LAYER_SEGMENTS = [1, 17, 64, 130, 257]
SEED, STREAM, STEP = 0x5EED0123456789AB, 9, 3
NAMES = ('out', 'dQ', 'dK', 'dV')


def device():
    return torch.device('cuda', 0)


def bound(want, narrow):
    """4 x the float32 CPU error over max |want|."""
    want = want.double()
    return 4. * float((narrow.double() - want).abs().max()) / \
        float(want.abs().max())


def check(name, got, want, narrow):
    want = want.double()
    allowed = bound(want, narrow)
    error = float((got.detach().cpu().double() - want).abs().max()) / \
        float(want.abs().max())
    print(f'{name}: error {error:.3g}, bound {allowed:.3g}, ratio '
          f'{error / allowed if allowed else float("inf"):.2f}')
    assert error <= allowed, (name, error, allowed)


###############################################################################
# The two entry points
###############################################################################


def attention_inputs(kind):
    """(q, k, v, dout) [80, sum T] on the CPU, float32: the `normal` and
    `peaked` kinds of tests/test_gpu_ops_transformer.py."""
    generator = torch.Generator().manual_seed({'normal': 1, 'peaked': 2}[kind])
    total = sum(ATTENTION_SEGMENTS)
    q, k, v, dout = (torch.randn(CHANNELS, total, generator=generator)
                     for _ in range(4))
    if kind == 'peaked':
        # logits of standard deviation 8
        q, k = q * math.sqrt(8.), k * math.sqrt(8.)
    return q, k, v, dout


@functools.lru_cache(maxsize=None)
def attention_masks(p, step=STEP):
    """Per segment bool [heads, T, T] (head, query, key), from the packed
    plan of ATTENTION_SEGMENTS."""
    offsets, ld = data.packed_plan(ATTENTION_SEGMENTS)
    return tuple(torch.from_numpy(spec.attention_segment_mask(
        SEED, STREAM, step, p, ld, HEADS, offset, count))
        for offset, count in zip(offsets, ATTENTION_SEGMENTS))


def attention_autograd(kind, p, dtype, wrong=None):
    """(out, dq, dk, dv) [80, sum T] of the masked attention by torch autograd
    in `dtype`, as float64.  p None: no mask."""
    q, k, v, dout = attention_inputs(kind)
    leaves = [t.detach().clone().to(dtype).requires_grad_(True)
              for t in (q, k, v)]
    masks = scale = None
    if p is not None:
        masks = attention_masks(p, STEP + 1 if wrong == 'step' else STEP)
        scale = float(spec.scale(p))
    outs, first = [], 0
    for index, count in enumerate(ATTENTION_SEGMENTS):
        part = [leaf[:, first:first + count] for leaf in leaves]
        out = data.attention(
            *part, None if masks is None else masks[index], scale or 1.,
            wrong if wrong in ('transposed', 'dv') else None)
        out.backward(dout[:, first:first + count].to(dtype))
        outs.append(out.detach())
        first += count
    return [torch.cat(outs, dim=1).double()] + \
        [leaf.grad.double() for leaf in leaves]


@functools.lru_cache(maxsize=None)
def attention_want(kind, p):
    return (attention_autograd(kind, p, torch.float64),
            attention_autograd(kind, p, torch.float32))


class Packed:
    """The inputs of `kind` on the packed layout of ATTENTION_SEGMENTS."""

    def __init__(self, kind):
        q, k, v, dout = attention_inputs(kind)
        self.layout = layout = ops._layout(
            device(), np.array(ATTENTION_SEGMENTS, dtype=np.int64))
        self.ld = ld = layout.plan.ld_frames
        assert (list(layout.plan.frame_off), ld) == \
            tuple(data.packed_plan(ATTENTION_SEGMENTS))
        self.columns = columns = layout.frame_columns
        self.tiles, self.n_tiles = layout.tiles(64)
        assert self.n_tiles == sum((n + 63) // 64 for n in ATTENTION_SEGMENTS)
        self.qk = layout.scatter(torch.cat([q, k]).to(device()), columns, ld)
        self.v = layout.scatter(v.to(device()), columns, ld).t().contiguous()
        self.dout = layout.scatter(dout.to(device()), columns, ld)
        self.inside = torch.zeros(ld, dtype=torch.bool, device=device())
        self.inside[columns] = True
        assert int(self.inside.sum()) == sum(ATTENTION_SEGMENTS) < ld
        self.lib = runtime.library()
        assert self.lib.emph_attention_dropout_backward_workspace(ld, HEADS) \
            == 3 * HEADS * ld
        self.workspace = torch.empty(int(
            self.lib.emph_attention_dropout_backward_workspace(ld, HEADS)),
            device=device())

    def forward(self, p):
        out = torch.full((CHANNELS, self.ld), SENTINEL, device=device())
        runtime.check(self.lib.emph_attention_dropout(
            self.qk.data_ptr(), self.v.data_ptr(), out.data_ptr(), self.ld,
            CHANNELS, HEADS, self.tiles.data_ptr(), self.n_tiles, 64, p, SEED,
            STREAM, STEP, runtime.stream()), 'emph_attention_dropout')
        return out

    def backward(self, out, p):
        dqkv = torch.full((3 * CHANNELS, self.ld), SENTINEL, device=device())
        runtime.check(self.lib.emph_attention_dropout_backward(
            self.qk.data_ptr(), self.v.data_ptr(), out.data_ptr(),
            self.dout.data_ptr(), dqkv.data_ptr(), self.ld, CHANNELS, HEADS,
            self.tiles.data_ptr(), self.n_tiles, 64,
            self.workspace.data_ptr(), p, SEED, STREAM, STEP,
            runtime.stream()), 'emph_attention_dropout_backward')
        return dqkv

    def written_inside_only(self, buffer):
        """Every element inside a segment was written, the gaps were left."""
        assert not bool((buffer[:, self.inside] == SENTINEL).any())
        assert bool((buffer[:, ~self.inside] == SENTINEL).all())
        assert bool(torch.isfinite(buffer[:, self.inside]).all())


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('kind', ['normal', 'peaked'])
def test_attention_dropout_against_float64_autograd(kind, p):
    packed = Packed(kind)
    outs = [packed.forward(p) for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    packed.written_inside_only(outs[0])
    grads = [packed.backward(outs[0], p) for _ in range(2)]
    assert torch.equal(grads[0], grads[1])
    packed.written_inside_only(grads[0])
    got = [outs[0].index_select(1, packed.columns)] + list(
        grads[0].index_select(1, packed.columns).split(CHANNELS))
    exact, narrow = attention_want(kind, p)
    for name, value, want, rounded in zip(NAMES, got, exact, narrow):
        check(f'attention dropout ({kind}, p={p}) {name}', value, want,
              rounded)


@pytest.mark.parametrize('kind', ['normal', 'peaked'])
def test_attention_dropout_without_dropout(kind):
    """p = 0: the backward IS `emph_attention_backward`, bit for bit; the
    forward, a different kernel, is within the bound of the unmasked oracle
    (as `emph_attention` is)."""
    packed = Packed(kind)
    lib = packed.lib
    plain = torch.full((CHANNELS, packed.ld), SENTINEL, device=device())
    runtime.check(lib.emph_attention(
        packed.qk.data_ptr(), packed.v.data_ptr(), plain.data_ptr(),
        packed.ld, CHANNELS, HEADS, packed.tiles.data_ptr(), packed.n_tiles,
        64, None, runtime.stream()), 'emph_attention')
    want = torch.full((3 * CHANNELS, packed.ld), SENTINEL, device=device())
    runtime.check(lib.emph_attention_backward(
        packed.qk.data_ptr(), packed.v.data_ptr(), plain.data_ptr(),
        packed.dout.data_ptr(), want.data_ptr(), packed.ld, CHANNELS, HEADS,
        packed.tiles.data_ptr(), packed.n_tiles, 64,
        packed.workspace.data_ptr(), runtime.stream()),
        'emph_attention_backward')
    assert torch.equal(packed.backward(plain, 0.), want)
    out = packed.forward(0.)
    packed.written_inside_only(out)
    exact, narrow = attention_want(kind, None)
    check(f'attention dropout ({kind}, p=0) out',
          out.index_select(1, packed.columns), exact[0], narrow[0])
    check(f'emph_attention ({kind}) out',
          plain.index_select(1, packed.columns), exact[0], narrow[0])
    apart = float((out - plain)[:, packed.inside].abs().max()) / \
        float(exact[0].abs().max())
    print(f'p = 0 forward against emph_attention ({kind}): {apart:.3g}')


def test_attention_dropout_refuses_other_shapes():
    """Return codes of calls that launch nothing."""
    lib = runtime.library()
    layout = ops._layout(device(), np.array([64], dtype=np.int64))
    tiles, n_tiles = layout.tiles(64)
    buffer = torch.full((1 << 16,), SENTINEL, device=device())
    pointer = buffer.data_ptr()
    for channels, heads in ((64, 2), (128, 2), (80, 1), (160, 4)):
        assert lib.emph_attention_dropout(
            pointer, pointer, pointer, 64, channels, heads, tiles.data_ptr(),
            n_tiles, 64, 0.1, SEED, STREAM, STEP, runtime.stream()) == -2
        assert lib.emph_attention_dropout_backward(
            pointer, pointer, pointer, pointer, pointer, 64, channels, heads,
            tiles.data_ptr(), n_tiles, 64, pointer, 0.1, SEED, STREAM, STEP,
            runtime.stream()) == -2
    torch.cuda.synchronize()
    assert bool((buffer == SENTINEL).all())


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('kind', ['normal', 'peaked'])
def test_the_bound_tells_a_wrong_mask(kind, p):
    """On the CPU: the restatement with the mask of step + 1, with the mask
    transposed between query and key, and with the mask left out of dV alone
    lies more than 100 x the bound from the right result, on every tensor
    the mistake reaches - a kernel that makes it cannot pass above."""
    exact, narrow = attention_want(kind, p)
    reached = {'step': NAMES, 'transposed': NAMES, 'dv': ('dV',)}
    for wrong, names in reached.items():
        found = attention_autograd(kind, p, torch.float64, wrong)
        for name, value, want, rounded in zip(NAMES, found, exact, narrow):
            allowed = bound(want, rounded)
            apart = float((value - want).abs().max()) / float(want.abs().max())
            print(f'{kind} p={p} {wrong} {name}: {apart:.3g} = '
                  f'{apart / allowed:.3g} x bound')
            if name in names:
                assert apart > 100. * allowed, (wrong, name, apart, allowed)
            else:
                assert apart <= 1e-12, (wrong, name, apart)


###############################################################################
# The ops
###############################################################################

LAYER_P, LAYER_BASE = 0.1, 5


def layer_cu(segments=LAYER_SEGMENTS):
    return torch.tensor(np.concatenate([[0], np.cumsum(segments)]))


@functools.lru_cache(maxsize=None)
def layer_case():
    """x, upstream [80, sum T] and the twelve parameters (the op's order) of a
    seeded `TransformerEncoderLayer`, on the CPU in float32."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        module = torch.nn.TransformerEncoderLayer(
            CHANNELS, HEADS, dim_feedforward=CHANNELS)
        values = dict(module.named_parameters())
        parameters = []
        for name in data.LAYER_NAMES:
            value = values[name].detach().clone()
            if 'norm' in name or name.endswith('bias'):
                # (torch starts them at 1 and 0)
                value = value + 0.1 * torch.randn(value.shape)
            parameters.append(value)
        x = torch.randn(CHANNELS, sum(LAYER_SEGMENTS))
        upstream = torch.randn(CHANNELS, sum(LAYER_SEGMENTS))
    return x, upstream, tuple(parameters)


def layer_restated(dtype, step=STEP):
    """(out, dx, twelve gradients) of the restatement in `dtype`."""
    x, upstream, parameters = layer_case()
    leaves = [t.detach().clone().to(dtype).requires_grad_(True)
              for t in (x,) + parameters]
    masks = data.LayerMasks(LAYER_SEGMENTS, LAYER_P, SEED, LAYER_BASE, step)
    out = data.layer(leaves[0], leaves[1:], LAYER_SEGMENTS, masks)
    out.backward(upstream.to(dtype))
    return [out.detach().double()] + [leaf.grad.double() for leaf in leaves]


@functools.lru_cache(maxsize=None)
def layer_want():
    return layer_restated(torch.float64), layer_restated(torch.float32)


def layer_leaves():
    x, upstream, parameters = layer_case()
    return [t.to(device()).requires_grad_(True)
            for t in (x,) + parameters], upstream.to(device())


def layer_call(leaves, step=STEP):
    return torch.ops.emphases_amd.encoder_layer_dropout(
        *leaves, layer_cu(), HEADS, LAYER_P, SEED, LAYER_BASE, step)


def test_encoder_layer_dropout_against_the_restatement():
    exact, narrow = layer_want()
    leaves, upstream = layer_leaves()
    out = layer_call(leaves)
    assert out.requires_grad
    out.backward(upstream)
    got = [out.detach()] + [leaf.grad for leaf in leaves]
    names = ('out', 'dx') + tuple('d ' + name for name in data.LAYER_NAMES)
    for name, value, want, rounded, leaf in zip(
            names, got, exact, narrow, [leaves[0]] + leaves):
        assert value.shape == leaf.shape and value.dtype == leaf.dtype
        check(f'encoder_layer_dropout {name}', value, want, rounded)
    # a pure function of its arguments; another step, another mask
    again, _ = layer_leaves()
    assert torch.equal(layer_call(again).detach(), out.detach())
    assert not torch.equal(layer_call(again, STEP + 1).detach(), out.detach())
    # ... and not the layer without dropout
    apart = float((exact[0] - torch.ops.emphases_amd.encoder_layer(
        *again, layer_cu(), HEADS).detach().cpu().double()).abs().max())
    assert apart > 0.1, apart


def test_encoder_layer_dropout_second_backward_and_other_shapes_raise():
    leaves, upstream = layer_leaves()
    out = layer_call(leaves)
    with pytest.raises(RuntimeError, match='differentiable once'):
        torch.autograd.grad((out * upstream).sum(), leaves[7],
                            create_graph=True)
    narrow = [torch.zeros(64, 70, device=device())] + [
        torch.zeros(shape, device=device()) for shape in (
            (192, 64), (192,), (64, 64), (64,), (64,), (64,), (64, 64), (64,),
            (64, 64), (64,), (64,), (64,))]
    with pytest.raises(NotImplementedError, match='channels'):
        torch.ops.emphases_amd.encoder_layer_dropout(
            *narrow, torch.tensor([0, 3, 70]), HEADS, 0.1, 0, 0, 0)
    with pytest.raises(NotImplementedError, match='heads'):
        torch.ops.emphases_amd.encoder_layer_dropout(
            *[leaf.detach() for leaf in leaves], layer_cu(), 4, 0.1, 0, 0, 0)


def test_opcheck_of_the_new_ops():
    leaves, _ = layer_leaves()
    cu = torch.tensor([0, 3, 70])
    leaves[0] = leaves[0][:, :70].detach().clone().requires_grad_(True)
    utils = ('test_schema', 'test_autograd_registration', 'test_faketensor')
    torch.library.opcheck(
        torch.ops.emphases_amd.encoder_layer_dropout.default,
        (*leaves, cu, HEADS, LAYER_P, SEED, LAYER_BASE, STEP),
        test_utils=utils)
    x = torch.randn(7, 33, device=device(), requires_grad=True)
    torch.library.opcheck(
        torch.ops.emphases_amd.dropout.default, (x, 0.1, SEED, 2, STEP),
        test_utils=utils)


@pytest.mark.parametrize('shape', [(80, 231), (7, 33), (5,), (0, 3)])
def test_dropout_op_is_the_specified_mask(shape):
    """Exact: a select and one float32 product."""
    generator = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=generator)
    upstream = torch.randn(shape, generator=generator)
    leaf = x.to(device()).requires_grad_(True)
    p = 0.1
    out = torch.ops.emphases_amd.dropout(leaf, p, SEED, 2, STEP)
    out.backward(upstream.to(device()))
    keep = torch.from_numpy(spec.keep_mask(
        SEED, 2, STEP, x.numel(), p).reshape(shape))
    scale = torch.tensor(spec.scale(p))
    zero = torch.zeros(())
    assert torch.equal(out.detach().cpu(), torch.where(keep, x * scale, zero))
    assert torch.equal(leaf.grad.cpu(),
                       torch.where(keep, upstream * scale, zero))
    if x.numel() > 100:
        assert 0.8 < float(keep.float().mean()) < 0.97


###############################################################################
# TransformerModel(reference_dropout=True)
###############################################################################

CONFIGS = {
    'intermediate_sum': dict(downsample_location='intermediate',
                             downsample_method='sum'),
    'loss_max': dict(downsample_location='loss', downsample_method='max'),
}


@functools.lru_cache(maxsize=None)
def golden(name='transformer_dropout.npz'):
    with np.load(os.path.join(GOLDEN, name)) as file:
        return {key: file[key] for key in file.files}


def golden_batch():
    batch = golden('transformer_train.npz')
    cu = lambda counts: torch.from_numpy(  # noqa: E731
        np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    return (torch.from_numpy(batch['features']).to(device()),
            cu(batch['frames']), torch.from_numpy(batch['bounds']),
            cu(batch['words'])), torch.from_numpy(batch['targets']).to(device())


def golden_model(name, reference_dropout=True):
    config = emphases_amd.Config(
        architecture='transformer', layers=2, **CONFIGS[name])
    return train.TransformerModel(
        config, seed=int(golden()[f'{name}/seed']),
        reference_dropout=reference_dropout).to(device())


def step_of(model, batch, targets):
    model.zero_grad(set_to_none=True)
    logits = model(*batch)
    loss = train.loss_fn(logits, targets, 'bce')
    loss.backward()
    return loss.detach(), logits.detach(), {
        key: parameter.grad.clone()
        for key, parameter in model.named_parameters()}


@pytest.mark.parametrize('name', list(CONFIGS))
def test_transformer_model_matches_the_reference_under_dropout(name):
    """Every gradient, the loss and the logits within 4 x `ref32_error` at
    steps = 3.

    MEASURED (MI355X): 'loss_max' worst 1.10 x ref32_error; 'intermediate_sum'
    worst 3.98 x (frame_encoder.model.layers.1.norm1.weight) - inside the
    bound by half a percent.  The thin margin is one site's: behind 'sum' the
    word decoder's first layer sees sums over a word's frames, its attention
    logits reach 392 (natural units; 1.2 to 2.3 in every other layer), and
    every gradient at and upstream of that attention carries its conditioning.
    float32 runs of the same mathematics scatter there: the reference's own
    is 2.2e-6 off float64 (`ref32_error`), this file's restatement in float32
    on the CPU 5.4e-6 (2.5 x), the reference without dropout through torch's
    MultiheadAttention 1.21e-5 (transformer_train.npz).  The kernels reached
    15 x with the row's log-sum-exp as one float, 5.18 x with the maximum and
    1 / sum apart, 3.98 x with the scores as two floats
    (csrc/transformer_grad.hip, `scores_split`; EXPERIMENTS has the variants
    and what they cost)."""
    recorded = golden()
    reference_error = float(recorded[f'{name}/ref32_error'])
    batch, targets = golden_batch()
    model = golden_model(name)
    model.train()
    model.steps = int(recorded[f'{name}/step'])
    assert model.steps == 3
    loss, logits, grads = step_of(model, batch, targets)
    want_loss = float(recorded[f'{name}/loss'])
    loss_error = abs(float(loss) - want_loss) / abs(want_loss)
    want_logits = recorded[f'{name}/logits']
    logit_error = np.abs(logits.cpu().numpy().astype(np.float64) -
                         want_logits).max() / np.abs(want_logits).max()
    print(f'{name}: loss {float(loss):.9g} (reference {want_loss:.9g}) error '
          f'{loss_error / reference_error:.2f}, logits '
          f'{logit_error / reference_error:.2f} (x ref32_error '
          f'{reference_error:.3g})')
    missed = {}
    wanted = golden(f'transformer_dropout_grads_{name}.npz')
    assert set(wanted) == set(grads)
    for key, value in grads.items():
        want = wanted[key].astype(np.float64)
        got = value.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        error = np.abs(got - want).max() / np.abs(want).max()
        print(f'{name} {key}: error {error / reference_error:.2f} '
              '(x ref32_error)')
        if not error <= 4. * reference_error:
            missed[key] = error
    assert loss_error <= 4. * reference_error
    assert logit_error <= 4. * reference_error
    assert not missed, (missed, reference_error)

    # the same steps twice: the same bits; another step: another loss
    again = step_of(model, batch, targets)
    assert torch.equal(again[0], loss) and torch.equal(again[1], logits)
    assert all(torch.equal(again[2][key], grads[key]) for key in grads)
    model.steps = 4
    other, _, _ = step_of(model, batch, targets)
    print(f'{name}: loss at steps 3 {float(loss):.9g}, at 4 {float(other):.9g}')
    assert float(other) != float(loss)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_eval_and_the_default_keep_their_bits(name):
    batch, targets = golden_batch()
    dropping, plain = golden_model(name), golden_model(name, False)
    dropping.steps = 3
    dropping.eval()
    plain.eval()
    with torch.no_grad():
        assert torch.equal(dropping(*batch), plain(*batch))
    # the default in training mode: `encoder_layer` as before, called here
    # directly
    plain.train()
    plain.steps = 3                                 # (ignored)
    loss, logits, grads = step_of(plain, batch, targets)
    leaves = {key: parameter.detach().clone().requires_grad_(True)
              for key, parameter in plain.named_parameters()}
    features, cu_frames, bounds, cu_words = batch
    conv = torch.ops.emphases_amd.conv1d_same_act

    def stack(x, prefix, cu, encoding):
        counts = np.diff(cu.numpy())
        x = x + torch.cat([encoding[:, :count] for count in counts], dim=1)
        for index in range(plain.config.layers):
            at = f'{prefix}.model.layers.{index}.'
            x = torch.ops.emphases_amd.encoder_layer(
                x, *[leaves[at + part] for part in data.LAYER_NAMES], cu,
                HEADS)
        return x
    x = conv(features, leaves['input_layer.weight'],
             leaves['input_layer.bias'], cu_frames, 'none')
    x = stack(x, 'frame_encoder', cu_frames, plain.frame_encoder.encoding)
    x = torch.ops.emphases_amd.segment_reduce(
        x, bounds, cu_frames, cu_words, plain.config.downsample_method)
    if plain.config.has_decoder:
        x = stack(x, 'word_decoder', cu_words, plain.word_decoder.encoding)
    direct = conv(x, leaves['output_layer.weight'],
                  leaves['output_layer.bias'], cu_words, 'none')[0]
    assert torch.equal(direct.detach(), logits)
    train.loss_fn(direct, targets, 'bce').backward()
    for key, leaf in leaves.items():
        assert torch.equal(leaf.grad, grads[key]), key
    # ... and under dropout the training model is another function
    dropping.train()
    with torch.no_grad():
        assert not torch.equal(dropping(*batch), logits)


def test_a_model_trained_under_dropout_saves_and_infers(tmp_path):
    name = 'intermediate_sum'
    batch, targets = golden_batch()
    model = golden_model(name)
    model.train()
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(2):
        optimizer.zero_grad(set_to_none=True)
        train.loss_fn(model(*batch), targets, 'bce').backward()
        optimizer.step()
        model.steps += 1
    assert model.steps == 2
    assert 'steps' not in model.state_dict()
    state = weights.load(model.state_dict(), model.config)
    assert list(state) == list(weights.parameter_shapes(model.config))
    for key, parameter in model.named_parameters():
        assert np.array_equal(state[key], parameter.detach().cpu().numpy())
    path = tmp_path / '00000002.pt'
    train.write_checkpoint(path, model.state_dict(), optimizer.state_dict(),
                           step=2)
    audio = torch.from_numpy(synth.audio(3, 211))
    alignment = emphases_amd.Alignment.from_frames(
        synth.word_frames(3, 211, 3, 40))
    emphases_amd.configure(model.config)
    try:
        from_file = emphases_amd.from_alignment_and_audio(
            alignment, audio, emphases_amd.SAMPLE_RATE, checkpoint=str(path),
            gpu=0)
    finally:
        emphases_amd.configure(emphases_amd.DEFAULT)
    direct = session.Session(engine_module.Engine(
        model.config, state, 0)).run([alignment], [audio], on_device=True)[0]
    assert from_file.shape == direct.shape and from_file.shape[1] > 1
    assert bool(torch.isfinite(from_file).all())
    assert torch.equal(from_file, direct)
