"""`precision='bf16x3'` of Transformer training on the MI355X:
`emph_attention_backward_split` alone through the C ABI, the op
`encoder_layer_split` against the float64 torch layer, and
`TransformerModel(precision='bf16x3')` against the reference's float64 run
(tests/golden/transformer_train*.npz) and against the inference engine.

The bound of every comparison is 4 x (emulated error + float32 error), per
tensor over max |want| (the rule of tests/test_gpu_train_precision.py): what
the piece arithmetic costs with exact accumulation (tests/
attention_split_emulation.py against float64, computed here on the CPU), what
float32 accumulation costs the float32 computation it is compared with
(torch's on the CPU for the kernel and the op, the reference's own
`ref32_error` for the goldens), and the project's factor 4.  Each figure is
printed before it is asserted.
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

import attention_split_emulation as emulation  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import engine as engine_module  # noqa: E402
from emphases_amd import ops, runtime, train, weights  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, 'golden')
CHANNELS, HEADS, DIM = 80, 2, 40
SENTINEL = 12345.
LONG_FROM = engine_module.GROUPED_FROM
# either side of the family threshold (128), of the 64-key stage and of the
# 256-position workgroup; 513 needs three workgroups
SEGMENTS = [1, 17, 64, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 513]
KINDS = ['normal', 'peaked', 'uniform']
ERANGE = -2


def device():
    return torch.device('cuda', 0)


###############################################################################
# emph_attention_backward_split
###############################################################################


def attention_inputs(kind, segments=tuple(SEGMENTS)):
    """(q, k, v, dout) [80, sum T] on the CPU, float32, built as
    tests/test_gpu_ops_transformer.py builds them."""
    generator = torch.Generator().manual_seed(
        {'normal': 1, 'peaked': 2, 'uniform': 3}[kind])
    total = sum(segments)
    q, k, v, dout = (torch.randn(CHANNELS, total, generator=generator)
                     for _ in range(4))
    if kind == 'peaked':
        q, k = q * math.sqrt(8.), k * math.sqrt(8.)
    if kind == 'uniform':
        first = 0
        for count in segments:
            k[:, first:first + count] = k[:, first:first + 1]
            first += count
    return q, k, v, dout


def long_columns(segments):
    """The columns (of the back-to-back layout) of the long segments."""
    first, columns = 0, []
    for count in segments:
        if count >= LONG_FROM:
            columns.append(np.arange(first, first + count))
        first += count
    return torch.from_numpy(np.concatenate(columns))


def attention_gradients(inputs, segments, how):
    """(dq, dk, dv) [80, sum T] float64 of the per-segment, per-head
    attention: `how` = torch.float64 / torch.float32 (torch autograd in that
    dtype) or 'emulated' (float64 with the kernels' piece arithmetic)."""
    q, k, v, dout = inputs
    dtype = torch.float64 if how == 'emulated' else how
    leaves = [t.detach().clone().to(dtype).requires_grad_(True)
              for t in (q, k, v)]
    first = 0
    for count in segments:
        for head in range(HEADS):
            rows = slice(head * DIM, (head + 1) * DIM)
            part = [leaf[rows, first:first + count].t() for leaf in leaves]
            if how == 'emulated':
                out = emulation.attention(*part, split=True)
            else:
                scores = part[0] @ part[1].t() / math.sqrt(DIM)
                out = torch.softmax(scores, dim=1) @ part[2]
            out.backward(dout[rows, first:first + count].t().to(dtype))
        first += count
    return [leaf.grad.double() for leaf in leaves]


@functools.lru_cache(maxsize=None)
def attention_want(kind):
    """(exact, float32, emulated) gradients; computed once, never changed."""
    inputs = attention_inputs(kind)
    return tuple(attention_gradients(inputs, SEGMENTS, how)
                 for how in (torch.float64, torch.float32, 'emulated'))


def split_backward(inputs, segments, launches=1):
    """dqkv [240, ld] of `launches` runs (the split forward on the long
    segments' table, then the new backward into a SENTINEL fill), the layout,
    and `out`."""
    q, k, v, dout = inputs
    layout = ops._layout(device(), np.array(segments, dtype=np.int64))
    ld, columns = layout.plan.ld_frames, layout.frame_columns
    stages, n_stages = layout.tiles(64, engine_module.LONG)
    tiles, n_tiles = layout.tiles(256, engine_module.LONG)
    assert n_tiles == sum((n + 255) // 256 for n in segments if n >= LONG_FROM)
    lib = runtime.library()
    qk = layout.scatter(torch.cat([q, k]).to(device()), columns, ld)
    v_major = layout.scatter(v.to(device()), columns, ld).t().contiguous()
    dout_packed = layout.scatter(dout.to(device()), columns, ld)
    out = torch.zeros((CHANNELS, ld), device=device())
    images = torch.empty(int(lib.emph_split_kv_bytes(
        ld, len(segments), CHANNELS, HEADS, 32)), dtype=torch.uint8,
        device=device())
    runtime.check(lib.emph_split_kv(
        qk.data_ptr(), v_major.data_ptr(), ld, CHANNELS, HEADS,
        stages.data_ptr(), n_stages, 64, 32, images.data_ptr(),
        runtime.stream()), 'emph_split_kv')
    runtime.check(lib.emph_attention_split(
        qk.data_ptr(), images.data_ptr(), out.data_ptr(), ld, CHANNELS, HEADS,
        tiles.data_ptr(), n_tiles, 256, None, 32, runtime.stream()),
        'emph_attention_split')
    size = int(lib.emph_attention_backward_split_bytes(
        ld, len(segments), CHANNELS, HEADS))
    assert size > 0
    scratch = torch.empty(size, dtype=torch.uint8, device=device())
    workspace = torch.empty(int(lib.emph_attention_backward_split_workspace(
        ld, HEADS)), device=device())
    results = []
    for _ in range(launches):
        dqkv = torch.full((3 * CHANNELS, ld), SENTINEL, device=device())
        runtime.check(lib.emph_attention_backward_split(
            qk.data_ptr(), v_major.data_ptr(), out.data_ptr(),
            dout_packed.data_ptr(), dqkv.data_ptr(), ld, CHANNELS, HEADS,
            tiles.data_ptr(), n_tiles, 256, scratch.data_ptr(),
            workspace.data_ptr(), runtime.stream()),
            'emph_attention_backward_split')
        results.append(dqkv)
    return results, layout


@pytest.mark.parametrize('kind', KINDS)
def test_attention_backward_split(kind):
    inputs = attention_inputs(kind)
    results, layout = split_backward(inputs, SEGMENTS, launches=2)
    assert torch.equal(results[0], results[1])
    dqkv = results[0]
    ld, columns = layout.plan.ld_frames, layout.frame_columns
    chosen = long_columns(SEGMENTS)
    inside = torch.zeros(ld, dtype=torch.bool, device=device())
    inside[columns[chosen.to(device())]] = True
    assert int(inside.sum()) == sum(n for n in SEGMENTS if n >= LONG_FROM)
    # every element of a long segment was written; the gaps AND the short
    # segments were left alone
    assert not bool((dqkv[:, inside] == SENTINEL).any())
    assert bool((dqkv[:, ~inside] == SENTINEL).all())
    assert bool(torch.isfinite(dqkv[:, inside]).all())
    got = dqkv.index_select(1, columns).cpu().double()[:, chosen]
    exact, narrow, emulated = attention_want(kind)
    failed = []
    for index, name in enumerate(('dQ', 'dK', 'dV')):
        rows = slice(index * CHANNELS, (index + 1) * CHANNELS)
        want = exact[index][:, chosen]
        # ('uniform': the exact dQ is zero - the scale cancels out of the
        # ratio, and every term is an absolute error)
        scale = 1. if (kind, name) == ('uniform', 'dQ') else \
            float(want.abs().max())
        emulated_error = float(
            (emulated[index][:, chosen] - want).abs().max()) / scale
        narrow_error = float(
            (narrow[index][:, chosen] - want).abs().max()) / scale
        error = float((got[rows] - want).abs().max()) / scale
        allowed = 4. * (emulated_error + narrow_error)
        print(f'attention backward split ({kind}) {name}: error {error:.3g}, '
              f'emulated {emulated_error:.3g}, float32 {narrow_error:.3g}, '
              f'bound {allowed:.3g}, ratio {error / allowed:.2f}')
        if not error <= allowed:
            failed.append((name, error, allowed))
    assert not failed, failed


def test_a_segment_does_not_depend_on_the_batch():
    inputs = attention_inputs('normal')
    (batch,), layout = split_backward(inputs, SEGMENTS)
    index = SEGMENTS.index(300)
    first = sum(SEGMENTS[:index])
    alone_inputs = [t[:, first:first + 300].contiguous() for t in inputs]
    (alone,), alone_layout = split_backward(alone_inputs, [300])
    columns = layout.frame_columns[first:first + 300]
    assert torch.equal(batch.index_select(1, columns),
                       alone.index_select(1, alone_layout.frame_columns))


def test_attention_backward_split_refuses_other_shapes():
    """Return codes of calls that launch nothing."""
    lib = runtime.library()
    layout = ops._layout(device(), np.array([256], dtype=np.int64))
    tiles, n_tiles = layout.tiles(256, engine_module.LONG)
    assert n_tiles == 1
    buffer = torch.zeros(1 << 16, device=device())
    pointer = buffer.data_ptr()
    for channels, heads in ((64, 2), (128, 2), (80, 1), (160, 4)):
        assert lib.emph_attention_backward_split(
            pointer, pointer, pointer, pointer, pointer, 256, channels, heads,
            tiles.data_ptr(), n_tiles, 256, pointer, pointer,
            runtime.stream()) == ERANGE
        assert lib.emph_attention_backward_split_bytes(
            256, 1, channels, heads) == -1
    torch.cuda.synchronize()
    assert not bool(buffer.any())


###############################################################################
# The op
###############################################################################


def layer_cu(segments):
    return torch.tensor(np.concatenate([[0], np.cumsum(segments)]))


def layer_leaves(case, requires_grad=True, dtype=torch.float32):
    x, upstream, parameters = case
    return [t.to(device(), dtype).requires_grad_(requires_grad)
            for t in (x,) + parameters], upstream.to(device())


def layer_torch32(case, segments):
    """[out, dx, twelve gradients] of the torch layer in float32 on the CPU,
    a segment at a time, as float64."""
    x, upstream, parameters = case
    module = torch.nn.TransformerEncoderLayer(
        CHANNELS, HEADS, dim_feedforward=CHANNELS, dropout=0.)
    with torch.no_grad():
        for name, value in zip(emulation.LAYER_NAMES, parameters):
            module.get_parameter(name).copy_(value)
    module.train()
    leaf = x.detach().clone().requires_grad_(True)
    outs, first = [], 0
    for count in segments:
        outs.append(module(leaf[:, first:first + count].t()[:, None])[:, 0].t())
        first += count
    out = torch.cat(outs, dim=1)
    out.backward(upstream)
    return [out.detach().double(), leaf.grad.double()] + [
        module.get_parameter(name).grad.double()
        for name in emulation.LAYER_NAMES]


def test_encoder_layer_split_gradients_against_torch():
    segments = emulation.LAYER_SEGMENTS
    case, exact, emulated, seed = emulation.layer_case()
    print(f'layer case: seed {seed}')
    narrow = layer_torch32(case, segments)
    leaves, upstream = layer_leaves(case)
    out = torch.ops.emphases_amd.encoder_layer_split(
        *leaves, layer_cu(segments), HEADS, 'bf16x3')
    assert out.requires_grad
    out.backward(upstream)
    got = [out.detach()] + [leaf.grad for leaf in leaves]
    names = ('out', 'dx') + tuple('d ' + name for name in emulation.LAYER_NAMES)
    failed = []
    for name, value, want, split, rounded, leaf in zip(
            names, got, exact, emulated, narrow, [leaves[0]] + leaves):
        assert value.shape == leaf.shape and value.dtype == leaf.dtype
        scale = float(want.abs().max())
        emulated_error = float((split - want).abs().max()) / scale
        narrow_error = float((rounded - want).abs().max()) / scale
        error = float((value.cpu().double() - want).abs().max()) / scale
        allowed = 4. * (emulated_error + narrow_error)
        print(f'encoder_layer_split {name}: error {error:.3g}, emulated '
              f'{emulated_error:.3g}, float32 {narrow_error:.3g}, bound '
              f'{allowed:.3g}, ratio {error / allowed:.2f}')
        if not error <= allowed:
            failed.append((name, error, allowed))
    assert not failed, failed
    # float64 leaves get float64 gradients
    doubles, _ = layer_leaves(case, dtype=torch.float64)
    out = torch.ops.emphases_amd.encoder_layer_split(
        *doubles, layer_cu(segments), HEADS, 'bf16x3')
    out.backward(upstream)
    assert all(leaf.grad.dtype == torch.float64 for leaf in doubles)
    assert torch.equal(doubles[0].grad.float(), leaves[0].grad)


def test_short_segments_alone_give_the_bits_of_encoder_layer():
    """No segment of 128 positions: the launches of `encoder_layer` on
    updated parameters, bit for bit."""
    segments = [1, 17, 64, 127]
    case = emulation._layer_case(emulation.FIRST_LAYER_SEED, tuple(segments))
    results = []
    for split in (False, True):
        leaves, upstream = layer_leaves(case)
        # (the op sees the parameters first, then one of them moves)
        assert not any([ops._weight_changes(leaf) for leaf in leaves[1:]])
        with torch.no_grad():
            leaves[7].add_(0)                  # what an optimizer step does
        assert ops._weight_changes(leaves[7])
        if split:
            out = torch.ops.emphases_amd.encoder_layer_split(
                *leaves, layer_cu(segments), HEADS, 'bf16x3')
        else:
            out = torch.ops.emphases_amd.encoder_layer(
                *leaves, layer_cu(segments), HEADS)
        out.backward(upstream)
        results.append([out.detach()] + [leaf.grad for leaf in leaves])
    for plain, split in zip(*results):
        assert torch.equal(plain, split)


def test_opcheck_encoder_layer_split():
    case = emulation._layer_case(emulation.FIRST_LAYER_SEED, (3, 140))
    leaves, _ = layer_leaves(case)
    torch.library.opcheck(
        torch.ops.emphases_amd.encoder_layer_split.default,
        (*leaves, torch.tensor([0, 3, 143]), HEADS, 'bf16x3'),
        test_utils=('test_schema', 'test_autograd_registration',
                    'test_faketensor'))


def test_second_backward_of_encoder_layer_split_raises():
    case = emulation._layer_case(emulation.FIRST_LAYER_SEED, (3, 140))
    leaves, upstream = layer_leaves(case)
    out = torch.ops.emphases_amd.encoder_layer_split(
        *leaves, torch.tensor([0, 3, 143]), HEADS, 'bf16x3')
    with pytest.raises(RuntimeError, match='differentiable once'):
        torch.autograd.grad((out * upstream).sum(), leaves[7],
                            create_graph=True)


###############################################################################
# TransformerModel
###############################################################################


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLDEN, 'transformer_train.npz')) as data:
        return {name: data[name] for name in data.files}


def golden_batch():
    data = golden()
    cu = lambda counts: torch.from_numpy(  # noqa: E731
        np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    return (torch.from_numpy(data['features']).to(device()),
            cu(data['frames']), torch.from_numpy(data['bounds']),
            cu(data['words'])), torch.from_numpy(data['targets']).to(device())


def golden_model(name, precision='bf16x3'):
    config = emphases_amd.Config(
        architecture='transformer', layers=2,
        **emulation.GOLDEN_CONFIGS[name])
    return train.TransformerModel(
        config, seed=int(golden()[f'{name}/seed']),
        precision=precision).to(device())


def emulated_errors(name):
    """(of the loss, of the logits, {parameter: of its gradient}): the
    emulation (c) against its own split=False, over max |want|."""
    results = emulation.golden_results(GOLDEN, name)
    (loss, logits, grads, _), (split_loss, split_logits, split_grads, _) = \
        results[False], results[True]
    return (abs(split_loss - loss) / abs(loss),
            np.abs(split_logits - logits).max() / np.abs(logits).max(),
            {key: np.abs(split_grads[key] - grads[key]).max() /
             np.abs(grads[key]).max() for key in grads})


@pytest.mark.parametrize('name', list(emulation.GOLDEN_CONFIGS))
def test_transformer_model_bf16x3_matches_the_reference(name):
    data = golden()
    reference_error = float(data[f'{name}/ref32_error'])
    loss_emulated, logits_emulated, emulated = emulated_errors(name)
    batch, targets = golden_batch()
    model = golden_model(name)
    assert max(int(n) for n in data['frames']) >= LONG_FROM
    results = []
    for mode in ('train', 'eval'):
        getattr(model, mode)()
        model.zero_grad(set_to_none=True)
        logits = model(*batch)
        loss = train.loss_fn(logits, targets, 'bce')
        loss.backward()
        results.append([logits.detach(), loss.detach()] + [
            parameter.grad.clone() for parameter in model.parameters()])
    # train() and eval() compute the same function, and the same batch twice
    # gives the same bits
    for one, other in zip(*results):
        assert torch.equal(one, other)
    want_loss = float(data[f'{name}/loss'])
    loss_error = abs(float(loss.detach()) - want_loss) / abs(want_loss)
    want_logits = data[f'{name}/logits']
    logit_error = np.abs(logits.detach().cpu().numpy().astype(np.float64) -
                         want_logits).max() / np.abs(want_logits).max()
    loss_allowed = 4. * (reference_error + loss_emulated)
    logit_allowed = 4. * (reference_error + logits_emulated)
    print(f'{name}: loss {float(loss.detach()):.9g} (reference '
          f'{want_loss:.9g}) error {loss_error:.3g}, bound {loss_allowed:.3g}; '
          f'logits {logit_error:.3g}, bound {logit_allowed:.3g}')
    missed = {}
    with np.load(os.path.join(
            GOLDEN, f'transformer_train_grads_{name}.npz')) as wanted:
        assert set(wanted.files) == {
            key for key, _ in model.named_parameters()}
        for key, parameter in model.named_parameters():
            want = wanted[key].astype(np.float64)
            got = parameter.grad.cpu().numpy().astype(np.float64)
            assert got.shape == want.shape
            error = np.abs(got - want).max() / np.abs(want).max()
            allowed = 4. * (reference_error + emulated[key])
            print(f'{name} {key}: error {error:.3g}, emulated '
                  f'{emulated[key]:.3g}, bound {allowed:.3g}, ratio '
                  f'{error / allowed:.2f}')
            if not error <= allowed:
                missed[key] = (error, allowed)
    assert loss_error <= loss_allowed
    assert logit_error <= logit_allowed
    assert not missed, missed


def test_transformer_model_bf16x3_trains_saves_and_infers():
    """Five Adam steps end below the first loss; the state loads into an f32
    model; the engine at precision='bf16x3' agrees with the model's eval
    logits within the bound the logits are held to."""
    name = 'intermediate_sum'
    batch, targets = golden_batch()
    model = golden_model(name)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(5):
        optimizer.zero_grad(set_to_none=True)
        loss = train.loss_fn(model(*batch), targets, 'bce')
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
    model.eval()
    with torch.no_grad():
        logits = model(*batch)
        losses.append(float(train.loss_fn(logits, targets, 'bce')))
    print('losses', ' '.join(f'{loss:.9g}' for loss in losses))
    assert losses[-1] < losses[0], losses

    # checkpoints do not record the precision
    plain = golden_model(name, precision='f32')
    assert list(plain.state_dict()) == list(model.state_dict())
    plain.load_state_dict(model.state_dict())
    for (key, one), (_, other) in zip(model.named_parameters(),
                                      plain.named_parameters()):
        assert torch.equal(one, other), key
    state = weights.load(model.state_dict(), model.config)
    engine = engine_module.Engine(model.config, state, 0, precision='bf16x3')
    data = golden()
    layout = ops._layout(device(), data['frames'], data['words'],
                         np.ascontiguousarray(data['bounds']))
    plan = layout.plan
    packed = layout.scatter(batch[0], layout.frame_columns, plan.ld_frames)
    with engine.lock:
        _, engine_logits = engine.forward(None, plan, features=packed)
        engine_logits = engine_logits[
            torch.from_numpy(plan.word_columns()).to(device())].clone()
    allowed = 4. * (float(data[f'{name}/ref32_error']) +
                    emulated_errors(name)[1])
    scale = float(logits.abs().max())
    apart = float((engine_logits - logits).abs().max()) / scale
    print(f'engine (bf16x3) against model logits: {apart:.3g}, bound '
          f'{allowed:.3g}, ratio {apart / allowed:.2f}')
    assert apart <= allowed
