"""`encoder_layer` under autograd on the MI355X: the two backward kernels
alone, the op against `torch.nn.TransformerEncoderLayer` in float64,
`torch.library.opcheck`, and `train.TransformerModel` against the reference's
float64 run (tests/golden/transformer_train*.npz) and against the inference
engine.

Every bound is 4 x the error of the same computation in float32 on the CPU
against float64, per tensor, scaled by max |want| (the convention of
`test_gpu_ops_autograd`): torch's for the kernels and the op (computed here),
the reference's own for the goldens (`ref32_error`).  Each figure is printed
before it is asserted.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

import emphases_amd
from emphases_amd import engine as engine_module
from emphases_amd import ops, runtime, train, weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CHANNELS, HEADS, DIM = 80, 2, 40
SENTINEL = 12345.
ATTENTION_SEGMENTS = [1, 2, 15, 16, 17, 63, 64, 65, 130, 257, 300]
NORM_SEGMENTS = [1, 17, 64, 130]
LAYER_SEGMENTS = [1, 17, 64, 130, 257]


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


###############################################################################
# emph_attention_backward
###############################################################################


def attention_inputs(kind):
    """(q, k, v, dout) [80, sum T] on the CPU, float32."""
    generator = torch.Generator().manual_seed(
        {'normal': 1, 'peaked': 2, 'uniform': 3}[kind])
    total = sum(ATTENTION_SEGMENTS)
    q, k, v, dout = (torch.randn(CHANNELS, total, generator=generator)
                     for _ in range(4))
    if kind == 'peaked':
        # logits q.k / sqrt(40) of unit-normal rows have a standard deviation
        # of 1; sqrt(8) on either side makes it 8
        q, k = q * math.sqrt(8.), k * math.sqrt(8.)
    if kind == 'uniform':
        first = 0
        for count in ATTENTION_SEGMENTS:
            k[:, first:first + count] = k[:, first:first + 1]
            first += count
    return q, k, v, dout


def attention_autograd(q, k, v, dout, dtype):
    """(dq, dk, dv) [80, sum T] of the per-segment, per-head softmax
    attention by torch autograd in `dtype`."""
    leaves = [t.detach().clone().to(dtype).requires_grad_(True)
              for t in (q, k, v)]
    first = 0
    for count in ATTENTION_SEGMENTS:
        for head in range(HEADS):
            rows = slice(head * DIM, (head + 1) * DIM)
            part = [leaf[rows, first:first + count] for leaf in leaves]
            scores = part[0].t() @ part[1] / math.sqrt(DIM)
            out = torch.softmax(scores, dim=1) @ part[2].t()        # [T, d]
            out.backward(dout[rows, first:first + count].t().to(dtype))
        first += count
    return [leaf.grad.double() for leaf in leaves]


@functools.lru_cache(maxsize=None)
def attention_want(kind):
    inputs = attention_inputs(kind)
    return (attention_autograd(*inputs, torch.float64),
            attention_autograd(*inputs, torch.float32))


@pytest.mark.parametrize('kind', ['normal', 'peaked', 'uniform'])
def test_attention_backward(kind):
    q, k, v, dout = attention_inputs(kind)
    layout = ops._layout(
        device(), np.array(ATTENTION_SEGMENTS, dtype=np.int64))
    ld = layout.plan.ld_frames
    columns = layout.frame_columns
    tiles, n_tiles = layout.tiles(64)
    assert n_tiles == sum((n + 63) // 64 for n in ATTENTION_SEGMENTS)
    lib = runtime.library()
    qk = layout.scatter(torch.cat([q, k]).to(device()), columns, ld)
    v_major = layout.scatter(v.to(device()), columns, ld).t().contiguous()
    dout_packed = layout.scatter(dout.to(device()), columns, ld)
    out = torch.zeros((CHANNELS, ld), device=device())
    runtime.check(lib.emph_attention(
        qk.data_ptr(), v_major.data_ptr(), out.data_ptr(), ld, CHANNELS, HEADS,
        tiles.data_ptr(), n_tiles, 64, None, runtime.stream()),
        'emph_attention')
    workspace = torch.empty(
        int(lib.emph_attention_backward_workspace(ld, HEADS)), device=device())
    results = []
    for _ in range(2):
        dqkv = torch.full((3 * CHANNELS, ld), SENTINEL, device=device())
        runtime.check(lib.emph_attention_backward(
            qk.data_ptr(), v_major.data_ptr(), out.data_ptr(),
            dout_packed.data_ptr(), dqkv.data_ptr(), ld, CHANNELS, HEADS,
            tiles.data_ptr(), n_tiles, 64, workspace.data_ptr(),
            runtime.stream()), 'emph_attention_backward')
        results.append(dqkv)
    assert torch.equal(results[0], results[1])
    dqkv = results[0]
    inside = torch.zeros(ld, dtype=torch.bool, device=device())
    inside[columns] = True
    assert int(inside.sum()) == sum(ATTENTION_SEGMENTS) < ld
    # every element inside a segment was written; the gaps were left alone
    assert not bool((dqkv[:, inside] == SENTINEL).any())
    assert bool((dqkv[:, ~inside] == SENTINEL).all())
    assert bool(torch.isfinite(dqkv[:, inside]).all())
    got = dqkv.index_select(1, columns)
    exact, narrow = attention_want(kind)
    for index, name in enumerate(('dQ', 'dK', 'dV')):
        check(f'attention backward ({kind}) {name}',
              got[index * CHANNELS:(index + 1) * CHANNELS], exact[index],
              narrow[index])


def test_attention_backward_refuses_other_shapes():
    """Return codes of calls that launch nothing."""
    lib = runtime.library()
    layout = ops._layout(device(), np.array([64], dtype=np.int64))
    tiles, n_tiles = layout.tiles(64)
    buffer = torch.zeros(1 << 16, device=device())
    pointer = buffer.data_ptr()
    for channels, heads in ((64, 2), (128, 2), (80, 1), (160, 4)):
        assert lib.emph_attention_backward(
            pointer, pointer, pointer, pointer, pointer, 64, channels, heads,
            tiles.data_ptr(), n_tiles, 64, pointer, runtime.stream()) == -2
    torch.cuda.synchronize()
    assert not bool(buffer.any())


###############################################################################
# emph_add_layernorm_backward
###############################################################################


@pytest.mark.parametrize('channels', [80, 128])
def test_add_layernorm_backward(channels):
    generator = torch.Generator().manual_seed(channels)
    total = sum(NORM_SEGMENTS)
    summed = torch.randn(channels, total, generator=generator)
    summed[:, 20] = 0.5            # a constant column: variance 0
    gamma = 1. + 0.1 * torch.randn(channels, generator=generator)
    beta = 0.1 * torch.randn(channels, generator=generator)
    dy = torch.randn(channels, total, generator=generator)
    eps = 1e-5

    def autograd(dtype):
        leaves = [t.detach().clone().to(dtype).requires_grad_(True)
                  for t in (summed, gamma, beta)]
        out = torch.nn.functional.layer_norm(
            leaves[0].t(), (channels,), leaves[1], leaves[2], eps)
        out.backward(dy.t().to(dtype))
        return [leaf.grad.double() for leaf in leaves]
    exact, narrow = autograd(torch.float64), autograd(torch.float32)

    layout = ops._layout(device(), np.array(NORM_SEGMENTS, dtype=np.int64))
    ld, columns = layout.plan.ld_frames, layout.frame_columns
    tiles, n_tiles = layout.tiles(64)
    lib = runtime.library()
    # what lies between the segments must reach no sum
    packed = torch.full((channels, ld), float('nan'), device=device())
    packed[:, columns] = summed.to(device())
    dy_packed = torch.full((channels, ld), float('nan'), device=device())
    dy_packed[:, columns] = dy.to(device())
    parts = int(lib.emph_add_layernorm_backward_parts(n_tiles))
    assert parts == n_tiles
    workspace = torch.empty(parts * 2 * channels, device=device())
    gamma_device = gamma.to(device())
    results = []
    for _ in range(2):
        ds = torch.full((channels, ld), SENTINEL, device=device())
        dgamma = torch.full((channels,), SENTINEL, device=device())
        dbeta = torch.full((channels,), SENTINEL, device=device())
        runtime.check(lib.emph_add_layernorm_backward(
            packed.data_ptr(), gamma_device.data_ptr(), dy_packed.data_ptr(),
            ds.data_ptr(), ld, channels, eps, tiles.data_ptr(), n_tiles, 64,
            workspace.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
            runtime.stream()), 'emph_add_layernorm_backward')
        results.append((ds, dgamma, dbeta))
    for one, other in zip(*results):
        assert torch.equal(one, other)
    ds, dgamma, dbeta = results[0]
    inside = torch.zeros(ld, dtype=torch.bool, device=device())
    inside[columns] = True
    assert bool(torch.isfinite(ds[:, inside]).all())
    assert bool((ds[:, ~inside] == SENTINEL).all())
    check(f'layernorm backward ({channels}) ds', ds.index_select(1, columns),
          exact[0], narrow[0])
    check(f'layernorm backward ({channels}) dgamma', dgamma, exact[1], narrow[1])
    check(f'layernorm backward ({channels}) dbeta', dbeta, exact[2], narrow[2])


def test_add_layernorm_backward_many_tiles():
    """More tiles than slabs: runs of two tiles (520 one-column segments)."""
    channels, count = 80, 520
    generator = torch.Generator().manual_seed(7)
    summed = torch.randn(channels, count, generator=generator)
    dy = torch.randn(channels, count, generator=generator)
    gamma = torch.ones(channels)
    layout = ops._layout(device(), np.ones(count, dtype=np.int64))
    ld, columns = layout.plan.ld_frames, layout.frame_columns
    tiles, n_tiles = layout.tiles(64)
    lib = runtime.library()
    parts = int(lib.emph_add_layernorm_backward_parts(n_tiles))
    assert n_tiles == count and parts == count // 2
    packed = layout.scatter(summed.to(device()), columns, ld)
    dy_packed = layout.scatter(dy.to(device()), columns, ld)
    workspace = torch.empty(parts * 2 * channels, device=device())
    ds = torch.zeros((channels, ld), device=device())
    dgamma = torch.zeros(channels, device=device())
    dbeta = torch.zeros(channels, device=device())
    runtime.check(lib.emph_add_layernorm_backward(
        packed.data_ptr(), gamma.to(device()).data_ptr(), dy_packed.data_ptr(),
        ds.data_ptr(), ld, channels, 1e-5, tiles.data_ptr(), n_tiles, 64,
        workspace.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
        runtime.stream()), 'emph_add_layernorm_backward')
    wide, wide_dy = summed.double(), dy.double()
    xhat = (wide - wide.mean(0)) / torch.sqrt(wide.var(0, unbiased=False) + 1e-5)
    narrow_hat = (summed - summed.mean(0)) / torch.sqrt(
        summed.var(0, unbiased=False) + 1e-5)
    check('layernorm backward (520 tiles) dgamma', dgamma,
          (wide_dy * xhat).sum(1), (dy * narrow_hat).sum(1))
    check('layernorm backward (520 tiles) dbeta', dbeta, wide_dy.sum(1),
          dy.sum(1))


###############################################################################
# The op
###############################################################################

LAYER_NAMES = ('self_attn.in_proj_weight', 'self_attn.in_proj_bias',
               'self_attn.out_proj.weight', 'self_attn.out_proj.bias',
               'norm1.weight', 'norm1.bias', 'linear1.weight', 'linear1.bias',
               'linear2.weight', 'linear2.bias', 'norm2.weight', 'norm2.bias')


def layer_cu(segments=LAYER_SEGMENTS):
    return torch.tensor(np.concatenate([[0], np.cumsum(segments)]))


@functools.lru_cache(maxsize=None)
def layer_case(channels=CHANNELS, segments=tuple(LAYER_SEGMENTS)):
    """x, upstream [C, sum T] and the twelve parameters (the op's order) of a
    seeded `TransformerEncoderLayer`, on the CPU in float32."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        module = torch.nn.TransformerEncoderLayer(
            channels, HEADS, dim_feedforward=channels, dropout=0.)
        values = dict(module.named_parameters())
        parameters = []
        for name in LAYER_NAMES:
            value = values[name].detach().clone()
            if 'norm' in name or name.endswith('bias'):
                # (torch starts them at 1 and 0)
                value = value + 0.1 * torch.randn(value.shape)
            parameters.append(value)
        x = torch.randn(channels, sum(segments))
        upstream = torch.randn(channels, sum(segments))
    return x, upstream, tuple(parameters)


def layer_torch(dtype):
    """(out, dx, twelve gradients) of the torch layer, a segment at a time."""
    x, upstream, parameters = layer_case()
    module = torch.nn.TransformerEncoderLayer(
        CHANNELS, HEADS, dim_feedforward=CHANNELS, dropout=0.).to(dtype)
    with torch.no_grad():
        for name, value in zip(LAYER_NAMES, parameters):
            module.get_parameter(name).copy_(value.to(dtype))
    module.train()
    leaf = x.detach().clone().to(dtype).requires_grad_(True)
    outs, first = [], 0
    for count in LAYER_SEGMENTS:
        outs.append(module(leaf[:, first:first + count].t()[:, None])[:, 0].t())
        first += count
    out = torch.cat(outs, dim=1)
    out.backward(upstream.to(dtype))
    return [out.detach().double(), leaf.grad.double()] + \
        [module.get_parameter(name).grad.double() for name in LAYER_NAMES]


@functools.lru_cache(maxsize=None)
def layer_want():
    return layer_torch(torch.float64), layer_torch(torch.float32)


def layer_leaves(requires_grad=True):
    x, upstream, parameters = layer_case()
    return [t.to(device()).requires_grad_(requires_grad)
            for t in (x,) + parameters], upstream.to(device())


def test_encoder_layer_gradients_against_torch():
    exact, narrow = layer_want()
    leaves, upstream = layer_leaves()
    out = torch.ops.emphases_amd.encoder_layer(*leaves, layer_cu(), HEADS)
    assert out.requires_grad
    out.backward(upstream)
    got = [out.detach()] + [leaf.grad for leaf in leaves]
    names = ('out', 'dx') + tuple('d ' + name for name in LAYER_NAMES)
    for name, value, want, rounded, leaf in zip(
            names, got, exact, narrow, [leaves[0]] + leaves):
        assert value.shape == leaf.shape and value.dtype == leaf.dtype
        check(f'encoder_layer {name}', value, want, rounded)
    # never-updated parameters: the same output bits with and without grad
    plain, _ = layer_leaves(requires_grad=False)
    again = torch.ops.emphases_amd.encoder_layer(*plain, layer_cu(), HEADS)
    assert not again.requires_grad
    assert torch.equal(again, out.detach())


def test_encoder_layer_after_an_update_and_in_double():
    """A parameter set whose version has changed runs the unfused,
    device-packed sequence: output and gradients within the same bounds; the
    gradients come back in the inputs' dtypes."""
    exact, narrow = layer_want()
    leaves, upstream = layer_leaves()
    assert not any([ops._weight_changes(leaf) for leaf in leaves[1:]])
    with torch.no_grad():
        leaves[7].add_(0)                      # what an optimizer step does
    assert ops._weight_changes(leaves[7])
    out = torch.ops.emphases_amd.encoder_layer(*leaves, layer_cu(), HEADS)
    out.backward(upstream)
    check('updated encoder_layer out', out, exact[0], narrow[0])
    check('updated encoder_layer dx', leaves[0].grad, exact[1], narrow[1])
    check('updated encoder_layer d linear1.weight', leaves[7].grad, exact[8],
          narrow[8])
    doubles = [leaf.detach().double().requires_grad_(True) for leaf in leaves]
    out = torch.ops.emphases_amd.encoder_layer(*doubles, layer_cu(), HEADS)
    out.backward(upstream)
    assert all(leaf.grad.dtype == torch.float64 for leaf in doubles)
    check('float64 leaves dx', doubles[0].grad, exact[1], narrow[1])


def test_opcheck_encoder_layer():
    leaves, _ = layer_leaves()
    cu = torch.tensor([0, 3, 70])
    leaves[0] = leaves[0][:, :70].detach().clone().requires_grad_(True)
    torch.library.opcheck(
        torch.ops.emphases_amd.encoder_layer.default, (*leaves, cu, HEADS),
        test_utils=('test_schema', 'test_autograd_registration',
                    'test_faketensor'))


def test_second_backward_raises_and_unasked_gradients_are_skipped():
    leaves, upstream = layer_leaves(requires_grad=False)
    leaves[11].requires_grad_(True)            # norm2.weight alone
    leaves[7].requires_grad_(True)             # ... and linear1.weight
    out = torch.ops.emphases_amd.encoder_layer(*leaves, layer_cu(), HEADS)
    with pytest.raises(RuntimeError, match='differentiable once'):
        torch.autograd.grad((out * upstream).sum(), leaves[7],
                            create_graph=True)
    out = torch.ops.emphases_amd.encoder_layer(*leaves, layer_cu(), HEADS)
    out.backward(upstream)
    exact, narrow = layer_want()
    check('d norm2.weight alone', leaves[11].grad, exact[12], narrow[12])
    check('d linear1.weight alone', leaves[7].grad, exact[8], narrow[8])
    assert all(leaf.grad is None for index, leaf in enumerate(leaves)
               if index not in (7, 11))
    # the walk back stops where nothing upstream asks: launches counted on
    # this thread (the library's own timer)
    counts = {}
    layout = ops._layout(device(), np.array(LAYER_SEGMENTS, dtype=np.int64))
    for name, need in (('all', [True] * 13),
                       ('norm2', [False] * 11 + [True, True]),
                       ('linear1', [False] * 7 + [True] + [False] * 5)):
        run = ops._LayerRun(leaves[0].detach(), [t.detach() for t in leaves[1:]],
                            HEADS, layout, 0)
        with runtime.LaunchTimer() as timer:
            grads = run.backward(upstream, need)
        counts[name] = timer.launches
        assert [g is not None for g in grads] == need
    print('launches of the backward:', counts)
    # norm2 alone: emph_add_layernorm_backward's two launches
    assert counts['norm2'] == 2 < counts['linear1'] < counts['all']


def test_layer_engine_cache_answers_for_its_own_tensors_alone():
    """The fused path (untouched parameters): `out_proj_weight.t()` shares
    address, version and shape with `out_proj_weight` and must get an engine
    of its own; an entry keeps no parameter alive."""
    import gc
    import weakref
    leaves, _ = layer_leaves(requires_grad=False)
    segments = [17, 64]
    leaves[0] = leaves[0][:, :sum(segments)].contiguous()
    cu = layer_cu(segments)

    def layer(out_proj_weight):
        return torch.ops.emphases_amd.encoder_layer(
            *leaves[:3], out_proj_weight, *leaves[4:], cu, HEADS)
    first = layer(leaves[3])
    turned = layer(leaves[3].t())
    assert torch.equal(turned, layer(leaves[3].t().contiguous()))
    assert not torch.equal(turned, first)
    alive = weakref.ref(leaves[3].untyped_storage())
    del leaves
    gc.collect()
    assert alive() is None


def test_backward_refuses_other_shapes():
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5)
        module = torch.nn.TransformerEncoderLayer(
            64, HEADS, dim_feedforward=64, dropout=0.)
        x = torch.randn(64, 70)
    values = dict(module.named_parameters())
    leaves = [x.to(device()).requires_grad_(True)] + [
        values[name].detach().to(device()).requires_grad_(True)
        for name in LAYER_NAMES]
    out = torch.ops.emphases_amd.encoder_layer(
        *leaves, torch.tensor([0, 3, 70]), HEADS)
    assert out.shape == (64, 70)               # the forward takes 64 channels
    with pytest.raises(NotImplementedError, match='channels'):
        out.sum().backward()


###############################################################################
# TransformerModel
###############################################################################

CONFIGS = {
    'intermediate_sum': dict(downsample_location='intermediate',
                             downsample_method='sum'),
    'loss_max': dict(downsample_location='loss', downsample_method='max'),
}


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


def golden_model(name):
    config = emphases_amd.Config(
        architecture='transformer', layers=2, **CONFIGS[name])
    return train.TransformerModel(
        config, seed=int(golden()[f'{name}/seed'])).to(device())


@pytest.mark.parametrize('name', list(CONFIGS))
def test_transformer_model_matches_the_reference(name):
    data = golden()
    reference_error = float(data[f'{name}/ref32_error'])
    batch, targets = golden_batch()
    model = golden_model(name)
    model.train()
    logits = model(*batch)
    loss = train.loss_fn(logits, targets, 'bce')
    loss.backward()
    want_loss = float(data[f'{name}/loss'])
    loss_error = abs(float(loss.detach()) - want_loss) / abs(want_loss)
    want_logits = data[f'{name}/logits']
    logit_error = np.abs(logits.detach().cpu().numpy().astype(np.float64) -
                         want_logits).max() / np.abs(want_logits).max()
    print(f'{name}: loss {float(loss.detach()):.9g} (reference {want_loss:.9g}) error '
          f'{loss_error / reference_error:.2f}, logits '
          f'{logit_error / reference_error:.2f} (x ref32_error '
          f'{reference_error:.3g})')
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
            print(f'{name} {key}: error {error / reference_error:.2f} '
                  '(x ref32_error)')
            if not error <= 4. * reference_error:
                missed[key] = error
    assert loss_error <= 4. * reference_error
    assert logit_error <= 4. * reference_error
    assert not missed, (missed, reference_error)


def test_transformer_model_trains_saves_and_infers():
    """Five Adam steps lower the loss; the trained state loads through
    `weights.load`; the inference engine, given that state and the same
    batch, agrees with the model's eval-mode logits."""
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
    # (Adam's first steps move every weight by about lr whatever its
    # gradient: the loss need not fall at EVERY step, and does not)
    assert losses[-1] < losses[0], losses

    state = weights.load(model.state_dict(), model.config)
    for key, parameter in model.named_parameters():
        assert np.array_equal(state[key], parameter.detach().cpu().numpy())
    engine = engine_module.Engine(model.config, state, 0)
    data = golden()
    layout = ops._layout(device(), data['frames'], data['words'],
                         np.ascontiguousarray(data['bounds']))
    plan = layout.plan
    packed = layout.scatter(batch[0], layout.frame_columns, plan.ld_frames)
    with engine.lock:
        _, engine_logits = engine.forward(None, plan, features=packed)
        engine_logits = engine_logits[
            torch.from_numpy(plan.word_columns()).to(device())].clone()
    reference_error = float(data[f'{name}/ref32_error'])
    scale = float(logits.abs().max())
    apart = float((engine_logits - logits).abs().max()) / scale
    print(f'engine against model logits: {apart / reference_error:.2f} '
          f'(x ref32_error {reference_error:.3g})')
    assert apart <= 4. * reference_error
