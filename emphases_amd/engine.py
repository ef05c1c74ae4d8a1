"""Device-side execution of the prominence path on one MI355X.

`Engine` owns the immutable per-(checkpoint, device) state — MFMA-ordered
weight packs, biases, the front-end tables, the sparse mel basis — and runs a
`batch.Plan` through the HIP kernels of libemphases_hip.so:

    audio -> log-mel (+loudness) -> input conv -> frame encoder (conv stack or
    transformer) -> word-boundary reduce -> word decoder -> output conv ->
    sigmoid/clamp

which is `Model.forward` + `postprocess` of the reference
(`emphases/model/core.py:39-138`, `emphases/core.py:335-342`) for every chunk
of the batch at once, with per-chunk (B=1) edge semantics.  The reference
keeps its model on function attributes of `infer` (`core.py:298-315`); here the
cache is an explicit object.
"""
import contextlib
import dataclasses
import functools
import os
import ctypes
import threading
import types
import typing

import numpy as np
import torch

from . import config as cfg
from . import melbasis
from . import runtime
from . import weights as weights_module

FRONTEND_BLOCK = None   # frames per front-end tile: emph_frontend_block()
# `precision` of an engine -> (bf16 pieces per operand of the frame-rate convs,
# `pieces` code of emph_attention_split, pieces per operand of the Transformer's
# projections and position-wise GEMMs: csrc/block_split.hip); 0: the fp32 kernels.
#   'bf16x3'       convs: two pieces, three products per term.  Attention: THREE pieces
#                  for queries and keys (six products: the scores' error sits in front
#                  of an exponential and would grow with their range), two behind the
#                  softmax.  Projections and block: three pieces (24 GEMMs and 12
#                  LayerNorms in a row: with two, 2e-5 on the scores of configs[2];
#                  with three, 2e-6 - the f32 kernels' own noise)
#   'bf16x3_fast'  ... two pieces there too: every GEMM but the scores at three
#                  products per term
#   'bf16x6'       attention, projections and block: three pieces everywhere (fp32
#                  grade); the convs stay fp32 (six products of the direct form would
#                  not beat fp32 F(4,3))
PRECISIONS = {'f32': (0, 0, 0), 'bf16x3': (2, 32, 3), 'bf16x3_fast': (2, 32, 2),
              'bf16x6': (0, 3, 3)}
ATTENTION_BLOCK = 64    # queries per attention wave (csrc/transformer.hip)
ATTENTION_GROUP = 256   # queries per attention workgroup (LDS-staged keys/values)
# Which kernel takes a segment depends on the segment alone (scores must not
# depend on the rest of the batch): frame-axis segments of at least
# GROUPED_FROM positions take the workgroup attention kernel, shorter ones the
# one-wave kernel; word-axis segments of at most FUSED_WORDS words take the
# one-launch decoder (csrc/word_transformer.hip), longer ones the per-layer
# kernels.
GROUPED_FROM = ATTENTION_GROUP // 2
FUSED_WORDS = 64
EVERYTHING = 1 << 30
SHORT, LONG = (0, GROUPED_FROM - 1), (GROUPED_FROM, EVERYTHING)
FEW_WORDS, MANY_WORDS = (0, FUSED_WORDS), (FUSED_WORDS + 1, EVERYTHING)
WORD_TILE = 16
SPAN_FIELDS = 8         # int32 fields per span of the conv stack (batch.py)
WINOGRAD_LDS_BUDGET = 160 * 1024
# the packed frame axis a launch may address: the 16-position split kernels
# take ld < 2^22 (csrc/block_split16.hip), the 32-position ones and the fp32
# projection / block / conv kernels less than 2^28 or 2^29.  A plan at or past
# the limit of its engine runs as consecutive sub-plans below it (`forward`)
SPLIT16_COLUMNS = 1 << 22
KERNEL_COLUMNS = 1 << 28
HEAD_DIMS = (32, 40, 64)


# (what `Engine.features` and `data.preprocess.datasets` say without a tracker)
TRACKS_NEEDED = (
    'pitch/periodicity features come from the third-party '
    '`penn` tracker; pass its outputs as tracks '
    '[2, ld_frames] (see core.from_alignments_and_audios '
    'pitch_tracker=)')


def check_supported(config, precision='f32'):
    """Raise ValueError for a configuration the kernels cannot run, before
    anything is allocated or launched: the limits the EMPH_REQUIRE checks of
    the kernels a configuration selects impose."""
    if precision not in PRECISIONS:
        raise ValueError(
            f'precision {precision!r} is not one of {sorted(PRECISIONS)}')
    channels = config.channels
    if channels > 128:
        # emph_segment_reduce, emph_add_layernorm, emph_word_decoder
        raise ValueError(f'channels {channels} > 128: the word reduce and '
                         'the LayerNorm hold at most 128 channels')
    if config.architecture == 'transformer':
        head_dim = channels // config.heads
        if head_dim not in HEAD_DIMS:
            # emph_attention, emph_attention_split
            raise ValueError(
                f'head dimension {head_dim} (channels {channels} / heads '
                f'{config.heads}) not in {{32, 40, 64}}')
    elif config.layers > 16:
        # emph_prominence_forward, emph_word_decoder
        raise ValueError(f'{config.layers} convolution layers > 16')
    if config.architecture == 'convolution' or not config.has_decoder:
        # the fused word stage (emph_word_decoder)
        if channels < 16 or channels % 16:
            raise ValueError(
                f'channels {channels} not a multiple of 16 in 16..128 (the '
                'fused word stage of this configuration)')
        if config.decoder_kernel_size not in (1, 3, 5):
            raise ValueError(
                f'decoder kernel size {config.decoder_kernel_size} not in '
                '{1, 3, 5} (the fused word stage of this configuration)')
        layers = config.layers if config.has_decoder else 0
        if runtime.library().emph_word_decoder_block(
                layers, config.decoder_kernel_size,
                config.decoder_kernel_size) < 16:
            raise ValueError(
                f'{layers} decoder layers of kernel size '
                f'{config.decoder_kernel_size}: the receptive field is too '
                "wide for the fused word stage's 64-word window")


@functools.lru_cache(maxsize=None)
def _default_mel_plan():
    """The balanced mel projection of the default basis (host, uint32), or
    None: built once per process (the placement of the lanes is a search)."""
    basis = melbasis.default()
    plan, _ = runtime.frontend_mel_plan(
        basis.row_start, basis.row_count, basis.row_offset, basis.values)
    return plan


###############################################################################
# Which kernels a configuration runs: decided once, without a device
###############################################################################


def conv_forms(c_out, c_in, kernel_size, winograd=True):
    """(F(2,3), F(4,3)): the Winograd packs a Conv1d of this shape gets, the
    frame-rate k = 3 layers whose transformed weights fit in one CU's LDS
    next to the output patches.  F(4,3): half the MFMA work, identity /
    ReLU, 64-position tiles."""
    if not winograd or kernel_size != 3:
        return False, False
    return (
        runtime.conv_winograd_lds_bytes(c_out, c_in) <= WINOGRAD_LDS_BUDGET,
        c_out <= 96 and c_in % 4 == 0 and
        runtime.conv_winograd4_lds_bytes(c_out, c_in) <= WINOGRAD_LDS_BUDGET)


class LayerPacks(typing.NamedTuple):
    """The fused forms one Transformer layer has weight packs for (every
    layer also carries the k = 1 convs and LayerNorm vectors of the per-layer
    form)."""
    qkv: bool           # Q / K / V projections as one launch, fp32
    block: bool         # the position-wise half as one launch, fp32
    split: bool         # both on the bf16 matrix pipe (csrc/block_split*.hip)
    block_qkv: bool     # block + the NEXT layer's projections, fp32


class LayerForm(typing.NamedTuple):
    """How one Transformer layer runs in one `Engine._transformer` call."""
    project: str        # 'split' | 'fused' | 'convs'
    block: str          # 'split' | 'fused' | 'convs'
    ahead: bool         # the block launch makes the next layer's Q / K / V too


class Route(typing.NamedTuple):
    """The launches of one batch's frame stage (`Paths.route`)."""
    one_call: bool      # emph_prominence_forward: the whole path in one C call
    stack: bool         # else emph_conv1d_stack / _composed / _split (or per layer)
    fold: bool          # per-word sums out of the last layer (or emph_segment_reduce)


@dataclasses.dataclass(frozen=True)
class Paths:
    """Everything `Engine` derives about its kernels from (configuration,
    checkpoint shapes, precision, winograd, conv_tile, EMPHASES_* switches):
    `decide` makes it, `Engine.__init__` packs by it, `forward` launches by
    it.  DESIGN.md lists the launch sequence of each class of configuration."""
    transformer: bool
    winograd: bool
    conv_tile: typing.Any
    split_pieces: int
    attention_pieces: int
    linear_pieces: int
    split_tile: int
    split_tables: bool          # tiles of `split_tile` frames are requested
    fuse_qkv: bool
    max_columns: int
    mel_plan: bool
    quad: bool
    stack: bool
    fold: bool
    split_conv: bool
    compose: bool
    sum_step: int
    fused_words: bool
    model: bool                 # the one-call model (emph_prominence_forward)
    word_transformer: bool      # the one-launch word Transformer
    frame_encoder: tuple        # LayerPacks per Transformer layer (conv: empty)
    word_decoder: tuple

    def frame_tile(self, plan):
        """Positions per conv wave on the frame axis.

        Default (`conv_tile=None`): the kernel FAMILY of a frame-rate layer is
        fixed by the configuration, never by the batch - F(4,3) (64-position
        tiles) where it is legal, else F(2,3), else the direct form - so an
        utterance's scores are bitwise the same alone, inside any batch and
        on any shard of any world size.  Within a family the tile size only
        partitions positions (same arithmetic per output), so it is picked by
        cost.  `conv_tile='auto'`: the round-3 policy, lowest latency - a
        handful of utterances takes the direct form's 16-position tiles,
        which agree with the Winograd kernels to 1e-6, not bitwise (one 10 s
        utterance: 4.6 us per layer less).

        Cost model: the chip runs 256 workgroups at a time (one per CU: the
        weights fill most of the LDS) of 4 waves (64-position tiles) or 8
        waves (16 / 32), so a launch costs (trips over the 256 CUs) x (time of
        one trip).  Microseconds per trip measured on the 80x80 k=3 layer
        (tools/micro/conv_bench.hip): Winograd 32: 24.0, Winograd 64: 26.7,
        direct 64: 33.5, direct 32: 31.3, direct 16: 16.1; Winograd F(4,3)
        (64-position tiles, identity / ReLU layers): 20.7."""
        if self.conv_tile is not None and self.conv_tile != 'auto':
            return self.conv_tile
        if self.conv_tile is None and self.quad:
            return 64
        frames = [segment.frames for segment in plan.segments]
        if self.winograd:
            cost = {64: 20.7 if self.quad else 26.7, 32: 23.2, 16: 16.1}
        else:
            cost = {64: 33.5, 32: 31.3, 16: 16.1}
        candidates = (64, 32, 16) if self.quad else (32, 64, 16)
        if self.conv_tile is None and self.winograd:
            candidates = (32, 64)       # stay inside the F(2,3) family
        best = None
        for tile in candidates:
            tiles = sum(-(-count // tile) for count in frames)
            # (four 64-position tiles per workgroup, F(4,3) included)
            waves = 4 if tile == 64 else 8
            groups = -(-tiles // waves)
            trips = -(-groups // 256)
            if best is None or trips * cost[tile] < best[0]:
                best = (trips * cost[tile], tile)
        return best[1]

    def route(self, tile, nested=False, stages=False, features=False,
              timers=False):
        """The frame stage of one batch at `tile` positions per conv wave
        (`nested`: the word pieces of another plan; `stages` / `features` /
        `timers`: whether forward() was given them).  `stack` and `fold` say
        what runs when the one call does not (an empty plan; `_pack` asks
        which tables they read: without `stages`).  By configuration and
        tile, never by batch."""
        whole = not nested and tile == 64 and not stages
        return Route(
            self.model and not (stages or features or timers) and
            not self.split_conv and
            tile in ((64,) if self.quad else (32, 64)),
            self.stack and whole, self.fold and whole)

    def forms(self, layers, fused=True, split=True):
        """`LayerForm` of each of a Transformer stack's `layers` (their
        `LayerPacks`), given the tile tables at hand: `fused` - tiles of at
        most 32 positions, which the one-launch projections and blocks own;
        `split` - of `split_tile` positions, for their split-bf16 forms."""
        result = []
        for index, packs in enumerate(layers):
            following = layers[index + 1] if index + 1 < len(layers) else None
            if fused and split and packs.split:
                result.append(LayerForm('split', 'split', bool(
                    self.fuse_qkv and following and following.split)))
                continue
            result.append(LayerForm(
                'fused' if fused and packs.qkv else 'convs',
                'fused' if fused and packs.block else 'convs',
                bool(fused and packs.block_qkv and self.fuse_qkv and
                     following)))
        return result


def decide(config, state, precision='f32', winograd=True, conv_tile=None,
           environ=None):
    """`Paths` of an engine of `config` over the host `state` (`weights.load`:
    the shapes count), or the ValueError its constructor raises.  Needs the
    library's host-only size queries and no device.  The EMPHASES_* switches
    are read here, from `environ` (default: the process's), nowhere else."""
    environ = os.environ if environ is None else environ
    check_supported(config, precision)
    split_pieces, attention_pieces, linear_pieces = PRECISIONS[precision]
    # positions per wave of the split position-wise kernels: 16
    # (csrc/block_split16.hip: two waves a SIMD, block + next projections in
    # one launch) or 32 (csrc/block_split.hip, one wave a SIMD)
    split_tile = int(environ.get('EMPHASES_SPLIT_TILE', 16))
    if split_tile not in (16, 32):
        raise ValueError('EMPHASES_SPLIT_TILE must be 16 or 32')
    on = lambda name: environ.get('EMPHASES_' + name, '1') != '0'  # noqa: E731
    convolution = config.architecture == 'convolution'
    transformer = config.architecture == 'transformer'
    channels, layers = config.channels, config.layers
    summed = config.downsample_method in ('sum', 'average')
    at_input = config.downsample_location == 'input'

    def shape(name):
        """(c_out, c_in, k) of a Conv1d / Linear weight."""
        return (tuple(state[name].shape) + (1,))[:3]
    # the frame-rate convs: the input layer, and the conv encoder's layers
    frame_layers = [shape('input_layer.weight')] + [
        shape(f'frame_encoder.{2 * i}.weight')
        for i in range(layers if convolution else 0)]
    packs = [conv_forms(*layer, winograd) for layer in frame_layers]
    # F(4,3) when every frame-rate k=3 layer has a pack and the activation
    # is one its register epilogue handles
    quad = bool(winograd and config.activation in (None, 'relu') and
                all(quad_pack for _, quad_pack in packs))
    # the per-word sum folded into the last frame-rate layer's epilogue
    # (emph_conv1d_winograd4_word_sums + emph_word_sums): by configuration,
    # never by batch.  EMPHASES_FOLD_WORD_SUMS=0: emph_segment_reduce
    fold = bool(quad and convolution and not at_input and summed and
                layers > 0 and channels % 4 == 0 and on('FOLD_WORD_SUMS'))
    # the frame-rate layers as a few launches of several layers each
    # (emph_conv1d_stack): the 80 -> 80, k = 3, identity / ReLU family.
    # EMPHASES_CONV_STACK=0: a launch per layer
    stack = bool(quad and convolution and not at_input and
                 all(layer == (80, 80, 3) for layer in frame_layers) and
                 on('CONV_STACK'))
    # precision='bf16x3': the same layers on the bf16 matrix pipe, direct
    # form, operands split into two bf16 pieces (csrc/conv_split.hip); up
    # to five layers per launch.  ('bf16x6' keeps the fp32 kernel here:
    # six products of the direct form would not beat F(4,3) in fp32)
    split_conv = stack and split_pieces == 2
    # the input layer has no activation (model/core.py:17-31,92-100): it and
    # the first encoder layer are one 5-tap layer, F(4,5), in the first
    # launch (emph_conv1d_stack_composed) - one allocation per checkpoint.
    # EMPHASES_CONV_COMPOSE=0: the two F(4,3) layers.  Only in front of a
    # per-word sum or average: outputs 0 and 3 of an F(4,5) quad carry
    # about twice the rounding error of F(4,3)'s, which a sum over a
    # word's frames averages out and 'max' / 'center' - one frame per word
    # and channel - hand on as it is (conv_max against float64: 3.4e-6 x
    # scale composed, where the opt-in precisions promise 3e-6)
    compose = bool(stack and not split_conv and layers > 0 and summed and
                   on('CONV_COMPOSE'))
    # the mel projection dealt evenly over the lanes (csrc/frontend.hip:
    # kQuads); EMPHASES_MEL_PLAN=0, or a basis that does not fit: one lane
    # per row.  Like the composed first conv layer only for the conv model
    # in front of a per-word sum or average: the mapping adds a row's
    # products in another order, as accurate against float64 as the old one
    # (worst 4.28e-6 both), but 'max' / 'center' hand single frames on and
    # the Transformer amplifies a last digit, and tests/test_gpu_paths.py
    # pins those rows to what was measured (conv_max: 2.87e-6 of the 3e-6
    # that precision='bf16x6' promises, 3.44e-6 with the plan; tf_64x2:
    # 5.6e-6 where 4.4e-6 +- 10 % is held)
    mel_plan = bool(on('MEL_PLAN') and convolution and summed and
                    _default_mel_plan() is not None)
    # emph_prominence_forward, or the step-by-step path: Transformer, word
    # pieces, extra feature rows, an encoder kernel other than 3, or
    # direct-form convs requested
    model = bool(convolution and winograd and not at_input and
                 config.num_features == cfg.NUM_MELS and
                 all(pack for pack, _ in packs))

    def square(prefix, names):
        return all(tuple(state[prefix + name].shape) == (channels, channels)
                   for name in names)

    def layer_packs(stack_name):
        """Per layer: the position-wise half as one launch (square weights,
        64 or 80 channels); at the opt-in precisions the same launches on the
        bf16 matrix pipe (80 channels in two heads: the projections write the
        split attention's per-head images); layer i's block with layer i +
        1's Q / K / V projections behind it in one launch (six packs and ten
        vectors must fit in LDS: 80 channels do)."""
        qkv = channels in (64, 80)
        blocks = [qkv and square(f'{stack_name}.model.layers.{i}.', (
            'self_attn.out_proj.weight', 'linear1.weight', 'linear2.weight'))
            for i in range(layers)]
        fits = (6 * channels * channels + 10 * channels) * 4 <= 160 * 1024
        return tuple(LayerPacks(
            qkv, block,
            bool(block and linear_pieces and channels == 80 and
                 config.heads == 2),
            block and qkv and fits and i + 1 < layers)
            for i, block in enumerate(blocks))
    return Paths(
        transformer=transformer, winograd=winograd, conv_tile=conv_tile,
        split_pieces=split_pieces, attention_pieces=attention_pieces,
        linear_pieces=linear_pieces, split_tile=split_tile,
        split_tables=bool(transformer and linear_pieces),
        # EMPHASES_FUSE_QKV=0: the block and the next layer's projections as
        # two launches
        fuse_qkv=on('FUSE_QKV'),
        # the packed frame axis of one pass stays below this (`sub_plans`)
        max_columns=SPLIT16_COLUMNS if (
            transformer and linear_pieces and split_tile == 16)
        else KERNEL_COLUMNS,
        mel_plan=mel_plan, quad=quad, stack=stack, fold=fold,
        split_conv=split_conv, compose=compose,
        # computed positions between two restarts of the folded running sum
        sum_step=32 if split_conv else 64,
        # fused word stage (csrc/decoder.hip): conv decoder, or no decoder
        fused_words=convolution or not config.has_decoder, model=model,
        # the whole word-rate Transformer decoder as one launch (segments of
        # at most 64 words): csrc/word_transformer.hip
        word_transformer=bool(
            transformer and config.has_decoder and channels in (64, 80) and
            config.heads == 2 and all(
                square(f'word_decoder.model.layers.{i}.',
                       ('linear1.weight', 'linear2.weight'))
                for i in range(layers))),
        frame_encoder=layer_packs('frame_encoder') if transformer else (),
        word_decoder=layer_packs('word_decoder')
        if transformer and config.has_decoder else ())


def a_weighting():
    """A-weighting minus REF_DB on the 8 kHz / 1024-bin grid the reference
    evaluates it on (`loudness.py:110-120`; librosa.A_weighting restated from
    its published formula — third-party, parity-unpinned)."""
    frequencies = np.fft.rfftfreq(n=1024, d=1.0 / 8000)
    f_sq = frequencies ** 2.0
    const = np.array([12194.217, 20.598997, 107.65265, 737.86223]) ** 2.0
    with np.errstate(divide='ignore'):
        weights = 2.0 + 20.0 * (
            np.log10(const[0]) + 2 * np.log10(f_sq)
            - np.log10(f_sq + const[0]) - np.log10(f_sq + const[1])
            - 0.5 * np.log10(f_sq + const[2])
            - 0.5 * np.log10(f_sq + const[3]))
    return (np.maximum(-80.0, weights) - cfg.REF_DB).astype(np.float32)


_Tensor = torch.Tensor      # (`Engine._call` asks once per argument)
_UNTIMED = contextlib.nullcontext()


class _Region:
    """One entry of `Engine.timers`: HIP events on the launch stream around
    the launches inside the `with` (`Engine._timed`)."""

    def __init__(self, engine, name, flops):
        self.engine, self.name, self.flops = engine, name, flops

    def __enter__(self):
        self.begin = torch.cuda.Event(enable_timing=True)
        self.end = torch.cuda.Event(enable_timing=True)
        # (with a `runtime.LaunchTimer` armed around the pass: the indices of
        # this region's launches among the timer's kernel-exact durations)
        self.first = self.engine.lib.emph_launch_timer_count()
        self.begin.record()

    def __exit__(self, error, *_):
        if error is None:
            engine = self.engine
            self.end.record()
            engine.timers.append((
                self.name, self.flops, self.begin, self.end, self.first,
                engine.lib.emph_launch_timer_count()))


class _Conv:
    """Device copy of one Conv1d / Linear in MFMA fragment order."""

    def __init__(self, weight, bias, device, winograd=False):
        weight = np.asarray(weight, dtype=np.float32)
        if weight.ndim == 2:
            weight = weight[:, :, None]
        self.c_out, self.c_in, self.kernel_size = weight.shape
        self.weight = weight
        self.pack = torch.from_numpy(runtime.conv_pack(weight)).to(device)
        pair, quad = conv_forms(*weight.shape, winograd)
        self.winograd = torch.from_numpy(
            runtime.conv_winograd_pack(weight)).to(device) if pair else None
        self.winograd4 = torch.from_numpy(
            runtime.conv_winograd4_pack(weight)).to(device) if quad else None
        self.bias = None if bias is None else torch.from_numpy(
            np.ascontiguousarray(bias, dtype=np.float32)).to(device)


class _PerLayer:
    """A Transformer layer's two operations, `project` (Q / K / V of x; returns
    whether K and V went out as the split attention's images) and
    `position_wise` (out_proj + norm1 + feed-forward + norm2 on `attended`,
    into x; with `following`, that layer's projections behind it - returns
    what its `project` would have, else None).  This family: a launch per
    Linear (k = 1 convs) and per LayerNorm, any shape; never with
    `following`."""

    def __init__(self, run):
        self.run, self.engine = run, run.engine
        self.channels = run.engine.config.channels
        self.heads = run.engine.config.heads
        self.eps = run.engine.config.layer_norm_eps

    def conv(self, layer, x, y, ldy, activation=None, **how):
        run = self.run
        self.engine._conv(layer, x, run.ld, y, ldy, run.meta, run.axis,
                          run.block, activation, **how)

    def add_layernorm(self, norm):
        run = self.run
        with self.engine._timed('add_layernorm'):
            self.engine._call(
                'emph_add_layernorm', run.x, run.projected, run.x, run.ld,
                self.channels, norm[0], norm[1], self.eps, 0, run.ld)

    def project(self, layer):
        run = self.run
        self.conv(layer['qk'], run.x, run.qk, run.ld)
        self.conv(layer['v'], run.x, run.v, self.channels, transpose_out=True)
        return False

    def position_wise(self, layer, following):
        run = self.run
        self.conv(layer['out'], run.attended, run.projected, run.ld)
        self.add_layernorm(layer['norm1'])
        self.conv(layer['linear1'], run.x, run.attended, run.ld, 'relu')
        self.conv(layer['linear2'], run.attended, run.projected, run.ld)
        self.add_layernorm(layer['norm2'])


class _Fused(_PerLayer):
    """... one fp32 launch each (csrc/block.hip), tiles of at most 32
    positions; 64 or 80 channels."""

    def __init__(self, run):
        super().__init__(run)
        self.tiles = run.engine._tiles(
            run.meta, run.axis, run.block, run.select)

    def project(self, layer):
        run = self.run
        with self.engine._timed(f'qkv_projection_{run.tag}', 6. * run.square):
            self.engine._call(
                'emph_qkv_projection', run.x, run.ld, run.qk, run.v,
                self.channels, *layer['qkv'], *self.tiles, run.block)
        return False

    def position_wise(self, layer, following):
        run = self.run
        # (attention has consumed qk / v: the next layer's go there)
        name, packs, rest = ('transformer_block', layer['block'], ()) \
            if following is None else \
            ('transformer_block_qkv', layer['block_qkv'], (run.qk, run.v))
        with self.engine._timed(f'{name}_{run.tag}', (
                6. if following is None else 12.) * run.square):
            self.engine._call(
                'emph_' + name, run.attended, run.x, run.ld, self.channels,
                *packs, self.eps, runtime.ACTIVATIONS['relu'], *self.tiles,
                run.block, *rest)
        return None if following is None else False


class _Split(_PerLayer):
    """... on the bf16 matrix pipe (80 channels in two heads), tiles of
    `split_tile` positions."""

    def __init__(self, run):
        super().__init__(run)
        self.tiles = run.engine._tiles(
            run.meta, run.axis, run.engine.split_tile, run.select)


class _Split16(_Split):
    """... tiles of 16 positions: one entry point, emph_position_wise_split
    (csrc/block_split16.hip), for the projections, the block, or the block
    with the next layer's projections."""

    def launch(self, name, flops, layer, following):
        run, engine = self.run, self.engine
        packs, vectors = (None, None) if layer is None \
            else layer['block_split']
        next_packs, next_bias = following['qkv_split'] if following \
            else (None, None)
        with engine._timed(f'{name}_{run.tag}', flops * run.square):
            engine._call(
                'emph_position_wise_split',
                None if layer is None else run.attended,
                run.x, run.ld, self.channels, self.heads, packs, vectors,
                next_packs, next_bias, engine.linear_pieces,
                engine.attention_pieces, self.eps, runtime.ACTIVATIONS['relu'],
                *self.tiles, 16, run.qk, run.v,
                run.images if run.projected_images and following else None)
        return run.projected_images if following else None

    def project(self, layer):
        return self.launch('qkv_projection_split', 6., None, layer)

    def position_wise(self, layer, following):
        if following is None:
            return self.launch('transformer_block_split', 6., layer, None)
        # (attention has consumed qk / v / the images: the next layer's go there)
        return self.launch('transformer_block_qkv_split', 12., layer, following)


class _Split32(_Split):
    """... tiles of 32 positions (EMPHASES_SPLIT_TILE=32, csrc/block_split.hip):
    an entry point per operation."""

    def timed(self, name, flops, entry, *arguments):
        with self.engine._timed(f'{name}_{self.run.tag}',
                                flops * self.run.square):
            self.engine._call(entry, *arguments)

    def project(self, layer):
        run, engine = self.run, self.engine
        packs, bias = layer['qkv_split']
        if run.projected_images:
            self.timed(
                'qkv_projection_split', 6., 'emph_qkv_projection_split_images',
                run.x, run.ld, run.qk, run.images, self.channels, self.heads,
                packs, engine.linear_pieces, engine.attention_pieces, bias,
                *self.tiles, 32)
        else:
            self.timed(
                'qkv_projection_split', 6., 'emph_qkv_projection_split',
                run.x, run.ld, run.qk, run.v, self.channels, packs,
                engine.linear_pieces, bias, *self.tiles, 32)
        return run.projected_images

    def position_wise(self, layer, following):
        run, engine = self.run, self.engine
        packs, vectors = layer['block_split']
        relu = runtime.ACTIVATIONS['relu']
        if following is None:
            return self.timed(
                'transformer_block_split', 6., 'emph_transformer_block_split',
                run.attended, run.x, run.ld, self.channels, packs,
                engine.linear_pieces, vectors, self.eps, relu, *self.tiles,
                32)
        next_packs, next_bias = following['qkv_split']
        self.timed(
            'transformer_block_qkv_split', 12.,
            'emph_transformer_block_qkv_split', run.attended, run.x, run.ld,
            self.channels, self.heads, packs, next_packs, engine.linear_pieces,
            engine.attention_pieces, vectors, next_bias, self.eps, relu,
            *self.tiles, 32, run.qk, run.v,
            run.images if run.projected_images else None)
        return run.projected_images


class Engine:
    """Weights + constants on one device, and the kernel sequence.

    `paths` (`decide`) is the one source of which kernels run.  The flags of
    the same names on the engine (`quad`, `stack`, `fold`, `split_conv`,
    `compose`, `sum_step`, `fused_words`, `split_tile`, `fuse_qkv`, the
    `*_pieces`) are copies made at construction, for the launch code and
    for readers outside; `model`, `mel_plan` and `word_transformer` are the
    packs it says to build.  Setting one on an instance changes no path.
    `max_columns` alone is read from the instance (`sub_plans`)."""

    def __init__(self, config=cfg.DEFAULT, state=None, device=None,
                 conv_tile=None, winograd=True, precision='f32'):
        """`precision`: 'f32' (default: every product on the fp32 matrix
        instruction) or an opt-in, 'bf16x3' / 'bf16x3_fast' / 'bf16x6': fp32
        operands split into two / three bf16 pieces, three / six products
        per term on the bf16 matrix pipe, fp32 accumulation (csrc/
        conv_split.hip, attention_split.hip, block_split.hip; the reference
        itself runs these matmuls under bf16 / fp16 autocast,
        core.py:594-607).  See `PRECISIONS` for what each name selects per
        kernel."""
        # (again in `decide`, which stands alone: here so that a refusal
        # comes before a device is asked for or a checkpoint is read)
        check_supported(config, precision)
        self.config = config
        self.precision = precision
        self.winograd = winograd
        self.conv_tile = conv_tile
        self.device = dev = runtime.require_gpu(device)
        self.lib = runtime.library()
        global FRONTEND_BLOCK
        FRONTEND_BLOCK = int(self.lib.emph_frontend_block())
        # when a list, every kernel launch is bracketed by HIP events on the
        # launch stream: (name, algorithmic flops, start, end)
        self.timers = None
        self._workspace = {}
        self._staging = {}
        # forward() returns workspace buffers: callers that may run on several
        # host threads hold this lock from pack_audio() until they have cloned
        # the scores (core.from_alignments_and_audios does)
        self.lock = threading.RLock()
        self.state = state = weights_module.load(state, config)
        # every choice of kernels is made here; the rest packs and uploads
        self.paths = paths = decide(
            config, state, precision, winograd, conv_tile)
        for name in ('split_pieces', 'attention_pieces', 'linear_pieces',
                     'split_tile', 'fuse_qkv', 'max_columns', 'quad', 'stack',
                     'fold', 'split_conv', 'compose', 'sum_step',
                     'fused_words'):
            setattr(self, name, getattr(paths, name))
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

        # Front-end constants
        self.table = to(runtime.frontend_table())
        basis = melbasis.default()
        self.mel_start = to(basis.row_start)
        self.mel_count = to(basis.row_count)
        self.mel_offset = to(basis.row_offset)
        self.mel_values = to(basis.values)
        self.mel_nnz = int(basis.values.size)
        self.mel_plan = to(_default_mel_plan().view(np.int32)) \
            if paths.mel_plan else None
        self.a_weights = to(a_weighting())

        # Model
        self.input_layer = _Conv(
            state['input_layer.weight'], state['input_layer.bias'], dev,
            winograd)
        self.frame_encoder = self._stack('frame_encoder')
        self.word_decoder = self._stack('word_decoder') \
            if config.has_decoder else None
        self.output_weight = to(state['output_layer.weight'])
        self.output_bias = to(state['output_layer.bias'])
        self.word_block = WORD_TILE
        if self.fused_words:
            layers = self.word_decoder if config.has_decoder else []
            self.decoder_layers = len(layers)
            self.decoder_packs = torch.from_numpy(np.concatenate([
                runtime.word_decoder_pack(l.weight) for l in layers])).to(dev) \
                if layers else None
            self.decoder_biases = torch.cat([l.bias for l in layers]) \
                if layers else None
            self.word_block = int(self.lib.emph_word_decoder_block(
                self.decoder_layers, config.decoder_kernel_size,
                config.decoder_kernel_size))
            # the tile request of the fused word stage (emph_word_decoder_tiles)
            self.decoder_tiles = (runtime.AXIS_DECODER, (
                self.decoder_layers, config.decoder_kernel_size,
                config.decoder_kernel_size))
        if config.architecture == 'transformer':
            self.position = to(weights_module.positional_encoding(
                cfg.MAX_POSITIONS, config.channels))
            # channel-major copy: what the input layer's epilogue adds when the
            # encoding is fused into it (emph_conv1d_winograd4_position)
            self.position_rows = self.position.t().contiguous()
        self.word_transformer = to(np.concatenate([
            runtime.word_transformer_pack(
                state, f'word_decoder.model.layers.{i}.', config.channels,
                config.heads) for i in range(config.layers)])) \
            if paths.word_transformer else None
        frame_stack = [self.input_layer] + list(self.frame_encoder) \
            if self.stack else []
        if self.stack:
            # one allocation, the input layer first: the layout
            # emph_prominence_forward checks for
            self._stack_packs = torch.cat(
                [layer.winograd4 for layer in frame_stack])
            self._stack_biases = torch.cat(
                [layer.bias for layer in frame_stack])
        if self.split_conv:
            self._split_packs = to(np.concatenate(
                [runtime.conv_split_pack(layer.weight) for layer in frame_stack]))
        self._compose_pack = None
        if self.compose:
            first = self.frame_encoder[0]
            self._compose_pack = to(runtime.conv_compose_pack(
                self.input_layer.weight, self.input_layer.bias.cpu().numpy(),
                first.weight, first.bias.cpu().numpy()))
        self.model = self._conv_model() if paths.model else None

    def lane(self):
        """A second handle on the same weights with its own workspace (and
        lock): what a batch in flight on another stream runs through."""
        import copy
        other = copy.copy(self)
        other._workspace = {}
        other._staging = {}
        other.timers = None
        other.lock = threading.RLock()
        return other

    def _conv_model(self):
        """`emph_conv_model` for emph_prominence_forward (the whole path in one
        C call; `Paths.model` says which configurations have one)."""
        config = self.config
        encoder = self.frame_encoder
        pick = (lambda l: l.winograd4) if self.quad else (lambda l: l.winograd)
        input_pack, input_bias = pick(self.input_layer), self.input_layer.bias
        if self.stack:
            size = input_pack.numel()
            input_pack = self._stack_packs[:size]
            self._encoder_packs = self._stack_packs[size:]
            input_bias = self._stack_biases[:config.channels]
            self._encoder_biases = self._stack_biases[config.channels:]
        else:
            self._encoder_packs = torch.cat([pick(l) for l in encoder]) \
                if encoder else torch.zeros(1, device=self.device)
            self._encoder_biases = torch.cat([l.bias for l in encoder]) \
                if encoder else torch.zeros(1, device=self.device)
        pointer = runtime.pointer
        return runtime.ConvModel(
            channels=config.channels, features=config.num_features,
            encoder_layers=len(encoder), decoder_layers=self.decoder_layers,
            decoder_kernel_size=config.decoder_kernel_size,
            activation=runtime.ACTIVATIONS[config.activation],
            reduction=runtime.REDUCTIONS[config.downsample_method],
            post=runtime.POSTPROCESS[config.loss],
            normalize=int(config.normalize), mel_nnz=self.mel_nnz,
            conv_variant=int(self.quad),
            table=pointer(self.table), mel_start=pointer(self.mel_start),
            mel_count=pointer(self.mel_count),
            mel_offset=pointer(self.mel_offset),
            mel_values=pointer(self.mel_values),
            input_pack=pointer(input_pack),
            input_bias=pointer(input_bias),
            encoder_packs=pointer(self._encoder_packs),
            encoder_biases=pointer(self._encoder_biases),
            decoder_packs=pointer(self.decoder_packs),
            decoder_biases=pointer(self.decoder_biases),
            out_weight=pointer(self.output_weight),
            out_bias=pointer(self.output_bias),
            compose=pointer(self._compose_pack if self.stack else None),
            mel_plan=pointer(self.mel_plan))

    def _stack(self, prefix):
        config, state, dev = self.config, self.state, self.device
        layers = []
        if config.architecture == 'convolution':
            for i in range(config.layers):
                layers.append(_Conv(
                    state[f'{prefix}.{2 * i}.weight'],
                    state[f'{prefix}.{2 * i}.bias'], dev,
                    self.winograd and prefix == 'frame_encoder'))
            return layers
        channels = config.channels
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        # (which of the fused forms a layer gets: `decide`, LayerPacks)
        decided = getattr(self.paths, prefix)
        for i, packs in enumerate(decided):
            p = f'{prefix}.model.layers.{i}.'
            in_w = state[p + 'self_attn.in_proj_weight']
            in_b = state[p + 'self_attn.in_proj_bias']
            block = None
            if packs.block:
                # the position-wise half of the layer as one launch
                block = (
                    to(np.concatenate([
                        runtime.linear_chain_pack(
                            state[p + 'self_attn.out_proj.weight'], True),
                        runtime.linear_chain_pack(
                            state[p + 'linear1.weight'], False),
                        runtime.linear_chain_pack(
                            state[p + 'linear2.weight'], False)])),
                    to(np.concatenate([
                        state[p + name].astype(np.float32) for name in (
                            'self_attn.out_proj.bias', 'norm1.weight',
                            'norm1.bias', 'linear1.bias', 'linear2.bias',
                            'norm2.weight', 'norm2.bias')])))
            qkv = None
            if packs.qkv:
                qkv = (to(np.concatenate([
                    runtime.linear_chain_pack(
                        in_w[part * channels:(part + 1) * channels], True)
                    for part in range(3)])), to(in_b.astype(np.float32)))
            # precision='bf16x3': the same two launches on the bf16 matrix pipe
            # (80 channels in two heads: the projections write the split
            # attention's per-head images)
            block_split = qkv_split = None
            if packs.split:
                pieces = self.linear_pieces
                pack = functools.partial(
                    runtime.linear_split_pack, pieces=pieces,
                    tile=self.split_tile)
                block_split = (
                    to(np.concatenate([
                        pack(state[p + name])
                        for name in ('self_attn.out_proj.weight',
                                     'linear1.weight', 'linear2.weight')])),
                    block[1])
                qkv_split = (to(np.concatenate([
                    pack(in_w[part * channels:(part + 1) * channels])
                    for part in range(3)])), qkv[1])
            layers.append(dict(
                packs=packs, block=block, qkv=qkv, block_split=block_split,
                qkv_split=qkv_split,
                qk=_Conv(in_w[:2 * channels], in_b[:2 * channels], dev),
                v=_Conv(in_w[2 * channels:], in_b[2 * channels:], dev),
                out=_Conv(state[p + 'self_attn.out_proj.weight'],
                          state[p + 'self_attn.out_proj.bias'], dev),
                linear1=_Conv(state[p + 'linear1.weight'],
                              state[p + 'linear1.bias'], dev),
                linear2=_Conv(state[p + 'linear2.weight'],
                              state[p + 'linear2.bias'], dev),
                norm1=(to(state[p + 'norm1.weight']),
                       to(state[p + 'norm1.bias'])),
                norm2=(to(state[p + 'norm2.weight']),
                       to(state[p + 'norm2.bias']))))
        # layer i's block with layer i + 1's Q / K / V projections behind it in
        # one launch (six packs and ten vectors must fit in LDS: 80 channels do)
        for i, packs in enumerate(decided):
            layers[i]['block_qkv'] = None
            if not packs.block_qkv:
                continue
            p = f'{prefix}.model.layers.{i + 1}.'
            block = layers[i]['block']
            in_w = state[p + 'self_attn.in_proj_weight']
            in_b = state[p + 'self_attn.in_proj_bias']
            layers[i]['block_qkv'] = (
                torch.cat([block[0]] + [to(runtime.linear_chain_pack(
                    in_w[part * channels:(part + 1) * channels], False))
                    for part in range(3)]),
                torch.cat([block[1], to(in_b.astype(np.float32))]))
        return layers

    ###########################################################################
    # Plan upload
    ###########################################################################

    def frame_tile(self, plan):
        """Positions per conv wave on the frame axis (`Paths.frame_tile`)."""
        return self.paths.frame_tile(plan)

    def _pinned(self, name, array):
        """`array` (int32 numpy) in a reusable pinned staging tensor: a fresh
        `pin_memory()` per batch costs up to milliseconds (hipHostMalloc).  The
        previous copy out of the buffer must have been consumed - the API
        paths synchronise on a batch before they reuse its engine - so the
        buffers rotate over a few slots to stay clear of copies in flight."""
        slots = self._staging.setdefault(name, [[], 0])
        ring, cursor = slots
        if len(ring) < 4:
            ring.append(None)
        index = cursor % len(ring)
        slots[1] = cursor + 1
        tensor = ring[index]
        if tensor is None or tensor.numel() < array.size:
            tensor = torch.empty(
                max(array.size, 1) * 3 // 2, dtype=torch.int32).pin_memory()
            ring[index] = tensor
        view = tensor[:array.size]
        np.copyto(view.numpy(), array)
        return view

    def prepare(self, plan):
        """The host half of `upload` ahead of time: tile tables, span table,
        word-sum tables and the packed metadata array, kept on the plan - what
        a prefetch thread does for batch i + 1 while batch i is submitted
        (`core.files_to_scores`).  Returns the plan."""
        if self.config.downsample_location != 'input':
            tile = self.frame_tile(plan)
            plan.prepared = (tile,) + self._pack(plan, tile, False)
        return plan

    def _pack(self, plan, tile, nested):
        requests = [
            (runtime.AXIS_FRAMES, FRONTEND_BLOCK),
            (runtime.AXIS_FRAMES, tile),
            self.decoder_tiles if self.fused_words
            else (runtime.AXIS_WORDS, self.word_block)]
        if self.paths.transformer:
            # (the fused projection / block kernels own 32 positions per wave,
            # whatever tile the input layer's conv kernel takes)
            requests += [(runtime.AXIS_FRAMES, ATTENTION_BLOCK),
                         (runtime.AXIS_FRAMES, ATTENTION_BLOCK) + SHORT,
                         (runtime.AXIS_FRAMES, ATTENTION_GROUP) + LONG,
                         (runtime.AXIS_FRAMES, 32)]
            if self.paths.split_tables:
                requests += [(runtime.AXIS_FRAMES, self.split_tile)]
            if not nested:
                requests += [(runtime.AXIS_WORDS, ATTENTION_BLOCK)]
                if self.paths.word_transformer:
                    requests += [
                        (runtime.AXIS_WORDS, ATTENTION_BLOCK) + FEW_WORDS,
                        (runtime.AXIS_WORDS, ATTENTION_BLOCK) + MANY_WORDS,
                        (runtime.AXIS_WORDS, self.word_block) + MANY_WORDS]
        requests = list(dict.fromkeys(requests))
        route = self.paths.route(tile, nested)
        host, offsets = plan.pack_metadata(
            requests, word_sums=route.fold, spans=route.stack,
            sum_step=self.sum_step)
        return host, offsets, route.fold, route.stack

    def upload(self, plan, tile=None, nested=False):
        """One H2D copy of all integer metadata; returns device views.
        (`nested`: the layout of the word pieces of another plan.)"""
        tile = tile or self.frame_tile(plan)
        prepared = getattr(plan, 'prepared', None)
        if prepared is not None and prepared[0] == tile and not nested:
            host, offsets, fold, stack = prepared[1:]
        else:
            host, offsets, fold, stack = self._pack(plan, tile, nested)
        pinned = self._pinned(('meta', nested), host)
        device_buffer = pinned.to(self.device, non_blocking=True)
        views = {'_buffer': device_buffer, '_pinned': pinned, 'tile': tile,
                 'positions': (plan.total_frames, plan.total_words)}
        for name, (start, size) in offsets.items():
            views[name] = (device_buffer[start:start + size], size)
        if fold:
            views['n_slots'] = plan.word_sum_tables(
                plan.stack_restarts(self.sum_step)
                if stack else None)['n_slots']
            views['word_sum_tables'] = runtime.WordSumTables(
                *[views[('word_sums', name)][0].data_ptr() for name in (
                    'slot_map', 'terms', 'first', 'lengths')],
                views['n_slots'])
        if self.config.downsample_location == 'input' and not nested and \
                len(plan):
            # every word is its own padded sequence: a second packed layout
            pieces = plan.pieces(self.config.downsample_method)
            piece_meta = self.upload(
                pieces.plan, self.frame_tile(pieces.plan), nested=True)
            extra = self._pinned('pieces', np.concatenate([
                pieces.gather.view(np.int32).ravel(),
                pieces.bounds.ravel(), pieces.word_piece,
                pieces.gather[:, 1].astype(np.int32)]))
            extra = extra.to(self.device, non_blocking=True)
            cut = pieces.gather.size * 2
            piece_meta['gather'] = extra[:cut]
            piece_meta['piece_bounds'] = extra[cut:cut + pieces.bounds.size]
            cut += pieces.bounds.size
            piece_meta['word_piece'] = extra[cut:cut + pieces.word_piece.size]
            # frames of each piece that are the word itself (the rest of the
            # piece is zero padding): the Transformer's key-padding mask
            piece_meta['key_counts'] = extra[cut + pieces.word_piece.size:]
            piece_meta['plan'] = pieces.plan
            piece_meta['_extra'] = extra
            views['pieces'] = piece_meta
        return views

    ###########################################################################
    # Kernel wrappers
    ###########################################################################

    def _timed(self, name, flops=0.):
        """`with self._timed(name, flops):` around the launches of a region
        of `timers`.  (Not a generator-based context manager: every launch of
        every forward enters one, timers or none.)"""
        return _UNTIMED if self.timers is None else _Region(self, name, flops)

    def _buffer(self, name, *shape):
        """Reusable float32 scratch tensor.  Contents are undefined: every
        kernel masks what lies outside a segment by selection, never by
        arithmetic, so stale or non-finite padding cannot leak into results."""
        key = (name, shape)
        tensor = self._workspace.get(key)
        if tensor is None:
            for stale in [k for k in self._workspace if k[0] == name]:
                del self._workspace[stale]
            tensor = torch.empty(shape, dtype=torch.float32, device=self.device)
            self._workspace[key] = tensor
        return tensor

    def pack_audio(self, audios):
        """All utterances (1-D float tensors) back to back in one device
        buffer: one copy per utterance straight into its slice (a host-side
        torch.cat of 64 x 10 s first costs 80 ms of page faults on 41 MB, and
        a pinned staging buffer is slower still to fill: 0.45 GB/s).  The
        returned tensor is a workspace buffer, valid until the next call."""
        lengths = [int(audio.shape[0]) for audio in audios]
        total = sum(lengths)
        packed = self._buffer('packed_audio', max(total, 1))[:total]
        offset = 0
        for audio, length in zip(audios, lengths):
            packed[offset:offset + length].copy_(audio, non_blocking=True)
            offset += length
        return packed

    def _call(self, name, *arguments):
        """The library's entry point `name` on the launch stream, checked:
        tensors go as their addresses, None and scalars as they are (a
        table: `*self._tiles(...)`); a failure raises under `name`.  (By exact
        type: isinstance() of a Tensor costs as much as all the rest.  A
        Tensor subclass - a Parameter as `audio` or `features`, say - is what
        ctypes refuses before it calls anything: then by isinstance.)"""
        function = getattr(self.lib, name)
        try:
            status = function(
                *[argument.data_ptr() if argument.__class__ is _Tensor
                  else argument for argument in arguments], runtime.stream())
        except ctypes.ArgumentError:
            status = function(
                *[argument.data_ptr() if isinstance(argument, _Tensor)
                  else argument for argument in arguments], runtime.stream())
        if status:
            runtime.check(status, name)

    @staticmethod
    def _table(entry, fields):
        """(address, entries) of an int32 table of `meta` whose entries have
        `fields` fields: the two arguments a launch takes it as."""
        entries, size = entry
        return entries.data_ptr(), size // fields

    def _tiles(self, meta, axis, block, select=()):
        """`_table` of the tile table of `block` positions on `axis`
        (`select`: of the segments of that size alone)."""
        return self._table(
            meta[('tiles', axis, block) + select], runtime.TILE_FIELDS)

    def _conv(self, layer, x, ldx, y, ldy, meta, axis, block, activation,
              transpose_out=False, position=False):
        """`position`: the layer feeds a Transformer encoder - add the
        positional encoding in the same launch when the F(4,3) kernel takes
        the layer.  Returns whether it did."""
        tiles = self._tiles(meta, axis, block)
        name = (f'conv1d_{"frames" if axis == runtime.AXIS_FRAMES else "words"}'
                f'_{layer.c_in}x{layer.c_out}_k{layer.kernel_size}')
        flops = 2. * layer.c_in * layer.c_out * layer.kernel_size * \
            meta['positions'][axis]
        code = runtime.ACTIVATIONS[activation]
        frames = axis == runtime.AXIS_FRAMES and not transpose_out
        if layer.winograd4 is not None and frames and block == 64 and \
                self.quad and activation in (None, 'relu'):
            with self._timed(name.replace('conv1d', 'conv1d_winograd4'), flops):
                self._call(
                    'emph_conv1d_winograd4' + ('_position' if position else ''),
                    x, ldx, y, ldy, layer.winograd4, layer.bias, layer.c_in,
                    layer.c_out, code, *tiles,
                    *((self.position_rows, cfg.MAX_POSITIONS)
                      if position else ()))
            return bool(position)
        if layer.winograd is not None and frames and block in (32, 64):
            # same algorithmic flops; the kernel executes two thirds of them
            with self._timed(name.replace('conv1d', 'conv1d_winograd'), flops):
                self._call('emph_conv1d_winograd', x, ldx, y, ldy,
                           layer.winograd, layer.bias, layer.c_in, layer.c_out,
                           code, *tiles, block)
            return False
        with self._timed(name, flops):
            self._call('emph_conv1d', x, ldx, y, ldy, layer.pack, layer.bias,
                       layer.c_in, layer.c_out, layer.kernel_size, code, *tiles,
                       block, int(transpose_out))
        return False

    def features(self, audio, plan, meta, tracks=None, config=None, out=None):
        """Feature matrix [num_features, ld_frames] of every segment
        (`data/preprocess/core.py:71-125`).  The pitch tracker (`penn`, a
        third-party neural network) runs outside the library: `tracks` =
        float32 device tensor [2, ld_frames] with its per-frame pitch (Hz) and
        periodicity on the packed frame axis (`batch.pack_tracks`); the
        log2 / normalisation / row placement of core.py:94-106,123 happens
        on the device.  `config`: another configuration's feature switches
        (`data.preprocess.mels.from_audio` asks for the mel rows alone).
        `out`: the caller's own rows [num_features, ld_frames] - rows of a
        larger matrix, say (`data.preprocess.from_files_to_files` puts the
        loudness row under the mel rows that way) - instead of the engine's
        workspace."""
        config = config or self.config
        rows = config.num_features
        if out is None:
            out = self._buffer('features', rows, plan.ld_frames)
        elif out.shape[0] < rows or out.stride(0) != plan.ld_frames or \
                out.dtype != torch.float32:
            raise ValueError('features: out must be float32 rows of ld_frames')
        mel_row = 0 if config.mel_feature else -1
        loud_row = rows - 1 if config.loudness_feature else -1
        if config.pitch_feature or config.periodicity_feature:
            if tracks is None or tuple(tracks.shape) != (2, plan.ld_frames):
                raise NotImplementedError(TRACKS_NEEDED)
            first = cfg.NUM_MELS if config.mel_feature else 0
            pitch_row = first if config.pitch_feature else -1
            periodicity_row = first + int(config.pitch_feature) \
                if config.periodicity_feature else -1
            with self._timed('pitch_rows'):
                self._call(
                    'emph_pitch_rows', tracks[0], tracks[1], out,
                    plan.ld_frames, pitch_row, periodicity_row,
                    int(config.normalize),
                    float(np.log2(np.float32(cfg.FMIN))),
                    float(np.log2(np.float32(cfg.FMAX))))
        tiles = self._tiles(meta, runtime.AXIS_FRAMES, FRONTEND_BLOCK)
        table = meta['table'][0]
        peak = None
        if config.loudness_feature:
            peak = torch.zeros(
                len(plan), dtype=torch.float32, device=self.device)
            with self._timed('frontend_peak'):
                self._call('emph_frontend_peak', audio, audio_format(audio),
                           table, *tiles, self.table, peak)
        if mel_row >= 0 or loud_row >= 0:
            with self._timed('frontend_logmel'):
                self._call(
                    'emph_logmel_planned', audio, audio_format(audio), table,
                    *tiles, self.table, self.mel_start, self.mel_count,
                    self.mel_offset, self.mel_values, self.mel_nnz,
                    self.mel_plan, out, plan.ld_frames, mel_row, loud_row,
                    peak, self.a_weights, int(config.normalize))
        return out

    def _transformer(self, layers, x, ld, plan, meta, axis, block, tag,
                     key_counts=None, positioned=False, select=()):
        """`Transformer.forward` (transformer.py:25-30) in place on x
        (`positioned`: the producer of x has added the encoding already).
        `key_counts`: int32 device tensor, real (unpadded) positions per
        segment, for the key-padding mask over zero-padded word pieces.
        `select`: (least, most) positions - only the segments of that size
        (their tiles), the others' columns are left alone."""
        config = self.config
        channels = config.channels
        if block > 32 and ('tiles', axis, 32) + select in meta:
            block = 32
        att = self._tiles(meta, axis, ATTENTION_BLOCK, select)
        if att[1] == 0:
            return x
        counts = plan.frames if axis == runtime.AXIS_FRAMES else plan.words
        if len(counts) and int(counts.max()) > cfg.MAX_POSITIONS:
            # transformer.py:40,51-52: the encoding table has 5000 rows
            raise RuntimeError(
                f'a chunk of {int(counts.max())} positions exceeds the '
                f'{cfg.MAX_POSITIONS}-entry positional encoding; pass a '
                'smaller batch_size')
        if not positioned:
            with self._timed('add_position'):
                self._call('emph_add_position', x, ld, self.position, channels,
                           cfg.MAX_POSITIONS, *att, ATTENTION_BLOCK)
        run = types.SimpleNamespace(
            engine=self, x=x, ld=ld, meta=meta, axis=axis, block=block,
            tag=tag, select=select,
            qk=self._buffer(tag + '_qk', 2 * channels, ld),
            v=self._buffer(tag + '_v', ld, channels),
            attended=self._buffer(tag + '_attended', channels, ld),
            projected=self._buffer(tag + '_projected', channels, ld),
            square=channels * channels * meta['positions'][axis])
        attention_flops = 4. * channels * float(
            (counts.astype(np.float64) ** 2).sum())
        # long segments: a workgroup of eight waves shares each key / value
        # block through LDS; short ones (the word axis, word pieces): one wave
        # per 64 queries straight from L2.  By SEGMENT, not by batch: two tile
        # tables, at most two launches per layer.
        launches = [(att, ATTENTION_BLOCK)]
        if axis == runtime.AXIS_FRAMES and not select and \
                ('tiles', axis, ATTENTION_GROUP) + LONG in meta:
            launches = [
                (tiles, size) for tiles, size in (
                    (self._tiles(meta, axis, ATTENTION_BLOCK, SHORT),
                     ATTENTION_BLOCK),
                    (self._tiles(meta, axis, ATTENTION_GROUP, LONG),
                     ATTENTION_GROUP)) if tiles[1]]
        # precision='bf16x3' / 'bf16x6': long segments take the bf16 matrix
        # pipe - the layer's keys and values are split once (all 64-position
        # tiles of the axis), the grouped launch reads the pieces
        images = None
        if self.attention_pieces and config.channels // config.heads == 40 and \
                any(size == ATTENTION_GROUP for _, size in launches):
            size = int(self.lib.emph_split_kv_bytes(
                ld, len(plan), channels, config.heads,
                self.attention_pieces))
            key = (tag + '_split_kv', (size,))
            images = self._workspace.get(key)
            if images is None:
                for stale in [k for k in self._workspace if k[0] == key[0]]:
                    del self._workspace[stale]
                images = torch.empty(
                    size, dtype=torch.uint8, device=self.device)
                self._workspace[key] = images
        run.images = images
        # ... or the projection kernel writes the pieces itself (no fp32 K and V,
        # no second pass): when every segment of the axis is a long one
        run.projected_images = images is not None and \
            all(size == ATTENTION_GROUP for _, size in launches)

        def attend(images_written):
            for tiles, size in launches:
                if images is None or size != ATTENTION_GROUP:
                    self._call('emph_attention', run.qk, run.v, run.attended,
                               ld, channels, config.heads, *tiles, size,
                               key_counts)
                    continue
                if not images_written:
                    self._call('emph_split_kv', run.qk, run.v, ld, channels,
                               config.heads, *att, ATTENTION_BLOCK,
                               self.attention_pieces, images)
                self._call('emph_attention_split', run.qk, images,
                           run.attended, ld, channels, config.heads, *tiles,
                           size, key_counts, self.attention_pieces)

        # how each layer projects Q / K / V and runs its position-wise half:
        # resolved once, from the decision and the tile tables at hand.  (The
        # 16-position split kernels address rows with 32-bit byte offsets:
        # `forward` keeps every packed axis below 2^22 columns for them,
        # `sub_plans`)
        forms = self.paths.forms(
            [layer['packs'] for layer in layers], block <= 32,
            axis == runtime.AXIS_FRAMES and
            ('tiles', axis, self.split_tile) + select in meta)
        families = {'convs': _PerLayer, 'fused': _Fused, 'split':
                    _Split16 if self.split_tile == 16 else _Split32}
        family = {name: families[name](run) for name in {
            name for form in forms for name in form[:2]}}
        ahead = None       # this layer's Q, K, V came out of the last block
        #                    (whether its K and V as the attention's images)
        for index, (layer, form) in enumerate(zip(layers, forms)):
            if ahead is None:
                ahead = family[form.project].project(layer)
            with self._timed(f'attention_{tag}', attention_flops):
                attend(ahead)
            ahead = family[form.block].position_wise(
                layer, layers[index + 1] if form.ahead else None)
        return x

    def _frame_stack(self, features, ld_f, a, b, out, ld_w, plan, meta, fold,
                     frames=True, words=True):
        """Input layer + frame encoder as groups of up to three layers per
        launch (`emph_conv1d_stack`: a workgroup owns a span of positions
        through the layers of a group, activations resident in LDS), then
        `emphases.downsample` into `out` - from running sums the last group
        leaves behind when the per-word sum is folded (`fold`), else by
        `emph_segment_reduce`.  Same launches as emph_prominence_forward."""
        config = self.config
        channels = config.channels
        spans = self._table(meta['conv_spans'], SPAN_FIELDS)
        # composed: the input layer and encoder layer 0 are the first launch's
        # first (5-tap) layer - one effective layer less
        skip = int(self.compose)
        total = 1 + len(self.frame_encoder) - skip
        most = int(self.lib.emph_conv_stack_max_layers())
        sums = self._buffer(
            'word_sums', max(meta.get('n_slots', 0), 1), channels)
        packs, pack = self._stack_packs, self.input_layer.winograd4.numel()
        if self.split_conv:
            # bf16x3: up to five layers per launch
            most = 5
            packs, pack = self._split_packs, int(
                self.lib.emph_conv_split_pack_size())
        groups = -(-total // most)
        relu_layers = config.activation == 'relu'
        source, buffers, done = features, (a, b), 0
        for group in range(groups if frames else 0):
            size = -(-(total - done) // (groups - group))
            relu = sum(1 << l for l in range(size)
                       if done + l + skip >= 1 and relu_layers)
            to_sums = fold and group == groups - 1
            target = sums if to_sums else buffers[group & 1]
            flops = 2. * 80 * 80 * 3 * plan.total_frames * (
                size + (skip if group == 0 else 0))
            # what the three entry points share: where from, where to, then
            # the layers' weights, then this
            ends = (source, ld_f, target, channels if to_sums else ld_f)
            rest = (size, relu, *spans,
                    meta[('word_sums', 'slot_map')][0] if to_sums else None)
            layer = done + skip          # the model's layer, input layer first
            with self._timed('conv1d_split_frames_80x80_k3' if self.split_conv
                             else 'conv1d_stack_frames_80x80_k3', flops):
                if self.split_conv:
                    self._call('emph_conv1d_split', *ends, packs[done * pack:],
                               self._stack_biases[done * channels:], *rest)
                elif self.compose and group == 0:
                    self._call(
                        'emph_conv1d_stack_composed', *ends, self._compose_pack,
                        packs[(layer + 1) * pack:] if size > 1 else None,
                        self._stack_biases[(layer + 1) * channels:]
                        if size > 1 else None, *rest)
                else:
                    self._call('emph_conv1d_stack', *ends, packs[layer * pack:],
                               self._stack_biases[layer * channels:], *rest)
            source = target
            done += size
        if words:
            self._downsample(source, ld_f, out, ld_w, meta, fold)

    def _last_layer_sums(self, x, ld_f, plan, meta):
        """The last frame-rate layer in front of a folded `_downsample`
        ('sum' / 'average', `core.py:438-454`) without the layer's output ever
        being written: running sums at the frames the words need."""
        layer = self.frame_encoder[-1]
        channels = self.config.channels
        sums = self._buffer('word_sums', max(meta['n_slots'], 1), channels)
        flops = 2. * layer.c_in * layer.c_out * 3 * plan.total_frames
        with self._timed(
                f'conv1d_winograd4_frames_{layer.c_in}x{layer.c_out}_k3', flops):
            self._call(
                'emph_conv1d_winograd4_word_sums', x, ld_f, sums, channels,
                layer.winograd4, layer.bias, layer.c_in, layer.c_out,
                runtime.ACTIVATIONS[self.config.activation],
                *self._tiles(meta, runtime.AXIS_FRAMES, 64),
                meta[('word_sums', 'slot_map')][0])

    def _downsample(self, source, ld, out, ld_w, meta, fold, bounds=None,
                    word_segment=None):
        """`emphases.downsample` into the word columns of `out`: a few signed
        terms per word of the running sums the last frame-rate launch left
        (`fold`), else `emph_segment_reduce` of `source` (`bounds`,
        `word_segment`: those of word pieces instead of the plan's words)."""
        channels = self.config.channels
        reduction = runtime.REDUCTIONS[self.config.downsample_method]
        if fold:
            sums = self._buffer('word_sums', max(meta['n_slots'], 1), channels)
            view = lambda name: meta[('word_sums', name)][0]  # noqa: E731
            with self._timed('word_sums'):
                self._call('emph_word_sums', sums, channels, view('terms'),
                           view('first'), view('lengths'), out, ld_w, channels,
                           ld_w, reduction)
            return
        with self._timed('segment_reduce'):
            self._call(
                'emph_segment_reduce', source, ld,
                meta['bounds'][0] if bounds is None else bounds, out, ld_w,
                channels, meta['table'][0],
                meta['word_segment'][0] if word_segment is None
                else word_segment, ld_w, reduction)

    def _stack_forward(self, layers, x, other, ld, plan, meta, axis, block,
                       tag, key_counts=None, positioned=False):
        """Frame encoder / word decoder; returns the tensor holding the
        result (x or other)."""
        config = self.config
        if config.architecture == 'convolution':
            for layer in layers:
                self._conv(layer, x, ld, other, ld, meta, axis, block,
                           config.activation)
                x, other = other, x
            return x
        if axis == runtime.AXIS_WORDS and self.word_transformer is not None \
                and key_counts is None and len(plan.words):
            # segments of up to 64 words: the whole decoder in one launch;
            # longer ones: the per-layer kernels on THEIR tiles (disjoint
            # columns of x; which path a segment takes depends on it alone)
            tiles = self._tiles(meta, axis, ATTENTION_BLOCK, FEW_WORDS)
            if tiles[1]:
                with self._timed('word_transformer'):
                    self._call('emph_word_transformer', x, ld, self.position,
                               cfg.MAX_POSITIONS, config.channels, config.heads,
                               self.word_transformer, len(layers),
                               config.layer_norm_eps, *tiles)
            if int(plan.words.max()) > FUSED_WORDS:
                self._transformer(
                    layers, x, ld, plan, meta, axis, block, tag, key_counts,
                    positioned, select=MANY_WORDS)
            return x
        return self._transformer(
            layers, x, ld, plan, meta, axis, block, tag, key_counts, positioned)

    ###########################################################################
    # Forward
    ###########################################################################

    def forward(self, audio, plan, meta=None, stages=None, features=None,
                tracks=None):
        """Scores of every word of every segment.

        audio: float32 (or int16 PCM) device tensor, all utterances back to
            back.
        Returns (scores, logits): float32 [ld_words] on the packed word axis
        (`plan.word_columns()` picks the valid entries; other entries are
        undefined).  The tensors are workspace buffers: they are overwritten
        by the next forward() of this engine."""
        config = self.config
        runs = self.sub_plans(plan)
        if runs is not None:
            if stages is not None:
                # (the stage dump is a test tap of one packed layout)
                raise ValueError(
                    'stages of a plan past the packed-axis limit: pass its '
                    'segments in smaller plans')
            return self._forward_runs(audio, plan, runs, tracks, features)
        meta = meta or self.upload(plan)
        block = meta['tile']
        channels = config.channels
        ld_f, ld_w = plan.ld_frames, plan.ld_words
        frames, words = runtime.AXIS_FRAMES, runtime.AXIS_WORDS
        route = self.paths.route(
            block, False, stages is not None, features is not None,
            self.timers is not None)
        if route.one_call and len(plan):
            # the whole path behind one C call
            check_bounds(plan, config.downsample_method)
            logits = self._buffer('logits', ld_w)
            scores = self._buffer('scores', ld_w)
            floats = self.lib.emph_prominence_workspace_floats(
                config.num_features, channels, ld_f, ld_w,
                meta.get('n_slots', 0))
            workspace = self._buffer('fused', int(floats))
            spans = self._table(meta['conv_spans'], SPAN_FIELDS) \
                if route.stack else (None, 0)
            self._call(
                'emph_prominence_forward', ctypes.byref(self.model), audio,
                audio_format(audio), meta['table'][0],
                *self._tiles(meta, frames, FRONTEND_BLOCK),
                *self._tiles(meta, frames, block), block,
                *self._tiles(meta, *self.decoder_tiles), meta['bounds'][0],
                meta['word_segment'][0], ld_f, ld_w, workspace, logits, scores,
                ctypes.byref(meta['word_sum_tables']) if route.fold else None,
                *spans)
            return scores, logits
        if features is None:
            features = self.features(audio, plan, meta, tracks=tracks)
        logits = self._buffer('logits', ld_w)
        scores = self._buffer('scores', ld_w)
        wa = self._buffer('words_a', channels, ld_w)
        if config.downsample_location == 'input':
            # model/core.py:41-87: gather every word into its own zero-padded
            # piece, encode the pieces as independent sequences, pool each
            # over its padded length into the word's column
            if stages is not None:
                stages['features'] = features.clone()
            piece_meta = meta['pieces']
            piece_plan = piece_meta['plan']
            ld_p = piece_plan.ld_frames
            gathered = self._buffer(
                'piece_features', config.num_features, ld_p)
            with self._timed('gather_columns'):
                self._call('emph_gather_columns', features, ld_f, gathered,
                           ld_p, config.num_features, piece_meta['gather'],
                           len(piece_plan))
            a = self._buffer('frames_a', channels, ld_p)
            b = self._buffer('frames_b', channels, ld_p)
            self._conv(self.input_layer, gathered, ld_p, a, ld_p, piece_meta,
                       frames, piece_meta['tile'], None)
            encoded = self._stack_forward(
                self.frame_encoder, a, b, ld_p, piece_plan, piece_meta,
                frames, piece_meta['tile'], 'pieces',
                key_counts=piece_meta['key_counts']
                if config.architecture == 'transformer' else None)
            self._downsample(
                encoded, ld_p, wa, ld_w, piece_meta, False,
                piece_meta['piece_bounds'], piece_meta['word_piece'])
        else:
            a = self._buffer('frames_a', channels, ld_f)
            b = self._buffer('frames_b', channels, ld_f)
            if route.stack:
                # the frame-rate layers a few at a time (emph_conv1d_stack),
                # the last launch straight into the per-word sums when folded
                check_bounds(plan, config.downsample_method)
                self._frame_stack(
                    features, ld_f, a, b, wa, ld_w, plan, meta, route.fold)
            else:
                # (the stage dump wants the input layer's own output)
                positioned = self._conv(
                    self.input_layer, features, ld_f, a, ld_f, meta, frames, block,
                    None, position=config.architecture == 'transformer' and
                    stages is None)
                if stages is not None:
                    stages['features'] = features.clone()
                    stages['input_layer'] = a.clone()
                # (the stage dump wants the encoder's own output: the taps keep
                # the unfolded reduce, which agrees to summation order)
                encoded = self._stack_forward(
                    self.frame_encoder[:-1] if route.fold
                    else self.frame_encoder, a, b, ld_f, plan, meta, frames,
                    block, 'frames', positioned=positioned)
                if stages is not None:
                    stages['encoder'] = encoded.clone()

                check_bounds(plan, config.downsample_method)
                if route.fold:
                    self._last_layer_sums(encoded, ld_f, plan, meta)
                self._downsample(encoded, ld_f, wa, ld_w, meta, route.fold)
        if stages is not None:
            stages['downsampled'] = wa.clone()
        return self._word_stage(wa, plan, meta, logits, scores)

    def sub_plans(self, plan):
        """None when one pass takes the whole plan; else the (first, end)
        segment ranges of consecutive sub-plans whose packed frame axes - and
        word-piece axes for DOWNSAMPLE_LOCATION='input' - each stay below
        `max_columns`.  Segments are independent, so the scores are bitwise
        those of one pass, with the same kernels at every size."""
        from . import batch
        pieces = self.config.downsample_location == 'input' and len(plan)
        if plan.ld_frames < self.max_columns and (not pieces or plan.pieces(
                self.config.downsample_method).plan.ld_frames <
                self.max_columns):
            # (the word-piece layout is the one upload() builds: cached)
            return None
        room = self.max_columns - batch.LEAD - batch.TAIL
        columns = [-(-plan.frames // batch.ALIGN) * batch.ALIGN]
        if pieces:
            # one piece per word, as long as the segment's longest word
            first = np.cumsum(plan.words) - plan.words
            longest = np.array([
                int(np.max(plan.segment_bounds[1, f:f + n] -
                           plan.segment_bounds[0, f:f + n])) if n else 0
                for f, n in zip(first, plan.words)], dtype=np.int64)
            columns.append(plan.words * (
                -(-longest // batch.ALIGN) * batch.ALIGN))
        columns = np.stack(columns)
        if (columns >= room).any():
            raise ValueError(
                f'one segment fills {int(columns.max())} packed columns, '
                f'more than the {room} of a pass')
        runs, first, used = [], 0, np.zeros(len(columns), dtype=np.int64)
        for index in range(len(plan)):
            if (used + columns[:, index] >= room).any():
                runs.append((first, index))
                first, used = index, 0 * used
            used += columns[:, index]
        runs.append((first, len(plan)))
        return runs

    def _forward_runs(self, audio, plan, runs, tracks, features=None):
        """forward() of a plan as the sub-plans `runs` (`sub_plans`), the
        scores and logits gathered on the plan's own word axis.  `tracks` /
        `features` on the plan's packed frame axis are re-packed per run."""
        from . import batch
        table = plan.table
        scores = self._buffer('whole_scores', plan.ld_words)
        logits = self._buffer('whole_logits', plan.ld_words)
        first_word = np.cumsum(plan.words) - plan.words
        for first, end in runs:
            rows = slice(first, end)
            count = end - first
            words = plan.words[rows]
            bounds = plan.segment_bounds[
                :, first_word[first]:first_word[first] + int(words.sum())]
            part = batch.Plan.from_columns(
                np.arange(count, dtype=np.int64), plan.start_word[rows],
                table[rows, runtime.SEG_START], table[rows, runtime.SEG_LENGTH],
                plan.frames[rows], words, bounds,
                table[rows, runtime.SEG_AUDIO_OFF],
                table[rows, runtime.SEG_AUDIO_LEN])

            def repack(rows):
                """`rows` [R, plan.ld_frames] -> [R, part.ld_frames]"""
                if rows is None:
                    return None
                out = torch.zeros((rows.shape[0], part.ld_frames),
                                  dtype=rows.dtype, device=rows.device)
                for i in range(count):
                    at, n = int(plan.frame_off[first + i]), int(part.frames[i])
                    to = int(part.frame_off[i])
                    out[:, to:to + n] = rows[:, at:at + n]
                return out
            part_scores, part_logits = self.forward(
                audio, part, tracks=repack(tracks), features=repack(features))
            # the run's word columns: one block, shifted
            at, size = int(plan.word_off[first]), part.ld_words - batch.LEAD - \
                batch.TAIL
            scores[at:at + size].copy_(
                part_scores[batch.LEAD:batch.LEAD + size])
            logits[at:at + size].copy_(
                part_logits[batch.LEAD:batch.LEAD + size])
        return scores, logits

    def _word_stage(self, wa, plan, meta, logits, scores):
        """Word embeddings -> word decoder -> output layer -> postprocess."""
        config = self.config
        channels = config.channels
        ld_w = plan.ld_words
        words = runtime.AXIS_WORDS
        if self.fused_words:
            with self._timed('word_decoder', 2. * channels * (
                    channels * config.decoder_kernel_size * self.decoder_layers
                    + config.decoder_kernel_size) * plan.total_words):
                self._call(
                    'emph_word_decoder', wa, ld_w,
                    *self._tiles(meta, *self.decoder_tiles), channels,
                    self.decoder_packs, self.decoder_biases,
                    self.decoder_layers, config.decoder_kernel_size,
                    runtime.ACTIVATIONS[config.activation],
                    self.output_weight, self.output_bias,
                    config.decoder_kernel_size,
                    runtime.POSTPROCESS[config.loss], logits, scores)
            return scores, logits
        wb = self._buffer('words_b', channels, ld_w)
        decoded = self._stack_forward(
            self.word_decoder, wa, wb, ld_w, plan, meta, words,
            self.word_block, 'words')
        with self._timed('output_layer'):
            self._call('emph_output_layer', decoded, ld_w, self.output_weight,
                       self.output_bias, channels, config.decoder_kernel_size,
                       meta['table'][0], meta['word_segment'][0], ld_w, words,
                       runtime.POSTPROCESS[config.loss], logits, scores)
        return scores, logits

    def splittable(self, plan, meta):
        """Whether forward() is `forward_frames()` + `forward_words()` for this
        configuration and layout: the default convolutional path (frame-rate
        layers by emph_conv1d_stack, per-word sums folded, one-launch decoder)."""
        route = self.paths.route(meta['tile'])
        return (self.config.downsample_location != 'input' and
                route.stack and route.fold and
                self.fused_words and len(plan) > 0 and
                self.sub_plans(plan) is None)

    def forward_frames(self, audio, plan, meta):
        """The frame-rate half of forward(): features and the frame-rate layers,
        up to the running sums the words are made of (left in the workspace)."""
        ld_f = plan.ld_frames
        channels = self.config.channels
        check_bounds(plan, self.config.downsample_method)
        features = self.features(audio, plan, meta)
        a = self._buffer('frames_a', channels, ld_f)
        b = self._buffer('frames_b', channels, ld_f)
        self._frame_stack(features, ld_f, a, b, None, plan.ld_words, plan, meta,
                          True, words=False)

    def forward_words(self, plan, meta):
        """The word-rate half: per-word sums -> decoder -> scores (same kernels,
        same bits as forward())."""
        ld_w = plan.ld_words
        logits = self._buffer('logits', ld_w)
        scores = self._buffer('scores', ld_w)
        wa = self._buffer('words_a', self.config.channels, ld_w)
        self._frame_stack(None, plan.ld_frames, None, None, wa, ld_w, plan, meta,
                          True, frames=False)
        return self._word_stage(wa, plan, meta, logits, scores)

    def capture(self, audio, plan, meta=None):
        """Capture forward() for this (audio buffer, plan) into a HIP graph.

        Returns `(replay, scores, logits)`: `replay()` re-enqueues the whole
        kernel sequence with one host call (about 10 us instead of one
        launch per kernel) and refreshes `scores` / `logits` in place.  The
        audio tensor may be refilled between replays; its address and the
        plan must not change."""
        if self.sub_plans(plan) is not None:
            raise ValueError('a plan past the packed-axis limit runs as '
                             'sub-plans: it cannot be captured as one graph')
        meta = meta or self.upload(plan)
        self.timers = None
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):       # warm up: attribute calls, buffers
            for _ in range(2):
                self.forward(audio, plan, meta)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        # thread-local capture: the RCCL watchdog thread of a multi-GPU run may
        # query events while this thread captures
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            scores, logits = self.forward(audio, plan, meta)
        # the graph holds raw pointers into the workspace (allocated by the
        # warm-up, outside the graph's pool): keep those tensors alive for as
        # long as the replay closure lives, even if a later forward() with
        # another layout drops them from the workspace
        held = (list(self._workspace.values()), meta, audio)

        def replay():
            graph.replay()
            return held[0] is not None
        return replay, scores, logits


def audio_format(audio):
    """EMPH_AUDIO_* of a packed audio tensor: float32, or 16-bit PCM (the
    front-end applies the x / 32768 of `load.wav` itself)."""
    if audio.dtype == torch.float32:
        return runtime.AUDIO_F32
    if audio.dtype == torch.int16:
        return runtime.AUDIO_PCM16
    raise TypeError(f'packed audio must be float32 or int16, not {audio.dtype}')


def check_bounds(plan, method):
    """Host-side replicas of the two cases where the reference raises
    (`core.py:449-452,459-466`)."""
    if method not in ('max', 'center'):
        return
    for segment in plan.segments:
        starts, ends = segment.bounds
        if method == 'max' and np.any(
                np.minimum(ends, segment.frames) <=
                np.minimum(starts, segment.frames)):
            raise IndexError(
                'max(): Expected reduction dim 1 to have non-zero size '
                '(empty word)')
        if method == 'center' and np.any(
                (starts + ends) // 2 >= segment.frames):
            raise IndexError('word center lies beyond the last frame')
