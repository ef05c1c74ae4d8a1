"""Launches on the packed layout that an op and its backward share: the
direct-form convolution, the weight gradient, and `_LayerRun`, one encoder
layer as an unfused sequence that keeps every intermediate."""
import torch

from .. import config as cfg
from .. import engine as engine_module
from .. import runtime
from .layout import DIRECT_TILE, GRAD_TILE, SPLIT_TILE
from .packs import _call, _device_pack, _float32

LAYER_CHANNELS, LAYER_HEADS = 80, 2      # emph_attention_backward
LAYER_EPS = cfg.Config(architecture='transformer').layer_norm_eps
# `precision` of encoder_layer_split -> the `pieces` code of emph_attention_split
# (three pieces for the scores, two behind the softmax: engine.PRECISIONS)
SPLIT_PIECES = {'bf16x3': 32}


def _conv1d(x, y, ld, pack, bias, c_in, c_out, kernel_size, activation,
            layout, transpose=False):
    """`emph_conv1d` in direct form on the 64-position tiles of `layout`:
    x [c_in, ld] -> y [c_out, ld] (`transpose`: y [ld, c_out])."""
    tiles, n_tiles = layout.tiles(DIRECT_TILE)
    _call('emph_conv1d', x, ld, y, c_out if transpose else ld, pack, bias,
          c_in, c_out, kernel_size, runtime.ACTIVATIONS[activation], tiles,
          n_tiles, DIRECT_TILE, int(transpose))


def _weight_grad(dy, x, ld, c_in, c_out, kernel_size, layout, dweight, dbias):
    """dweight [c_out, c_in, kernel_size] and dbias [c_out] (float32, to
    fill) by `emph_conv_weight_grad_any`; zeros when there is no tile."""
    tiles, n_tiles = layout.tiles(GRAD_TILE)
    if not n_tiles:
        dweight.zero_()
        dbias.zero_()
        return
    workspace = torch.empty(
        int(runtime.library().emph_conv_weight_grad_any_workspace(
            c_in, c_out, kernel_size, n_tiles)),
        dtype=torch.float32, device=dy.device)
    _call('emph_conv_weight_grad_any', dy, ld, x, ld, c_in, c_out,
          kernel_size, tiles, n_tiles, GRAD_TILE, workspace, dweight, dbias)


class _LayerRun:
    """One encoder layer as an UNFUSED sequence of launches on the packed
    layout that keeps every intermediate (what the backward walks back
    through, and the forward of a parameter set that is being trained): Q / K
    and V by `emph_conv1d` k = 1, `emph_attention`, out_proj,
    `emph_add_layernorm`, linear1 + ReLU, linear2, `emph_add_layernorm`.  The
    weights are packed on the device (`_device_pack`): nothing is copied to
    the host.

    `dropout` = (p, seed, stream_base, step) draws the reference's four
    dropouts of the layer (`train/dropout.py`): `emph_attention_dropout` in
    place of `emph_attention` under stream_base, and `emph_dropout` in place
    on `projected`, `hidden` and `fed` (whole packed buffers [rows, ld]) under
    stream_base + 1, + 2, + 3.

    `pieces` (a code of `SPLIT_PIECES`): the attention core on the bf16
    matrix pipe for the segments of at least `engine.GROUPED_FROM` positions
    (`emph_split_kv` + `emph_attention_split`, `emph_attention_backward_split`);
    shorter ones keep the fp32 kernels through a tile table of their own.  By
    segment length alone: a segment's result does not depend on the batch.

    `key_counts` (int32 device table, one per segment: `_Layout.key_counts`):
    only a segment's leading `key_counts[i]` positions are keys, the rest is
    zero padding behind `src_key_padding_mask`; `emph_attention` takes the
    table and the way back is `emph_attention_backward_keys`.  Neither with
    `dropout` nor with `pieces`."""

    def __init__(self, x, tensors, heads, layout, index, dropout=None,
                 pieces=0, key_counts=None):
        (self.in_w, self.in_b, self.out_w, self.out_b, self.norm1_w,
         self.norm1_b, self.ff1_w, self.ff1_b, self.ff2_w, self.ff2_b,
         self.norm2_w, self.norm2_b) = tensors
        self.layout, self.index, self.heads = layout, index, int(heads)
        self.dropout, self.pieces = dropout, int(pieces)
        self.key_counts = key_counts
        if key_counts is not None and (dropout is not None or self.pieces):
            raise NotImplementedError(
                'key_counts with dropout or with pieces: the masked and the '
                'bf16 attention kernels take no key-padding mask')
        self.ld = ld = layout.plan.ld_frames
        self.channels = channels = int(x.shape[0])
        self.device = x.device
        self.tiles, self.n_tiles = layout.tiles(DIRECT_TILE)
        bias = _float32(self.in_b)
        self.x = layout.scatter(x, layout.frame_columns, ld)
        self.qk = self.zeros(2 * channels)
        self.conv(self.x, self.qk, self.pack(self.in_w, (0, 2 * channels)),
                  bias, channels, 2 * channels)
        self.v = torch.zeros((ld, channels), dtype=torch.float32,
                             device=self.device)
        self.conv(self.x, self.v,
                  self.pack(self.in_w, (2 * channels, 3 * channels)),
                  bias[2 * channels:], channels, channels, transpose=True)
        self.attended = self.zeros(channels)
        self.attention()
        self.projected = self.zeros(channels)
        self.conv(self.attended, self.projected, self.pack(self.out_w),
                  _float32(self.out_b), channels, channels)
        self.drop(self.projected, 1)
        self.normed1 = self.zeros(channels)
        self.add_layernorm(self.x, self.projected, self.normed1, self.norm1_w,
                           self.norm1_b)
        hidden = int(self.ff1_w.shape[0])
        self.hidden = self.zeros(hidden)
        self.conv(self.normed1, self.hidden, self.pack(self.ff1_w),
                  _float32(self.ff1_b), channels, hidden, activation='relu')
        self.drop(self.hidden, 2)
        self.fed = self.zeros(channels)
        self.conv(self.hidden, self.fed, self.pack(self.ff2_w),
                  _float32(self.ff2_b), hidden, channels)
        self.drop(self.fed, 3)
        self.normed2 = self.zeros(channels)
        self.add_layernorm(self.normed1, self.fed, self.normed2, self.norm2_w,
                           self.norm2_b)

    def zeros(self, rows):
        return torch.zeros((rows, self.ld), dtype=torch.float32,
                           device=self.device)

    def pack(self, weight, rows=None, flipped=False):
        return _device_pack(weight, self.index, flipped, rows)

    def drop(self, buffer, site):
        """The mask of stream_base + `site` on a packed buffer or on its
        gradient, in place (nothing without `dropout`)."""
        if self.dropout is None:
            return
        p, seed, base, step = self.dropout
        _call('emph_dropout', buffer, buffer.numel(), 0, p, seed, base + site,
              step)

    def conv(self, x, y, pack, bias, c_in, c_out, activation=None,
             transpose=False):
        _conv1d(x, y, self.ld, pack, bias, c_in, c_out, 1, activation,
                self.layout, transpose)

    def attention(self):
        """`attended` of `qk` and `v`; under `dropout` the masked kernel with
        its four mask arguments."""
        name, tile, mask = 'emph_attention', DIRECT_TILE, (self.key_counts,)
        if self.dropout is not None:
            name, tile, mask = 'emph_attention_dropout', GRAD_TILE, self.dropout
        tiles, n_tiles = self.tiles, self.n_tiles
        if self.pieces:
            tiles, n_tiles = self.layout.tiles(tile, engine_module.SHORT)
            self.attention_split()
        if n_tiles or not self.pieces:
            _call(name, self.qk, self.v, self.attended, self.ld,
                  self.channels, self.heads, tiles, n_tiles, tile, *mask)

    def attention_split(self):
        """`attended` of the long segments: their keys and values split once,
        then the workgroup kernel on the bf16 pipe."""
        stages, n_stages = self.layout.tiles(DIRECT_TILE, engine_module.LONG)
        tiles, n_tiles = self.layout.tiles(SPLIT_TILE, engine_module.LONG)
        if not n_tiles:
            return
        size = int(runtime.library().emph_split_kv_bytes(
            self.ld, len(self.layout.plan), self.channels, self.heads,
            self.pieces))
        images = torch.empty(size, dtype=torch.uint8, device=self.device)
        _call('emph_split_kv', self.qk, self.v, self.ld, self.channels,
              self.heads, stages, n_stages, DIRECT_TILE, self.pieces, images)
        _call('emph_attention_split', self.qk, images, self.attended, self.ld,
              self.channels, self.heads, tiles, n_tiles, SPLIT_TILE, None,
              self.pieces)

    def add_layernorm(self, x, r, y, gamma, beta):
        _call('emph_add_layernorm', x, r, y, self.ld, self.channels,
              _float32(gamma), _float32(beta), LAYER_EPS, 0, self.ld)

    # ---- the way back

    def layernorm_backward(self, summed, gamma, dy):
        """(ds, dgamma, dbeta) of `emph_add_layernorm_backward`."""
        ds = self.zeros(self.channels)
        dgamma = torch.empty(self.channels, dtype=torch.float32,
                             device=self.device)
        dbeta = torch.empty_like(dgamma)
        parts = int(runtime.library().emph_add_layernorm_backward_parts(
            self.n_tiles))
        workspace = torch.empty(max(1, parts * 2 * self.channels),
                                dtype=torch.float32, device=self.device)
        _call('emph_add_layernorm_backward', summed, _float32(gamma), dy, ds,
              self.ld, self.channels, LAYER_EPS, self.tiles, self.n_tiles,
              GRAD_TILE, workspace, dgamma, dbeta)
        return ds, dgamma, dbeta

    def attention_backward(self, dattended):
        """dQ | dK | dV [3 C, ld] of `dattended`; under `dropout` the masked
        kernel with its four mask arguments, under `key_counts` the padded
        one with the table in front of the workspace."""
        name, mask = 'emph_attention_backward', ()
        if self.dropout is not None:
            name, mask = 'emph_attention_dropout_backward', self.dropout
        dqkv = self.zeros(3 * self.channels)
        library = runtime.library()
        sizes = [getattr(library, name + '_workspace')]
        if self.key_counts is not None:
            name = 'emph_attention_backward_keys'
        if self.pieces:
            # (one buffer serves both launches: they walk other segments)
            sizes.append(library.emph_attention_backward_split_workspace)
        workspace = torch.empty(
            max(1, *[int(size(self.ld, self.heads)) for size in sizes]),
            dtype=torch.float32, device=self.device)
        tiles, n_tiles = self.tiles, self.n_tiles
        if self.pieces:
            tiles, n_tiles = self.layout.tiles(GRAD_TILE, engine_module.SHORT)
            self.attention_backward_split(dattended, dqkv, workspace)
        if n_tiles or not self.pieces:
            table = () if self.key_counts is None else (self.key_counts,)
            _call(name, self.qk, self.v, self.attended, dattended, dqkv,
                  self.ld, self.channels, self.heads, tiles, n_tiles,
                  GRAD_TILE, *table, workspace, *mask)
        return dqkv

    def attention_backward_split(self, dattended, dqkv, workspace):
        """The long segments' columns of `dqkv` on the bf16 pipe (`workspace`:
        at least `emph_attention_backward_split_workspace` floats)."""
        tiles, n_tiles = self.layout.tiles(SPLIT_TILE, engine_module.LONG)
        if not n_tiles:
            return
        size = int(runtime.library().emph_attention_backward_split_bytes(
            self.ld, len(self.layout.plan), self.channels, self.heads))
        images = torch.empty(size, dtype=torch.uint8, device=self.device)
        _call('emph_attention_backward_split', self.qk, self.v, self.attended,
              dattended, dqkv, self.ld, self.channels, self.heads, tiles,
              n_tiles, SPLIT_TILE, images, workspace)

    def backward(self, grad, need):
        """The thirteen gradients (packed dx gathered by the caller; None
        where `need` is False), walking back only as far as `need` asks."""
        channels, ld, device = self.channels, self.ld, self.device
        hidden = self.hidden.shape[0]
        out = [None] * 13

        def linear_grads(dy, x, weight, slot, rows=None):
            """dweight and dbias of a Linear layer into `out[slot]`,
            `out[slot + 1]` (`rows`: as slices of that many rows)."""
            if not (need[slot] or need[slot + 1]):
                return
            c_out, c_in = weight.shape
            dweight = torch.empty((c_out, c_in), dtype=torch.float32,
                                  device=device)
            dbias = torch.empty(c_out, dtype=torch.float32, device=device)
            for first in range(0, c_out, rows or c_out):
                last = first + (rows or c_out)
                _weight_grad(dy[first:last], x, ld, c_in, last - first, 1,
                             self.layout, dweight[first:last],
                             dbias[first:last])
            out[slot] = dweight if need[slot] else None
            out[slot + 1] = dbias if need[slot + 1] else None

        dy = self.layout.scatter(grad, self.layout.frame_columns, ld)
        ds2, dgamma, dbeta = self.layernorm_backward(
            self.normed1 + self.fed, self.norm2_w, dy)
        dfed = ds2
        if self.dropout is not None:
            dfed = ds2.clone()
            self.drop(dfed, 3)
        out[11], out[12] = (dgamma if need[11] else None,
                            dbeta if need[12] else None)
        if not any(need[:11]):
            return out
        linear_grads(dfed, self.hidden, self.ff2_w, 9)
        if not any(need[:9]):
            return out
        dhidden = self.zeros(hidden)
        self.conv(dfed, dhidden, self.pack(self.ff2_w, flipped=True), None,
                  channels, hidden)
        # (the kept `hidden` is positive only where the ReLU passed AND the
        # mask kept: the activation gradient below selects by either)
        self.drop(dhidden, 2)
        _call('emph_activation_gradient', self.hidden, dhidden,
              dhidden.numel(), runtime.ACTIVATIONS['relu'])
        linear_grads(dhidden, self.normed1, self.ff1_w, 7)
        if not any(need[:7]):
            return out
        dnormed1 = self.zeros(channels)
        self.conv(dhidden, dnormed1, self.pack(self.ff1_w, flipped=True), None,
                  hidden, channels)
        dnormed1 += ds2
        ds1, dgamma, dbeta = self.layernorm_backward(
            self.x + self.projected, self.norm1_w, dnormed1)
        out[5], out[6] = (dgamma if need[5] else None,
                          dbeta if need[6] else None)
        dprojected = ds1
        if self.dropout is not None:
            dprojected = ds1.clone()
            self.drop(dprojected, 1)
        linear_grads(dprojected, self.attended, self.out_w, 3)
        if not any(need[:3]):
            return out
        dattended = self.zeros(channels)
        self.conv(dprojected, dattended, self.pack(self.out_w, flipped=True),
                  None, channels, channels)
        dqkv = self.attention_backward(dattended)
        linear_grads(dqkv, self.x, self.in_w, 1, rows=channels)
        if need[0]:
            dx = self.zeros(channels)
            self.conv(dqkv, dx, self.pack(self.in_w, flipped=True), None,
                      3 * channels, channels)
            dx += ds1
            out[0] = dx
        return out
