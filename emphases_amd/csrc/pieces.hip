// Backward of the pooling at DOWNSAMPLE_LOCATION = 'input'
// (emphases/model/core.py:54-71 under autograd: mean / max / sum over the
// PADDED axis of every word piece, or the column length // 2 for 'center').
//
// The forward is emph_segment_reduce with the piece tables (batch.Pieces):
// piece p is a segment of its own on the piece layout's frame axis and pools
// into the ORIGINAL word column of its word.  emph_segment_broadcast and
// emph_segment_reduce_backward find a frame's word through the segment
// table's own word offsets, which the piece layout does not have (every piece
// has one word, and it lives in another layout); this kernel takes the word
// column of a piece from a table of its own instead.
//
// HBM-bound: channels x (the pieces' columns) floats are written once, in
// 256-byte rows; the reads are one float per (channel, piece) - and, for
// 'max', the forward's input once more.  Deterministic: no atomics, every
// column of a piece is written by exactly one thread, alignment gaps are
// neither read nor written.
#include <math.h>

#include "common.h"

namespace emph {

// One workgroup per 64-column tile of a piece; a wave owns channels wave,
// wave + 4, ... and its 64 lanes are the 64 columns of the tile.
//
// max: the gradient goes to the FIRST column of [0, L) whose value equals the
// pooled value `y` (torch's tie rule for max(dim)).  Inside the tile that is a
// ballot: the lowest matching lane.  The columns of the piece in front of the
// tile are searched 64 at a time by the whole wave.
__global__ __launch_bounds__(256) void piece_pool_backward_kernel(
    const float* __restrict__ dword, int64_t ldw, const int64_t* __restrict__ pieces,
    const int32_t* __restrict__ piece_column, const float* __restrict__ x, int64_t ldx,
    const float* __restrict__ y, float* __restrict__ dx, int64_t ld_dx, int channels,
    const int32_t* __restrict__ tiles, int mode) {
    const Tile tile = load_tile(tiles, blockIdx.x);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int t = tile.first + lane;
    const bool inside = t < tile.count;               // tile.count = L
    const int64_t column = piece_column[tile.segment];
    const int length = static_cast<int>(pieces[static_cast<int64_t>(tile.segment) * 4 + 1]);
    const float scale = mode == EMPH_REDUCE_AVERAGE ? 1.f / static_cast<float>(tile.count) : 1.f;
    const uint64_t earlier = (uint64_t{1} << lane) - 1;
    const int64_t at = static_cast<int64_t>(tile.offset) + t;
    for (int c = wave; c < channels; c += 4) {
        const float g = dword[static_cast<int64_t>(c) * ldw + column];
        float value;
        if (mode == EMPH_REDUCE_SUM) {
            value = g;
        } else if (mode == EMPH_REDUCE_AVERAGE) {
            value = g * scale;
        } else if (mode == EMPH_REDUCE_CENTER) {
            value = t == (length >> 1) ? g : 0.f;
        } else {
            const float top = y[static_cast<int64_t>(c) * ldw + column];
            const float* source = x + static_cast<int64_t>(c) * ldx + tile.offset;
            const bool match = inside && source[t] == top;
            bool seen = (__ballot(match) & earlier) != 0;
            uint64_t before = 0;
            for (int u0 = 0; u0 < tile.first; u0 += 64) {
                const int u = u0 + lane;
                before |= __ballot(u < tile.first && source[u] == top);
            }
            seen = seen || before != 0;
            value = (match && !seen) ? g : 0.f;
        }
        if (inside) dx[static_cast<int64_t>(c) * ld_dx + at] = value;
    }
}

}  // namespace emph

using namespace emph;

extern "C" {

int emph_piece_pool_backward(const float* dword, int64_t ldw, const int64_t* pieces,
                             const int32_t* piece_column, int32_t n_pieces, const float* x,
                             int64_t ldx, const float* y, float* dx, int64_t ld_dx,
                             int32_t channels, const int32_t* tiles, int32_t n_tiles,
                             int32_t mode, void* stream) {
    EMPH_REQUIRE(mode >= EMPH_REDUCE_SUM && mode <= EMPH_REDUCE_CENTER, EMPH_EINVAL,
                 "emph_piece_pool_backward: unknown mode %d", mode);
    EMPH_REQUIRE(n_tiles >= 0 && n_pieces >= 0 && (n_tiles == 0) == (n_pieces == 0) &&
                     n_tiles >= n_pieces,
                 EMPH_EINVAL, "emph_piece_pool_backward: %d tiles for %d pieces", n_tiles,
                 n_pieces);
    if (n_tiles == 0) return EMPH_OK;
    EMPH_REQUIRE(dword && pieces && piece_column && dx && tiles, EMPH_EINVAL,
                 "emph_piece_pool_backward: null pointer");
    EMPH_REQUIRE(mode != EMPH_REDUCE_MAX || (x && y), EMPH_EINVAL,
                 "emph_piece_pool_backward: max needs the forward's input and output");
    EMPH_REQUIRE(channels > 0 && ldw > 0 && ld_dx > 0 && (mode != EMPH_REDUCE_MAX || ldx > 0),
                 EMPH_EINVAL, "emph_piece_pool_backward: bad shape");
    EMPH_LAUNCH(piece_pool_backward_kernel, dim3(n_tiles), dim3(256), 0,
                static_cast<hipStream_t>(stream), dword, ldw, pieces, piece_column, x, ldx, y,
                dx, ld_dx, channels, tiles, mode);
    return check_launch("emph_piece_pool_backward");
}

}  // extern "C"
