// The small backward kernels of the differentiable operator seams
// (emphases_amd/ops.py): the backward of emph_segment_reduce for all four
// reductions and the gradient of the four activations.  (The heavy one, the
// weight gradient of a Conv1d of any shape, is csrc/conv_grad_any.hip; the
// data gradient is emph_conv1d itself on a transposed, tap-flipped pack.)
//
// Replaces what autograd does for emphases.downsample
// (emphases/core.py:426-469: slice + sum / mean / max / index per word) and for
// the activation of model/layers/convolution.py:28 (ReLU, GELU, SiLU,
// LeakyReLU: config/hparam-search/activation-*.py).
//
// Everything here is deterministic: no atomics, every output element is
// written by exactly one thread.
#include <math.h>

#include "common.h"
#include "step.h"

namespace emph {

// One workgroup per 64-frame tile; a wave owns channels wave, wave + 4, ...
// and its 64 lanes are the 64 frames of the tile.  A lane finds the word of
// its frame by bisection over the segment's (sorted, non-overlapping) words.
//
// max: the gradient goes to the FIRST frame of the word whose value equals
// the word's maximum `y` (torch's tie rule for max(dim)).  Inside the tile
// that is a ballot: the lowest matching lane of the word.  Only the word that
// covers the tile's first frame can begin in an earlier tile; its earlier
// frames are searched 64 at a time by the whole wave.
__global__ __launch_bounds__(256) void segment_reduce_backward_kernel(
    const float* __restrict__ dword, int64_t ldw, const int32_t* __restrict__ bounds,
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ y,
    float* __restrict__ dx, int64_t ld_dx, int channels, const int64_t* __restrict__ seg,
    const int32_t* __restrict__ tiles, int mode) {
    const Tile tile = load_tile(tiles, blockIdx.x);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int t = tile.first + lane;
    const bool inside = t < tile.count;
    const int64_t* row = seg + static_cast<int64_t>(tile.segment) * EMPH_SEG_FIELDS;
    const int64_t word_off = row[EMPH_SEG_WORD_OFF];
    const int words = static_cast<int>(row[EMPH_SEG_WORDS]);
    const int frames = tile.count;
    // the last word whose start is <= t
    int low = 0, high = words;
    while (low < high) {
        const int middle = (low + high) >> 1;
        if (bounds[word_off + middle] <= t) low = middle + 1; else high = middle;
    }
    const int word = low - 1;
    bool covered = false;
    int64_t column = 0;
    int start = 0, end = 0, center = -1;
    if (word >= 0 && inside) {
        column = word_off + word;
        const int raw_start = bounds[column], raw_end = bounds[ldw + column];
        // Python slice semantics, as the forward (core.py:446-454)
        start = max(0, min(raw_start, frames));
        end = max(start, min(raw_end, frames));
        center = (raw_start + raw_end) >> 1;
        covered = t < end;
    }
    const float scale =
        (mode == EMPH_REDUCE_AVERAGE && covered) ? 1.f / static_cast<float>(end - start) : 1.f;
    // lanes of this tile that belong to the same word and lie before this one
    const int first_lane = max(start - tile.first, 0);
    const uint64_t earlier =
        covered ? ((uint64_t{1} << lane) - 1) & ~((uint64_t{1} << first_lane) - 1) : 0;
    // the word that reaches into the tile from the left (wave-uniform)
    const int carry_covered = __builtin_amdgcn_readfirstlane(covered && start < tile.first);
    const int carry_start = __builtin_amdgcn_readfirstlane(start);
    const int carry_word = __builtin_amdgcn_readfirstlane(word);

    const int64_t at = static_cast<int64_t>(tile.offset) + t;
    for (int c = wave; c < channels; c += 4) {
        float value = 0.f;
        const float g = covered ? dword[static_cast<int64_t>(c) * ldw + column] : 0.f;
        if (mode == EMPH_REDUCE_SUM) {
            value = g;
        } else if (mode == EMPH_REDUCE_AVERAGE) {
            value = covered ? g * scale : 0.f;
        } else if (mode == EMPH_REDUCE_CENTER) {
            value = (covered && t == center) ? g : 0.f;
        } else {
            const float top = covered ? y[static_cast<int64_t>(c) * ldw + column] : 0.f;
            const float own = inside ? x[static_cast<int64_t>(c) * ldx + at] : 0.f;
            const bool match = covered && own == top;
            const uint64_t matches = __ballot(match);
            bool seen = (matches & earlier) != 0;
            if (carry_covered) {
                const float carry_top = __shfl(top, 0);
                const float* source = x + static_cast<int64_t>(c) * ldx + tile.offset;
                uint64_t before = 0;
                for (int u0 = carry_start; u0 < tile.first; u0 += 64) {
                    const int u = u0 + lane;
                    before |= __ballot(u < tile.first && source[u] == carry_top);
                }
                if (before != 0 && word == carry_word) seen = true;
            }
            value = (match && !seen) ? g : 0.f;
        }
        if (inside) dx[static_cast<int64_t>(c) * ld_dx + at] = value;
    }
}

template <int ACT>
__global__ __launch_bounds__(256) void activation_gradient_kernel(
    const float4* __restrict__ source, float4* __restrict__ gradient, int64_t quads) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= quads) return;
    const float4 s = source[i];
    float4 g = gradient[i];
    g.x = activation_gradient<ACT>(s.x, g.x);
    g.y = activation_gradient<ACT>(s.y, g.y);
    g.z = activation_gradient<ACT>(s.z, g.z);
    g.w = activation_gradient<ACT>(s.w, g.w);
    gradient[i] = g;
}

}  // namespace emph

using namespace emph;

extern "C" {

int emph_segment_reduce_backward(const float* dword, int64_t ldw, const int32_t* bounds,
                                 const float* x, int64_t ldx, const float* y, float* dx,
                                 int64_t ld_dx, int32_t channels, const int64_t* seg,
                                 const int32_t* tiles, int32_t n_tiles, int32_t mode,
                                 void* stream) {
    if (n_tiles == 0) return EMPH_OK;
    EMPH_REQUIRE(dword && bounds && dx && seg && tiles, EMPH_EINVAL,
                 "emph_segment_reduce_backward: null pointer");
    EMPH_REQUIRE(mode >= EMPH_REDUCE_SUM && mode <= EMPH_REDUCE_CENTER, EMPH_EINVAL,
                 "emph_segment_reduce_backward: unknown mode %d", mode);
    EMPH_REQUIRE(mode != EMPH_REDUCE_MAX || (x && y), EMPH_EINVAL,
                 "emph_segment_reduce_backward: max needs the forward's input and output");
    EMPH_REQUIRE(channels > 0 && n_tiles > 0 && ldw > 0 && ldx > 0 && ld_dx > 0, EMPH_EINVAL,
                 "emph_segment_reduce_backward: bad shape");
    EMPH_LAUNCH(segment_reduce_backward_kernel, dim3(n_tiles), dim3(256), 0,
                static_cast<hipStream_t>(stream), dword, ldw, bounds, x, ldx, y, dx, ld_dx,
                channels, seg, tiles, mode);
    return check_launch("emph_segment_reduce_backward");
}

int emph_activation_gradient(const float* source, float* gradient, int64_t count,
                             int32_t activation, void* stream) {
    EMPH_REQUIRE(activation >= EMPH_ACT_NONE && activation <= EMPH_ACT_LEAKY_RELU, EMPH_EINVAL,
                 "emph_activation_gradient: unknown activation %d", activation);
    if (count == 0 || activation == EMPH_ACT_NONE) return EMPH_OK;
    EMPH_REQUIRE(source && gradient, EMPH_EINVAL, "emph_activation_gradient: null pointer");
    EMPH_REQUIRE(count > 0 && count % 4 == 0 &&
                     (reinterpret_cast<uintptr_t>(source) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(gradient) & 15) == 0,
                 EMPH_EINVAL, "emph_activation_gradient: count and pointers in 16-byte units");
    const int64_t quads = count / 4;
    const dim3 grid(static_cast<unsigned>((quads + 255) / 256));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float4* from = reinterpret_cast<const float4*>(source);
    float4* to = reinterpret_cast<float4*>(gradient);
    switch (activation) {
        case EMPH_ACT_RELU:
            EMPH_LAUNCH(activation_gradient_kernel<EMPH_ACT_RELU>, grid, dim3(256), 0, s, from,
                        to, quads);
            break;
        case EMPH_ACT_GELU:
            EMPH_LAUNCH(activation_gradient_kernel<EMPH_ACT_GELU>, grid, dim3(256), 0, s, from,
                        to, quads);
            break;
        case EMPH_ACT_SILU:
            EMPH_LAUNCH(activation_gradient_kernel<EMPH_ACT_SILU>, grid, dim3(256), 0, s, from,
                        to, quads);
            break;
        default:
            EMPH_LAUNCH(activation_gradient_kernel<EMPH_ACT_LEAKY_RELU>, grid, dim3(256), 0, s,
                        from, to, quads);
            break;
    }
    return check_launch("emph_activation_gradient");
}

}  // extern "C"
