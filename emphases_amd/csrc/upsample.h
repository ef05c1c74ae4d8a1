// Word -> frame interpolation of emphases.upsample (emphases/core.py:472-544)
// for one frame of one utterance: shared by emph_upsample and
// emph_frame_loss_grad (csrc/frame_head.hip), which interpolates its targets
// on the fly.
#pragma once

#include "common.h"

namespace emph {

// Centre of the word in packed column `column`, in frames: start + (end -
// start) / 2 (core.py:487-488).  A multiple of 0.5, exact in float.
__device__ __forceinline__ float word_centre(const int32_t* __restrict__ bounds,
                                             int64_t ldw, int64_t column) {
    const int start = bounds[column], end = bounds[ldw + column];
    return static_cast<float>(start) + static_cast<float>(end - start) * 0.5f;
}

// #{w : centre_w <= frame_time} - 1 over the `words` (>= 1) words whose first
// column is `word_off`: the sum of torch.ge of core.py:507-510, by bisection
// (the words are sorted and disjoint, so their centres ascend strictly).
__device__ __forceinline__ int upsample_index(const int32_t* __restrict__ bounds,
                                              int64_t ldw, int64_t word_off, int words,
                                              float frame_time) {
    int low = 0, high = words;
    while (low < high) {
        const int middle = (low + high) >> 1;
        if (word_centre(bounds, ldw, word_off + middle) <= frame_time)
            low = middle + 1;
        else
            high = middle;
    }
    return low - 1;
}

// The value at frame centre `frame_time` of the row `x` (its first word at
// x[0]) for the index of upsample_index.  One word: the constant
// (core.py:494-495).  EMPH_UPSAMPLE_NEAREST: the last word whose centre is not
// right of the frame (core.py:530-537).  EMPH_UPSAMPLE_LINEAR: the line through
// words j = clamp(index, 0, words - 2) and j + 1, extrapolated at both ends,
// as x_j + slope (f - c_j): the reference's slope f + intercept
// (core.py:501-524) cancels at large f.
__device__ __forceinline__ float upsample_value(const float* __restrict__ x,
                                                const int32_t* __restrict__ bounds,
                                                int64_t ldw, int64_t word_off, int words,
                                                int index, float frame_time, int method) {
    if (words == 1) return x[0];
    if (method == EMPH_UPSAMPLE_NEAREST) return x[min(max(index, 0), words - 1)];
    const int j = min(max(index, 0), words - 2);
    const float left = word_centre(bounds, ldw, word_off + j);
    const float right = word_centre(bounds, ldw, word_off + j + 1);
    const float slope = (x[j + 1] - x[j]) / (right - left);
    return x[j] + slope * (frame_time - left);
}

}  // namespace emph
