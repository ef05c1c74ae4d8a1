// What conv_grad.hip (fp32 MFMA) and conv_grad_split.hip (bf16x3) share: the
// tile and slab geometry of the weight gradient and the fixed-order sum of the
// slabs.
#pragma once

#include <stdint.h>

#include "common.h"

namespace emph {

constexpr int kGradTile = 64;            // positions per staged tile
constexpr int kGradOut = 80;             // output channels (5 m-tiles)
constexpr int kGradParts = 256;          // at most one slab per CU

inline int grad_tiles_per_part(int n_tiles) {
    return (n_tiles + kGradParts - 1) / kGradParts;
}

// dweight, dbias = the sum of `parts` slabs [weight_count + 80] in a fixed order
// (conv_grad.hip: conv_weight_grad_sum_kernel)
int conv_weight_grad_sum(const float* slabs, int parts, int64_t weight_count, float* dweight,
                         float* dbias, hipStream_t stream, const char* what);

}  // namespace emph
