// Dropout of the training step (torch.nn.Dropout after every activation of
// the conv stacks, emphases/model/layers/convolution.py:29-30, under DROPOUT of
// config/hparam-search/dropout-{05,10}.py): the forward mask and the backward
// of activation + dropout.
//
// The mask is a specification, restated on the host in
// emphases_amd/train/dropout.py: Philox-4x32-10 (Salmon et al., SC'11) with
// counter (q_lo, q_hi, stream, step) and key (seed_lo, seed_hi) for quad
// q = (origin + flat index) / 4; the four output words belong to elements
// 4 q .. 4 q + 3 in order; an element is kept iff its word >= threshold.
// A pure function of its arguments: no state, no atomics, the same bits on
// every launch and for every launch shape.
//
// The backward regenerates nothing: the saved output after dropout is
// positive exactly where the pre-activation was positive AND the element was
// kept (scale > 0), so `y > 0` is the product of the two masks.
#include <math.h>

#include "common.h"
#include "step.h"

namespace emph {

// (the generator itself is step.h's, shared with grid.hip; its constants are
// part of the specification above)
static_assert(kPhiloxM0 == 0xD2511F53u && kPhiloxM1 == 0xCD9E8D57u &&
                  kPhiloxW0 == 0x9E3779B9u && kPhiloxW1 == 0xBB67AE85u,
              "Philox-4x32 multipliers and Weyl constants");

// (a select, never a product with 0: what lies in padding columns is undefined)
__host__ __device__ __forceinline__ float4 dropout_quad(float4 v, uint64_t quad,
                                                        uint32_t stream_id, uint32_t step,
                                                        uint32_t seed_lo, uint32_t seed_hi,
                                                        uint32_t threshold, float scale) {
    const Words r = dropout_words(quad, stream_id, step, seed_lo, seed_hi);
    v.x = r.x >= threshold ? v.x * scale : 0.f;
    v.y = r.y >= threshold ? v.y * scale : 0.f;
    v.z = r.z >= threshold ? v.z * scale : 0.f;
    v.w = r.w >= threshold ? v.w * scale : 0.f;
    return v;
}

// One quad per thread.  A Philox call is a chain of 10 dependent (mul_hi,
// mul_lo) pairs, but at 8 waves per SIMD the other waves hide it: measured
// (tools/micro/dropout_bench.hip), 2, 4 and 8 independent quads per thread are
// each slower than one, which runs within 10 % of the same stream without the
// generator.
__global__ __launch_bounds__(256) void dropout_kernel(
    float4* __restrict__ x, int64_t quads, uint64_t first_quad, uint32_t stream_id,
    uint32_t step, uint32_t seed_lo, uint32_t seed_hi, uint32_t threshold, float scale) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= quads) return;
    x[i] = dropout_quad(x[i], first_quad + static_cast<uint64_t>(i), stream_id, step, seed_lo,
                        seed_hi, threshold, scale);
}

__global__ __launch_bounds__(256) void activation_dropout_backward_kernel(
    const float4* __restrict__ y, float4* __restrict__ gradient, int64_t quads, float scale) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= quads) return;
    const float4 out = y[i];
    float4 g = gradient[i];
    g.x = out.x > 0.f ? g.x * scale : 0.f;
    g.y = out.y > 0.f ? g.y * scale : 0.f;
    g.z = out.z > 0.f ? g.z * scale : 0.f;
    g.w = out.w > 0.f ? g.w * scale : 0.f;
    gradient[i] = g;
}

}  // namespace emph

using namespace emph;

extern "C" {

int emph_dropout(float* x, int64_t count, int64_t origin, float p, uint64_t seed,
                 uint32_t stream_id, uint32_t step, void* stream) {
    EMPH_REQUIRE(x, EMPH_EINVAL, "emph_dropout: null pointer");
    EMPH_REQUIRE(p >= 0.f && p < 1.f, EMPH_EINVAL, "emph_dropout: p %g (0 <= p < 1)",
                 static_cast<double>(p));
    EMPH_REQUIRE(count >= 0 && count % 4 == 0 && origin >= 0 && origin % 4 == 0 &&
                     (reinterpret_cast<uintptr_t>(x) & 15) == 0,
                 EMPH_EINVAL, "emph_dropout: count, origin and pointer in 16-byte units");
    EMPH_REQUIRE(count < (int64_t{1} << 39), EMPH_EINVAL, "emph_dropout: count out of range");
    if (count == 0) return EMPH_OK;
    const int64_t quads = count / 4;
    EMPH_LAUNCH(dropout_kernel, dim3(static_cast<unsigned>((quads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<float4*>(x),
                quads, static_cast<uint64_t>(origin / 4), stream_id, step,
                static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32),
                dropout_threshold(p), dropout_scale(p));
    return check_launch("emph_dropout");
}

int emph_activation_dropout_backward(const float* y, float* gradient, int64_t count,
                                     int32_t activation, float p, void* stream) {
    EMPH_REQUIRE(y && gradient, EMPH_EINVAL, "emph_activation_dropout_backward: null pointer");
    EMPH_REQUIRE(activation == EMPH_ACT_RELU, EMPH_EINVAL,
                 "emph_activation_dropout_backward: activation %d (relu only)", activation);
    EMPH_REQUIRE(p >= 0.f && p < 1.f, EMPH_EINVAL,
                 "emph_activation_dropout_backward: p %g (0 <= p < 1)", static_cast<double>(p));
    EMPH_REQUIRE(count >= 0 && count % 4 == 0 && count < (int64_t{1} << 39) &&
                     (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(gradient) & 15) == 0,
                 EMPH_EINVAL,
                 "emph_activation_dropout_backward: count and pointers in 16-byte units");
    if (count == 0) return EMPH_OK;
    const int64_t quads = count / 4;
    EMPH_LAUNCH(activation_dropout_backward_kernel,
                dim3(static_cast<unsigned>((quads + 255) / 256)), dim3(256), 0,
                static_cast<hipStream_t>(stream), reinterpret_cast<const float4*>(y),
                reinterpret_cast<float4*>(gradient), quads, dropout_scale(p));
    return check_launch("emph_activation_dropout_backward");
}

}  // extern "C"
