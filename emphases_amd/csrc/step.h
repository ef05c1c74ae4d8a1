// Device functions that more than one file of the training step uses: the
// fixed-order block sum, the backward of the output projection for any odd
// kernel size (train.hip launches it at 3, grid.hip at 1, 3, 5 and 7), the
// derivative of the four activations (autograd.hip, grid.hip) and the Philox
// generator of the dropout masks (dropout.hip, grid.hip).  One definition
// each, so that two entry points that promise the same bits run the same code.
#pragma once

#include <math.h>

#include "common.h"

namespace emph {

// Sum of `value` over the 256 threads of the block, in a fixed order (a
// binary tree over thread indices); valid in thread 0.
template <typename T>
__device__ __forceinline__ T block_sum(T value, T* shared) {
    shared[threadIdx.x] = value;
    __syncthreads();
#pragma unroll
    for (int width = 128; width > 0; width >>= 1) {
        if (static_cast<int>(threadIdx.x) < width)
            shared[threadIdx.x] += shared[threadIdx.x + width];
        __syncthreads();
    }
    const T total = shared[0];
    __syncthreads();
    return total;
}

// dx of Conv1d(channels, 1, K): a thread per (channel, column).
template <int K>
__global__ __launch_bounds__(256) void output_backward_data_kernel(
    const float* __restrict__ dlogit, const float* __restrict__ weight,
    const int32_t* __restrict__ word_segment, int channels, int64_t columns,
    float* __restrict__ dx, int64_t ldx) {
    const int64_t index = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (index >= columns * channels) return;
    const int c = static_cast<int>(index / columns);
    const int64_t column = index - c * columns;
    const int segment = word_segment[column];
    float value = 0.f;
    if (segment >= 0) {
        // dx[c][w] = sum_j W[c][j] dlogit[w - j + (K - 1) / 2], inside the segment
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int64_t from = column - j + (K - 1) / 2;
            if (from >= 0 && from < columns && word_segment[from] == segment)
                value = fmaf(weight[c * K + j], dlogit[from], value);
        }
    }
    dx[static_cast<int64_t>(c) * ldx + column] = value;
}

// dW and db of Conv1d(channels, 1, K): block c < channels sums the K taps of
// channel c, block `channels` sums the bias.
template <int K>
__global__ __launch_bounds__(256) void output_backward_weight_kernel(
    const float* __restrict__ dlogit, const float* __restrict__ x, int64_t ldx,
    const int32_t* __restrict__ word_segment, int channels, int64_t columns,
    float* __restrict__ dweight, float* __restrict__ dbias) {
    __shared__ float shared[256];
    const int c = blockIdx.x;
    float sum[K];
#pragma unroll
    for (int j = 0; j < K; ++j) sum[j] = 0.f;
    for (int64_t column = threadIdx.x; column < columns; column += 256) {
        const int segment = word_segment[column];
        if (segment < 0) continue;
        const float g = dlogit[column];
        if (c == channels) {
            sum[0] += g;
            continue;
        }
        // dW[c][j] = sum_w dlogit[w] x[c][w + j - (K - 1) / 2], x zero outside
        // the segment (a select: what lies there is never read)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int64_t from = column + j - (K - 1) / 2;
            if (from >= 0 && from < columns && word_segment[from] == segment)
                sum[j] = fmaf(g, x[static_cast<int64_t>(c) * ldx + from], sum[j]);
        }
    }
    if (c == channels) {
        const float total = block_sum(sum[0], shared);
        if (threadIdx.x == 0) dbias[0] = total;
        return;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float total = block_sum(sum[j], shared);
        if (threadIdx.x == 0) dweight[c * K + j] = total;
    }
}

template <int K>
inline int launch_output_backward(const float* dlogit, const float* x, int64_t ldx,
                                  const float* weight, const int32_t* word_segment,
                                  int channels, int64_t columns, float* dweight, float* dbias,
                                  float* dx, int64_t ld_dx, hipStream_t s, const char* what) {
    EMPH_LAUNCH(output_backward_weight_kernel<K>, dim3(channels + 1), dim3(256), 0, s, dlogit,
                x, ldx, word_segment, channels, columns, dweight, dbias);
    if (int status = check_launch(what)) return status;
    const int64_t threads = columns * channels;
    EMPH_LAUNCH(output_backward_data_kernel<K>,
                dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, s, dlogit,
                weight, word_segment, channels, columns, dx, ld_dx);
    return check_launch(what);
}

constexpr float kLeakySlope = 0.01f;      // torch.nn.LeakyReLU default

// g act'(.): `source` is the saved OUTPUT for ReLU and LeakyReLU (its sign is
// the pre-activation's), the PRE-ACTIVATION for GELU and SiLU.
template <int ACT>
__device__ __forceinline__ float activation_gradient(float source, float g) {
    if (ACT == EMPH_ACT_NONE) return g;
    if (ACT == EMPH_ACT_RELU) return source > 0.f ? g : 0.f;
    if (ACT == EMPH_ACT_LEAKY_RELU) return source > 0.f ? g : g * kLeakySlope;
    if (ACT == EMPH_ACT_GELU) {
        // ATen's GeluBackward, exact form: cdf + x pdf
        const float cdf = 0.5f * (1.f + erff(source * 0.70710678118654752440f));
        const float pdf = expf(-0.5f * source * source) * 0.39894228040143267794f;
        return g * (cdf + source * pdf);
    }
    // ATen's silu_backward: sigmoid (1 + x (1 - sigmoid))
    const float sigmoid = 1.f / (1.f + expf(-source));
    return g * (sigmoid * (1.f + source * (1.f - sigmoid)));
}

// Philox-4x32-10 (Salmon et al., SC'11): the generator of the dropout masks,
// specified in dropout.hip and emphases_amd/train/dropout.py.
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
struct Words {
    uint32_t x, y, z, w;
};

__host__ __device__ __forceinline__ Words philox4x32_10(Words c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t first = static_cast<uint64_t>(kPhiloxM0) * c.x;
        const uint64_t second = static_cast<uint64_t>(kPhiloxM1) * c.z;
        c = Words{static_cast<uint32_t>(second >> 32) ^ c.y ^ k0, static_cast<uint32_t>(second),
                  static_cast<uint32_t>(first >> 32) ^ c.w ^ k1, static_cast<uint32_t>(first)};
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    return c;
}

// The words of quad `quad` of layer `stream_id` at step `step`.
__host__ __device__ __forceinline__ Words dropout_words(uint64_t quad, uint32_t stream_id,
                                                        uint32_t step, uint32_t seed_lo,
                                                        uint32_t seed_hi) {
    return philox4x32_10(
        Words{static_cast<uint32_t>(quad), static_cast<uint32_t>(quad >> 32), stream_id, step},
        seed_lo, seed_hi);
}

// float32(1 / (1 - p)), formed in double and rounded once.
inline float dropout_scale(float p) {
    return static_cast<float>(1.0 / (1.0 - static_cast<double>(p)));
}

// min(round(p 2^32), 2^32 - 1); p 2^32 is exact in double, halves go to even.
inline uint32_t dropout_threshold(float p) {
    const double scaled = nearbyint(static_cast<double>(p) * 4294967296.0);
    return scaled >= 4294967295.0 ? 0xFFFFFFFFu : static_cast<uint32_t>(scaled);
}

}  // namespace emph
