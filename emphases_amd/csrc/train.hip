// The small kernels of the training step of the convolution model: loss and
// its gradient, the backward of the output projection, of the activation and
// of the frame -> word reduce, the Adam update, and the gather that rebuilds
// the MFMA weight packs from the flat parameter buffer.  (The heavy one, the
// weight gradient of a Conv1d, is csrc/conv_grad.hip; the data gradient is
// emph_conv1d itself on a transposed, tap-flipped pack.)
//
// Replaces what autograd and torch.optim.Adam do for the reference's loop
// (emphases/train/core.py:111-142): loss 315-353, `scaler.scale(loss)
// .backward()` 136, `scaler.step(optimizer)` 139 - in fp32, no GradScaler.
//
// Everything here is deterministic: no floating-point atomics, every
// reduction in a fixed order that does not depend on the launch.
#include <math.h>

#include "common.h"
#include "step.h"

namespace emph {

__global__ __launch_bounds__(256) void take_kernel(
    const float* __restrict__ src, const int32_t* __restrict__ index,
    float* __restrict__ out, int64_t count) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= count) return;
    const int32_t from = index[i];
    out[i] = from < 0 ? 0.f : src[from];
}

// One workgroup: thread i owns columns i, i + 256, ... of the packed word
// axis (in that order), then the fixed tree.  The loss is a few thousand
// terms at the most, so each term and the sum are formed in double and the
// mean is rounded to float once: the scalar carries the error of the logits
// alone, not another ulp or two of its own.  The gradient stays in float.
__global__ __launch_bounds__(256) void loss_grad_kernel(
    const float* __restrict__ logits, const float* __restrict__ targets,
    const int32_t* __restrict__ word_segment, int64_t columns, int64_t valid_words,
    int form, float* __restrict__ loss, float* __restrict__ dlogit) {
    // (the gradient's 1 / N is a float, as autograd's is; the mean divides)
    const float inverse_count = static_cast<float>(1.0 / static_cast<double>(valid_words));
    __shared__ double shared[256];
    double sum = 0.;
    for (int64_t column = threadIdx.x; column < columns; column += 256) {
        float gradient = 0.f;
        if (word_segment[column] >= 0) {
            const float z = logits[column], y = targets[column];
            if (form == 0) {
                // binary_cross_entropy_with_logits, the stable form of ATen
                const double wide = z;
                sum += fmax(wide, 0.) - wide * y + log1p(exp(-fabs(wide)));
                gradient = (1.f / (1.f + expf(-z)) - y) * inverse_count;
            } else {
                const float d = z - y;
                const double wide = static_cast<double>(z) - y;
                sum += wide * wide;
                gradient = 2.f * d * inverse_count;
            }
        }
        dlogit[column] = gradient;
    }
    const double total = block_sum(sum, shared);
    if (threadIdx.x == 0) loss[0] = static_cast<float>(total / static_cast<double>(valid_words));
}

// (the backward of the output projection is step.h's, for any kernel size)

__global__ __launch_bounds__(256) void activation_backward_kernel(
    const float4* __restrict__ y, float4* __restrict__ gradient, int64_t quads) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= quads) return;
    const float4 out = y[i];
    float4 g = gradient[i];
    // (a select, not a product: what lies outside the segments is undefined)
    g.x = out.x > 0.f ? g.x : 0.f;
    g.y = out.y > 0.f ? g.y : 0.f;
    g.z = out.z > 0.f ? g.z : 0.f;
    g.w = out.w > 0.f ? g.w : 0.f;
    gradient[i] = g;
}

// One workgroup per 64-frame tile: 64 frames x 4 channel lanes.  A thread
// finds the word of its frame by bisection over the segment's (sorted,
// non-overlapping) words, then walks the channels.
__global__ __launch_bounds__(256) void segment_broadcast_kernel(
    const float* __restrict__ dword, int64_t ldw, const int32_t* __restrict__ bounds,
    float* __restrict__ dx, int64_t ldx, int channels, const int64_t* __restrict__ seg,
    const int32_t* __restrict__ tiles, int mode) {
    const Tile tile = load_tile(tiles, blockIdx.x);
    const int t = tile.first + (threadIdx.x & 63);
    if (t >= tile.count) return;
    const int64_t* row = seg + static_cast<int64_t>(tile.segment) * EMPH_SEG_FIELDS;
    const int64_t word_off = row[EMPH_SEG_WORD_OFF];
    const int words = static_cast<int>(row[EMPH_SEG_WORDS]);
    // the last word whose start is <= t
    int low = 0, high = words;
    while (low < high) {
        const int middle = (low + high) >> 1;
        if (bounds[word_off + middle] <= t) low = middle + 1; else high = middle;
    }
    const int word = low - 1;
    float scale = 0.f;
    int64_t column = 0;
    if (word >= 0) {
        column = word_off + word;
        const int start = bounds[column], end = bounds[ldw + column];
        if (t < end)
            scale = mode == EMPH_REDUCE_AVERAGE ? 1.f / static_cast<float>(end - start) : 1.f;
    }
    float* out = dx + tile.offset + t;
    for (int c = threadIdx.x >> 6; c < channels; c += 4) {
        float value = 0.f;
        if (scale != 0.f) {
            value = dword[static_cast<int64_t>(c) * ldw + column];
            if (mode == EMPH_REDUCE_AVERAGE) value *= scale;
        }
        out[static_cast<int64_t>(c) * ldx] = value;
    }
}

// torch.optim.Adam, single-tensor arithmetic (torch/optim/adam.py,
// _single_tensor_adam): lerp, mul + addcmul, sqrt / sqrt(bc2) + eps, addcdiv.
// weight1 = 1 - beta1 and weight2 = 1 - beta2 are formed in double and rounded
// once, as torch's Python scalars are: 1.f - 0.999f is 2e-6 off 0.001f.
struct AdamScalars {
    float weight1, beta2, weight2, step_size, correction2_sqrt, eps;
};

// The update of ONE element: what both kernels below evaluate, so that they
// give the same bits.  Which products the compiler fuses into their sums is
// its choice per kernel (it fused only the last line of adam_step_kernel when
// that held these expressions itself, and the second line as well once they
// were inlined), so the choice is written down: contraction off, and the one
// fused multiply-add spelled out.  These are the roundings adam_step_kernel
// always had.
__device__ __forceinline__ void adam_update(float* __restrict__ parameter, float g,
                                            float* __restrict__ exp_avg,
                                            float* __restrict__ exp_avg_sq, int64_t i,
                                            const AdamScalars& s) {
#pragma clang fp contract(off)
    const float m = exp_avg[i] + s.weight1 * (g - exp_avg[i]);
    const float v = exp_avg_sq[i] * s.beta2 + s.weight2 * g * g;
    exp_avg[i] = m;
    exp_avg_sq[i] = v;
    const float denominator = sqrtf(v) / s.correction2_sqrt + s.eps;
    parameter[i] = fmaf(-s.step_size, m / denominator, parameter[i]);
}

__global__ __launch_bounds__(256) void adam_step_kernel(
    float* __restrict__ parameter, const float* __restrict__ gradient,
    float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, int64_t count,
    AdamScalars scalars) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= count) return;
    adam_update(parameter, gradient[i], exp_avg, exp_avg_sq, i, scalars);
}

// The same update with the gradients where autograd left them: one tensor per
// parameter, each anywhere.  A launch carries a table of up to kAdamTable
// tensors in its arguments (2.3 KB of the 4 KB a launch may pass): the
// gradient's address, the tensor's first element in the flat buffers, its
// count, and the prefix sums of the tensors' workgroup counts.  A workgroup
// finds its tensor by bisection over that prefix - the same for every lane,
// so scalar loads of the arguments - and then is adam_step_kernel's workgroup
// on that tensor: 256 consecutive elements, plain 4-byte loads and stores
// (a gradient is aligned to its element and to nothing more).
constexpr int kAdamTable = EMPH_ADAM_TABLE;

struct AdamTable {
    const float* gradient[kAdamTable];
    int64_t offset[kAdamTable];
    int32_t count[kAdamTable];
    int32_t first_block[kAdamTable + 1];   // first_block[tensors] = the grid
    int32_t tensors;
};

__global__ __launch_bounds__(256) void adam_step_gathered_kernel(
    float* __restrict__ parameter, float* __restrict__ exp_avg,
    float* __restrict__ exp_avg_sq, AdamTable table, AdamScalars scalars) {
    const int block = static_cast<int>(blockIdx.x);
    // the last tensor whose first workgroup is <= block (no tensor is empty,
    // so first_block is strictly increasing)
    int low = 0, high = table.tensors - 1;
    while (low < high) {
        const int middle = (low + high + 1) >> 1;
        if (table.first_block[middle] <= block) low = middle; else high = middle - 1;
    }
    const int local = (block - table.first_block[low]) * 256 + static_cast<int>(threadIdx.x);
    if (local >= table.count[low]) return;
    const float g = table.gradient[low][local];
    adam_update(parameter, g, exp_avg, exp_avg_sq, table.offset[low] + local, scalars);
}

}  // namespace emph

using namespace emph;

extern "C" {

int emph_take(const float* src, const int32_t* index, float* out, int64_t count,
              void* stream) {
    if (count == 0) return EMPH_OK;
    EMPH_REQUIRE(src && index && out, EMPH_EINVAL, "emph_take: null pointer");
    EMPH_REQUIRE(count > 0 && count < (int64_t{1} << 39), EMPH_ERANGE,
                 "emph_take: count out of range");
    EMPH_LAUNCH(take_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256),
                0, static_cast<hipStream_t>(stream), src, index, out, count);
    return check_launch("emph_take");
}

int emph_loss_grad(const float* logits, const float* targets,
                   const int32_t* word_segment, int64_t columns, int64_t valid_words,
                   int32_t form, float* loss, float* dlogit, void* stream) {
    EMPH_REQUIRE(logits && targets && word_segment && loss && dlogit, EMPH_EINVAL,
                 "emph_loss_grad: null pointer");
    EMPH_REQUIRE(form == 0 || form == 1, EMPH_EINVAL,
                 "emph_loss_grad: form %d (0 = bce, 1 = mse)", form);
    EMPH_REQUIRE(columns > 0 && valid_words > 0 && valid_words <= columns, EMPH_EINVAL,
                 "emph_loss_grad: bad shape");
    EMPH_LAUNCH(loss_grad_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream),
                logits, targets, word_segment, columns, valid_words, form, loss, dlogit);
    return check_launch("emph_loss_grad");
}

int emph_output_layer_backward(const float* dlogit, const float* x, int64_t ldx,
                               const float* weight, const int32_t* word_segment,
                               int32_t channels, int32_t kernel_size, int64_t columns,
                               float* dweight, float* dbias, float* dx, int64_t ld_dx,
                               void* stream) {
    EMPH_REQUIRE(dlogit && x && weight && word_segment && dweight && dbias && dx,
                 EMPH_EINVAL, "emph_output_layer_backward: null pointer");
    EMPH_REQUIRE(kernel_size == 3, EMPH_ERANGE,
                 "emph_output_layer_backward: kernel_size %d (3)", kernel_size);
    EMPH_REQUIRE(channels > 0 && channels <= 1024 && columns > 0 && columns <= ldx &&
                     columns <= ld_dx,
                 EMPH_EINVAL, "emph_output_layer_backward: bad shape");
    return launch_output_backward<3>(dlogit, x, ldx, weight, word_segment, channels, columns,
                                     dweight, dbias, dx, ld_dx,
                                     static_cast<hipStream_t>(stream),
                                     "emph_output_layer_backward");
}

int emph_activation_backward(const float* y, float* gradient, int64_t count,
                             int32_t activation, void* stream) {
    if (count == 0) return EMPH_OK;
    EMPH_REQUIRE(y && gradient, EMPH_EINVAL, "emph_activation_backward: null pointer");
    EMPH_REQUIRE(activation == EMPH_ACT_RELU, EMPH_EINVAL,
                 "emph_activation_backward: activation %d (relu only)", activation);
    EMPH_REQUIRE(count > 0 && count % 4 == 0 &&
                     (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(gradient) & 15) == 0,
                 EMPH_EINVAL, "emph_activation_backward: count and pointers in 16-byte units");
    const int64_t quads = count / 4;
    EMPH_LAUNCH(activation_backward_kernel, dim3(static_cast<unsigned>((quads + 255) / 256)),
                dim3(256), 0, static_cast<hipStream_t>(stream),
                reinterpret_cast<const float4*>(y), reinterpret_cast<float4*>(gradient), quads);
    return check_launch("emph_activation_backward");
}

int emph_segment_broadcast(const float* dword, int64_t ldw, const int32_t* bounds,
                           float* dx, int64_t ldx, int32_t channels, const int64_t* seg,
                           const int32_t* tiles, int32_t n_tiles, int32_t mode,
                           void* stream) {
    if (n_tiles == 0) return EMPH_OK;
    EMPH_REQUIRE(dword && bounds && dx && seg && tiles, EMPH_EINVAL,
                 "emph_segment_broadcast: null pointer");
    EMPH_REQUIRE(mode == EMPH_REDUCE_SUM || mode == EMPH_REDUCE_AVERAGE, EMPH_EINVAL,
                 "emph_segment_broadcast: mode %d (sum or average)", mode);
    EMPH_REQUIRE(channels > 0 && n_tiles > 0, EMPH_EINVAL,
                 "emph_segment_broadcast: bad shape");
    EMPH_LAUNCH(segment_broadcast_kernel, dim3(n_tiles), dim3(256), 0,
                static_cast<hipStream_t>(stream), dword, ldw, bounds, dx, ldx, channels, seg,
                tiles, mode);
    return check_launch("emph_segment_broadcast");
}

int emph_adam_step(float* parameter, const float* gradient, float* exp_avg,
                   float* exp_avg_sq, int64_t count, double beta1, double beta2,
                   float step_size, float correction2_sqrt, float eps, void* stream) {
    if (count == 0) return EMPH_OK;
    EMPH_REQUIRE(parameter && gradient && exp_avg && exp_avg_sq, EMPH_EINVAL,
                 "emph_adam_step: null pointer");
    EMPH_REQUIRE(count > 0 && count < (int64_t{1} << 39), EMPH_ERANGE,
                 "emph_adam_step: count out of range");
    EMPH_LAUNCH(adam_step_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256),
                0, static_cast<hipStream_t>(stream), parameter, gradient, exp_avg, exp_avg_sq,
                count,
                AdamScalars{static_cast<float>(1.0 - beta1), static_cast<float>(beta2),
                            static_cast<float>(1.0 - beta2), step_size, correction2_sqrt, eps});
    return check_launch("emph_adam_step");
}

int emph_adam_step_gathered(float* parameters, const float* const* gradients,
                            const int64_t* offsets, const int64_t* counts, int32_t tensors,
                            float* exp_avg, float* exp_avg_sq, double beta1, double beta2,
                            float step_size, float correction2_sqrt, float eps, void* stream) {
    if (tensors == 0) return EMPH_OK;
    EMPH_REQUIRE(tensors > 0, EMPH_EINVAL, "emph_adam_step_gathered: %d tensors", tensors);
    EMPH_REQUIRE(parameters && gradients && offsets && counts && exp_avg && exp_avg_sq,
                 EMPH_EINVAL, "emph_adam_step_gathered: null pointer");
    // every tensor is checked before the first launch: a refusal updates nothing
    for (int32_t t = 0; t < tensors; ++t) {
        EMPH_REQUIRE(counts[t] >= 0 && offsets[t] >= 0, EMPH_EINVAL,
                     "emph_adam_step_gathered: tensor %d: negative count or offset", t);
        EMPH_REQUIRE(counts[t] < (int64_t{1} << 30) && offsets[t] < (int64_t{1} << 39),
                     EMPH_ERANGE, "emph_adam_step_gathered: tensor %d: count or offset out of range",
                     t);
        EMPH_REQUIRE(counts[t] == 0 || gradients[t], EMPH_EINVAL,
                     "emph_adam_step_gathered: tensor %d: null gradient", t);
        EMPH_REQUIRE(counts[t] == 0 || (reinterpret_cast<uintptr_t>(gradients[t]) & 3) == 0,
                     EMPH_EINVAL,
                     "emph_adam_step_gathered: tensor %d: gradient not 4-byte aligned", t);
    }
    const AdamScalars scalars{static_cast<float>(1.0 - beta1), static_cast<float>(beta2),
                              static_cast<float>(1.0 - beta2), step_size, correction2_sqrt, eps};
    AdamTable table;
    table.tensors = 0;
    table.first_block[0] = 0;
    for (int32_t t = 0; t <= tensors; ++t) {
        if (t < tensors && counts[t] == 0) continue;   // (takes no place in a table)
        // a launch when the next tensor finds the table full (of workgroups too), and
        // after the last tensor
        const int64_t blocks = t < tensors ? (counts[t] + 255) / 256 : 0;
        const bool full = table.tensors == kAdamTable ||
                          table.first_block[table.tensors] + blocks > (int64_t{1} << 30);
        if ((t == tensors || full) && table.tensors > 0) {
            EMPH_LAUNCH(adam_step_gathered_kernel,
                        dim3(static_cast<unsigned>(table.first_block[table.tensors])), dim3(256),
                        0, static_cast<hipStream_t>(stream), parameters, exp_avg, exp_avg_sq,
                        table, scalars);
            const int status = check_launch("emph_adam_step_gathered");
            if (status != EMPH_OK) return status;
            table.tensors = 0;
        }
        if (t == tensors) break;
        const int slot = table.tensors++;
        table.gradient[slot] = gradients[t];
        table.offset[slot] = offsets[t];
        table.count[slot] = static_cast<int32_t>(counts[t]);
        table.first_block[slot + 1] = table.first_block[slot] + static_cast<int32_t>(blocks);
    }
    return EMPH_OK;
}

}  // extern "C"
