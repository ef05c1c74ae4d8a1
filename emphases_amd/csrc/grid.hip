// What the fused step of the reference's hyperparameter grid
// (emphases_amd.train.GridTrainer: any activation, channel count and kernel
// size at DOWNSAMPLE_LOCATION 'intermediate') needs beyond the kernels of the
// default model:
//
// * the backward of the output projection Conv1d(channels, 1, k) for
//   k = 1, 3, 5, 7 (config/hparam-search/decoder-kernel-{1,5}.py): step.h's
//   kernels, the ones emph_output_layer_backward launches at k = 3;
// * activation + dropout out of place on a kept pre-activation (GELU and
//   SiLU differentiate at the pre-activation, so the convolution writes it and
//   this pass writes the layer's output);
// * the backward of activation + dropout for every activation, with the mask
//   regenerated from its Philox counters: off the saved output it can be read
//   for ReLU only (dropout.hip).
//
// The two elementwise kernels are streams at HBM rate, laid out as
// dropout.hip's: one float4 and one Philox call per thread.  Nothing here
// uses atomics or passes anything between workgroups: the same arguments give
// the same bits on every launch.
#include <math.h>

#include "common.h"
#include "step.h"

namespace emph {

struct Mask {
    uint32_t stream_id, step, seed_lo, seed_hi, threshold;
    float scale;
};

// act(z) with the bits of emph_conv1d's epilogue: behind GELU, SiLU and
// LeakyReLU store_patch() adds a zero in place of the bias it has already
// added, which turns -0 into +0.
template <int ACT>
__device__ __forceinline__ float activate_as_epilogue(float z) {
    const float y = activate<ACT>(z);
    return ACT > EMPH_ACT_RELU ? y + 0.f : y;
}

// y = kept ? act(z) scale : +0 (a select: a dropped NaN becomes 0).  DROP =
// false is p = 0: every element kept, scale 1, no generator.
template <int ACT, bool DROP>
__global__ __launch_bounds__(256) void activation_dropout_kernel(
    const float4* z, float4* y, int64_t quads, Mask mask) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= quads) return;
    float4 v = z[i];
    v.x = activate_as_epilogue<ACT>(v.x);
    v.y = activate_as_epilogue<ACT>(v.y);
    v.z = activate_as_epilogue<ACT>(v.z);
    v.w = activate_as_epilogue<ACT>(v.w);
    if (DROP) {
        const Words r = dropout_words(static_cast<uint64_t>(i), mask.stream_id, mask.step,
                                      mask.seed_lo, mask.seed_hi);
        v.x = r.x >= mask.threshold ? v.x * mask.scale : 0.f;
        v.y = r.y >= mask.threshold ? v.y * mask.scale : 0.f;
        v.z = r.z >= mask.threshold ? v.z * mask.scale : 0.f;
        v.w = r.w >= mask.threshold ? v.w * mask.scale : 0.f;
    }
    y[i] = v;
}

// gradient = kept ? act'(source) (gradient scale) : 0, in place.
template <int ACT, bool DROP>
__global__ __launch_bounds__(256) void activation_dropout_gradient_kernel(
    const float4* __restrict__ source, float4* __restrict__ gradient, int64_t quads,
    Mask mask) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= quads) return;
    const float4 s = source[i];
    float4 g = gradient[i];
    if (DROP) {
        const Words r = dropout_words(static_cast<uint64_t>(i), mask.stream_id, mask.step,
                                      mask.seed_lo, mask.seed_hi);
        g.x = r.x >= mask.threshold ? activation_gradient<ACT>(s.x, g.x * mask.scale) : 0.f;
        g.y = r.y >= mask.threshold ? activation_gradient<ACT>(s.y, g.y * mask.scale) : 0.f;
        g.z = r.z >= mask.threshold ? activation_gradient<ACT>(s.z, g.z * mask.scale) : 0.f;
        g.w = r.w >= mask.threshold ? activation_gradient<ACT>(s.w, g.w * mask.scale) : 0.f;
    } else {
        g.x = activation_gradient<ACT>(s.x, g.x);
        g.y = activation_gradient<ACT>(s.y, g.y);
        g.z = activation_gradient<ACT>(s.z, g.z);
        g.w = activation_gradient<ACT>(s.w, g.w);
    }
    gradient[i] = g;
}

template <int ACT>
void launch_activation_dropout(const float* z, float* y, int64_t quads, bool drop, Mask mask,
                               hipStream_t s) {
    const dim3 grid(static_cast<unsigned>((quads + 255) / 256));
    const float4* from = reinterpret_cast<const float4*>(z);
    float4* to = reinterpret_cast<float4*>(y);
    if (drop)
        EMPH_LAUNCH((activation_dropout_kernel<ACT, true>), grid, dim3(256), 0, s, from, to,
                    quads, mask);
    else
        EMPH_LAUNCH((activation_dropout_kernel<ACT, false>), grid, dim3(256), 0, s, from, to,
                    quads, mask);
}

template <int ACT>
void launch_activation_dropout_gradient(const float* source, float* gradient, int64_t quads,
                                        bool drop, Mask mask, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>((quads + 255) / 256));
    const float4* from = reinterpret_cast<const float4*>(source);
    float4* to = reinterpret_cast<float4*>(gradient);
    if (drop)
        EMPH_LAUNCH((activation_dropout_gradient_kernel<ACT, true>), grid, dim3(256), 0, s,
                    from, to, quads, mask);
    else
        EMPH_LAUNCH((activation_dropout_gradient_kernel<ACT, false>), grid, dim3(256), 0, s,
                    from, to, quads, mask);
}

inline Mask make_mask(float p, uint64_t seed, uint32_t stream_id, uint32_t step) {
    return Mask{stream_id, step, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32),
                dropout_threshold(p), dropout_scale(p)};
}

}  // namespace emph

using namespace emph;

extern "C" {

int emph_output_layer_backward_any(const float* dlogit, const float* x, int64_t ldx,
                                   const float* weight, const int32_t* word_segment,
                                   int32_t channels, int32_t kernel_size, int64_t columns,
                                   float* dweight, float* dbias, float* dx, int64_t ld_dx,
                                   void* stream) {
    const char* what = "emph_output_layer_backward_any";
    EMPH_REQUIRE(dlogit && x && weight && word_segment && dweight && dbias && dx,
                 EMPH_EINVAL, "emph_output_layer_backward_any: null pointer");
    EMPH_REQUIRE(kernel_size == 1 || kernel_size == 3 || kernel_size == 5 || kernel_size == 7,
                 EMPH_ERANGE, "emph_output_layer_backward_any: kernel_size %d (1, 3, 5 or 7)",
                 kernel_size);
    EMPH_REQUIRE(channels > 0 && channels <= 1024 && columns > 0 && columns <= ldx &&
                     columns <= ld_dx && columns < (int64_t{1} << 28),
                 EMPH_EINVAL, "emph_output_layer_backward_any: bad shape");
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (kernel_size) {
        case 1:
            return launch_output_backward<1>(dlogit, x, ldx, weight, word_segment, channels,
                                             columns, dweight, dbias, dx, ld_dx, s, what);
        case 3:
            return launch_output_backward<3>(dlogit, x, ldx, weight, word_segment, channels,
                                             columns, dweight, dbias, dx, ld_dx, s, what);
        case 5:
            return launch_output_backward<5>(dlogit, x, ldx, weight, word_segment, channels,
                                             columns, dweight, dbias, dx, ld_dx, s, what);
        default:
            return launch_output_backward<7>(dlogit, x, ldx, weight, word_segment, channels,
                                             columns, dweight, dbias, dx, ld_dx, s, what);
    }
}

int emph_activation_dropout(const float* z, float* y, int64_t count, int32_t activation,
                            float p, uint64_t seed, uint32_t stream_id, uint32_t step,
                            void* stream) {
    EMPH_REQUIRE(z && y, EMPH_EINVAL, "emph_activation_dropout: null pointer");
    EMPH_REQUIRE(activation >= EMPH_ACT_NONE && activation <= EMPH_ACT_LEAKY_RELU, EMPH_EINVAL,
                 "emph_activation_dropout: unknown activation %d", activation);
    EMPH_REQUIRE(p >= 0.f && p < 1.f, EMPH_EINVAL, "emph_activation_dropout: p %g (0 <= p < 1)",
                 static_cast<double>(p));
    EMPH_REQUIRE(count >= 0 && count % 4 == 0 && count < (int64_t{1} << 39) &&
                     (reinterpret_cast<uintptr_t>(z) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(y) & 15) == 0,
                 EMPH_EINVAL, "emph_activation_dropout: count and pointers in 16-byte units");
    if (count == 0) return EMPH_OK;
    const int64_t quads = count / 4;
    const bool drop = p > 0.f;
    const Mask mask = make_mask(p, seed, stream_id, step);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (activation) {
        case EMPH_ACT_NONE:
            launch_activation_dropout<EMPH_ACT_NONE>(z, y, quads, drop, mask, s);
            break;
        case EMPH_ACT_RELU:
            launch_activation_dropout<EMPH_ACT_RELU>(z, y, quads, drop, mask, s);
            break;
        case EMPH_ACT_GELU:
            launch_activation_dropout<EMPH_ACT_GELU>(z, y, quads, drop, mask, s);
            break;
        case EMPH_ACT_SILU:
            launch_activation_dropout<EMPH_ACT_SILU>(z, y, quads, drop, mask, s);
            break;
        default:
            launch_activation_dropout<EMPH_ACT_LEAKY_RELU>(z, y, quads, drop, mask, s);
            break;
    }
    return check_launch("emph_activation_dropout");
}

int emph_activation_dropout_gradient(const float* source, float* gradient, int64_t count,
                                     int32_t activation, float p, uint64_t seed,
                                     uint32_t stream_id, uint32_t step, void* stream) {
    EMPH_REQUIRE(source && gradient, EMPH_EINVAL,
                 "emph_activation_dropout_gradient: null pointer");
    EMPH_REQUIRE(activation >= EMPH_ACT_NONE && activation <= EMPH_ACT_LEAKY_RELU, EMPH_EINVAL,
                 "emph_activation_dropout_gradient: unknown activation %d", activation);
    EMPH_REQUIRE(p >= 0.f && p < 1.f, EMPH_EINVAL,
                 "emph_activation_dropout_gradient: p %g (0 <= p < 1)", static_cast<double>(p));
    EMPH_REQUIRE(count >= 0 && count % 4 == 0 && count < (int64_t{1} << 39) &&
                     (reinterpret_cast<uintptr_t>(source) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(gradient) & 15) == 0,
                 EMPH_EINVAL,
                 "emph_activation_dropout_gradient: count and pointers in 16-byte units");
    const bool drop = p > 0.f;
    // (the identity without dropout: nothing to do, as emph_activation_gradient)
    if (count == 0 || (activation == EMPH_ACT_NONE && !drop)) return EMPH_OK;
    const int64_t quads = count / 4;
    const Mask mask = make_mask(p, seed, stream_id, step);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (activation) {
        case EMPH_ACT_NONE:
            launch_activation_dropout_gradient<EMPH_ACT_NONE>(source, gradient, quads, drop,
                                                              mask, s);
            break;
        case EMPH_ACT_RELU:
            launch_activation_dropout_gradient<EMPH_ACT_RELU>(source, gradient, quads, drop,
                                                              mask, s);
            break;
        case EMPH_ACT_GELU:
            launch_activation_dropout_gradient<EMPH_ACT_GELU>(source, gradient, quads, drop,
                                                              mask, s);
            break;
        case EMPH_ACT_SILU:
            launch_activation_dropout_gradient<EMPH_ACT_SILU>(source, gradient, quads, drop,
                                                              mask, s);
            break;
        default:
            launch_activation_dropout_gradient<EMPH_ACT_LEAKY_RELU>(source, gradient, quads,
                                                                    drop, mask, s);
            break;
    }
    return check_launch("emph_activation_dropout_gradient");
}

}  // extern "C"
