// The frame-rate end of the decoder-less models (DOWNSAMPLE_LOCATION
// 'inference' in train mode, emphases/model/core.py:117-122): emphases.upsample
// (emphases/core.py:472-544), output_layer on the frame axis with its backward,
// and the frame-rate loss against word targets interpolated on the fly
// (emphases/train/core.py:324-353).
//
// The word-rate kernels of csrc/train.hip are one workgroup over "a few
// thousand" columns (loss_grad_kernel) or 81 workgroups that each walk every
// column (output_backward_weight_kernel); the frame axis of a training batch
// is 75 000 columns, so everything here is a workgroup per 64-frame tile (or
// per fixed run of tiles) of the frame tile table.
//
// Deterministic: no atomics, every sum in an order fixed by the tile table
// alone.  A tap outside its own utterance contributes zero by a select on the
// value and reads an address inside the utterance: the columns between the
// utterances may hold anything, NaN included.
#include <math.h>

#include "common.h"
#include "upsample.h"

namespace emph {

constexpr int kHeadChannels = 80;                  // frame_head_backward_kernel
constexpr int kHeadPerWave = kHeadChannels / 4;    // channels of a wave
constexpr int kHeadMaxParts = 1024;

// Sum over the 64 lanes of a wave in a fixed order (xor butterfly); every lane
// holds it.
template <typename T>
__device__ __forceinline__ T wave_sum(T value) {
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) value += __shfl_xor(value, offset);
    return value;
}

// One workgroup per 64-frame tile: a lane per frame, the four waves stride
// the channels.
__global__ __launch_bounds__(256) void upsample_kernel(
    const float* __restrict__ x, int64_t ldw, const int32_t* __restrict__ bounds,
    float* __restrict__ out, int64_t ldx, int channels, const int64_t* __restrict__ seg,
    const int32_t* __restrict__ tiles, int method) {
    const Tile tile = load_tile(tiles, blockIdx.x);
    const int t = tile.first + (threadIdx.x & 63);
    if (t >= tile.count) return;
    const Span words = load_span(seg, tile.segment, EMPH_AXIS_WORDS);
    if (words.count < 1) return;
    const float frame_time = static_cast<float>(t) + 0.5f;
    const int index = upsample_index(bounds, ldw, words.offset, words.count, frame_time);
    float* target = out + tile.offset + t;
    for (int c = threadIdx.x >> 6; c < channels; c += 4)
        target[static_cast<int64_t>(c) * ldx] =
            upsample_value(x + static_cast<int64_t>(c) * ldw + words.offset, bounds, ldw,
                           words.offset, words.count, index, frame_time, method);
}

// One workgroup per 64-frame tile: a lane per frame, wave w sums channels w,
// w + 4, ... (taps 0, 1, 2 of a channel in that order); the four partial sums
// meet in LDS and are added in wave order, then the bias.
__global__ __launch_bounds__(256) void frame_head_kernel(
    const float* __restrict__ h, int64_t ldh, const float* __restrict__ weight,
    const float* __restrict__ bias, int channels, const int32_t* __restrict__ tiles,
    float* __restrict__ logits) {
    extern __shared__ float shared[];
    float* w = shared;                       // [channels][3]
    float* partial = shared + channels * 3;  // [4][64]
    for (int index = threadIdx.x; index < channels * 3; index += 256) w[index] = weight[index];
    __syncthreads();
    const Tile tile = load_tile(tiles, blockIdx.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = tile.first + lane;
    const bool live = t < tile.count;
    const bool has_left = live && t > 0, has_right = live && t + 1 < tile.count;
    // (a dead lane reads the tile's first frame, a missing tap the centre)
    const int64_t column = static_cast<int64_t>(tile.offset) + (live ? t : tile.first);
    const int left_at = has_left ? -1 : 0, right_at = has_right ? 1 : 0;
    const float* base = h + column;
    float acc = 0.f;
#pragma unroll 5
    for (int c = wave; c < channels; c += 4) {
        const float* row = base + static_cast<int64_t>(c) * ldh;
        const float left = row[left_at], centre = row[0], right = row[right_at];
        acc = fmaf(w[c * 3 + 0], has_left ? left : 0.f, acc);
        acc = fmaf(w[c * 3 + 1], centre, acc);
        acc = fmaf(w[c * 3 + 2], has_right ? right : 0.f, acc);
    }
    partial[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave != 0 || !live) return;
    float sum = partial[lane];
#pragma unroll
    for (int other = 1; other < 4; ++other) sum += partial[other * 64 + lane];
    logits[column] = sum + bias[0];
}

// One wave per 64-frame tile: a lane per frame.  The target of the frame is
// interpolated from the packed word targets (upsample.h), clamped to [0, 1]
// under 'linear' (train/core.py:335-336).  Each term of the loss is formed in
// double, as loss_grad_kernel's; the tile's sum goes to partials[tile].  The
// gradient is in float with a float 1 / N, as autograd's.
__global__ __launch_bounds__(64) void frame_loss_grad_kernel(
    const float* __restrict__ logits, const float* __restrict__ targets,
    const int32_t* __restrict__ bounds, int64_t ldw, const int64_t* __restrict__ seg,
    const int32_t* __restrict__ tiles, int64_t valid_frames, int form, int method,
    double* __restrict__ partials, float* __restrict__ dlogit) {
    const float inverse_count = static_cast<float>(1.0 / static_cast<double>(valid_frames));
    const Tile tile = load_tile(tiles, blockIdx.x);
    const int t = tile.first + threadIdx.x;
    const Span words = load_span(seg, tile.segment, EMPH_AXIS_WORDS);
    double term = 0.;
    if (t < tile.count && words.count >= 1) {
        const int64_t column = static_cast<int64_t>(tile.offset) + t;
        const float frame_time = static_cast<float>(t) + 0.5f;
        const int index = upsample_index(bounds, ldw, words.offset, words.count, frame_time);
        float y = upsample_value(targets + words.offset, bounds, ldw, words.offset,
                                 words.count, index, frame_time, method);
        if (method == EMPH_UPSAMPLE_LINEAR) y = fminf(fmaxf(y, 0.f), 1.f);
        const float z = logits[column];
        float gradient;
        if (form == 0) {
            // binary_cross_entropy_with_logits, the stable form of ATen
            const double wide = z;
            term = fmax(wide, 0.) - wide * y + log1p(exp(-fabs(wide)));
            gradient = (1.f / (1.f + expf(-z)) - y) * inverse_count;
        } else {
            const double wide = static_cast<double>(z) - y;
            term = wide * wide;
            gradient = 2.f * (z - y) * inverse_count;
        }
        dlogit[column] = gradient;
    }
    const double total = wave_sum(term);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// One workgroup: thread i adds partials i, i + 256, ... in that order, then a
// binary tree over the thread indices; the mean is rounded to float once.
__global__ __launch_bounds__(256) void frame_loss_sum_kernel(
    const double* __restrict__ partials, int count, int64_t valid_frames,
    float* __restrict__ loss) {
    __shared__ double shared[256];
    double sum = 0.;
    for (int index = threadIdx.x; index < count; index += 256) sum += partials[index];
    shared[threadIdx.x] = sum;
    __syncthreads();
#pragma unroll
    for (int width = 128; width > 0; width >>= 1) {
        if (static_cast<int>(threadIdx.x) < width)
            shared[threadIdx.x] += shared[threadIdx.x + width];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        loss[0] = static_cast<float>(shared[0] / static_cast<double>(valid_frames));
}

// Workgroup `part` owns tiles [part * per, (part + 1) * per): a lane per frame
// u, wave w owns channels w, w + 4, ...  With g_j = dlogit[u - j + 1] (zero
// outside the utterance) one load of h[c][u] serves
//   dW[c][j] += g_j h[c][u]     (= sum_t dlogit[t] h[c][t + j - 1], t = u - j + 1)
//   dx[c][u]  = sum_j W[c][j] g_j
// so h is read once and dx written once.  The per-lane sums are folded over
// the wave by a fixed butterfly and go to slab `part`: [channels][3] and the
// bias gradient (wave 0) behind them.
__global__ __launch_bounds__(256) void frame_head_backward_kernel(
    const float* __restrict__ dlogit, const float* __restrict__ h, int64_t ldh,
    const float* __restrict__ weight, int channels, const int32_t* __restrict__ tiles,
    int n_tiles, int per, float* __restrict__ dx, int64_t ld_dx, float* __restrict__ slabs) {
    __shared__ float w[kHeadChannels * 3];
    for (int index = threadIdx.x; index < channels * 3; index += 256) w[index] = weight[index];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc[kHeadPerWave][3];
#pragma unroll
    for (int k = 0; k < kHeadPerWave; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.f;
    float bias_sum = 0.f;
    const int begin = blockIdx.x * per, end = min(n_tiles, begin + per);
    for (int index = begin; index < end; ++index) {
        const Tile tile = load_tile(tiles, index);
        const int u = tile.first + lane;
        const bool live = u < tile.count;
        const bool has_left = live && u > 0, has_right = live && u + 1 < tile.count;
        const int64_t column = static_cast<int64_t>(tile.offset) + (live ? u : tile.first);
        const float at_right = dlogit[column + (has_right ? 1 : 0)];
        const float at_centre = dlogit[column];
        const float at_left = dlogit[column - (has_left ? 1 : 0)];
        const float g0 = has_right ? at_right : 0.f;
        const float g1 = live ? at_centre : 0.f;
        const float g2 = has_left ? at_left : 0.f;
        bias_sum += g1;
        // every load of the tile in flight at once (clamped address, selected
        // value), then the sums, then the stores: a load behind a
        // conditional store waits for it, a round trip per channel
        float value[kHeadPerWave];
#pragma unroll
        for (int k = 0; k < kHeadPerWave; ++k) {
            const int c = min(wave + 4 * k, channels - 1);
            value[k] = h[static_cast<int64_t>(c) * ldh + column];
        }
#pragma unroll
        for (int k = 0; k < kHeadPerWave; ++k) {
            const float v = (live && wave + 4 * k < channels) ? value[k] : 0.f;
            acc[k][0] = fmaf(g0, v, acc[k][0]);
            acc[k][1] = fmaf(g1, v, acc[k][1]);
            acc[k][2] = fmaf(g2, v, acc[k][2]);
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < kHeadPerWave; ++k) {
                const int c = wave + 4 * k;
                if (c < channels)
                    dx[static_cast<int64_t>(c) * ld_dx + column] =
                        fmaf(w[c * 3 + 2], g2, fmaf(w[c * 3 + 1], g1, w[c * 3 + 0] * g0));
            }
        }
    }
    // the butterfly of wave_sum, step by step over all the sums at once: the
    // exchanges of a step are independent and overlap
    float* slab = slabs + static_cast<int64_t>(blockIdx.x) * (channels * 3 + 1);
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) {
        float other[kHeadPerWave][3];
#pragma unroll
        for (int k = 0; k < kHeadPerWave; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) other[k][j] = __shfl_xor(acc[k][j], offset);
#pragma unroll
        for (int k = 0; k < kHeadPerWave; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[k][j] += other[k][j];
    }
#pragma unroll
    for (int k = 0; k < kHeadPerWave; ++k) {
        const int c = wave + 4 * k;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (lane == 0 && c < channels) slab[c * 3 + j] = acc[k][j];
    }
    const float total = wave_sum(bias_sum);
    if (threadIdx.x == 0) slab[channels * 3] = total;
}

// One wave per element of the slab: lane i adds parts i, i + 64, ... in that
// order, then the butterfly.
__global__ __launch_bounds__(64) void frame_head_reduce_kernel(
    const float* __restrict__ slabs, int parts, int stride, float* __restrict__ dweight,
    float* __restrict__ dbias) {
    const int element = blockIdx.x;
    float sum = 0.f;
    for (int part = threadIdx.x; part < parts; part += 64)
        sum += slabs[static_cast<int64_t>(part) * stride + element];
    sum = wave_sum(sum);
    if (threadIdx.x != 0) return;
    if (element == stride - 1) dbias[0] = sum; else dweight[element] = sum;
}

static int tiles_per_part(int n_tiles) { return (n_tiles + kHeadMaxParts - 1) / kHeadMaxParts; }

}  // namespace emph

using namespace emph;

extern "C" {

int emph_upsample(const float* x, int64_t ldw, const int32_t* bounds, float* out,
                  int64_t ldx, int32_t channels, const int64_t* seg, const int32_t* tiles,
                  int32_t n_tiles, int32_t method, void* stream) {
    if (n_tiles == 0) return EMPH_OK;
    EMPH_REQUIRE(x && bounds && out && seg && tiles, EMPH_EINVAL, "emph_upsample: null pointer");
    EMPH_REQUIRE(method == EMPH_UPSAMPLE_LINEAR || method == EMPH_UPSAMPLE_NEAREST, EMPH_EINVAL,
                 "emph_upsample: method %d (0 = linear, 1 = nearest)", method);
    EMPH_REQUIRE(channels > 0 && n_tiles > 0 && ldw > 0 && ldx > 0, EMPH_EINVAL,
                 "emph_upsample: bad shape");
    EMPH_LAUNCH(upsample_kernel, dim3(n_tiles), dim3(256), 0, static_cast<hipStream_t>(stream),
                x, ldw, bounds, out, ldx, channels, seg, tiles, method);
    return check_launch("emph_upsample");
}

int emph_frame_head(const float* h, int64_t ldh, const float* weight, const float* bias,
                    int32_t channels, int32_t kernel_size, const int32_t* tiles,
                    int32_t n_tiles, float* logits, void* stream) {
    if (n_tiles == 0) return EMPH_OK;
    EMPH_REQUIRE(h && weight && bias && tiles && logits, EMPH_EINVAL,
                 "emph_frame_head: null pointer");
    EMPH_REQUIRE(kernel_size == 3, EMPH_ERANGE, "emph_frame_head: kernel_size %d (3)",
                 kernel_size);
    EMPH_REQUIRE(channels > 0 && channels <= 1024, EMPH_ERANGE,
                 "emph_frame_head: channels %d (1..1024)", channels);
    EMPH_REQUIRE(n_tiles > 0 && ldh > 0, EMPH_EINVAL, "emph_frame_head: bad shape");
    EMPH_LAUNCH(frame_head_kernel, dim3(n_tiles), dim3(256),
                (channels * 3 + 256) * sizeof(float), static_cast<hipStream_t>(stream), h, ldh,
                weight, bias, channels, tiles, logits);
    return check_launch("emph_frame_head");
}

int emph_frame_loss_grad(const float* logits, const float* targets, const int32_t* bounds,
                         int64_t ldw, const int64_t* seg, const int32_t* tiles,
                         int32_t n_tiles, int64_t valid_frames, int32_t form, int32_t method,
                         double* workspace, float* loss, float* dlogit, void* stream) {
    EMPH_REQUIRE(logits && targets && bounds && seg && tiles && workspace && loss && dlogit,
                 EMPH_EINVAL, "emph_frame_loss_grad: null pointer");
    EMPH_REQUIRE(form == 0 || form == 1, EMPH_EINVAL,
                 "emph_frame_loss_grad: form %d (0 = bce, 1 = mse)", form);
    EMPH_REQUIRE(method == EMPH_UPSAMPLE_LINEAR || method == EMPH_UPSAMPLE_NEAREST, EMPH_EINVAL,
                 "emph_frame_loss_grad: method %d (0 = linear, 1 = nearest)", method);
    EMPH_REQUIRE(n_tiles > 0 && ldw > 0 && valid_frames > 0 &&
                     valid_frames <= static_cast<int64_t>(n_tiles) * 64,
                 EMPH_EINVAL, "emph_frame_loss_grad: bad shape");
    hipStream_t s = static_cast<hipStream_t>(stream);
    EMPH_LAUNCH(frame_loss_grad_kernel, dim3(n_tiles), dim3(64), 0, s, logits, targets, bounds,
                ldw, seg, tiles, valid_frames, form, method, workspace, dlogit);
    if (int status = check_launch("emph_frame_loss_grad")) return status;
    EMPH_LAUNCH(frame_loss_sum_kernel, dim3(1), dim3(256), 0, s, workspace, n_tiles,
                valid_frames, loss);
    return check_launch("emph_frame_loss_grad");
}

int32_t emph_frame_head_parts(int32_t n_tiles) {
    if (n_tiles <= 0) return 0;
    const int per = tiles_per_part(n_tiles);
    return (n_tiles + per - 1) / per;
}

int emph_frame_head_backward(const float* dlogit, const float* h, int64_t ldh,
                             const float* weight, int32_t channels, int32_t kernel_size,
                             const int32_t* tiles, int32_t n_tiles, float* workspace,
                             float* dweight, float* dbias, float* dx, int64_t ld_dx,
                             void* stream) {
    EMPH_REQUIRE(dlogit && h && weight && tiles && workspace && dweight && dbias && dx,
                 EMPH_EINVAL, "emph_frame_head_backward: null pointer");
    EMPH_REQUIRE(kernel_size == 3, EMPH_ERANGE, "emph_frame_head_backward: kernel_size %d (3)",
                 kernel_size);
    EMPH_REQUIRE(channels > 0 && channels <= kHeadChannels, EMPH_ERANGE,
                 "emph_frame_head_backward: channels %d (1..%d)", channels, kHeadChannels);
    EMPH_REQUIRE(n_tiles > 0 && ldh > 0 && ld_dx > 0, EMPH_EINVAL,
                 "emph_frame_head_backward: bad shape");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int per = tiles_per_part(n_tiles);
    const int parts = emph_frame_head_parts(n_tiles);
    EMPH_LAUNCH(frame_head_backward_kernel, dim3(parts), dim3(256), 0, s, dlogit, h, ldh, weight,
                channels, tiles, n_tiles, per, dx, ld_dx, workspace);
    if (int status = check_launch("emph_frame_head_backward")) return status;
    const int stride = channels * 3 + 1;
    EMPH_LAUNCH(frame_head_reduce_kernel, dim3(stride), dim3(64), 0, s, workspace, parts, stride,
                dweight, dbias);
    return check_launch("emph_frame_head_backward");
}

}  // extern "C"
