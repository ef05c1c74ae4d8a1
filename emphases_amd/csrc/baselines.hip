// The pitch-variance baseline (emphases/baselines/pitch_variance/core.py:12-53)
// over a ragged batch: spread(x) = torch.quantile(x, .95) - torch.quantile(x, .05)
// of log2 pitch for every word and every whole utterance, then word spread -
// utterance spread.  The reference calls torch.quantile twice per word in a
// Python loop; here one workgroup selects the four order statistics of one
// segment (s[lo] and s[hi] for both quantiles), all segments of the batch in
// one launch, and a second launch writes the zero-centred scores.
//
// Selection is exact: floats become order-preserving uint32 keys and four
// rounds of 8-bit radix selection narrow each wanted rank down to one key.  The
// histograms are integer LDS counters, so the result does not depend on the
// order in which threads count; the segment streams from global memory in each
// round (L2 holds it after the first), so any length works.  The quantile
// arithmetic is ATen's (Sorting.cpp quantile + the CPU lerp kernel): rank
// r = q * (n - 1) in float32, lo = floor(r), hi = ceil(r), w = r - lo, result
// w < 0.5 ? fma(w, b - a, a) : fma(w - 1, b - a, b) - and a segment holding a
// NaN gives NaN (ATen sorts NaN last and moves both ranks onto it).
#include <math.h>

#include "common.h"

namespace emph {

namespace {

constexpr int kSpreadThreads = 256;
constexpr int kTargets = 4;        // s[lo .05], s[hi .05], s[lo .95], s[hi .95]

// -0 and +0 compare equal in torch's sort; both become the key of +0
__device__ __forceinline__ uint32_t order_key(float value) {
    uint32_t bits = __float_as_uint(value);
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__device__ __forceinline__ float key_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// at::native lerp as the CPU kernel computes it (fused multiply-add)
__device__ __forceinline__ float aten_lerp(float a, float b, float w) {
    const float d = b - a;
    return fabsf(w) < 0.5f ? __fmaf_rn(w, d, a) : __fmaf_rn(w - 1.f, d, b);
}

// the ranks ATen's quantile reads for q over n sorted values
__device__ __forceinline__ void quantile_ranks(float q, int64_t n, int64_t& lo, int64_t& hi,
                                               float& w) {
    const float r = __fmul_rn(q, static_cast<float>(n - 1));
    lo = static_cast<int64_t>(r);
    hi = static_cast<int64_t>(ceilf(r));
    w = r - static_cast<float>(lo);
}

__device__ __forceinline__ float load_value(const float* values, int64_t index, int transform) {
    const float value = values[index];
    return transform == EMPH_SPREAD_LOG2 ? log2f(value) : value;
}

// segments int64 [n][3] = (first column, columns, row of the segment to
// subtract or -1); stats float32 [n][3] = (q .05, q .95, spread)
__global__ __launch_bounds__(kSpreadThreads) void quantile_spread_kernel(
    const float* __restrict__ values, int64_t ld, const int64_t* __restrict__ segments,
    int transform, float* __restrict__ stats, float* __restrict__ selected) {
    __shared__ uint32_t histogram[kTargets][256];
    __shared__ uint32_t prefix[kTargets];
    __shared__ int64_t remaining[kTargets];
    __shared__ int owner[kTargets];
    __shared__ int any_nan;
    const int64_t row = blockIdx.x;
    const int64_t start = segments[row * 3 + 0];
    const int64_t count = segments[row * 3 + 1];
    const bool whole = segments[row * 3 + 2] < 0;
    float* out = stats + row * 3;
    // (the host refuses empty segments before the launch: this only keeps an
    // inconsistent table from reading outside `values`)
    if (start < 0 || count < 1 || start > ld - count) {
        if (threadIdx.x == 0) out[0] = out[1] = out[2] = __builtin_nanf("");
        return;
    }
    int64_t lo05, hi05, lo95, hi95;
    float w05, w95;
    quantile_ranks(0.05f, count, lo05, hi05, w05);
    quantile_ranks(0.95f, count, lo95, hi95, w95);
    if (threadIdx.x < kTargets) {
        const int t = threadIdx.x;
        prefix[t] = 0u;
        remaining[t] = t == 0 ? lo05 : t == 1 ? hi05 : t == 2 ? lo95 : hi95;
        owner[t] = 0;
    }
    if (threadIdx.x == 0) any_nan = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int round = 0; round < 4; ++round) {
        const int shift = 24 - 8 * round;
        const uint32_t high = round == 0 ? 0u : 0xffffffffu << (shift + 8);
        for (int i = threadIdx.x; i < kTargets * 256; i += kSpreadThreads)
            (&histogram[0][0])[i] = 0u;
        __syncthreads();
        uint32_t wanted[kTargets];
        bool counts[kTargets];
#pragma unroll
        for (int t = 0; t < kTargets; ++t) {
            wanted[t] = prefix[t];
            counts[t] = owner[t] == t;
        }
        bool nan_seen = false;
        for (int64_t i = threadIdx.x; i < count; i += kSpreadThreads) {
            const float value = load_value(values, start + i, transform);
            if (round == 0 && selected != nullptr && whole) selected[start + i] = value;
            if (value != value) {
                nan_seen = true;
                continue;
            }
            const uint32_t key = order_key(value);
            const uint32_t digit = (key >> shift) & 255u;
#pragma unroll
            for (int t = 0; t < kTargets; ++t)
                if (counts[t] && ((key ^ wanted[t]) & high) == 0u)
                    atomicAdd(&histogram[t][digit], 1u);
        }
        if (nan_seen) any_nan = 1;
        __syncthreads();
        if (any_nan) {
            if (threadIdx.x == 0) out[0] = out[1] = out[2] = __builtin_nanf("");
            return;
        }
        // wave t finds the digit of target t: lane l scans bins 4l .. 4l + 3
        {
            const int t = wave;
            const uint32_t* bins = histogram[owner[t]];
            const uint32_t c0 = bins[4 * lane], c1 = bins[4 * lane + 1];
            const uint32_t c2 = bins[4 * lane + 2], c3 = bins[4 * lane + 3];
            const uint32_t own = c0 + c1 + c2 + c3;
            uint32_t inclusive = own;
#pragma unroll
            for (int offset = 1; offset < 64; offset <<= 1) {
                const uint32_t other = __shfl_up(inclusive, offset);
                if (lane >= offset) inclusive += other;
            }
            const int64_t want = remaining[t];
            const int64_t below = static_cast<int64_t>(inclusive - own);
            const bool here = want >= below && want < static_cast<int64_t>(inclusive);
            __syncthreads();     // every wave has read prefix / remaining / owner
            if (here) {
                int64_t left = want - below;
                uint32_t digit = 4u * lane;
                const uint32_t c[4] = {c0, c1, c2, c3};
                for (int k = 0; k < 4; ++k) {
                    if (left < static_cast<int64_t>(c[k])) break;
                    left -= c[k];
                    ++digit;
                }
                prefix[t] |= digit << shift;
                remaining[t] = left;
            }
        }
        __syncthreads();
        // targets whose prefixes agree share one histogram in the next round
        if (threadIdx.x < kTargets) {
            int first = threadIdx.x;
            for (int u = 0; u < static_cast<int>(threadIdx.x); ++u)
                if (prefix[u] == prefix[threadIdx.x]) {
                    first = u;
                    break;
                }
            owner[threadIdx.x] = first;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float q05 = aten_lerp(key_value(prefix[0]), key_value(prefix[1]), w05);
        const float q95 = aten_lerp(key_value(prefix[2]), key_value(prefix[3]), w95);
        out[0] = q05;
        out[1] = q95;
        out[2] = q95 - q05;
    }
}

// out[i] = spread of row i - spread of the row it names (rows 0 .. n_rows)
__global__ __launch_bounds__(256) void spread_difference_kernel(
    const float* __restrict__ stats, const int64_t* __restrict__ segments, int64_t n_rows,
    int64_t n_segments, float* __restrict__ out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t base = segments[i * 3 + 2];
    out[i] = base >= 0 && base < n_segments ? stats[i * 3 + 2] - stats[base * 3 + 2]
                                             : __builtin_nanf("");
}

}  // namespace

}  // namespace emph

using namespace emph;

extern "C" {

int emph_quantile_spreads(const float* values, int64_t ld, const int64_t* segments,
                          int64_t n_segments, int32_t transform, float* stats, float* selected,
                          float* out, int64_t n_rows, void* stream) {
    if (n_segments == 0) return EMPH_OK;
    EMPH_REQUIRE(values && segments && stats, EMPH_EINVAL,
                 "emph_quantile_spreads: null pointer");
    EMPH_REQUIRE(transform == EMPH_SPREAD_IDENTITY || transform == EMPH_SPREAD_LOG2,
                 EMPH_EINVAL, "emph_quantile_spreads: unknown transform %d", transform);
    EMPH_REQUIRE(n_segments > 0 && n_segments < (int64_t{1} << 31) && ld >= 0, EMPH_ERANGE,
                 "emph_quantile_spreads: %lld segments", static_cast<long long>(n_segments));
    EMPH_REQUIRE(n_rows >= 0 && n_rows <= n_segments && (n_rows == 0 || out), EMPH_EINVAL,
                 "emph_quantile_spreads: %lld output rows of %lld segments",
                 static_cast<long long>(n_rows), static_cast<long long>(n_segments));
    const hipStream_t hip_stream = static_cast<hipStream_t>(stream);
    EMPH_LAUNCH(quantile_spread_kernel, dim3(static_cast<unsigned>(n_segments)),
                dim3(kSpreadThreads), 0, hip_stream, values, ld, segments, transform, stats,
                selected);
    int status = check_launch("emph_quantile_spreads");
    if (status != EMPH_OK || n_rows == 0) return status;
    EMPH_LAUNCH(spread_difference_kernel, dim3(static_cast<unsigned>((n_rows + 255) / 256)),
                dim3(256), 0, hip_stream, stats, segments, n_rows, n_segments, out);
    return check_launch("emph_quantile_spreads");
}

}  // extern "C"
