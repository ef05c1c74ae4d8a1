// Backward of the Transformer encoder pieces of transformer.hip
// (emphases/model/layers/transformer.py:13-52 under autograd): the attention
// core and the post-LN residual.  The linear layers are kernel_size-1
// convolutions, whose gradients conv.hip and conv_grad_any.hip already have.
//
// Attention backward (fp32 MFMA, scores recomputed, never materialised; torch's
// math backend keeps a 2 x T x T fp32 matrix per utterance and layer).  With
// P = softmax(S), S = Q K^T / sqrt(d), O = P V and D_i = sum_c dO_ic O_ic:
//     dV = P^T dO        dP = dO V^T        dS = P o (dP - D)
//     dQ = dS K / sqrt(d)                   dK = dS^T Q / sqrt(d)
// Two launches over the 64-wide tile table, neither with atomics:
//   1. per QUERY tile: the row log-sum-exp (online, statistics only) and D into
//      the workspace, then a second loop over the keys for dQ.  As in the
//      forward, the query is the MFMA column: S^T = K Q^T and dP^T = V dO^T
//      land in the D layout (row = 4 (lane >> 4) + r), which IS the B-operand
//      layout of dQ^T = K^T dS^T with k-step r taking keys {4 g + r}.
//   2. per KEY tile: the key is the MFMA column: S = Q K^T and dP = dO V^T with
//      the tile's K^T and V^T held in registers as B operands; P and dS feed
//      dV^T = dO^T P and dK^T = Q^T dS as B operands where they stand.
// Every output element is written by one lane, its sum taken in key (query)
// order: the same inputs give the same bits.
#include <math.h>

#include "common.h"

namespace emph {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float grad_rows_max(float x) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false,
                                              false);
    x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false,
                                              false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float grad_rows_sum(float x) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false,
                                              false);
    x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false,
                                              false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

constexpr float kLog2e = 1.44269504088896340736f;
constexpr int kGradTile = 64;      // positions per tile of both passes
constexpr int kGradWaves = 2;      // waves per tile: 32 positions each

// grid = (n_tiles, heads); block = 128: wave w owns queries [32 w, 32 w + 32)
// of the tile.  `stats` = [2][heads][ld]: the row log-sum-exp in log2 units,
// then D.
template <int D>
__global__ __launch_bounds__(64 * kGradWaves) void attention_backward_query_kernel(
    const float* __restrict__ qk, const float* __restrict__ v, const float* __restrict__ out,
    const float* __restrict__ dout, float* __restrict__ dqkv, float* __restrict__ stats,
    int64_t ld, int channels, int heads, const int32_t* __restrict__ tiles) {
    constexpr int QT = kGradTile / kGradWaves / 16;
    constexpr int KSTEPS = D / 4;
    constexpr int MT = (D + 15) / 16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15;
    const int kk = lane >> 4;
    const int head = blockIdx.y;
    const Tile span = load_tile(tiles, blockIdx.x);
    const int q0 = span.first + 16 * QT * wave;
    const int count = span.count;
    if (q0 >= count) return;                       // wave-uniform; no barrier below
    const float scale = 1.f / sqrtf(static_cast<float>(D));
    const float scale2 = kLog2e * scale;

    const int64_t head_row = static_cast<int64_t>(head * D) * ld + span.offset;
    const float* q_rows = qk + head_row;
    const float* k_rows = qk + static_cast<int64_t>(channels) * ld + head_row;
    const float* v_rows = v + static_cast<int64_t>(span.offset) * channels + head * D;
    const float* o_rows = out + head_row;
    const float* do_rows = dout + head_row;

    // B operands of the query tile: Q^T (scaled into log2 units) and dO^T, and
    // D_i from the same loads
    float bq[QT][KSTEPS], bdo[QT][KSTEPS], delta[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int query = q0 + 16 * t + col;
        const bool live = query < count;
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const int64_t at = static_cast<int64_t>(4 * s + kk) * ld + query;
            bq[t][s] = live ? q_rows[at] * scale2 : 0.f;
            bdo[t][s] = live ? do_rows[at] : 0.f;
            sum = fmaf(bdo[t][s], live ? o_rows[at] : 0.f, sum);
        }
        delta[t] = grad_rows_sum(sum);
    }

    // ---- pass 1: log-sum-exp of every row (per-lane online maximum and sum
    // over the lane's keys, combined over the four key rows at the end)
    float top[QT], total[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        top[t] = -INFINITY;
        total[t] = 0.f;
    }
    for (int key0 = 0; key0 < count; key0 += 16) {
        float ak[KSTEPS];
        const int key = min(key0 + col, count - 1);
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
            ak[s] = k_rows[static_cast<int64_t>(4 * s + kk) * ld + key];
        f32x4 s4[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) s4[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
            for (int t = 0; t < QT; ++t)
                s4[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ak[s], bq[t][s], s4[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (key0 + 4 * kk + r >= count) s4[t][r] = -INFINITY;
            const float high =
                fmaxf(fmaxf(fmaxf(s4[t][0], s4[t][1]), fmaxf(s4[t][2], s4[t][3])), top[t]);
            if (high > -INFINITY) {                // (a lane whose keys are all masked so far)
                float sum = total[t] * __builtin_amdgcn_exp2f(top[t] - high);
#pragma unroll
                for (int r = 0; r < 4; ++r) sum += __builtin_amdgcn_exp2f(s4[t][r] - high);
                total[t] = sum;
                top[t] = high;
            }
        }
    }
    float lse[QT];
    float* lse_row = stats + static_cast<int64_t>(head) * ld + span.offset;
    float* delta_row = stats + static_cast<int64_t>(heads + head) * ld + span.offset;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const float high = grad_rows_max(top[t]);          // finite: key 0 exists
        const float mine =
            top[t] == -INFINITY ? 0.f : total[t] * __builtin_amdgcn_exp2f(top[t] - high);
        lse[t] = high + log2f(grad_rows_sum(mine));
        const int query = q0 + 16 * t + col;
        if (kk == 0 && query < count) {
            lse_row[query] = lse[t];
            delta_row[query] = delta[t];
        }
    }

    // ---- pass 2: dQ^T[d][query] = sum_key K^T[d][key] dS^T[key][query]
    f32x4 dq[QT][MT];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m) dq[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int key0 = 0; key0 < count; key0 += 16) {
        float ak[KSTEPS], av[KSTEPS], akt[4][MT];
        const int key = min(key0 + col, count - 1);
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            ak[s] = k_rows[static_cast<int64_t>(4 * s + kk) * ld + key];
            av[s] = v_rows[static_cast<int64_t>(key) * channels + 4 * s + kk];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tkey = min(key0 + 4 * kk + r, count - 1);
#pragma unroll
            for (int m = 0; m < MT; ++m)
                akt[r][m] = k_rows[static_cast<int64_t>(min(16 * m + col, D - 1)) * ld + tkey];
        }
        f32x4 s4[QT], dp4[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            s4[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp4[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                s4[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ak[s], bq[t][s], s4[t], 0, 0, 0);
                dp4[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bdo[t][s], dp4[t], 0, 0, 0);
            }
        // a key past the segment: probability 0 (selected; the clamped loads
        // above only feed such rows)
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = key0 + 4 * kk + r < count
                                    ? __builtin_amdgcn_exp2f(s4[t][r] - lse[t])
                                    : 0.f;
                s4[t][r] = p * (dp4[t][r] - delta[t]);
            }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    dq[t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(akt[r][m], s4[t][r],
                                                                    dq[t][m], 0, 0, 0);
    }
    float* dq_rows = dqkv + head_row;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int query = q0 + 16 * t + col;
        if (query >= count) continue;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 16 * m + 4 * kk + r;
                if (d < D) dq_rows[static_cast<int64_t>(d) * ld + query] = dq[t][m][r] * scale;
            }
    }
}

// grid = (n_tiles, heads); block = 128: wave w owns keys [32 w, 32 w + 32) of
// the tile and walks the segment's queries 16 at a time.
template <int D>
__global__ __launch_bounds__(64 * kGradWaves) void attention_backward_key_kernel(
    const float* __restrict__ qk, const float* __restrict__ v, const float* __restrict__ dout,
    float* __restrict__ dqkv, const float* __restrict__ stats, int64_t ld, int channels,
    int heads, const int32_t* __restrict__ tiles) {
    constexpr int KT = kGradTile / kGradWaves / 16;
    constexpr int KSTEPS = D / 4;
    constexpr int MT = (D + 15) / 16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 15;
    const int kk = lane >> 4;
    const int head = blockIdx.y;
    const Tile span = load_tile(tiles, blockIdx.x);
    const int k0 = span.first + 16 * KT * wave;
    const int count = span.count;
    if (k0 >= count) return;                       // wave-uniform; no barrier below
    const float scale = 1.f / sqrtf(static_cast<float>(D));
    const float scale2 = kLog2e * scale;

    const int64_t head_row = static_cast<int64_t>(head * D) * ld + span.offset;
    const float* q_rows = qk + head_row;
    const float* k_rows = qk + static_cast<int64_t>(channels) * ld + head_row;
    const float* v_rows = v + static_cast<int64_t>(span.offset) * channels + head * D;
    const float* do_rows = dout + head_row;
    const float* lse_row = stats + static_cast<int64_t>(head) * ld + span.offset;
    const float* delta_row = stats + static_cast<int64_t>(heads + head) * ld + span.offset;

    // B operands of the key tile: K^T (scaled into log2 units) and V^T.  A key
    // past the segment is a clamped copy: its column is never stored.
    float bk[KT][KSTEPS], bv[KT][KSTEPS];
#pragma unroll
    for (int u = 0; u < KT; ++u) {
        const int key = min(k0 + 16 * u + col, count - 1);
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            bk[u][s] = k_rows[static_cast<int64_t>(4 * s + kk) * ld + key] * scale2;
            bv[u][s] = v_rows[static_cast<int64_t>(key) * channels + 4 * s + kk];
        }
    }
    f32x4 dk[KT][MT], dv[KT][MT];
#pragma unroll
    for (int u = 0; u < KT; ++u)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            dk[u][m] = f32x4{0.f, 0.f, 0.f, 0.f};
            dv[u][m] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    for (int q0 = 0; q0 < count; q0 += 16) {
        float aq[KSTEPS], ado[KSTEPS], aqt[4][MT], adot[4][MT], lse[4], delta[4];
        const int query = min(q0 + col, count - 1);
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const int64_t at = static_cast<int64_t>(4 * s + kk) * ld + query;
            aq[s] = q_rows[at];
            ado[s] = do_rows[at];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tquery = min(q0 + 4 * kk + r, count - 1);
            lse[r] = lse_row[tquery];
            delta[r] = delta_row[tquery];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int64_t at = static_cast<int64_t>(min(16 * m + col, D - 1)) * ld + tquery;
                aqt[r][m] = q_rows[at];
                adot[r][m] = do_rows[at];
            }
        }
#pragma unroll
        for (int u = 0; u < KT; ++u) {
            f32x4 s4 = f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 dp4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) {
                s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[s], bk[u][s], s4, 0, 0, 0);
                dp4 = __builtin_amdgcn_mfma_f32_16x16x4f32(ado[s], bv[u][s], dp4, 0, 0, 0);
            }
            // s4[r] = score(query q0 + 4 kk + r, key col); a query past the
            // segment contributes nothing (selected)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = q0 + 4 * kk + r < count
                                    ? __builtin_amdgcn_exp2f(s4[r] - lse[r])
                                    : 0.f;
                s4[r] = p;
                dp4[r] = p * (dp4[r] - delta[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    dv[u][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(adot[r][m], s4[r],
                                                                    dv[u][m], 0, 0, 0);
                    dk[u][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(aqt[r][m], dp4[r],
                                                                    dk[u][m], 0, 0, 0);
                }
        }
    }
    float* dk_rows = dqkv + static_cast<int64_t>(channels) * ld + head_row;
    float* dv_rows = dqkv + static_cast<int64_t>(2 * channels) * ld + head_row;
#pragma unroll
    for (int u = 0; u < KT; ++u) {
        const int key = k0 + 16 * u + col;
        if (key >= count) continue;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 16 * m + 4 * kk + r;
                if (d < D) {
                    dk_rows[static_cast<int64_t>(d) * ld + key] = dk[u][m][r] * scale;
                    dv_rows[static_cast<int64_t>(d) * ld + key] = dv[u][m][r];
                }
            }
    }
}

// Backward of y = LayerNorm(s) * gamma + beta over channels, s = x + r:
//     xhat = (s - mean) rstd      g = dy gamma
//     ds = rstd (g - mean_c(g) - xhat mean_c(g xhat))
//     dgamma[c] = sum_t dy xhat   dbeta[c] = sum_t dy
// The thread layout of add_layernorm_kernel (64 columns x 4 channel slices,
// statistics recomputed as the forward computes them).  Workgroup p walks the
// fixed run of tiles [p run, (p + 1) run), keeps the channel sums of its
// columns per lane, reduces them over the wave's 64 columns by a butterfly and
// writes slab p = [2][channels]; layernorm_backward_sum_kernel adds the slabs.
template <int CMAX>
__global__ __launch_bounds__(256) void add_layernorm_backward_kernel(
    const float* __restrict__ s, const float* __restrict__ gamma, const float* __restrict__ dy,
    float* __restrict__ ds, int64_t ld, int channels, float eps,
    const int32_t* __restrict__ tiles, int n_tiles, int run, float* __restrict__ slabs) {
    constexpr int PER = (CMAX + 3) / 4;
    __shared__ float partial[4][4][64];
    const int lane = threadIdx.x & 63;
    const int slice = threadIdx.x >> 6;
    const float width = static_cast<float>(channels);
    float scale[PER], sum_gamma[PER], sum_beta[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int c = 4 * j + slice;
        scale[j] = c < channels ? gamma[c] : 0.f;
        sum_gamma[j] = 0.f;
        sum_beta[j] = 0.f;
    }
    const int first_tile = blockIdx.x * run;
    const int last_tile = min(first_tile + run, n_tiles);
    for (int tile = first_tile; tile < last_tile; ++tile) {
        const Tile span = load_tile(tiles, tile);
        const int position = span.first + lane;
        const bool live = position < span.count;
        const int64_t column = span.offset + (live ? position : span.count - 1);
        float value[PER], gradient[PER];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int c = 4 * j + slice;
            value[j] = 0.f;
            gradient[j] = 0.f;
            if (c < channels) {
                value[j] = s[static_cast<int64_t>(c) * ld + column];
                gradient[j] = live ? dy[static_cast<int64_t>(c) * ld + column] : 0.f;
                sum += value[j];
            }
        }
        partial[0][slice][lane] = sum;
        __syncthreads();
        const float mean = (partial[0][0][lane] + partial[0][1][lane] + partial[0][2][lane] +
                            partial[0][3][lane]) / width;
        float square = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if (4 * j + slice < channels)
                square = fmaf(value[j] - mean, value[j] - mean, square);
        partial[1][slice][lane] = square;
        __syncthreads();
        const float variance = (partial[1][0][lane] + partial[1][1][lane] +
                                partial[1][2][lane] + partial[1][3][lane]) / width;
        const float rstd = 1.f / sqrtf(variance + eps);
        float sum_g = 0.f, sum_gx = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            value[j] = (value[j] - mean) * rstd;              // xhat (0 beyond channels: unused)
            sum_gamma[j] = fmaf(gradient[j], value[j], sum_gamma[j]);
            sum_beta[j] += gradient[j];
            gradient[j] *= scale[j];                          // g
            sum_g += gradient[j];
            sum_gx = fmaf(gradient[j], value[j], sum_gx);
        }
        partial[2][slice][lane] = sum_g;
        partial[3][slice][lane] = sum_gx;
        __syncthreads();
        const float mean_g = (partial[2][0][lane] + partial[2][1][lane] + partial[2][2][lane] +
                              partial[2][3][lane]) / width;
        const float mean_gx = (partial[3][0][lane] + partial[3][1][lane] +
                               partial[3][2][lane] + partial[3][3][lane]) / width;
        if (live) {
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int c = 4 * j + slice;
                if (c < channels)
                    ds[static_cast<int64_t>(c) * ld + column] =
                        rstd * (gradient[j] - mean_g - value[j] * mean_gx);
            }
        }
        // (partial[0] is next written behind the three barriers above)
    }
    float* slab = slabs + static_cast<int64_t>(blockIdx.x) * 2 * channels;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        float a = sum_gamma[j], b = sum_beta[j];
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
            a += __shfl_xor(a, step);
            b += __shfl_xor(b, step);
        }
        const int c = 4 * j + slice;
        if (lane == 0 && c < channels) {
            slab[c] = a;
            slab[channels + c] = b;
        }
    }
}

// grid = ceil(2 channels / 16); block = 256 = 16 outputs x 16 strided runs of
// the slabs; the sixteen run sums are then added in order.
__global__ __launch_bounds__(256) void layernorm_backward_sum_kernel(
    const float* __restrict__ slabs, int parts, int channels, float* __restrict__ dgamma,
    float* __restrict__ dbeta) {
    __shared__ float runs[16][16];
    const int which = threadIdx.x & 15;
    const int strand = threadIdx.x >> 4;
    const int output = blockIdx.x * 16 + which;
    float sum = 0.f;
    if (output < 2 * channels)
        for (int part = strand; part < parts; part += 16)
            sum += slabs[static_cast<int64_t>(part) * 2 * channels + output];
    runs[strand][which] = sum;
    __syncthreads();
    if (strand == 0 && output < 2 * channels) {
        float all = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) all += runs[i][which];
        if (output < channels)
            dgamma[output] = all;
        else
            dbeta[output - channels] = all;
    }
}

constexpr int kLayerNormParts = 512;

}  // namespace emph

using namespace emph;

extern "C" {

int64_t emph_attention_backward_workspace(int64_t ld, int32_t heads) {
    if (ld <= 0 || heads <= 0) return 0;
    return 2 * static_cast<int64_t>(heads) * ld;
}

int emph_attention_backward(const float* qk, const float* v, const float* out,
                            const float* dout, float* dqkv, int64_t ld, int32_t channels,
                            int32_t heads, const int32_t* tiles, int32_t n_tiles,
                            int32_t tile_n, float* workspace, void* stream) {
    EMPH_REQUIRE(heads > 0 && channels > 0 && channels % heads == 0 && channels == 80 &&
                     heads == 2,
                 EMPH_ERANGE,
                 "emph_attention_backward: channels %d, heads %d (only 80 channels in 2 heads "
                 "of 40)", channels, heads);
    EMPH_REQUIRE(tile_n == kGradTile, EMPH_EINVAL,
                 "emph_attention_backward: tile_n %d (the 64-wide tile table)", tile_n);
    EMPH_REQUIRE(n_tiles >= 0 && ld > 0, EMPH_EINVAL, "emph_attention_backward: bad shape");
    if (n_tiles == 0) return EMPH_OK;
    EMPH_REQUIRE(qk && v && out && dout && dqkv && tiles && workspace, EMPH_EINVAL,
                 "emph_attention_backward: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    dim3 grid(n_tiles, heads);
    EMPH_LAUNCH(attention_backward_query_kernel<40>, grid, dim3(64 * kGradWaves), 0, s, qk, v,
                out, dout, dqkv, workspace, ld, channels, heads, tiles);
    int status = check_launch("emph_attention_backward (queries)");
    if (status != EMPH_OK) return status;
    EMPH_LAUNCH(attention_backward_key_kernel<40>, grid, dim3(64 * kGradWaves), 0, s, qk, v,
                dout, dqkv, workspace, ld, channels, heads, tiles);
    return check_launch("emph_attention_backward (keys)");
}

int32_t emph_add_layernorm_backward_parts(int32_t n_tiles) {
    if (n_tiles <= 0) return 0;
    const int run = (n_tiles + kLayerNormParts - 1) / kLayerNormParts;
    return (n_tiles + run - 1) / run;
}

int emph_add_layernorm_backward(const float* s, const float* gamma, const float* dy, float* ds,
                                int64_t ld, int32_t channels, float eps, const int32_t* tiles,
                                int32_t n_tiles, int32_t tile_n, float* workspace,
                                float* dgamma, float* dbeta, void* stream) {
    EMPH_REQUIRE(channels > 0 && channels <= 128, EMPH_ERANGE,
                 "emph_add_layernorm_backward: channels %d not in 1..128", channels);
    EMPH_REQUIRE(tile_n == 64, EMPH_EINVAL,
                 "emph_add_layernorm_backward: tile_n %d (the 64-wide tile table)", tile_n);
    EMPH_REQUIRE(n_tiles >= 0 && ld > 0, EMPH_EINVAL,
                 "emph_add_layernorm_backward: bad shape");
    EMPH_REQUIRE(dgamma && dbeta, EMPH_EINVAL, "emph_add_layernorm_backward: null pointer");
    EMPH_REQUIRE(n_tiles == 0 || (s && gamma && dy && ds && tiles && workspace), EMPH_EINVAL,
                 "emph_add_layernorm_backward: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int parts = emph_add_layernorm_backward_parts(n_tiles);
    if (parts > 0) {
        const int run = (n_tiles + parts - 1) / parts;
        if (channels <= 80)
            EMPH_LAUNCH(add_layernorm_backward_kernel<80>, dim3(parts), dim3(256), 0, st, s,
                        gamma, dy, ds, ld, channels, eps, tiles, n_tiles, run, workspace);
        else
            EMPH_LAUNCH(add_layernorm_backward_kernel<128>, dim3(parts), dim3(256), 0, st, s,
                        gamma, dy, ds, ld, channels, eps, tiles, n_tiles, run, workspace);
        int status = check_launch("emph_add_layernorm_backward");
        if (status != EMPH_OK) return status;
    }
    // (no tile: the sums over nothing, zeros)
    EMPH_LAUNCH(layernorm_backward_sum_kernel, dim3((2 * channels + 15) / 16), dim3(256), 0, st,
                workspace, parts, channels, dgamma, dbeta);
    return check_launch("emph_add_layernorm_backward (sum)");
}

}  // extern "C"
