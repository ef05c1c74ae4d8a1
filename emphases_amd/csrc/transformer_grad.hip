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
//
// Under the reference's dropout (emph_attention_dropout and its backward) the
// softmax weights carry a specified Philox mask M and the scale s = 1/(1-p):
//     O = (M o P s) V     dV = (M o P s)^T dO     dS = P o (s M o dP - D)
// with D unchanged.  Both passes are templates on `DROP`; the mask is
// regenerated in each of them and in the forward, never stored.
#include <math.h>

#include "common.h"
#include "step.h"

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

// The attention mask of training (emphases_amd/train/dropout.py,
// `attention_keep_mask`): key quad k / 4 of (head, packed query column) has the
// Philox counter (k / 4, head ld + column, stream, step) under the key `seed`;
// its four words belong to keys 4 (k / 4) .. + 3 of the segment, in order, and
// a weight is kept iff its word >= threshold.  Never stored: the forward and
// both passes of the backward regenerate it.
struct AttentionMask {
    uint32_t seed_lo, seed_hi, stream_id, step, threshold;
    float scale;
};

// bit r: key 4 quad + r of `row` = head ld + packed query column is kept
__device__ __forceinline__ uint32_t attention_keep_bits(const AttentionMask& mask, uint32_t quad,
                                                        uint32_t row) {
    const Words w =
        philox4x32_10(Words{quad, row, mask.stream_id, mask.step}, mask.seed_lo, mask.seed_hi);
    return (w.x >= mask.threshold ? 1u : 0u) | (w.y >= mask.threshold ? 2u : 0u) |
           (w.z >= mask.threshold ? 4u : 0u) | (w.w >= mask.threshold ? 8u : 0u);
}

// The value of lane (lane ^ XOR) of the aligned group of four lanes (quad-permute DPP).
template <int XOR>
__device__ __forceinline__ uint32_t quad_lane_xor(uint32_t x) {
    constexpr int control = (0 ^ XOR) | ((1 ^ XOR) << 2) | ((2 ^ XOR) << 4) | ((3 ^ XOR) << 6);
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(
        static_cast<int>(x), static_cast<int>(x), control, 0xf, 0xf, false));
}

// The scores of the masked kernels as TWO floats, high + low.  One chain of
// KSTEPS accumulating MFMAs rounds its running sum at the size of the logit
// every step; behind 'sum' the word decoder's first layer has logits of
// several hundred (log2 units), whose ulp of 6e-5 then stands in every weight
// of a peaked row.  Here chains of two k-steps start from zero and are added
// by TwoSum (Knuth), the rounding errors kept in `low`; a weight is
// exp2((high - max) + low), the first difference exact between neighbours.
// The price is VALU work beside the MFMAs (EXPERIMENTS: about 5 ms of the 36.6 ms
// masked step); the plain backward does not pay it.
constexpr int kScoreChain = 2;
template <int KSTEPS>
__device__ __forceinline__ f32x4 scores_split(const float (&a)[KSTEPS], const float (&b)[KSTEPS],
                                              f32x4& low) {
    f32x4 high = f32x4{0.f, 0.f, 0.f, 0.f};
    low = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int first = 0; first < KSTEPS; first += kScoreChain) {
        f32x4 part = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = first; s < first + kScoreChain && s < KSTEPS; ++s)
            part = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], part, 0, 0, 0);
        if (first == 0) {
            high = part;
        } else {
            const f32x4 sum = high + part;
            const f32x4 shift = sum - high;
            low += (high - (sum - shift)) + (part - shift);
            high = sum;
        }
    }
    return high;
}

// grid = (n_tiles, heads); block = 128: wave w owns queries [32 w, 32 w + 32)
// of the tile.  `stats` = [2][heads][ld]: the row log-sum-exp in log2 units,
// then D ([3][heads][ld] under DROP: the row maximum, D, 1 / sum).
// DROP: the weights were dropped in the forward (emph_attention_dropout);
// without it `mask` is unused and the code is that of the plain backward.
template <int D, bool DROP, bool KEYS>
__global__ __launch_bounds__(64 * kGradWaves) void attention_backward_query_kernel(
    const float* __restrict__ qk, const float* __restrict__ v, const float* __restrict__ out,
    const float* __restrict__ dout, float* __restrict__ dqkv, float* __restrict__ stats,
    int64_t ld, int channels, int heads, const int32_t* __restrict__ tiles,
    const int32_t* __restrict__ key_counts, AttentionMask mask) {
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
    // KEYS: only the segment's leading `keys` positions are keys, the rest is
    // padding behind src_key_padding_mask (every position stays a query).  The
    // loads below clamp to the last REAL key: a padded K or V row is never read.
    const int keys = KEYS ? min(max(key_counts[span.segment], 1), count) : count;
    // ONE real key in front of padding: the softmax is the constant 1 and its
    // derivative zero.  dP (an MFMA chain) and D (dO . O, summed another way)
    // are then two roundings of the same sum, and their difference, 4e-6 where
    // the sums are of size 10, would stand in dQ and, added over the queries,
    // in dK: dS is selected to 0 instead, as a softmax backward that takes D
    // from P and dP gives it.  (Not without padding, n = k = 1: there the bits
    // are those of the plain backward.)
    const bool single = KEYS && keys == 1 && count > 1;
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
    for (int key0 = 0; key0 < keys; key0 += 16) {
        float ak[KSTEPS];
        const int key = min(key0 + col, keys - 1);
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
            ak[s] = k_rows[static_cast<int64_t>(4 * s + kk) * ld + key];
        f32x4 s4[QT], low4[QT];
        if constexpr (DROP) {
#pragma unroll
            for (int t = 0; t < QT; ++t) s4[t] = scores_split<KSTEPS>(ak, bq[t], low4[t]);
        } else {
#pragma unroll
            for (int t = 0; t < QT; ++t) s4[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
                for (int t = 0; t < QT; ++t)
                    s4[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ak[s], bq[t][s], s4[t], 0, 0,
                                                                 0);
        }
#pragma unroll
        for (int t = 0; t < QT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (key0 + 4 * kk + r >= keys) s4[t][r] = -INFINITY;
            const float high =
                fmaxf(fmaxf(fmaxf(s4[t][0], s4[t][1]), fmaxf(s4[t][2], s4[t][3])), top[t]);
            if (high > -INFINITY) {                // (a lane whose keys are all masked so far)
                float sum = total[t] * __builtin_amdgcn_exp2f(top[t] - high);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (DROP)
                        sum += __builtin_amdgcn_exp2f((s4[t][r] - high) + low4[t][r]);
                    else
                        sum += __builtin_amdgcn_exp2f(s4[t][r] - high);
                }
                total[t] = sum;
                top[t] = high;
            }
        }
    }
    // DROP keeps the row maximum and 1 / sum apart (a third row of `stats`):
    // P = exp2(S - max) / sum adds up to 1 whatever the size of the logits,
    // where max + log2(sum) as ONE float loses ulp(max) of every weight of the
    // row alike, which dS = P o (dP - D) does not forgive once the row is
    // peaked (dP - D cancels) - logits of several hundred reach the word
    // decoder behind 'sum'.
    float lse[QT], inverse[QT];
    float* lse_row = stats + static_cast<int64_t>(head) * ld + span.offset;
    float* delta_row = stats + static_cast<int64_t>(heads + head) * ld + span.offset;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const float high = grad_rows_max(top[t]);          // finite: key 0 exists
        const float mine =
            top[t] == -INFINITY ? 0.f : total[t] * __builtin_amdgcn_exp2f(top[t] - high);
        if constexpr (DROP) {
            lse[t] = high;
            inverse[t] = 1.f / grad_rows_sum(mine);
        } else {
            lse[t] = high + log2f(grad_rows_sum(mine));
        }
        const int query = q0 + 16 * t + col;
        if (kk == 0 && query < count) {
            lse_row[query] = lse[t];
            delta_row[query] = delta[t];
            if constexpr (DROP)
                stats[static_cast<int64_t>(2 * heads + head) * ld + span.offset + query] =
                    inverse[t];
        }
    }

    // ---- pass 2: dQ^T[d][query] = sum_key K^T[d][key] dS^T[key][query]
    f32x4 dq[QT][MT];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m) dq[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int key0 = 0; key0 < keys; key0 += 16) {
        float ak[KSTEPS], av[KSTEPS], akt[4][MT];
        const int key = min(key0 + col, keys - 1);
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            ak[s] = k_rows[static_cast<int64_t>(4 * s + kk) * ld + key];
            av[s] = v_rows[static_cast<int64_t>(key) * channels + 4 * s + kk];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tkey = min(key0 + 4 * kk + r, keys - 1);
#pragma unroll
            for (int m = 0; m < MT; ++m)
                akt[r][m] = k_rows[static_cast<int64_t>(min(16 * m + col, D - 1)) * ld + tkey];
        }
        f32x4 s4[QT], dp4[QT], low4[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            s4[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp4[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if constexpr (DROP) {
#pragma unroll
            for (int t = 0; t < QT; ++t) s4[t] = scores_split<KSTEPS>(ak, bq[t], low4[t]);
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
                for (int t = 0; t < QT; ++t)
                    dp4[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bdo[t][s], dp4[t], 0,
                                                                  0, 0);
        } else {
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    s4[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ak[s], bq[t][s], s4[t], 0, 0,
                                                                 0);
                    dp4[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bdo[t][s], dp4[t], 0,
                                                                  0, 0);
                }
        }
        // a key past the last one: probability 0 (selected; the clamped loads
        // above only feed such rows)
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            if constexpr (DROP) {
                // the lane's four keys are one quad of its query: one call
                const uint32_t keep = attention_keep_bits(
                    mask, static_cast<uint32_t>(key0 / 4 + kk),
                    static_cast<uint32_t>(head * ld + span.offset + q0 + 16 * t + col));
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    dp4[t][r] = (keep >> r & 1u) ? dp4[t][r] * mask.scale : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float exponent = s4[t][r] - lse[t];
                if constexpr (DROP) exponent += low4[t][r];
                float p = key0 + 4 * kk + r < keys ? __builtin_amdgcn_exp2f(exponent) : 0.f;
                if constexpr (DROP) p *= inverse[t];
                s4[t][r] = single ? 0.f : p * (dp4[t][r] - delta[t]);
            }
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
// the tile and walks the segment's queries 16 at a time.  KEYS: a block of 16
// keys at or past the segment's last real key does no MFMA work and a padded
// key's dK and dV columns are stored as zeros.
template <int D, bool DROP, bool KEYS>
__global__ __launch_bounds__(64 * kGradWaves) void attention_backward_key_kernel(
    const float* __restrict__ qk, const float* __restrict__ v, const float* __restrict__ dout,
    float* __restrict__ dqkv, const float* __restrict__ stats, int64_t ld, int channels,
    int heads, const int32_t* __restrict__ tiles, const int32_t* __restrict__ key_counts,
    AttentionMask mask) {
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
    const int keys = KEYS ? min(max(key_counts[span.segment], 1), count) : count;
    const bool real = !KEYS || k0 < keys;          // wave-uniform: any real key here
    // (one real key in front of padding: dS = 0, see the query pass)
    const bool single = KEYS && keys == 1 && count > 1;
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
    // past the last one is a clamped copy: its column is never stored (KEYS:
    // stored as zeros).
    float bk[KT][KSTEPS], bv[KT][KSTEPS];
#pragma unroll
    for (int u = 0; u < KT; ++u) {
        const int key = min(k0 + 16 * u + col, keys - 1);
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

    for (int q0 = 0; q0 < (real ? count : 0); q0 += 16) {
        float aq[KSTEPS], ado[KSTEPS], aqt[4][MT], adot[4][MT], lse[4], delta[4], inverse[4];
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
            if constexpr (DROP)
                inverse[r] = stats[static_cast<int64_t>(2 * heads + head) * ld + span.offset +
                                   tquery];
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
            if (KEYS && k0 + 16 * u >= keys) continue;     // wave-uniform: padding only
            f32x4 s4 = f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 dp4 = f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 low4;
            if constexpr (DROP) {
                s4 = scores_split<KSTEPS>(aq, bk[u], low4);
#pragma unroll
                for (int s = 0; s < KSTEPS; ++s)
                    dp4 = __builtin_amdgcn_mfma_f32_16x16x4f32(ado[s], bv[u][s], dp4, 0, 0, 0);
            } else {
#pragma unroll
                for (int s = 0; s < KSTEPS; ++s) {
                    s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[s], bk[u][s], s4, 0, 0, 0);
                    dp4 = __builtin_amdgcn_mfma_f32_16x16x4f32(ado[s], bv[u][s], dp4, 0, 0, 0);
                }
            }
            // s4[r] = score(query q0 + 4 kk + r, key col); a query past the
            // segment contributes nothing (selected)
            uint32_t keep = 0;                     // bit r: (query q0 + 4 kk + r, key col) kept
            if constexpr (DROP) {
                // The lane holds four QUERIES of one key, a quad of the mask
                // four KEYS of one query: lane 4 a + b of an aligned group of
                // four calls for (query q0 + 4 kk + b, the keys of columns
                // 4 a .. 4 a + 3) and the group transposes the bits: lane
                // b ^ j holds query b ^ j, whose bit b is this lane's key.
                const uint32_t bits = attention_keep_bits(
                    mask, static_cast<uint32_t>((k0 + 16 * u) / 4 + (col >> 2)),
                    static_cast<uint32_t>(head * ld + span.offset + q0 + 4 * kk + (col & 3)));
                const uint32_t b = col & 3;
                keep = (bits >> b & 1u) << b | (quad_lane_xor<1>(bits) >> b & 1u) << (b ^ 1u) |
                       (quad_lane_xor<2>(bits) >> b & 1u) << (b ^ 2u) |
                       (quad_lane_xor<3>(bits) >> b & 1u) << (b ^ 3u);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float exponent = s4[r] - lse[r];
                if constexpr (DROP) exponent += low4[r];
                float p = q0 + 4 * kk + r < count ? __builtin_amdgcn_exp2f(exponent) : 0.f;
                if constexpr (DROP) {
                    p *= inverse[r];
                    const bool kept = keep >> r & 1u;
                    s4[r] = kept ? p * mask.scale : 0.f;
                    dp4[r] = p * ((kept ? dp4[r] * mask.scale : 0.f) - delta[r]);
                } else {
                    s4[r] = p;
                    dp4[r] = single ? 0.f : p * (dp4[r] - delta[r]);
                }
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
        const bool padded = key >= keys;           // (never without KEYS)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 16 * m + 4 * kk + r;
                if (d < D) {
                    dk_rows[static_cast<int64_t>(d) * ld + key] =
                        padded ? 0.f : dk[u][m][r] * scale;
                    dv_rows[static_cast<int64_t>(d) * ld + key] = padded ? 0.f : dv[u][m][r];
                }
            }
    }
}

// The attention of TRAINING: O = (M o P scale) V with the mask above on the
// softmax weights (the dropout inside nn.MultiheadAttention).  The query pass
// of the backward with its second loop turned to the forward product: the
// statistics stay in registers, and O^T[d][query] = sum_key V^T[d][key]
// P~^T[key][query] takes the dropped weights as B operands where they stand.
// grid = (n_tiles, heads); block = 128: wave w owns queries [32 w, 32 w + 32).
template <int D>
__global__ __launch_bounds__(64 * kGradWaves) void attention_dropout_kernel(
    const float* __restrict__ qk, const float* __restrict__ v, float* __restrict__ out,
    int64_t ld, int channels, const int32_t* __restrict__ tiles, AttentionMask mask) {
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
    const float scale2 = kLog2e / sqrtf(static_cast<float>(D));

    const int64_t head_row = static_cast<int64_t>(head * D) * ld + span.offset;
    const float* q_rows = qk + head_row;
    const float* k_rows = qk + static_cast<int64_t>(channels) * ld + head_row;
    const float* v_rows = v + static_cast<int64_t>(span.offset) * channels + head * D;

    float bq[QT][KSTEPS];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int query = q0 + 16 * t + col;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
            bq[t][s] = query < count
                           ? q_rows[static_cast<int64_t>(4 * s + kk) * ld + query] * scale2
                           : 0.f;
    }

    // ---- pass 1: the row log-sum-exp, as the backward takes it
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
        f32x4 s4[QT], low4[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) s4[t] = scores_split<KSTEPS>(ak, bq[t], low4[t]);
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
                for (int r = 0; r < 4; ++r)
                    sum += __builtin_amdgcn_exp2f((s4[t][r] - high) + low4[t][r]);
                total[t] = sum;
                top[t] = high;
            }
        }
    }
    // (the maximum and 1 / sum apart, as the masked backward keeps them)
    float lse[QT], inverse[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const float high = grad_rows_max(top[t]);          // finite: key 0 exists
        const float mine =
            top[t] == -INFINITY ? 0.f : total[t] * __builtin_amdgcn_exp2f(top[t] - high);
        lse[t] = high;
        inverse[t] = 1.f / grad_rows_sum(mine);
    }

    // ---- pass 2: O^T[d][query] = sum_key V^T[d][key] P~^T[key][query]
    f32x4 o[QT][MT];
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m) o[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int key0 = 0; key0 < count; key0 += 16) {
        float ak[KSTEPS], avt[4][MT];
        const int key = min(key0 + col, count - 1);
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
            ak[s] = k_rows[static_cast<int64_t>(4 * s + kk) * ld + key];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tkey = min(key0 + 4 * kk + r, count - 1);
#pragma unroll
            for (int m = 0; m < MT; ++m)
                avt[r][m] = v_rows[static_cast<int64_t>(tkey) * channels + min(16 * m + col, D - 1)];
        }
        f32x4 s4[QT], low4[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) s4[t] = scores_split<KSTEPS>(ak, bq[t], low4[t]);
        // a key past the segment: weight 0 (selected; the clamped loads above
        // only feed such rows)
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const uint32_t keep = attention_keep_bits(
                mask, static_cast<uint32_t>(key0 / 4 + kk),
                static_cast<uint32_t>(head * ld + span.offset + q0 + 16 * t + col));
#pragma unroll
            for (int r = 0; r < 4; ++r)
                s4[t][r] = key0 + 4 * kk + r < count && (keep >> r & 1u)
                               ? __builtin_amdgcn_exp2f((s4[t][r] - lse[t]) + low4[t][r]) *
                                     inverse[t] * mask.scale
                               : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    o[t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(avt[r][m], s4[t][r], o[t][m],
                                                                   0, 0, 0);
    }
    float* o_rows = out + head_row;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int query = q0 + 16 * t + col;
        if (query >= count) continue;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 16 * m + 4 * kk + r;
                if (d < D) o_rows[static_cast<int64_t>(d) * ld + query] = o[t][m][r];
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

// The body of emph_attention_backward (`key_counts` NULL: every position a
// key) and of emph_attention_backward_keys, under the entry's own `name`.
static int attention_backward_launch(const char* name, const float* qk, const float* v,
                                     const float* out, const float* dout, float* dqkv,
                                     int64_t ld, int32_t channels, int32_t heads,
                                     const int32_t* tiles, int32_t n_tiles, int32_t tile_n,
                                     const int32_t* key_counts, float* workspace,
                                     void* stream) {
    EMPH_REQUIRE(heads > 0 && channels > 0 && channels % heads == 0 && channels == 80 &&
                     heads == 2,
                 EMPH_ERANGE,
                 "%s: channels %d, heads %d (only 80 channels in 2 heads of 40)", name,
                 channels, heads);
    EMPH_REQUIRE(tile_n == kGradTile, EMPH_EINVAL, "%s: tile_n %d (the 64-wide tile table)",
                 name, tile_n);
    EMPH_REQUIRE(n_tiles >= 0 && ld > 0, EMPH_EINVAL, "%s: bad shape", name);
    if (n_tiles == 0) return EMPH_OK;
    EMPH_REQUIRE(qk && v && out && dout && dqkv && tiles && workspace, EMPH_EINVAL,
                 "%s: null pointer", name);
    hipStream_t s = static_cast<hipStream_t>(stream);
    dim3 grid(n_tiles, heads);
    if (key_counts != nullptr)
        EMPH_LAUNCH((attention_backward_query_kernel<40, false, true>), grid,
                    dim3(64 * kGradWaves), 0, s, qk, v, out, dout, dqkv, workspace, ld,
                    channels, heads, tiles, key_counts, AttentionMask{});
    else
        EMPH_LAUNCH((attention_backward_query_kernel<40, false, false>), grid,
                    dim3(64 * kGradWaves), 0, s, qk, v, out, dout, dqkv, workspace, ld,
                    channels, heads, tiles, key_counts, AttentionMask{});
    int status = check_launch(key_counts != nullptr ? "emph_attention_backward_keys (queries)"
                                                    : "emph_attention_backward (queries)");
    if (status != EMPH_OK) return status;
    if (key_counts != nullptr)
        EMPH_LAUNCH((attention_backward_key_kernel<40, false, true>), grid,
                    dim3(64 * kGradWaves), 0, s, qk, v, dout, dqkv, workspace, ld, channels,
                    heads, tiles, key_counts, AttentionMask{});
    else
        EMPH_LAUNCH((attention_backward_key_kernel<40, false, false>), grid,
                    dim3(64 * kGradWaves), 0, s, qk, v, dout, dqkv, workspace, ld, channels,
                    heads, tiles, key_counts, AttentionMask{});
    return check_launch(key_counts != nullptr ? "emph_attention_backward_keys (keys)"
                                              : "emph_attention_backward (keys)");
}

int emph_attention_backward(const float* qk, const float* v, const float* out,
                            const float* dout, float* dqkv, int64_t ld, int32_t channels,
                            int32_t heads, const int32_t* tiles, int32_t n_tiles,
                            int32_t tile_n, float* workspace, void* stream) {
    return attention_backward_launch("emph_attention_backward", qk, v, out, dout, dqkv, ld,
                                     channels, heads, tiles, n_tiles, tile_n, nullptr,
                                     workspace, stream);
}

int emph_attention_backward_keys(const float* qk, const float* v, const float* out,
                                 const float* dout, float* dqkv, int64_t ld, int32_t channels,
                                 int32_t heads, const int32_t* tiles, int32_t n_tiles,
                                 int32_t tile_n, const int32_t* key_counts, float* workspace,
                                 void* stream) {
    return attention_backward_launch(
        key_counts != nullptr ? "emph_attention_backward_keys" : "emph_attention_backward", qk,
        v, out, dout, dqkv, ld, channels, heads, tiles, n_tiles, tile_n, key_counts, workspace,
        stream);
}

// (word 1 of the counter, head ld + column, stays inside 32 bits)
constexpr int64_t kMaskedColumns = int64_t{1} << 28;

static AttentionMask attention_mask(float p, uint64_t seed, uint32_t stream_id, uint32_t step) {
    return AttentionMask{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32),
                         stream_id, step, dropout_threshold(p), dropout_scale(p)};
}

int64_t emph_attention_dropout_backward_workspace(int64_t ld, int32_t heads) {
    if (ld <= 0 || heads <= 0) return 0;
    return 3 * static_cast<int64_t>(heads) * ld;
}

int emph_attention_dropout(const float* qk, const float* v, float* out, int64_t ld,
                           int32_t channels, int32_t heads, const int32_t* tiles,
                           int32_t n_tiles, int32_t tile_n, float p, uint64_t seed,
                           uint32_t stream_id, uint32_t step, void* stream) {
    EMPH_REQUIRE(channels == 80 && heads == 2, EMPH_ERANGE,
                 "emph_attention_dropout: channels %d, heads %d (only 80 channels in 2 heads "
                 "of 40)", channels, heads);
    EMPH_REQUIRE(tile_n == kGradTile, EMPH_EINVAL,
                 "emph_attention_dropout: tile_n %d (the 64-wide tile table)", tile_n);
    EMPH_REQUIRE(p >= 0.f && p < 1.f, EMPH_EINVAL, "emph_attention_dropout: p %g (0 <= p < 1)",
                 static_cast<double>(p));
    EMPH_REQUIRE(n_tiles >= 0 && ld > 0, EMPH_EINVAL, "emph_attention_dropout: bad shape");
    EMPH_REQUIRE(ld < kMaskedColumns, EMPH_ERANGE, "emph_attention_dropout: ld >= 2^28");
    if (n_tiles == 0) return EMPH_OK;
    EMPH_REQUIRE(qk && v && out && tiles, EMPH_EINVAL, "emph_attention_dropout: null pointer");
    EMPH_LAUNCH(attention_dropout_kernel<40>, dim3(n_tiles, heads), dim3(64 * kGradWaves), 0,
                static_cast<hipStream_t>(stream), qk, v, out, ld, channels, tiles,
                attention_mask(p, seed, stream_id, step));
    return check_launch("emph_attention_dropout");
}

int emph_attention_dropout_backward(const float* qk, const float* v, const float* out,
                                    const float* dout, float* dqkv, int64_t ld,
                                    int32_t channels, int32_t heads, const int32_t* tiles,
                                    int32_t n_tiles, int32_t tile_n, float* workspace, float p,
                                    uint64_t seed, uint32_t stream_id, uint32_t step,
                                    void* stream) {
    EMPH_REQUIRE(channels == 80 && heads == 2, EMPH_ERANGE,
                 "emph_attention_dropout_backward: channels %d, heads %d (only 80 channels in "
                 "2 heads of 40)", channels, heads);
    EMPH_REQUIRE(tile_n == kGradTile, EMPH_EINVAL,
                 "emph_attention_dropout_backward: tile_n %d (the 64-wide tile table)", tile_n);
    EMPH_REQUIRE(p >= 0.f && p < 1.f, EMPH_EINVAL,
                 "emph_attention_dropout_backward: p %g (0 <= p < 1)", static_cast<double>(p));
    EMPH_REQUIRE(n_tiles >= 0 && ld > 0, EMPH_EINVAL,
                 "emph_attention_dropout_backward: bad shape");
    EMPH_REQUIRE(ld < kMaskedColumns, EMPH_ERANGE,
                 "emph_attention_dropout_backward: ld >= 2^28");
    // p = 0 keeps every weight at scale 1: the plain backward, bit for bit
    if (p == 0.f)
        return emph_attention_backward(qk, v, out, dout, dqkv, ld, channels, heads, tiles,
                                       n_tiles, tile_n, workspace, stream);
    if (n_tiles == 0) return EMPH_OK;
    EMPH_REQUIRE(qk && v && out && dout && dqkv && tiles && workspace, EMPH_EINVAL,
                 "emph_attention_dropout_backward: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    dim3 grid(n_tiles, heads);
    const AttentionMask mask = attention_mask(p, seed, stream_id, step);
    EMPH_LAUNCH((attention_backward_query_kernel<40, true, false>), grid,
                dim3(64 * kGradWaves), 0, s, qk, v, out, dout, dqkv, workspace, ld, channels,
                heads, tiles, static_cast<const int32_t*>(nullptr), mask);
    int status = check_launch("emph_attention_dropout_backward (queries)");
    if (status != EMPH_OK) return status;
    EMPH_LAUNCH((attention_backward_key_kernel<40, true, false>), grid, dim3(64 * kGradWaves),
                0, s, qk, v, dout, dqkv, workspace, ld, channels, heads, tiles,
                static_cast<const int32_t*>(nullptr), mask);
    return check_launch("emph_attention_dropout_backward (keys)");
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
