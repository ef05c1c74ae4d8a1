// Backward of the attention core (transformer_grad.hip: emph_attention_backward)
// for LONG segments on the bf16 matrix pipe, every fp32 operand split into bf16
// pieces as attention_split.hip splits the forward's - the `'bf16x3'` rule of
// the engine for attention:
//     S  = Q K^T / sqrt(d)     THREE pieces per operand, six products (the
//                              scores' error sits in front of an exponential)
//     dP = dO V^T   dV = P^T dO   dQ = dS K   dK = dS^T Q
//                              TWO pieces per operand, three products; P and dS
//                              are split as fp32 values where they stand in the
//                              accumulators, as the forward splits P
// pieces rounded to nearest (split.h); accumulation, the row log-sum-exp,
// D_i = sum_c dO_ic O_ic and dS = P o (dP - D) stay fp32.
//
// Three launches, none with atomics:
//   0. per 64 positions of a long segment and head: the IMAGES - every operand
//      that is streamed through LDS, split once and laid out as its MFMA
//      fragment reads it (a stage = 64 positions, `GradImages`):
//        "row" layout   [d / 8][position][8 d]      A fragment of X[position][d],
//                       k = d: Q (scaled into log2 units), K, V, dO
//        "turned" layout [position / 8][d][8 positions], the positions of each
//                       16 permuted to the accumulator layout (position
//                       8 h + 4 a + i holds 8 a + 4 h + i, as the forward's V
//                       image): A fragment of X^T[d][position], k = position:
//                       K, Q, dO; row D is zeros (what rows D .. 63 read)
//   1. per 256 QUERIES (eight waves of 32, the tile table of
//      attention_split.hip): the query is the MFMA column.  A first walk over
//      the keys takes the row log-sum-exp (scores only), written with D into
//      the workspace; a second one S^T = K Q^T and dP^T = V dO^T, dS^T in the
//      accumulators, which ARE the B operand of dQ^T = K^T dS^T once split.
//   2. per 256 KEYS: the key is the MFMA column, K and V of the wave's 32 keys
//      stay in registers as B operands; the queries stream: S = Q K^T,
//      dP = dO V^T, then dV^T = dO^T P and dK^T = Q^T dS.
// A stage of images reaches LDS through registers: the next stage's loads are
// in flight during the products of this one.  Every element of dqkv inside a
// covered segment is written by one lane, its sum taken in key (query) order:
// the same inputs give the same bits, and a segment's result does not depend
// on what else is in the batch.
#include <math.h>

#include "common.h"
#include "split.h"

namespace emph {

constexpr int kGradSplitWaves = 8;
constexpr int kGradSplitThreads = 64 * kGradSplitWaves;
constexpr int kGradSplitTile = 32 * kGradSplitWaves;     // positions per workgroup
constexpr float kGradLog2e = 1.44269504088896340736f;
// (tile offsets are int32, and the neighbours' limit: engine.KERNEL_COLUMNS)
constexpr int64_t kGradSplitColumns = int64_t{1} << 28;

// One stage (64 positions of one segment and head), [what the query pass stages]
// [what the key pass stages]; slots as SplitImages'.
template <int D>
struct GradImages {
    static constexpr int kOctets = (D + 15) / 16 * 2;
    static constexpr int kRowBytes = kOctets * kSplitStage * 16;      // a piece, row layout
    static constexpr int kRows = D + 1;
    static constexpr int kTurnedBytes = (kSplitStage / 8) * kRows * 16;
    // the query pass: K (3 pieces), V (2), K turned (2)
    static constexpr int kKey = 0;
    static constexpr int kValue = 3 * kRowBytes;
    static constexpr int kKeyTurned = 5 * kRowBytes;
    static constexpr int kScoreBytes = 3 * kRowBytes;                 // its first walk
    static constexpr int kQueryPass = 5 * kRowBytes + 2 * kTurnedBytes;
    // the key pass (from kQueryPass on): Q (3), dO (2), Q turned (2), dO turned (2)
    static constexpr int kQuery = 0;
    static constexpr int kDout = 3 * kRowBytes;
    static constexpr int kQueryTurned = 5 * kRowBytes;
    static constexpr int kDoutTurned = 5 * kRowBytes + 2 * kTurnedBytes;
    static constexpr int kKeyPass = 5 * kRowBytes + 4 * kTurnedBytes;
    static constexpr int kStageBytes = kQueryPass + kKeyPass;
};

// BYTES of a stage: global memory -> registers (issued early) -> LDS
template <int BYTES>
struct StageCopy {
    static constexpr int kUnits = BYTES / 16;
    static constexpr int kPasses = (kUnits + kGradSplitThreads - 1) / kGradSplitThreads;
    u32x4 held[kPasses];
    __device__ __forceinline__ void fetch(const unsigned char* source, int tid) {
#pragma unroll
        for (int pass = 0; pass < kPasses; ++pass) {
            const int unit = pass * kGradSplitThreads + tid;
            if (unit < kUnits) held[pass] = *reinterpret_cast<const u32x4*>(source + 16 * unit);
        }
    }
    __device__ __forceinline__ void put(unsigned char* lds, int tid) const {
#pragma unroll
        for (int pass = 0; pass < kPasses; ++pass) {
            const int unit = pass * kGradSplitThreads + tid;
            if (unit < kUnits) *reinterpret_cast<u32x4*>(lds + 16 * unit) = held[pass];
        }
    }
};

// grid = (n_tiles of 256, 4 stages of a tile, heads); block = 256
template <int D>
__global__ __launch_bounds__(256) void grad_images_kernel(
    const float* __restrict__ qk, const float* __restrict__ v, const float* __restrict__ dout,
    int64_t ld, int channels, int heads, const int32_t* __restrict__ tiles,
    unsigned char* __restrict__ images) {
    typedef GradImages<D> Images;
    constexpr int STAGE = kSplitStage;
    const Tile tile = load_tile(tiles, blockIdx.x);
    const int first = tile.first + STAGE * static_cast<int>(blockIdx.y);
    if (first >= tile.count) return;
    const int head = blockIdx.z;
    const int valid = min(STAGE, tile.count - first);          // >= 1
    const int slot = (tile.offset >> 6) + tile.segment + (first >> 6);
    unsigned char* stage =
        images + (static_cast<int64_t>(slot) * heads + head) * Images::kStageBytes;
    const int64_t column0 = static_cast<int64_t>(tile.offset) + first;
    const float scale2 = kGradLog2e / sqrtf(static_cast<float>(D));
    const float* q_rows = qk + static_cast<int64_t>(head * D) * ld + column0;
    const float* k_rows = q_rows + static_cast<int64_t>(channels) * ld;
    const float* do_rows = dout + static_cast<int64_t>(head * D) * ld + column0;
    const float* v_rows = v + column0 * channels + head * D;

    // row layout: Q (scaled), K, V, dO.  What lies beyond the segment or beyond D is
    // ZERO (selected: the padding of the packed axis may hold NaN)
    constexpr int ROW_TASKS = Images::kOctets * STAGE;
    for (int task = threadIdx.x; task < 4 * ROW_TASKS; task += blockDim.x) {
        const int position = task % STAGE, octet = task / STAGE % Images::kOctets;
        const int which = task / ROW_TASKS;
        const bool live = position < valid && octet < D / 8;
        const int p = min(position, valid - 1), o = min(octet, D / 8 - 1);
        float values[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float x;
            if (which == 2) {
                x = v_rows[static_cast<int64_t>(p) * channels + 8 * o + e];
            } else {
                const float* rows = which == 0 ? q_rows : which == 1 ? k_rows : do_rows;
                x = rows[static_cast<int64_t>(8 * o + e) * ld + p];
            }
            if (which == 0) x *= scale2;
            values[e] = live ? x : 0.f;
        }
        const int byte = (octet * STAGE + position) * 16;
        if (which < 2) {
            u32x4 parts[3];
            split_eight<3>(values, parts);
            unsigned char* base =
                stage + (which == 0 ? Images::kQueryPass + Images::kQuery : Images::kKey);
#pragma unroll
            for (int piece = 0; piece < 3; ++piece)
                *reinterpret_cast<u32x4*>(base + piece * Images::kRowBytes + byte) = parts[piece];
        } else {
            u32x4 parts[2];
            split_eight<2>(values, parts);
            unsigned char* base =
                stage + (which == 2 ? Images::kValue : Images::kQueryPass + Images::kDout);
#pragma unroll
            for (int piece = 0; piece < 2; ++piece)
                *reinterpret_cast<u32x4*>(base + piece * Images::kRowBytes + byte) = parts[piece];
        }
    }
    // turned layout: K, Q, dO (unscaled), row D zeros
    constexpr int TURNED_TASKS = (STAGE / 8) * Images::kRows;
    for (int task = threadIdx.x; task < 3 * TURNED_TASKS; task += blockDim.x) {
        const int chunk = task % (STAGE / 8), row = task / (STAGE / 8) % Images::kRows;
        const int which = task / TURNED_TASKS;
        const float* rows = (which == 0 ? k_rows : which == 1 ? q_rows : do_rows) +
                            static_cast<int64_t>(min(row, D - 1)) * ld;
        const int group = chunk >> 1, h = chunk & 1;
        float values[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int position = 16 * group + 8 * (e >> 2) + 4 * h + (e & 3);
            const float x = rows[min(position, valid - 1)];
            values[e] = row < D && position < valid ? x : 0.f;
        }
        u32x4 parts[2];
        split_eight<2>(values, parts);
        unsigned char* base =
            stage + (which == 0 ? Images::kKeyTurned
                                : Images::kQueryPass +
                                      (which == 1 ? Images::kQueryTurned : Images::kDoutTurned));
        const int byte = (chunk * Images::kRows + row) * 16;
#pragma unroll
        for (int piece = 0; piece < 2; ++piece)
            *reinterpret_cast<u32x4*>(base + piece * Images::kTurnedBytes + byte) = parts[piece];
    }
}

// A fragment of a row-layout piece: lane (position `local + column`, half) of k-step s
template <int D>
__device__ __forceinline__ u32x4 row_fragment(const unsigned char* piece, int s, int half,
                                              int position) {
    return *reinterpret_cast<const u32x4*>(piece + ((2 * s + half) * kSplitStage + position) * 16);
}

// A fragment of a turned piece: row 32 m + column (rows D .. read the zero row), the
// eight positions of (k-step ks, half) of the block at `local`
template <int D>
__device__ __forceinline__ u32x4 turned_fragment(const unsigned char* piece, int local, int ks,
                                                 int half, int row) {
    return *reinterpret_cast<const u32x4*>(
        piece + (((local >> 3) + 2 * ks + half) * GradImages<D>::kRows + min(row, D)) * 16);
}

// the wave's 32 positions as B operands of k = d: `rows` channel-major (stride ld)
// or position-major (stride 1 between d), times `factor`, PIECES pieces; `other`
// (optional): sum_d x[d] other[d] over the lane's d, for D_i
template <int D, int PIECES, bool POSITION_MAJOR>
__device__ __forceinline__ void column_operand(const float* rows, int64_t stride, int position,
                                               bool live, int half, float factor,
                                               u32x4 (&parts)[(D + 15) / 16][PIECES],
                                               const float* other, float& dot) {
    constexpr int KSTEPS = (D + 15) / 16;
    float raw[KSTEPS][8], second[KSTEPS][8];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int d = min(16 * s + 8 * half + e, D - 1);
            const int64_t at = POSITION_MAJOR ? static_cast<int64_t>(position) * stride + d
                                              : static_cast<int64_t>(d) * stride + position;
            raw[s][e] = rows[at];
            second[s][e] = other != nullptr ? other[at] : 0.f;
        }
    dot = 0.f;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        float values[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool inside = live && 16 * s + 8 * half + e < D;
            values[e] = inside ? raw[s][e] * factor : 0.f;
            dot = fmaf(inside ? raw[s][e] : 0.f, inside ? second[s][e] : 0.f, dot);
        }
        split_eight<PIECES>(values, parts[s]);
    }
}

// grid = (n_tiles, heads); block = 512: wave w owns queries [32 w, 32 w + 32) of the
// tile.  `stats` = [2][heads][ld]: the row log-sum-exp in log2 units, then D.
template <int D>
__global__ __launch_bounds__(kGradSplitThreads) void attention_backward_split_query_kernel(
    const float* __restrict__ qk, const float* __restrict__ out, const float* __restrict__ dout,
    const unsigned char* __restrict__ images, float* __restrict__ dqkv,
    float* __restrict__ stats, int64_t ld, int channels, int heads,
    const int32_t* __restrict__ tiles) {
    typedef GradImages<D> Images;
    constexpr int KSTEPS = (D + 15) / 16;
    constexpr int STAGE = kSplitStage;
    static_assert(D > 32 && D <= 48, "two m-tiles of 32 rows, three k-steps of 16");
    __shared__ __align__(16) unsigned char lds[Images::kQueryPass];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int column = lane & 31;
    const int half = lane >> 5;
    const int head = blockIdx.y;
    const Tile span = load_tile(tiles, blockIdx.x);
    const int count = span.count;
    const int q0 = span.first + 32 * wave;
    const bool working = q0 < count;                       // wave-uniform
    const int query = q0 + column;
    const bool live = query < count;
    const int stages = (count + STAGE - 1) / STAGE;
    const int64_t stage_stride = static_cast<int64_t>(heads) * Images::kStageBytes;
    const unsigned char* source =
        images + (static_cast<int64_t>((span.offset >> 6) + span.segment) * heads + head) *
                     Images::kStageBytes;
    const float scale = 1.f / sqrtf(static_cast<float>(D));
    const int64_t head_row = static_cast<int64_t>(head * D) * ld + span.offset;

    // B operands of the wave's queries: Q^T in log2 units (three pieces), dO^T (two),
    // and D_i from the same loads
    u32x4 bq[KSTEPS][3], bdo[KSTEPS][2];
    float delta, unused;
    {
        const int at = min(query, count - 1);
        column_operand<D, 3, false>(qk + head_row, ld, at, live, half, kGradLog2e * scale, bq,
                                    nullptr, unused);
        column_operand<D, 2, false>(dout + head_row, ld, at, live, half, 1.f, bdo,
                                    out + head_row, delta);
        delta += __shfl_xor(delta, 32);
    }

    // S^T of the block of 32 keys at `local` of the staged keys, in log2 units
    auto scores = [&](int local) {
        f32x16 s16;
#pragma unroll
        for (int r = 0; r < 16; ++r) s16[r] = 0.f;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            u32x4 ak[3];
#pragma unroll
            for (int piece = 0; piece < 3; ++piece)
                ak[piece] = row_fragment<D>(lds + Images::kKey + piece * Images::kRowBytes, s,
                                            half, local + column);
            s16 = split_product<3>(ak, bq[s], s16);
        }
        return s16;
    };

    // ---- first walk: the row log-sum-exp (per-lane online maximum and sum over the
    // lane's keys, the two halves combined at the end)
    float top = -INFINITY, total = 0.f;
    {
        StageCopy<Images::kScoreBytes> copy;
        copy.fetch(source, tid);
#pragma unroll 1
        for (int stage = 0; stage < stages; ++stage) {
            __syncthreads();
            copy.put(lds, tid);
            __syncthreads();
            if (stage + 1 < stages) copy.fetch(source + (stage + 1) * stage_stride, tid);
            if (!working) continue;
#pragma unroll 1
            for (int local = 0; local < STAGE; local += 32) {
                const int key0 = stage * STAGE + local;
                if (key0 >= count) break;
                f32x16 s16 = scores(local);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (key0 + 8 * (r >> 2) + 4 * half + (r & 3) >= count) s16[r] = -INFINITY;
                float high = top;
#pragma unroll
                for (int r = 0; r < 16; ++r) high = fmaxf(high, s16[r]);
                if (high > -INFINITY) {            // (a lane whose keys are all masked so far)
                    float sum = total * __builtin_amdgcn_exp2f(top - high);
#pragma unroll
                    for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f(s16[r] - high);
                    total = sum;
                    top = high;
                }
            }
        }
    }
    float lse = 0.f;
    if (working) {
        const float high = fmaxf(top, __shfl_xor(top, 32));        // finite: key 0 exists
        const float mine = top == -INFINITY ? 0.f : total * __builtin_amdgcn_exp2f(top - high);
        lse = high + log2f(mine + __shfl_xor(mine, 32));
        if (half == 0 && live) {
            stats[static_cast<int64_t>(head) * ld + span.offset + query] = lse;
            stats[static_cast<int64_t>(heads + head) * ld + span.offset + query] = delta;
        }
    }

    // ---- second walk: dQ^T[d][query] = sum_key K^T[d][key] dS^T[key][query]
    f32x16 dq[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[m][r] = 0.f;
    {
        StageCopy<Images::kQueryPass> copy;
        copy.fetch(source, tid);
#pragma unroll 1
        for (int stage = 0; stage < stages; ++stage) {
            __syncthreads();
            copy.put(lds, tid);
            __syncthreads();
            if (stage + 1 < stages) copy.fetch(source + (stage + 1) * stage_stride, tid);
            if (!working) continue;
#pragma unroll 1
            for (int local = 0; local < STAGE; local += 32) {
                const int key0 = stage * STAGE + local;
                if (key0 >= count) break;
                f32x16 s16 = scores(local);
                f32x16 dp16;
#pragma unroll
                for (int r = 0; r < 16; ++r) dp16[r] = 0.f;
#pragma unroll
                for (int s = 0; s < KSTEPS; ++s) {
                    u32x4 av[2];
#pragma unroll
                    for (int piece = 0; piece < 2; ++piece)
                        av[piece] = row_fragment<D>(
                            lds + Images::kValue + piece * Images::kRowBytes, s, half,
                            local + column);
                    dp16 = split_product<2>(av, bdo[s], dp16);
                }
                // a key past the segment: probability 0 (selected)
                u32x4 bds[2][2];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    float ds[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int r = 8 * ks + e;
                        const float p = key0 + 8 * (r >> 2) + 4 * half + (r & 3) < count
                                            ? __builtin_amdgcn_exp2f(s16[r] - lse)
                                            : 0.f;
                        ds[e] = p * (dp16[r] - delta);
                    }
                    split_eight<2>(ds, bds[ks]);
                }
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        u32x4 akt[2];
#pragma unroll
                        for (int piece = 0; piece < 2; ++piece)
                            akt[piece] = turned_fragment<D>(
                                lds + Images::kKeyTurned + piece * Images::kTurnedBytes, local,
                                ks, half, 32 * m + column);
                        dq[m] = split_product<2>(akt, bds[ks], dq[m]);
                    }
            }
        }
    }
    if (!working || !live) return;
    float* dq_rows = dqkv + head_row;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = 32 * m + 8 * (r >> 2) + 4 * half + (r & 3);
            if (d < D) dq_rows[static_cast<int64_t>(d) * ld + query] = dq[m][r] * scale;
        }
}

// grid = (n_tiles, heads); block = 512: wave w owns keys [32 w, 32 w + 32) of the tile
// and walks the segment's queries, 64 to a stage.
template <int D>
__global__ __launch_bounds__(kGradSplitThreads) void attention_backward_split_key_kernel(
    const float* __restrict__ qk, const float* __restrict__ v,
    const unsigned char* __restrict__ images, float* __restrict__ dqkv,
    const float* __restrict__ stats, int64_t ld, int channels, int heads,
    const int32_t* __restrict__ tiles) {
    typedef GradImages<D> Images;
    constexpr int KSTEPS = (D + 15) / 16;
    constexpr int STAGE = kSplitStage;
    static_assert(D > 32 && D <= 48, "two m-tiles of 32 rows, three k-steps of 16");
    __shared__ __align__(16) unsigned char lds[Images::kKeyPass];
    __shared__ __align__(16) float rows_lds[2][STAGE];        // log-sum-exp, D of the stage

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int column = lane & 31;
    const int half = lane >> 5;
    const int head = blockIdx.y;
    const Tile span = load_tile(tiles, blockIdx.x);
    const int count = span.count;
    const int k0 = span.first + 32 * wave;
    const bool working = k0 < count;                       // wave-uniform
    const int key = k0 + column;
    const bool live = key < count;
    const int stages = (count + STAGE - 1) / STAGE;
    const int64_t stage_stride = static_cast<int64_t>(heads) * Images::kStageBytes;
    const unsigned char* source =
        images + (static_cast<int64_t>((span.offset >> 6) + span.segment) * heads + head) *
                     Images::kStageBytes + Images::kQueryPass;
    const float scale = 1.f / sqrtf(static_cast<float>(D));
    const int64_t head_row = static_cast<int64_t>(head * D) * ld + span.offset;

    // B operands of the wave's keys: K^T (three pieces; Q carries the scale), V^T (two)
    u32x4 bk[KSTEPS][3], bv[KSTEPS][2];
    {
        float unused;
        const int at = min(key, count - 1);
        column_operand<D, 3, false>(qk + static_cast<int64_t>(channels) * ld + head_row, ld, at,
                                    live, half, 1.f, bk, nullptr, unused);
        column_operand<D, 2, true>(v + static_cast<int64_t>(span.offset) * channels + head * D,
                                   channels, at, live, half, 1.f, bv, nullptr, unused);
    }
    // (threads 0 .. 127 carry the stage's log-sum-exp and D; a query past the segment
    // reads the last one's, and its probability is selected to 0)
    const float* stat_row =
        stats + static_cast<int64_t>((tid >> 6 & 1) * heads + head) * ld + span.offset;
    auto fetch_stat = [&](int stage) {
        return tid < 2 * STAGE ? stat_row[min(stage * STAGE + (tid & 63), count - 1)] : 0.f;
    };

    f32x16 dk[2], dv[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            dk[m][r] = 0.f;
            dv[m][r] = 0.f;
        }
    StageCopy<Images::kKeyPass> copy;
    copy.fetch(source, tid);
    float stat = fetch_stat(0);
#pragma unroll 1
    for (int stage = 0; stage < stages; ++stage) {
        __syncthreads();
        copy.put(lds, tid);
        if (tid < 2 * STAGE) rows_lds[tid >> 6][tid & 63] = stat;
        __syncthreads();
        if (stage + 1 < stages) {
            copy.fetch(source + (stage + 1) * stage_stride, tid);
            stat = fetch_stat(stage + 1);
        }
        if (!working) continue;
#pragma unroll 1
        for (int local = 0; local < STAGE; local += 32) {
            const int query0 = stage * STAGE + local;
            if (query0 >= count) break;
            f32x16 s16, dp16;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s16[r] = 0.f;
                dp16[r] = 0.f;
            }
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) {
                u32x4 aq[3], ado[2];
#pragma unroll
                for (int piece = 0; piece < 3; ++piece)
                    aq[piece] = row_fragment<D>(lds + Images::kQuery + piece * Images::kRowBytes,
                                                s, half, local + column);
#pragma unroll
                for (int piece = 0; piece < 2; ++piece)
                    ado[piece] = row_fragment<D>(lds + Images::kDout + piece * Images::kRowBytes,
                                                 s, half, local + column);
                s16 = split_product<3>(aq, bk[s], s16);
                dp16 = split_product<2>(ado, bv[s], dp16);
            }
            // register r: query query0 + 8 (r / 4) + 4 half + r % 4, key `column`; a query
            // past the segment contributes nothing (selected)
            u32x4 bp[2][2], bds[2][2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                float p[8], ds[8];
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const int within = local + 16 * ks + 8 * g + 4 * half;
                    const float4 lse4 = *reinterpret_cast<const float4*>(&rows_lds[0][within]);
                    const float4 delta4 = *reinterpret_cast<const float4*>(&rows_lds[1][within]);
                    const float lse[4] = {lse4.x, lse4.y, lse4.z, lse4.w};
                    const float delta[4] = {delta4.x, delta4.y, delta4.z, delta4.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = 8 * ks + 4 * g + i;
                        const float weight = stage * STAGE + within + i < count
                                                 ? __builtin_amdgcn_exp2f(s16[r] - lse[i])
                                                 : 0.f;
                        p[4 * g + i] = weight;
                        ds[4 * g + i] = weight * (dp16[r] - delta[i]);
                    }
                }
                split_eight<2>(p, bp[ks]);
                split_eight<2>(ds, bds[ks]);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    u32x4 adot[2], aqt[2];
#pragma unroll
                    for (int piece = 0; piece < 2; ++piece) {
                        adot[piece] = turned_fragment<D>(
                            lds + Images::kDoutTurned + piece * Images::kTurnedBytes, local, ks,
                            half, 32 * m + column);
                        aqt[piece] = turned_fragment<D>(
                            lds + Images::kQueryTurned + piece * Images::kTurnedBytes, local, ks,
                            half, 32 * m + column);
                    }
                    dv[m] = split_product<2>(adot, bp[ks], dv[m]);
                    dk[m] = split_product<2>(aqt, bds[ks], dk[m]);
                }
        }
    }
    if (!working || !live) return;
    float* dk_rows = dqkv + static_cast<int64_t>(channels) * ld + head_row;
    float* dv_rows = dqkv + static_cast<int64_t>(2 * channels) * ld + head_row;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = 32 * m + 8 * (r >> 2) + 4 * half + (r & 3);
            if (d < D) {
                dk_rows[static_cast<int64_t>(d) * ld + key] = dk[m][r] * scale;
                dv_rows[static_cast<int64_t>(d) * ld + key] = dv[m][r];
            }
        }
}

}  // namespace emph

using namespace emph;

extern "C" {

int64_t emph_attention_backward_split_workspace(int64_t ld, int32_t heads) {
    if (ld <= 0 || heads <= 0) return 0;
    return 2 * static_cast<int64_t>(heads) * ld;
}

int64_t emph_attention_backward_split_bytes(int64_t ld, int32_t n_segments, int32_t channels,
                                            int32_t heads) {
    if (ld <= 0 || n_segments < 0 || channels != 80 || heads != 2) return -1;
    const int64_t slots = ld / kSplitStage + n_segments + 1;
    return slots * heads * GradImages<40>::kStageBytes;
}

int emph_attention_backward_split(const float* qk, const float* v, const float* out,
                                  const float* dout, float* dqkv, int64_t ld, int32_t channels,
                                  int32_t heads, const int32_t* tiles, int32_t n_tiles,
                                  int32_t tile_n, void* images, float* workspace,
                                  void* stream) {
    EMPH_REQUIRE(channels == 80 && heads == 2, EMPH_ERANGE,
                 "emph_attention_backward_split: channels %d, heads %d (only 80 channels in 2 "
                 "heads of 40)", channels, heads);
    EMPH_REQUIRE(tile_n == kGradSplitTile, EMPH_EINVAL,
                 "emph_attention_backward_split: tile_n %d (a workgroup owns %d positions)",
                 tile_n, kGradSplitTile);
    EMPH_REQUIRE(n_tiles >= 0 && ld > 0, EMPH_EINVAL, "emph_attention_backward_split: bad shape");
    EMPH_REQUIRE(ld < kGradSplitColumns, EMPH_ERANGE,
                 "emph_attention_backward_split: ld >= 2^28");
    if (n_tiles == 0) return EMPH_OK;
    EMPH_REQUIRE(qk && v && out && dout && dqkv && tiles && images && workspace, EMPH_EINVAL,
                 "emph_attention_backward_split: null pointer");
    EMPH_REQUIRE((reinterpret_cast<uintptr_t>(images) & 15) == 0, EMPH_EINVAL,
                 "emph_attention_backward_split: images must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned char* bytes = static_cast<unsigned char*>(images);
    EMPH_LAUNCH(grad_images_kernel<40>, dim3(n_tiles, kGradSplitTile / kSplitStage, heads),
                dim3(256), 0, s, qk, v, dout, ld, channels, heads, tiles, bytes);
    int status = check_launch("emph_attention_backward_split (images)");
    if (status != EMPH_OK) return status;
    dim3 grid(n_tiles, heads);
    EMPH_LAUNCH(attention_backward_split_query_kernel<40>, grid, dim3(kGradSplitThreads), 0, s,
                qk, out, dout, static_cast<const unsigned char*>(bytes), dqkv, workspace, ld,
                channels, heads, tiles);
    status = check_launch("emph_attention_backward_split (queries)");
    if (status != EMPH_OK) return status;
    EMPH_LAUNCH(attention_backward_split_key_kernel<40>, grid, dim3(kGradSplitThreads), 0, s, qk,
                v, static_cast<const unsigned char*>(bytes), dqkv, workspace, ld, channels,
                heads, tiles);
    return check_launch("emph_attention_backward_split (keys)");
}

}  // extern "C"
