// The bf16x3 side of the training step (precision='bf16x3' of emphases_amd.train):
//
//   emph_conv_weight_grad_split   weight and bias gradient of Conv1d(80, 80, 3, 'same')
//                                 on the bf16 matrix pipe - the contract of
//                                 emph_conv_weight_grad (conv_grad.hip) for
//                                 c_in = c_out = 80, k = 3;
//   emph_conv_split_pack_device   emph_conv_split_pack (conv_split.hip, host) of many
//                                 layers straight from the flat parameter buffer, in
//                                 one launch - what emph_take does for the fp32 packs.
//
// 'bf16x3' as in conv_split.hip: hi = bf16(a), lo = bf16(a - hi), both rounded to
// nearest, the subtraction in fp32; a term is lo.hi + hi.lo + hi.hi, accumulated in
// fp32.
//
// Weight gradient: the GEMM of conv_grad.hip,
//     D[co, (j, ci)] = sum_t dy[co][t] x[ci][t + j - 1],   M = 80, N = 3 x 80, K = positions
// on v_mfma_f32_16x16x32_bf16: five m-tiles, fifteen n-tiles (tap j, channels
// 16 ct .. 16 ct + 15) split over four waves (4, 4, 4, 3), a k-step is 32 positions.
//   * A workgroup walks a contiguous run of 64-position tiles of the tile table and
//     keeps its 5 x 4 accumulators for the whole run.  Per tile it stages dy and x as
//     bf16 pieces in LDS, [piece][channel][72] (64 positions + 8 of padding): both
//     operands are contiguous along the contraction axis, so the fragment of a lane -
//     eight consecutive positions of channel lane % 16 - is one 16-byte read, and rows
//     144 bytes apart put the sixteen channels of a quarter-wave on sixteen different
//     16-byte bank groups.
//   * The +-1 shift of a tap would break the 16-byte alignment of that read, so x is
//     staged THREE times, image j holding x[ci][t + j - 1] at position t: every value
//     is split once and its two pieces written to (up to) three places.  Positions
//     outside the segment hold zeros - selected while loading, never multiplied.
//   * db[co] = sum_t dy[co][t] stays fp32: a thread adds up the dy values it stages
//     (its lane's position of twenty rows), a wave adds its lanes at the end.
//   * The next tile's values are requested into registers before this tile's MFMAs
//     and committed to LDS after them, as in conv_grad.hip.
//   * One slab per workgroup in the layout of (weight, bias); conv_grad.hip's second
//     launch adds the slabs in a fixed order.  No atomics: the same bits every launch.
#include <stdint.h>

#include "common.h"
#include "conv_grad.h"
#include "split.h"

namespace emph {

typedef float gs_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGsChannels = 80;
constexpr int kGsRowBytes = 144;                              // 72 bf16, 64 used
constexpr int kGsPieceBytes = kGsChannels * kGsRowBytes;      // 11 520
constexpr int kGsImageBytes = 2 * kGsPieceBytes;              // high, low
constexpr int kGsLdsBytes = 4 * kGsImageBytes;                // dy + three images of x: 90 KB
constexpr int kGsWaveTiles = 4;                               // n-tiles per wave (15 in all)
constexpr int kGsLoads = kGsChannels * kGradTile / 256;       // 20 rows per thread

__device__ __forceinline__ gs_f32x4 mfma16(const u32x4& a, const u32x4& b, const gs_f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// grid = parts; block = 256
__global__ __launch_bounds__(256) void conv_weight_grad_split_kernel(
    const float* __restrict__ dy, int64_t ld_dy, const float* __restrict__ x, int64_t ldx,
    const int32_t* __restrict__ tiles, int n_tiles, int tiles_per_part,
    float* __restrict__ slabs) {
    extern __shared__ __align__(16) unsigned char grad_split_lds[];
    unsigned char* dy_image = grad_split_lds;                     // [piece][80][144 B]
    unsigned char* x_image = grad_split_lds + kGsImageBytes;      // [tap][piece][80][144 B]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kk = lane >> 4;
    const int col = lane & 15;
    const int first_tile = blockIdx.x * tiles_per_part;
    const int last_tile = min(first_tile + tiles_per_part, n_tiles);

    float dy_next[kGsLoads], x_next[kGsLoads], halo_next = 0.f;
    float bias_sum[kGsLoads];
#pragma unroll
    for (int i = 0; i < kGsLoads; ++i) bias_sum[i] = 0.f;

    auto request = [&](int tile_index) {
        const Tile tile = load_tile(tiles, tile_index);
        const int t = tile.first + lane;
        const bool inside = t < tile.count;
        const float* dy_base = dy + tile.offset + t;
        const float* x_base = x + tile.offset + t;
#pragma unroll
        for (int i = 0; i < kGsLoads; ++i) {
            const int row = 4 * i + wave;
            dy_next[i] = inside ? dy_base[static_cast<int64_t>(row) * ld_dy] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kGsLoads; ++i) {
            const int row = 4 * i + wave;
            x_next[i] = inside ? x_base[static_cast<int64_t>(row) * ldx] : 0.f;
        }
        if (tid < 2 * kGsChannels) {
            const int row = tid >> 1;
            const int u = (tid & 1) ? tile.first + kGradTile : tile.first - 1;
            halo_next = (u >= 0 && u < tile.count)
                            ? x[static_cast<int64_t>(row) * ldx + tile.offset + u]
                            : 0.f;
        }
    };
    // position `lane` of row 4 i + wave: dy once, x into image 1 at its own position,
    // into image 0 one to the right and into image 2 one to the left; the two columns
    // that come from the neighbouring tiles are the halo threads'
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < kGsLoads; ++i) {
            const int row = 4 * i + wave;
            bias_sum[i] += dy_next[i];
            uint32_t pieces[2];
            split_pair<2>(dy_next[i], x_next[i], pieces);
            unsigned char* dy_row = dy_image + row * kGsRowBytes + 2 * lane;
            unsigned char* x_row = x_image + row * kGsRowBytes + 2 * lane;
#pragma unroll
            for (int piece = 0; piece < 2; ++piece) {
                const uint16_t dy_bits = static_cast<uint16_t>(pieces[piece] & 0xffffu);
                const uint16_t x_bits = static_cast<uint16_t>(pieces[piece] >> 16);
                const int at = piece * kGsPieceBytes;
                *reinterpret_cast<uint16_t*>(dy_row + at) = dy_bits;
                *reinterpret_cast<uint16_t*>(x_row + kGsImageBytes + at) = x_bits;
                if (lane + 1 < kGradTile)
                    *reinterpret_cast<uint16_t*>(x_row + at + 2) = x_bits;
                if (lane >= 1)
                    *reinterpret_cast<uint16_t*>(x_row + 2 * kGsImageBytes + at - 2) = x_bits;
            }
        }
        if (tid < 2 * kGsChannels) {
            uint32_t pieces[2];
            split_pair<2>(halo_next, 0.f, pieces);
            unsigned char* target = x_image + (tid >> 1) * kGsRowBytes +
                                    ((tid & 1) ? 2 * kGsImageBytes + 2 * (kGradTile - 1) : 0);
            *reinterpret_cast<uint16_t*>(target) = static_cast<uint16_t>(pieces[0] & 0xffffu);
            *reinterpret_cast<uint16_t*>(target + kGsPieceBytes) =
                static_cast<uint16_t>(pieces[1] & 0xffffu);
        }
    };

    // this wave's n-tiles: q = 5 j + ct (tap j, channels 16 ct ..), q < 15
    int b_offset[kGsWaveTiles];
#pragma unroll
    for (int i = 0; i < kGsWaveTiles; ++i) {
        const int q = min(wave * kGsWaveTiles + i, 14);
        const int j = q / 5, ct = q - 5 * j;
        b_offset[i] = j * kGsImageBytes + (16 * ct + col) * kGsRowBytes + 16 * kk;
    }
    const int a_offset = col * kGsRowBytes + 16 * kk;

    gs_f32x4 acc[5][kGsWaveTiles];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int i = 0; i < kGsWaveTiles; ++i) acc[m][i] = gs_f32x4{0.f, 0.f, 0.f, 0.f};

    if (first_tile < last_tile) request(first_tile);
    for (int tile_index = first_tile; tile_index < last_tile; ++tile_index) {
        __syncthreads();                  // the previous tile's reads are done
        commit();
        __syncthreads();
        if (tile_index + 1 < last_tile) request(tile_index + 1);
#pragma unroll
        for (int step = 0; step < kGradTile / 32; ++step) {
            u32x4 a_high[5], a_low[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                const unsigned char* source =
                    dy_image + a_offset + 16 * m * kGsRowBytes + 64 * step;
                a_high[m] = *reinterpret_cast<const u32x4*>(source);
                a_low[m] = *reinterpret_cast<const u32x4*>(source + kGsPieceBytes);
            }
#pragma unroll
            for (int i = 0; i < kGsWaveTiles; ++i) {
                if (wave * kGsWaveTiles + i > 14) continue;        // wave-uniform
                const unsigned char* source = x_image + b_offset[i] + 64 * step;
                const u32x4 b_high = *reinterpret_cast<const u32x4*>(source);
                const u32x4 b_low = *reinterpret_cast<const u32x4*>(source + kGsPieceBytes);
#pragma unroll
                for (int m = 0; m < 5; ++m) {
                    // the small products first
                    acc[m][i] = mfma16(a_low[m], b_high, acc[m][i]);
                    acc[m][i] = mfma16(a_high[m], b_low, acc[m][i]);
                    acc[m][i] = mfma16(a_high[m], b_high, acc[m][i]);
                }
            }
        }
    }

    // ---- the slab: D[row = 4 kk + r][col] of m-tile m, n-tile q
    constexpr int64_t kWeights = static_cast<int64_t>(kGradOut) * kGsChannels * 3;
    float* slab = slabs + static_cast<int64_t>(blockIdx.x) * (kWeights + kGradOut);
#pragma unroll
    for (int i = 0; i < kGsWaveTiles; ++i) {
        const int q = wave * kGsWaveTiles + i;
        if (q > 14) continue;
        const int j = q / 5, ct = q - 5 * j;
        const int ci = 16 * ct + col;
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * m + 4 * kk + r;
                slab[(static_cast<int64_t>(co) * kGsChannels + ci) * 3 + j] = acc[m][i][r];
            }
    }
    // db: the wave's 64 positions of row 4 i + wave, a butterfly over the lanes (the
    // same order every launch)
#pragma unroll
    for (int i = 0; i < kGsLoads; ++i) {
        float sum = bias_sum[i];
#pragma unroll
        for (int distance = 32; distance >= 1; distance >>= 1)
            sum += __shfl_xor(sum, distance, 64);
        if (lane == 0) slab[kWeights + 4 * i + wave] = sum;
    }
}

// Element `i` of the launch is source weight index[i] (-1: zero) of pack i / 23 040:
// i % 23 040 = (group of (tap, block, m-tile)) * 512 + lane * 8 + e, whose two pieces
// lie 1 KB apart (emph_conv_split_pack).  Rounding in integer arithmetic, as the host
// function does it: the bytes are the same for every finite weight.
constexpr int kPackElements = 3 * 5 * 3 * 512;                  // per layer

__device__ __forceinline__ uint32_t pack_bf16_bits(float value) {
    uint32_t bits = __float_as_uint(value);
    bits += 0x7fffu + ((bits >> 16) & 1u);
    return bits >> 16;
}

__global__ __launch_bounds__(256) void conv_split_pack_kernel(
    const float* __restrict__ weights, const int32_t* __restrict__ index,
    uint16_t* __restrict__ packs, int64_t count) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= count) return;
    const int32_t from = index[i];
    const float weight = from < 0 ? 0.f : weights[from];
    const uint32_t high = pack_bf16_bits(weight);
    const uint32_t low = pack_bf16_bits(weight - __uint_as_float(high << 16));
    const int64_t group = i >> 9;
    const int64_t at = group * 1024 + (i & 511);
    packs[at] = static_cast<uint16_t>(high);
    packs[at + 512] = static_cast<uint16_t>(low);
}

}  // namespace emph

using namespace emph;

extern "C" {

int emph_conv_weight_grad_split(const float* dy, int64_t ld_dy, const float* x, int64_t ldx,
                                int32_t c_in, int32_t c_out, int32_t kernel_size,
                                const int32_t* tiles, int32_t n_tiles, int32_t tile_n,
                                float* workspace, float* dweight, float* dbias, void* stream) {
    EMPH_REQUIRE(dy && x && tiles && workspace && dweight && dbias, EMPH_EINVAL,
                 "emph_conv_weight_grad_split: null pointer");
    EMPH_REQUIRE(c_in == kGsChannels && c_out == kGradOut && kernel_size == 3, EMPH_ERANGE,
                 "emph_conv_weight_grad_split: c_in %d, c_out %d, kernel_size %d (80, 80, 3)",
                 c_in, c_out, kernel_size);
    EMPH_REQUIRE(tile_n == kGradTile, EMPH_ERANGE,
                 "emph_conv_weight_grad_split: tile_n %d (64)", tile_n);
    EMPH_REQUIRE(n_tiles > 0, EMPH_EINVAL, "emph_conv_weight_grad_split: no tiles");
    EMPH_REQUIRE(ldx > 0 && ldx < (int64_t{1} << 28) && ld_dy > 0 &&
                     ld_dy < (int64_t{1} << 28),
                 EMPH_ERANGE, "emph_conv_weight_grad_split: leading dimension out of range");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int per_part = grad_tiles_per_part(n_tiles);
    const int parts = emph_conv_weight_grad_parts(n_tiles);
    auto kernel = conv_weight_grad_split_kernel;
    static LdsReservation reserved;
    if (int status = reserve_lds(reserved, reinterpret_cast<const void*>(kernel), kGsLdsBytes,
                                 "emph_conv_weight_grad_split"))
        return status;
    EMPH_LAUNCH(kernel, dim3(parts), dim3(256), kGsLdsBytes, s, dy, ld_dy, x, ldx, tiles,
                n_tiles, per_part, workspace);
    if (int status = check_launch("emph_conv_weight_grad_split")) return status;
    return conv_weight_grad_sum(workspace, parts,
                                static_cast<int64_t>(kGradOut) * kGsChannels * 3, dweight,
                                dbias, s, "emph_conv_weight_grad_split");
}

int emph_conv_split_pack_device(const float* weights, const int32_t* index, void* packs,
                                int32_t count, void* stream) {
    if (count == 0) return EMPH_OK;
    EMPH_REQUIRE(weights && index && packs, EMPH_EINVAL,
                 "emph_conv_split_pack_device: null pointer");
    EMPH_REQUIRE(count > 0 && count <= 4096, EMPH_ERANGE,
                 "emph_conv_split_pack_device: %d packs (0 .. 4096)", count);
    EMPH_REQUIRE((reinterpret_cast<uintptr_t>(packs) & 15) == 0, EMPH_EINVAL,
                 "emph_conv_split_pack_device: the packs must be 16-byte aligned");
    const int64_t elements = static_cast<int64_t>(count) * kPackElements;
    EMPH_LAUNCH(conv_split_pack_kernel, dim3(static_cast<unsigned>((elements + 255) / 256)),
                dim3(256), 0, static_cast<hipStream_t>(stream), weights, index,
                static_cast<uint16_t*>(packs), elements);
    return check_launch("emph_conv_split_pack_device");
}

}  // extern "C"
