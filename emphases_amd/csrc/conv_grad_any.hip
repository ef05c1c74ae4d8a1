// Weight and bias gradient of Conv1d(c_in, c_out, k, padding='same') for every
// shape of the operator seams (c_in, c_out 1..128, k in {1, 3, 5, 7}) over
// ragged segments on the fp32 matrix cores (v_mfma_f32_16x16x4_f32):
// conv_grad.hip's formulation with the shape as an argument.
//
// Replaces what autograd computes for the `weight` and `bias` of a
// torch.nn.Conv1d of the convolution model (emphases/model/core.py:17-37,
// model/layers/convolution.py:25-28) in the configurations of
// config/downsample/ and config/hparam-search/ (channels 64 / 128, kernel
// sizes 1 / 5 / 7):
//   dW[co][ci][j] = sum_t dy[co][t] x[ci][t + j - H]     db[co] = sum_t dy[co][t]
// with H = (k - 1) / 2, summed inside every segment, x zero outside its segment.
//
// Formulation: a GEMM  D[co, (j, ci)] = DY[co, t] X[t, (j, ci)]  with
// MT = ceil(c_out / 16) m-tiles, k taps x CT = ceil(c_in / 16) n-tiles + ONE
// extra n-tile whose B operand is a row of ones (its column 0 is db),
// K = positions.
//   * A workgroup (4 waves) walks a contiguous run of 64-position tiles of the
//     tile table.  Per tile it stages dy [16 MT x 64] and x [16 CT x (64 + 2 H)]
//     (H halo columns each side, zero outside the segment - selected, never
//     multiplied; a row past c_out / c_in repeats the last one: it reaches
//     only rows / columns of D that are never written) in LDS; the next tile's
//     values are requested into registers before this tile's MFMAs and
//     committed to LDS after them.
//   * THE SPLIT.  A wave keeps 4 n-tiles: MT x 4 accumulators, 128 registers a
//     lane at MT = 8, next to <= 67 of staged loads - inside the 512 of a wave
//     that has its SIMD to itself (256 threads a workgroup, one workgroup a
//     CU).  A workgroup therefore covers 16 n-tiles, and the k CT + 1 n-tiles
//     (57 at 128 x 128 x 7) are cut into slices of 16 over grid.y - not into
//     more passes over the positions: every slice walks the same run of tiles
//     once and stages the same dy / x (second and later slices read them from
//     L2).  (80, 80, 3) is exactly one slice.  LDS: (16 MT + 16 CT + 16) rows of
//     76 floats, 83 KB at 128 x 128 (dynamic, of the CU's 160 KB).  Row stride
//     76 = 4 mod 8 like conv_grad.hip's 68: A and B fragments are ds_read_b32
//     with the same bank pattern.
//   * Instantiated for every MT in 1..8 and for CT rounded up to 1, 5, 6 or 8
//     staged channel tiles (the n-tiles follow the true ceil(c_in / 16): a
//     rounded-up CT stages rows no n-tile reads).
//   * Workgroup (part, slice) writes its n-tiles of slab `part`
//     [c_out (k c_in) + c_out] in the layout of (weight, bias); the slices of
//     a part write disjoint elements and together all of them.  A second
//     launch adds the slabs in a fixed order that depends on the number of
//     parts, i.e. on the tile count, alone: no atomics, no hand-off between
//     workgroups, the same bits every launch.  The workspace is one slab per
//     part: up to 256 x (c_out k c_in + c_out) floats, 117 MB at 128 x 128 x 7
//     (7.4 MB at 80 x 80 x 3); it scales with k c_in c_out, not with the batch.
#include <stdint.h>

#include "common.h"
#include "conv_grad.h"

namespace emph {

typedef float any_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAnyStride = 76;           // floats per LDS row (64 + 6 used)
constexpr int kAnyWaveTiles = 4;         // n-tiles a wave accumulates
constexpr int kAnySlice = 4 * kAnyWaveTiles;
constexpr int kAnyMaxChannels = 128;
constexpr int kAnyHaloLoads = kAnyMaxChannels * 6 / 256;            // 3

// grid = (parts, slices); block = 256; dynamic LDS (16 MT + 16 CT + 16) * 76 floats
template <int MT, int CT>
__global__ __launch_bounds__(256) void conv_weight_grad_any_kernel(
    const float* __restrict__ dy, int64_t ld_dy, const float* __restrict__ x, int64_t ldx,
    int c_in, int c_out, int kernel_size, const int32_t* __restrict__ tiles, int n_tiles,
    int tiles_per_part, float* __restrict__ slabs) {
    constexpr int S = kAnyStride;
    constexpr int NT = kAnyWaveTiles;
    constexpr int DY_LOADS = 16 * MT * kGradTile / 256;    // 4 MT
    constexpr int X_LOADS = 16 * CT * kGradTile / 256;     // 4 CT
    constexpr int rows = 16 * CT;                 // staged rows of x
    extern __shared__ float any_lds[];
    const int ct_count = (c_in + 15) >> 4;
    const int halo = (kernel_size - 1) >> 1;
    const int last_q = kernel_size * ct_count;    // the n-tile of ones
    float* dy_lds = any_lds;
    float* x_lds = any_lds + 16 * MT * S;         // rows + 16 rows

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int loader = tid >> 6;                  // (a vector value: row addresses per lane)
    const int kk = lane >> 4;
    const int col = lane & 15;
    const int first_tile = blockIdx.x * tiles_per_part;
    const int last_tile = min(first_tile + tiles_per_part, n_tiles);
    const int halo_entries = 16 * ct_count * 2 * halo;

    // the extra n-tile: row 0 ones (-> db in column 0), rows 1..15 zeros
    for (int index = tid; index < 16 * S; index += 256)
        x_lds[rows * S + index] = index < S ? 1.f : 0.f;

    float dy_next[DY_LOADS], x_next[X_LOADS], halo_next[kAnyHaloLoads];
    auto request = [&](int tile_index) {
        const Tile tile = load_tile(tiles, tile_index);
        const int t = tile.first + lane;
        const bool inside = t < tile.count;
        const float* dy_base = dy + tile.offset + t;
        const float* x_base = x + tile.offset + t;
#pragma unroll
        for (int i = 0; i < DY_LOADS; ++i) {
            const int row = min(4 * i + loader, c_out - 1);
            dy_next[i] = inside ? dy_base[static_cast<int64_t>(row) * ld_dy] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < X_LOADS; ++i) {
            const int row = min(4 * i + loader, c_in - 1);
            x_next[i] = inside ? x_base[static_cast<int64_t>(row) * ldx] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kAnyHaloLoads; ++i) {
            const int index = tid + 256 * i;
            halo_next[i] = 0.f;
            if (index < halo_entries) {
                const int row = index / (2 * halo);
                const int h = index - row * 2 * halo;
                const int u = h < halo ? tile.first - halo + h : tile.first + kGradTile + h - halo;
                if (u >= 0 && u < tile.count && row < c_in)
                    halo_next[i] = x[static_cast<int64_t>(row) * ldx + tile.offset + u];
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < DY_LOADS; ++i) dy_lds[(4 * i + loader) * S + lane] = dy_next[i];
#pragma unroll
        for (int i = 0; i < X_LOADS; ++i)
            x_lds[(4 * i + loader) * S + lane + halo] = x_next[i];
#pragma unroll
        for (int i = 0; i < kAnyHaloLoads; ++i) {
            const int index = tid + 256 * i;
            if (index < halo_entries) {
                const int row = index / (2 * halo);
                const int h = index - row * 2 * halo;
                x_lds[row * S + (h < halo ? h : kGradTile + h)] = halo_next[i];
            }
        }
    };

    // this wave's n-tiles: q = j * ct_count + ct (tap j, channels 16 ct ..),
    // q = last_q is the tile of ones; x[ci][t + j - H] lies at column t + j
    const int q0 = blockIdx.y * kAnySlice + wave * NT;
    int b_offset[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int q = q0 + i;
        const int j = q / ct_count, ct = q - j * ct_count;
        b_offset[i] = q < last_q ? (16 * ct + col) * S + kk + j : (rows + col) * S + kk;
    }
    const int a_offset = col * S + kk;

    any_f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[m][i] = any_f32x4{0.f, 0.f, 0.f, 0.f};

    if (first_tile < last_tile) request(first_tile);
    for (int tile_index = first_tile; tile_index < last_tile; ++tile_index) {
        __syncthreads();                  // the previous tile's reads are done
        commit();
        __syncthreads();
        if (tile_index + 1 < last_tile) request(tile_index + 1);
        if (q0 > last_q) continue;                             // wave-uniform
#pragma unroll 2
        for (int step = 0; step < kGradTile / 4; ++step) {
            float a[MT], b[NT];
#pragma unroll
            for (int m = 0; m < MT; ++m) a[m] = dy_lds[a_offset + 16 * m * S + 4 * step];
#pragma unroll
            for (int i = 0; i < NT; ++i)
                b[i] = q0 + i <= last_q ? x_lds[b_offset[i] + 4 * step] : 0.f;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                if (q0 + i > last_q) continue;                 // wave-uniform
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    acc[m][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a[m], b[i], acc[m][i], 0, 0, 0);
            }
        }
    }

    // ---- the slab: D[row = 4 kk + r][col] of m-tile m, n-tile q
    const int64_t weight_count = static_cast<int64_t>(c_out) * c_in * kernel_size;
    float* slab = slabs + static_cast<int64_t>(blockIdx.x) * (weight_count + c_out);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int q = q0 + i;
        if (q > last_q) continue;
        const int j = q / ct_count, ct = q - j * ct_count;
        const int ci = 16 * ct + col;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * m + 4 * kk + r;
                if (co >= c_out) continue;
                if (q == last_q) {
                    if (col == 0) slab[weight_count + co] = acc[m][i][r];
                } else if (ci < c_in) {
                    slab[(static_cast<int64_t>(co) * c_in + ci) * kernel_size + j] =
                        acc[m][i][r];
                }
            }
    }
}

// conv_grad.hip's fixed-order sum with the bias count as an argument: a
// workgroup owns 64 consecutive elements, wave w adds slabs w, w + 4, ... in
// index order, then ((w0 + w1) + (w2 + w3)).
__global__ __launch_bounds__(256) void conv_weight_grad_any_sum_kernel(
    const float* __restrict__ slabs, int parts, int64_t weight_count, int bias_count,
    float* __restrict__ dweight, float* __restrict__ dbias) {
    __shared__ float partial[4][64];
    const int64_t total = weight_count + bias_count;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 64 + lane;
    float sum = 0.f;
    if (i < total) {
        const float* column = slabs + i;
        int part = wave;
        for (; part + 28 < parts; part += 32) {
            float value[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) value[k] = column[(part + 4 * k) * total];
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += value[k];
        }
        for (; part < parts; part += 4) sum += column[part * total];
    }
    partial[wave][lane] = sum;
    __syncthreads();
    if (wave != 0 || i >= total) return;
    sum = (partial[0][lane] + partial[1][lane]) + (partial[2][lane] + partial[3][lane]);
    if (i < weight_count) dweight[i] = sum; else dbias[i - weight_count] = sum;
}

template <int MT, int CT>
int launch_weight_grad_any_tiles(const float* dy, int64_t ld_dy, const float* x, int64_t ldx,
                                 int c_in, int c_out, int kernel_size, const int32_t* tiles,
                                 int n_tiles, int per_part, int parts, float* slabs,
                                 hipStream_t stream) {
    static LdsReservation reservation;
    constexpr size_t lds = static_cast<size_t>(16 * MT + 16 * CT + 16) * kAnyStride * 4;
    if (int status = reserve_lds(
            reservation, reinterpret_cast<const void*>(&conv_weight_grad_any_kernel<MT, CT>),
            lds, "emph_conv_weight_grad_any"))
        return status;
    const int ct_count = (c_in + 15) / 16;
    const int slices = (kernel_size * ct_count + 1 + kAnySlice - 1) / kAnySlice;
    EMPH_LAUNCH((conv_weight_grad_any_kernel<MT, CT>), dim3(parts, slices), dim3(256), lds,
                stream, dy, ld_dy, x, ldx, c_in, c_out, kernel_size, tiles, n_tiles, per_part,
                slabs);
    return check_launch("emph_conv_weight_grad_any");
}

template <int MT, typename... Args>
int launch_weight_grad_any(int c_in, Args... args) {
    const int ct_count = (c_in + 15) / 16;
    if (ct_count <= 1) return launch_weight_grad_any_tiles<MT, 1>(args...);
    if (ct_count <= 5) return launch_weight_grad_any_tiles<MT, 5>(args...);
    if (ct_count <= 6) return launch_weight_grad_any_tiles<MT, 6>(args...);
    return launch_weight_grad_any_tiles<MT, 8>(args...);
}

static bool weight_grad_any_shape(int c_in, int c_out, int kernel_size) {
    return c_in >= 1 && c_in <= kAnyMaxChannels && c_out >= 1 && c_out <= kAnyMaxChannels &&
           (kernel_size == 1 || kernel_size == 3 || kernel_size == 5 || kernel_size == 7);
}

}  // namespace emph

using namespace emph;

extern "C" {

int64_t emph_conv_weight_grad_any_workspace(int32_t c_in, int32_t c_out, int32_t kernel_size,
                                            int32_t n_tiles) {
    if (!weight_grad_any_shape(c_in, c_out, kernel_size) || n_tiles <= 0) return 0;
    return static_cast<int64_t>(emph_conv_weight_grad_parts(n_tiles)) *
           (static_cast<int64_t>(c_out) * c_in * kernel_size + c_out);
}

int emph_conv_weight_grad_any(const float* dy, int64_t ld_dy, const float* x, int64_t ldx,
                              int32_t c_in, int32_t c_out, int32_t kernel_size,
                              const int32_t* tiles, int32_t n_tiles, int32_t tile_n,
                              float* workspace, float* dweight, float* dbias, void* stream) {
    EMPH_REQUIRE(weight_grad_any_shape(c_in, c_out, kernel_size), EMPH_ERANGE,
                 "emph_conv_weight_grad_any: c_in %d, c_out %d (1..128), kernel_size %d "
                 "(1, 3, 5, 7)", c_in, c_out, kernel_size);
    EMPH_REQUIRE(tile_n == kGradTile, EMPH_ERANGE,
                 "emph_conv_weight_grad_any: tile_n %d (64)", tile_n);
    EMPH_REQUIRE(dy && x && tiles && workspace && dweight && dbias, EMPH_EINVAL,
                 "emph_conv_weight_grad_any: null pointer");
    EMPH_REQUIRE(n_tiles > 0, EMPH_EINVAL, "emph_conv_weight_grad_any: no tiles");
    EMPH_REQUIRE(ldx > 0 && ldx < (int64_t{1} << 28) && ld_dy > 0 &&
                     ld_dy < (int64_t{1} << 28),
                 EMPH_ERANGE, "emph_conv_weight_grad_any: leading dimension out of range");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int per_part = grad_tiles_per_part(n_tiles);
    const int parts = emph_conv_weight_grad_parts(n_tiles);
    int status = EMPH_OK;
    switch ((c_out + 15) / 16) {
#define EMPH_ANY_CASE(MT)                                                                  \
    case MT:                                                                               \
        status = launch_weight_grad_any<MT>(c_in, dy, ld_dy, x, ldx, c_in, c_out,         \
                                            kernel_size, tiles, n_tiles, per_part, parts,  \
                                            workspace, s);                                 \
        break;
        EMPH_ANY_CASE(1) EMPH_ANY_CASE(2) EMPH_ANY_CASE(3) EMPH_ANY_CASE(4)
        EMPH_ANY_CASE(5) EMPH_ANY_CASE(6) EMPH_ANY_CASE(7) EMPH_ANY_CASE(8)
#undef EMPH_ANY_CASE
    }
    if (status) return status;
    const int64_t weight_count = static_cast<int64_t>(c_out) * c_in * kernel_size;
    EMPH_LAUNCH(conv_weight_grad_any_sum_kernel,
                dim3(static_cast<unsigned>((weight_count + c_out + 63) / 64)), dim3(256), 0, s,
                workspace, parts, weight_count, c_out, dweight, dbias);
    return check_launch("emph_conv_weight_grad_any");
}

}  // extern "C"
