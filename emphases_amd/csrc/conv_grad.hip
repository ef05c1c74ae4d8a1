// Weight and bias gradient of Conv1d(c_in, 80, 3, padding='same') over ragged
// segments on the fp32 matrix cores (v_mfma_f32_16x16x4_f32).
//
// Replaces what autograd computes for the `weight` and `bias` of every
// torch.nn.Conv1d of the convolution model (emphases/model/core.py:17-21,
// model/layers/convolution.py:25-28) under `loss.backward()`
// (emphases/train/core.py:136):
//   dW[co][ci][j] = sum_t dy[co][t] x[ci][t + j - 1]     db[co] = sum_t dy[co][t]
// summed inside every segment, x zero outside its segment.
//
// Formulation: a GEMM  D[co, (j, ci)] = DY[co, t] X[t, (j, ci)]  with M = 80
// (5 m-tiles), N = 3 taps x CT tiles of 16 input channels + ONE extra n-tile
// whose B operand is a column of ones (its column 0 is db), K = positions.
//   * A workgroup (4 waves) walks a contiguous run of 64-position tiles of the
//     tile table.  Per tile it stages dy [80 x 64] and x [16 CT x 66] (one
//     halo column each side, zero outside the segment - selected, never
//     multiplied) in LDS; the next tile's values are requested into registers
//     before this tile's MFMAs and committed to LDS after them.
//   * The n-tiles are split over the waves (NT = 4 or 5 each); a wave keeps
//     its 5 x NT accumulators (80 - 100 registers a lane) for the whole run.
//     Row stride 68 floats: A and B fragments are conflict-free ds_read_b32.
//   * The workgroup writes ONE slab [80 (3 c_in) + 80] in the layout of
//     (weight, bias).  A second launch adds the slabs in a fixed order: no
//     atomics, no hand-off between workgroups, the same bits every launch.
#include <stdint.h>

#include "common.h"
#include "conv_grad.h"

namespace emph {

typedef float grad_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGradStride = 68;          // floats per LDS row (66 used)

__host__ __device__ constexpr int grad_wave_tiles(int ct) { return (3 * ct + 1 + 3) / 4; }

// grid = parts; block = 256
template <int CT>
__global__ __launch_bounds__(256) void conv_weight_grad_kernel(
    const float* __restrict__ dy, int64_t ld_dy, const float* __restrict__ x, int64_t ldx,
    int c_in, const int32_t* __restrict__ tiles, int n_tiles, int tiles_per_part,
    float* __restrict__ slabs) {
    constexpr int S = kGradStride;
    constexpr int NT = grad_wave_tiles(CT);
    constexpr int ROWS = 16 * CT;                 // staged rows of x
    constexpr int DY_LOADS = kGradOut * kGradTile / 256;   // 20
    constexpr int X_LOADS = ROWS * kGradTile / 256;        // 4 CT
    __shared__ float dy_lds[kGradOut * S];
    __shared__ float x_lds[(ROWS + 16) * S];      // + the n-tile of ones

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kk = lane >> 4;
    const int col = lane & 15;
    const int first_tile = blockIdx.x * tiles_per_part;
    const int last_tile = min(first_tile + tiles_per_part, n_tiles);

    // the extra n-tile: row 0 ones (-> db in column 0), rows 1..15 zeros
    for (int index = tid; index < 16 * S; index += 256)
        x_lds[ROWS * S + index] = index < S ? 1.f : 0.f;

    float dy_next[DY_LOADS], x_next[X_LOADS], halo_next = 0.f;
    auto request = [&](int tile_index) {
        const Tile tile = load_tile(tiles, tile_index);
        const int t = tile.first + lane;
        const bool inside = t < tile.count;
        const float* dy_base = dy + tile.offset + t;
        const float* x_base = x + tile.offset + t;
#pragma unroll
        for (int i = 0; i < DY_LOADS; ++i) {
            const int row = 4 * i + (tid >> 6);
            dy_next[i] = inside ? dy_base[static_cast<int64_t>(row) * ld_dy] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < X_LOADS; ++i) {
            const int row = 4 * i + (tid >> 6);
            x_next[i] = (inside && row < c_in) ? x_base[static_cast<int64_t>(row) * ldx] : 0.f;
        }
        if (tid < 2 * ROWS) {
            const int row = tid >> 1;
            const int u = (tid & 1) ? tile.first + kGradTile : tile.first - 1;
            halo_next = (u >= 0 && u < tile.count && row < c_in)
                            ? x[static_cast<int64_t>(row) * ldx + tile.offset + u]
                            : 0.f;
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < DY_LOADS; ++i)
            dy_lds[(4 * i + (tid >> 6)) * S + lane] = dy_next[i];
#pragma unroll
        for (int i = 0; i < X_LOADS; ++i)
            x_lds[(4 * i + (tid >> 6)) * S + lane + 1] = x_next[i];
        if (tid < 2 * ROWS)
            x_lds[(tid >> 1) * S + ((tid & 1) ? kGradTile + 1 : 0)] = halo_next;
    };

    // this wave's n-tiles: q = j * CT + ct (tap j, channels 16 ct ..), q = 3 CT
    // is the tile of ones
    int b_offset[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int q = wave * NT + i;
        const int j = q / CT, ct = q - j * CT;
        b_offset[i] = q < 3 * CT ? (16 * ct + col) * S + kk + j : (ROWS + col) * S + kk;
    }
    const int a_offset = col * S + kk;

    grad_f32x4 acc[5][NT];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[m][i] = grad_f32x4{0.f, 0.f, 0.f, 0.f};

    if (first_tile < last_tile) request(first_tile);
    for (int tile_index = first_tile; tile_index < last_tile; ++tile_index) {
        __syncthreads();                  // the previous tile's reads are done
        commit();
        __syncthreads();
        if (tile_index + 1 < last_tile) request(tile_index + 1);
#pragma unroll 4
        for (int step = 0; step < kGradTile / 4; ++step) {
            float a[5], b[NT];
#pragma unroll
            for (int m = 0; m < 5; ++m) a[m] = dy_lds[a_offset + 16 * m * S + 4 * step];
#pragma unroll
            for (int i = 0; i < NT; ++i) b[i] = x_lds[b_offset[i] + 4 * step];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                if (wave * NT + i > 3 * CT) continue;          // wave-uniform
#pragma unroll
                for (int m = 0; m < 5; ++m)
                    acc[m][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a[m], b[i], acc[m][i], 0, 0, 0);
            }
        }
    }

    // ---- the slab: D[row = 4 kk + r][col] of m-tile m, n-tile q
    const int64_t weight_count = static_cast<int64_t>(kGradOut) * c_in * 3;
    float* slab = slabs + static_cast<int64_t>(blockIdx.x) * (weight_count + kGradOut);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int q = wave * NT + i;
        if (q > 3 * CT) continue;
        const int j = q / CT, ct = q - j * CT;
        const int ci = 16 * ct + col;
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * m + 4 * kk + r;
                if (q == 3 * CT) {
                    if (col == 0) slab[weight_count + co] = acc[m][i][r];
                } else if (ci < c_in) {
                    slab[(static_cast<int64_t>(co) * c_in + ci) * 3 + j] = acc[m][i][r];
                }
            }
    }
}

// out[i] = the sum of slabs[.][i] in a fixed order: a workgroup owns 64
// consecutive elements, wave w adds slabs w, w + 4, ... in index order (the
// loads of eight slabs in flight at once), then ((w0 + w1) + (w2 + w3)).  The
// order depends on `parts` alone, i.e. on the tile count, never on the launch.
__global__ __launch_bounds__(256) void conv_weight_grad_sum_kernel(
    const float* __restrict__ slabs, int parts, int64_t weight_count,
    float* __restrict__ dweight, float* __restrict__ dbias) {
    __shared__ float partial[4][64];
    const int64_t total = weight_count + kGradOut;
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

int conv_weight_grad_sum(const float* slabs, int parts, int64_t weight_count, float* dweight,
                         float* dbias, hipStream_t stream, const char* what) {
    const int64_t total = weight_count + kGradOut;
    EMPH_LAUNCH(conv_weight_grad_sum_kernel, dim3(static_cast<unsigned>((total + 63) / 64)),
                dim3(256), 0, stream, slabs, parts, weight_count, dweight, dbias);
    return check_launch(what);
}

}  // namespace emph

using namespace emph;

extern "C" {

int32_t emph_conv_weight_grad_parts(int32_t n_tiles) {
    if (n_tiles <= 0) return 0;
    const int per_part = grad_tiles_per_part(n_tiles);
    return (n_tiles + per_part - 1) / per_part;
}

int emph_conv_weight_grad(const float* dy, int64_t ld_dy, const float* x, int64_t ldx,
                          int32_t c_in, int32_t c_out, int32_t kernel_size,
                          const int32_t* tiles, int32_t n_tiles, int32_t tile_n,
                          float* workspace, float* dweight, float* dbias, void* stream) {
    EMPH_REQUIRE(dy && x && tiles && workspace && dweight && dbias, EMPH_EINVAL,
                 "emph_conv_weight_grad: null pointer");
    EMPH_REQUIRE(c_out == kGradOut && kernel_size == 3, EMPH_ERANGE,
                 "emph_conv_weight_grad: c_out %d, kernel_size %d (80, 3)", c_out,
                 kernel_size);
    EMPH_REQUIRE(c_in >= 1 && c_in <= 96, EMPH_ERANGE,
                 "emph_conv_weight_grad: c_in %d not in 1..96", c_in);
    EMPH_REQUIRE(tile_n == kGradTile, EMPH_ERANGE,
                 "emph_conv_weight_grad: tile_n %d (64)", tile_n);
    EMPH_REQUIRE(n_tiles > 0, EMPH_EINVAL, "emph_conv_weight_grad: no tiles");
    EMPH_REQUIRE(ldx > 0 && ldx < (int64_t{1} << 28) && ld_dy > 0 &&
                     ld_dy < (int64_t{1} << 28),
                 EMPH_ERANGE, "emph_conv_weight_grad: leading dimension out of range");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int per_part = grad_tiles_per_part(n_tiles);
    const int parts = emph_conv_weight_grad_parts(n_tiles);
    if (c_in <= 80) {
        EMPH_LAUNCH(conv_weight_grad_kernel<5>, dim3(parts), dim3(256), 0, s, dy, ld_dy, x,
                    ldx, c_in, tiles, n_tiles, per_part, workspace);
    } else {
        EMPH_LAUNCH(conv_weight_grad_kernel<6>, dim3(parts), dim3(256), 0, s, dy, ld_dy, x,
                    ldx, c_in, tiles, n_tiles, per_part, workspace);
    }
    if (int status = check_launch("emph_conv_weight_grad")) return status;
    return conv_weight_grad_sum(workspace, parts, static_cast<int64_t>(kGradOut) * c_in * 3,
                                dweight, dbias, s, "emph_conv_weight_grad");
}

}  // extern "C"
