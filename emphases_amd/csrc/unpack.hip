// Packed feature matrix -> the contiguous tensors of a feature cache.
//
// The front-end leaves the features of a batch as ONE matrix [rows][ld] whose
// segments start on multiples of 16 columns (batch.py).  A feature cache holds
// one C-contiguous [rows_k][frames_k] tensor per file and feature
// (emphases/data/preprocess/mels.py:62-86, loudness.py:27-51), which the
// reference gets from a computation per file.  emph_unpack_rows takes the whole
// batch apart in one launch: the blocks land back to back (at offsets the caller
// chooses) in one buffer, which then crosses to the host in one copy.
//
// It is a ragged copy, bound by memory bandwidth: every float is read once and
// written once.  A block is walked as the FLAT run of its rows_k * frames_k
// output floats.  That run starts wherever the caller put it, so up to three
// head floats bring it to a 16-byte boundary, the bulk is stored as aligned
// float4 (1 KiB per wave instruction) and up to three tail floats finish it.
// The four source floats of a stored float4 lie side by side in one row of x
// unless the float4 straddles the end of a row: they are fetched with one
// 16-byte load that asks for 4-byte alignment only (source rows start 64-byte
// aligned, but the row length frames_k is arbitrary, so the source of an aligned
// destination is not aligned from the second row on), or one float at a time
// across the row ends (every float4 of a block with fewer than four frames).
#include "common.h"

namespace emph {

namespace {

constexpr int kUnpackThreads = 256;
// float4 stores of one unit of work: four per lane
constexpr int kUnpackUnit = 4 * kUnpackThreads;
// workgroups a launch aims for (eight per compute unit) and the most / fewest
// that share one block
constexpr int kUnpackGroups = 2048;
constexpr int kUnpackMostSlices = 64;
constexpr int kUnpackFewestSlices = 8;

// a float4 that promises 4-byte alignment only: one global_load_dwordx4
typedef float float4_unaligned __attribute__((ext_vector_type(4), aligned(4)));
typedef float float4_aligned __attribute__((ext_vector_type(4), aligned(16)));

// grid.x = table entry, grid.y = slices of the entry: slice j takes the units j,
// j + grid.y, ... of the block's float4 run, so a 30 000-frame file is spread over
// every slice while all but the first slice of a 2-frame file leave at once.
__global__ __launch_bounds__(kUnpackThreads) void unpack_rows_kernel(
    const float* __restrict__ x, int64_t ld, const int64_t* __restrict__ table,
    float* __restrict__ out) {
    const int64_t* entry = table + 5 * static_cast<int64_t>(blockIdx.x);
    const int64_t column = entry[0], frames = entry[1], row = entry[2], rows = entry[3],
                  target = entry[4];
    // an entry that does not lie inside a row of x, or with a negative field, is not
    // touched (the table is device memory: the host side cannot refuse it)
    if (column < 0 || frames <= 0 || row < 0 || rows <= 0 || target < 0 ||
        frames > ld - column || rows > (int64_t{1} << 31) / frames)
        return;
    const uint32_t width = static_cast<uint32_t>(frames);
    const uint32_t total = static_cast<uint32_t>(rows * frames);   // < 2^31
    const float* __restrict__ source = x + row * ld + column;
    float* __restrict__ y = out + target;
    const uint32_t misplaced = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(y) >> 2) & 3u;
    const uint32_t head = min(total, (4u - misplaced) & 3u);
    const uint32_t body = (total - head) >> 2;                     // float4 stores
    const uint32_t tail = total - head - 4u * body;
    const uint32_t t = threadIdx.x;

    if (blockIdx.y == 0 && t < 8) {
        // lanes 0..2: the head, lanes 4..6: the tail
        const bool at_end = t >= 4;
        const uint32_t k = t & 3u;
        if (k < (at_end ? tail : head)) {
            const uint32_t i = at_end ? head + 4u * body + k : k;
            const uint32_t r = i / width;
            y[i] = source[r * ld + (i - r * width)];
        }
    }
    const uint32_t units = (body + kUnpackUnit - 1) / kUnpackUnit;
    for (uint32_t unit = blockIdx.y; unit < units; unit += gridDim.y) {
#pragma unroll
        for (int trip = 0; trip < kUnpackUnit / kUnpackThreads; ++trip) {
            const uint32_t q = unit * kUnpackUnit + trip * kUnpackThreads + t;
            if (q >= body) continue;
            const uint32_t i = head + 4u * q;
            uint32_t r = i / width;
            uint32_t f = i - r * width;
            const float* p = source + r * ld + f;
            float4_aligned value;
            if (f + 4u <= width) {
                value = *reinterpret_cast<const float4_unaligned*>(p);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    value[j] = source[r * ld + f];
                    if (++f == width) {
                        f = 0;
                        ++r;
                    }
                }
            }
            *reinterpret_cast<float4_aligned*>(y + i) = value;
        }
    }
}

}  // namespace

}  // namespace emph

using namespace emph;

extern "C" {

int emph_unpack_rows(const float* x, int64_t ld, const int64_t* table, int32_t n, float* out,
                     void* stream) {
    EMPH_REQUIRE(n >= 0, EMPH_EINVAL, "emph_unpack_rows: %d entries", n);
    if (n == 0) return EMPH_OK;
    EMPH_REQUIRE(x && table && out, EMPH_EINVAL, "emph_unpack_rows: null pointer");
    EMPH_REQUIRE(ld > 0, EMPH_EINVAL, "emph_unpack_rows: leading dimension %lld",
                 static_cast<long long>(ld));
    EMPH_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(table) & 7) == 0,
                 EMPH_EINVAL, "emph_unpack_rows: misaligned pointer");
    EMPH_REQUIRE(n <= (1 << 20), EMPH_ERANGE, "emph_unpack_rows: %d entries in one launch", n);
    int slices = kUnpackGroups / n;
    slices = slices < kUnpackFewestSlices ? kUnpackFewestSlices : slices;
    slices = slices > kUnpackMostSlices ? kUnpackMostSlices : slices;
    EMPH_LAUNCH(unpack_rows_kernel, dim3(static_cast<unsigned>(n), slices),
                dim3(kUnpackThreads), 0, static_cast<hipStream_t>(stream), x, ld, table, out);
    return check_launch("emph_unpack_rows");
}

}  // extern "C"
