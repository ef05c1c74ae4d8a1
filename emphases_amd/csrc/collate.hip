// Batch assembly for training from a device-resident dataset: one launch copies
// the frames and the targets of every item of a batch out of the resident
// arrays into the packed ragged layout of a plan (batch.py) and zeroes every
// other column of both outputs, so the caller needs no memset and may reuse
// dirty buffers.  What the reference does on the host per step
// (emphases/data/collate.py:11-78) and `Trainer.prepare` after it.
//
// Plain copies: no LDS, no arithmetic on the values (the result is bitwise the
// source).  The grid covers the packed column range, not the items: a
// workgroup owns 256 columns (a quad of 4 per lane) of 16 channels (4 per
// wave), so 75 utterances x 1 000 frames x 80 channels are 1 480 workgroups
// of 16-byte loads and stores, each wave-instruction 1 KiB of one row.
#include "common.h"

namespace emph {

constexpr int kCollateFields = 6;     // int64 per item, include/emphases_hip.h
constexpr int kCollateColumns = 256;  // columns per wave: a quad per lane
constexpr int kCollateChannels = 16;  // channels per workgroup: 4 per wave

// Where a packed axis of an item lives: (source, count, packed) fields.
struct CollateAxis {
    int source, count, packed;
};
constexpr CollateAxis kCollateFrames = {0, 1, 2};
constexpr CollateAxis kCollateWords = {3, 4, 5};

// Last item whose first packed column is <= column (the items rise along the
// packed axis), -1 when there is none.
__device__ __forceinline__ int collate_find(const int64_t* __restrict__ items, int n_items,
                                            int field, int64_t column) {
    int low = 0, high = n_items;
    while (low < high) {
        const int middle = (low + high) >> 1;
        if (items[static_cast<int64_t>(middle) * kCollateFields + field] <= column)
            low = middle + 1;
        else
            high = middle;
    }
    return low - 1;
}

// Source index of one packed column, -1 for a column that holds no data (LEAD,
// TAIL, padding, a gap) or whose item does not lie inside the source.
__device__ __forceinline__ int64_t collate_source(const int64_t* __restrict__ items,
                                                  int n_items, CollateAxis axis,
                                                  int64_t column, int64_t limit) {
    const int item = collate_find(items, n_items, axis.packed, column);
    if (item < 0) return -1;
    const int64_t* row = items + static_cast<int64_t>(item) * kCollateFields;
    const int64_t source = row[axis.source], count = row[axis.count];
    const int64_t local = column - row[axis.packed];
    if (count <= 0 || count > limit || source < 0 || source > limit - count) return -1;
    return local < count ? source + local : -1;
}

__global__ __launch_bounds__(256) void collate_kernel(
    const float* __restrict__ features, int64_t ld_cache, const float* __restrict__ targets,
    int64_t total_words, const int64_t* __restrict__ items, int n_items, int channels,
    int64_t ld_frames, int64_t ld_words, float* __restrict__ out_features,
    float* __restrict__ out_targets, int64_t frame_blocks, int groups, int frames_vector,
    int words_vector) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t block = blockIdx.x;
    const bool words = block >= frame_blocks * groups;

    // The rows this wave moves: [first, last) step 4 of x (row length ldx,
    // `limit` valid columns) into y (row length ldy), and the quad's column.
    const float* x;
    float* y;
    int64_t ldx, ldy, limit, column;
    int first, last, vector;
    CollateAxis axis;
    if (words) {
        // one row: the four waves take four column blocks
        column = ((block - frame_blocks * groups) * 4 + wave) * kCollateColumns + 4 * lane;
        x = targets, y = out_targets, ldx = 0, ldy = ld_words, limit = total_words;
        first = 0, last = 1, vector = words_vector, axis = kCollateWords;
    } else {
        const int group = static_cast<int>(block % groups);
        column = (block / groups) * kCollateColumns + 4 * lane;
        x = features, y = out_features, ldx = ld_cache, ldy = ld_frames, limit = ld_cache;
        first = group * kCollateChannels + wave;
        last = min(channels, (group + 1) * kCollateChannels);
        vector = frames_vector, axis = kCollateFrames;
    }
    if (column >= ldy || first >= last) return;       // (ldy is a multiple of 4)

    // A quad that lies inside one item with a 16-byte aligned source moves as
    // one load and one store per row; any other quad column by column.
    int64_t source[4] = {-1, -1, -1, -1};
    bool whole = false;
    const int item = collate_find(items, n_items, axis.packed, column);
    if (item >= 0 && vector) {
        const int64_t* row = items + static_cast<int64_t>(item) * kCollateFields;
        const int64_t from = row[axis.source], count = row[axis.count];
        const int64_t local = column - row[axis.packed];
        whole = count > 0 && count <= limit && from >= 0 && from <= limit - count &&
                local + 4 <= count && ((from + local) & 3) == 0;
        source[0] = from + local;
    }
    if (!whole) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            source[j] = collate_source(items, n_items, axis, column + j, limit);
    }

    constexpr int kRows = kCollateChannels / 4;
    float4 value[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int c = first + 4 * r;
        value[r] = float4{0.f, 0.f, 0.f, 0.f};
        if (c >= last) continue;
        const float* line = x + static_cast<int64_t>(c) * ldx;
        if (whole) {
            value[r] = *reinterpret_cast<const float4*>(line + source[0]);
        } else {
            if (source[0] >= 0) value[r].x = line[source[0]];
            if (source[1] >= 0) value[r].y = line[source[1]];
            if (source[2] >= 0) value[r].z = line[source[2]];
            if (source[3] >= 0) value[r].w = line[source[3]];
        }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int c = first + 4 * r;
        if (c < last)
            *reinterpret_cast<float4*>(y + static_cast<int64_t>(c) * ldy + column) = value[r];
    }
}

}  // namespace emph

using namespace emph;

extern "C" {

int emph_collate(const float* features, int64_t ld_cache, const float* targets,
                 int64_t total_words, const int64_t* items, int32_t n_items,
                 int32_t channels, int64_t ld_frames, int64_t ld_words,
                 float* out_features, float* out_targets, void* stream) {
    EMPH_REQUIRE(features && targets && items && out_features && out_targets, EMPH_EINVAL,
                 "emph_collate: null pointer");
    EMPH_REQUIRE(n_items > 0, EMPH_EINVAL, "emph_collate: %d items", n_items);
    EMPH_REQUIRE(channels > 0 && ld_cache > 0 && total_words > 0 && ld_frames > 0 &&
                     ld_words > 0 && ld_frames % 4 == 0 && ld_words % 4 == 0 &&
                     (reinterpret_cast<uintptr_t>(out_features) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(out_targets) & 15) == 0,
                 EMPH_EINVAL,
                 "emph_collate: bad shape (positive sizes; packed rows of whole, "
                 "16-byte aligned quads)");
    const int64_t frame_blocks = (ld_frames + kCollateColumns - 1) / kCollateColumns;
    const int64_t word_blocks = (ld_words + 4 * kCollateColumns - 1) / (4 * kCollateColumns);
    const int groups = (channels + kCollateChannels - 1) / kCollateChannels;
    const int64_t blocks = frame_blocks * groups + word_blocks;
    EMPH_REQUIRE(blocks < (int64_t{1} << 31), EMPH_ERANGE,
                 "emph_collate: %lld workgroups", static_cast<long long>(blocks));
    const int frames_vector =
        (reinterpret_cast<uintptr_t>(features) & 15) == 0 && ld_cache % 4 == 0;
    const int words_vector = (reinterpret_cast<uintptr_t>(targets) & 15) == 0;
    EMPH_LAUNCH(collate_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                static_cast<hipStream_t>(stream), features, ld_cache, targets, total_words,
                items, n_items, channels, ld_frames, ld_words, out_features, out_targets,
                frame_blocks, groups, frames_vector, words_vector);
    return check_launch("emph_collate");
}

}  // extern "C"
