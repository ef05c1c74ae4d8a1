// Backward of the log-mel front-end (emph_logmel, csrc/frontend.hip): the
// gradient of the packed audio from the gradient of the mel rows.
//
// Replaces what autograd does in the reference for mels.from_audio
// (data/preprocess/mels.py:16-109): the backward of F.pad(reflect), torch.stft,
// sqrt, the mel matmul, clamp and log.  Nothing is saved by the forward: the
// spectrum of every frame is recomputed here from the audio.  This file stands
// alone: it reads the table of emph_frontend_table_fill (window, W1024^k) but
// shares no code with frontend.hip and brings its own 1024-point transform.
// The window differentiated is the one in the table passed: ops.py passes the
// forward's table with the reference's float32 torch.hann_window in its place.
//
// Per frame f of a chunk (p = the reflect-padded chunk, w = periodic Hann,
// B = the mel basis as row runs, g = the cotangent of the log-mel rows):
//
//   X_k  = sum_n w_n p[160 f + n] e^{-2 pi i k n / 1024}        k = 0..512
//   s_k  = sqrt(re_k^2 + im_k^2 + 1e-6)
//   m_r  = sum_k B[r,k] s_k              rising k within the row's run
//   q_r  = m_r >= 1e-5 ? g_r / m_r : 0   (torch's clamp(min=): passes at >=)
//   G_k  = sum_r B[r,k] q_r              rising r
//   D_k  = G_k X_k / s_k                 (s_k >= 1e-3; X = 0 gives exactly 0)
//   t_n  = w_n Re sum_{k=0}^{512} D_k e^{+2 pi i k n / 1024}    n = 0..1023
//
// ONE-SIDED WEIGHTING.  t is an unnormalised inverse transform in which each
// of the 513 one-sided bins counts ONCE: no factor 2 on bins 1..511 (the
// forward produced each of them once) and no 1/N.  With im_k = -sum w p sin as
// the forward defines it, t_n = w_n sum_k (dre_k cos - dim_k sin)(2 pi k n /
// 1024).  It is computed as Re FFT(conj(D) padded with zeros to 1024 bins) with
// the same forward transform that makes X.
//
// Then, per chunk of S samples and F frames,
//
//   P[j]  = sum_f t^(f)[j - 160 f]                               overlap-add
//   dx[n] = P[n + 432] + P[432 - n] (1 <= n <= 432)
//                      + P[2 (S - 1) - n + 432] (S - 433 <= n <= S - 2)
//
// the exact adjoint of the index map of the forward's load_edge; what would
// flow into the 432 zeros around an utterance (emphases/core.py:357-358) is
// dropped, and only chunk samples backed by audio are written.
//
// TWO LAUNCHES.  A: one workgroup per tile of 8 frames (the forward's tile
// table).  It transforms the frames one after the other and overlap-adds
// their t INSIDE THE TILE, in LDS: 7 * 160 + 1024 = 2144 floats per tile go to
// the workspace instead of 8 * 1024.  B: one workgroup per tile again, for the
// samples the tile owns ([160 f0, 160 (f0 + 8)), the chunk's last tile up to
// S): it gathers P from at most two neighbouring tiles and folds the mirrors.
//
// ORDER OF EVERY SUM (no atomics; every element is written by one thread; a
// chunk's gradient is the same bits alone or anywhere in a batch):
//   m_r          rising k, one thread per row, one fma per bin
//   G_k          rising r, one thread per bin
//   transforms   radix-4 Stockham, the same butterflies for every frame
//   P in a tile  rising f (the tile's frames are added one after the other)
//   P[j]         the earlier tile's part + the later tile's part
//   dx[n]        (P[n + 432] + left mirror) + right mirror
// Tiles start at multiples of 8 frames of their chunk, so all of this depends
// on the chunk alone.
//
// WORKSPACE CAP.  The tile table is walked in runs of kRunSlots - 2 = 4094
// tiles; launch A of a run also recomputes the tile on either side, whose
// parts launch B of the run reads.  The workspace is min(n_tiles, kRunSlots)
// slots of 2144 floats: at most 4096 * 2144 floats = 33.5 MiB, whatever the
// batch.  The tiles of a chunk must be consecutive rows of the tile table in
// rising order, as emph_plan_tiles makes them.
//
// WHERE THE TIME GOES.  64 x 10 s = 64 000 frames: launch A 783 us (two runs),
// launch B 22 us, the forward 55 us.  Launch A sits on LDS: the two 1024-point
// complex transforms of a frame are five radix-4 passes each through LDS, 211
// KB of LDS traffic a frame against 20 KB of HBM traffic a tile - by counting,
// bounds of 194 us (LDS), 81 us (VALU), 25 us (HBM); it reaches 0.25 of the
// first.  The rest is the 14 workgroup barriers a frame around those round
// trips and the mel stage, which keeps 80 of 256 threads busy.  Launch B is a
// gather of at most six floats per sample.  tools/logmel_backward_bench.py,
// profiles/logmel_backward.json.
#include <math.h>

#include "common.h"

namespace emph {

namespace {

constexpr int kGradFrames = 8;                                  // emph_frontend_block()
constexpr int kTileStep = kGradFrames * kHop;                   // samples a tile owns
constexpr int kTileSpan = (kGradFrames - 1) * kHop + kFft;      // floats of P per tile
constexpr int kRunSlots = 4096;                                 // workspace cap, in tiles
constexpr int kRunTiles = kRunSlots - 2;

// emph_frontend_table_fill's layout (checked against emph_frontend_table_size)
constexpr int kGradTabWindow = 0;                               // [1024] Hann / 2
constexpr int kGradTabTw = 1024 + 2 * 512 + 2 * 64;             // [514] complex W1024^k
constexpr int kGradTabSize = kGradTabTw + 2 * 514;

// a transform buffer: one complex of padding after every 32
__device__ __forceinline__ int grad_slot(int a) { return a + (a >> 5); }
constexpr int kBufferComplex = 1024 + 32;

struct GradChunk {
    const float* origin;  // address of chunk position 0 (may lie before the buffer)
    int64_t shift;        // audio index of chunk position 0
    int length;           // samples in the chunk
    int r_lo, r_hi;       // chunk positions backed by audio
    int frames;
    int64_t frame_off;
};

__device__ __forceinline__ GradChunk grad_chunk(const float* audio, const int64_t* seg,
                                                int segment) {
    const int64_t* row = seg + static_cast<int64_t>(segment) * EMPH_SEG_FIELDS;
    const int64_t audio_off = row[EMPH_SEG_AUDIO_OFF];
    const int64_t audio_len = row[EMPH_SEG_AUDIO_LEN];
    const int64_t start = row[EMPH_SEG_START];
    const int64_t length = row[EMPH_SEG_LENGTH];
    GradChunk chunk;
    chunk.shift = audio_off + start - kPad;
    chunk.origin = audio + chunk.shift;
    chunk.length = static_cast<int>(length);
    const int64_t lo = kPad - start, hi = audio_len + kPad - start;
    chunk.r_lo = static_cast<int>(lo < 0 ? 0 : (lo > length ? length : lo));
    chunk.r_hi = static_cast<int>(hi < 0 ? 0 : (hi > length ? length : hi));
    chunk.frames = static_cast<int>(row[EMPH_SEG_FRAMES]);
    chunk.frame_off = row[EMPH_SEG_FRAME_OFF];
    return chunk;
}

__device__ __forceinline__ float2 grad_cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// One radix-4 Stockham pass of the forward 1024-point transform, 256 threads,
// one butterfly each: pass LOG (p = 1 << LOG = 1, 4, 16, 64, 256) takes
// x[i + 256 q] W^(q k 256 / p), k = i mod p, to y[4 (i - k) + k + q p].  After
// the five passes the spectrum is in natural order.
template <int LOG>
__device__ __forceinline__ void grad_pass(const float2* x, float2* y, int i, const float2* w) {
    constexpr int p = 1 << LOG;
    const int k = i & (p - 1);
    const int j = ((i - k) << 2) + k;
    float2 u0 = x[grad_slot(i)];
    float2 u1 = x[grad_slot(i + 256)];
    float2 u2 = x[grad_slot(i + 512)];
    float2 u3 = x[grad_slot(i + 768)];
    if (LOG > 0) {
        u1 = grad_cmul(u1, w[0]);
        u2 = grad_cmul(u2, w[1]);
        u3 = grad_cmul(u3, w[2]);
    }
    const float2 v0 = make_float2(u0.x + u2.x, u0.y + u2.y);
    const float2 v1 = make_float2(u0.x - u2.x, u0.y - u2.y);
    const float2 v2 = make_float2(u1.x + u3.x, u1.y + u3.y);
    const float2 v3 = make_float2(u1.y - u3.y, u3.x - u1.x);      // -i (u1 - u3)
    y[grad_slot(j)] = make_float2(v0.x + v2.x, v0.y + v2.y);
    y[grad_slot(j + p)] = make_float2(v1.x + v3.x, v1.y + v3.y);
    y[grad_slot(j + 2 * p)] = make_float2(v0.x - v2.x, v0.y - v2.y);
    y[grad_slot(j + 3 * p)] = make_float2(v1.x - v3.x, v1.y - v3.y);
}

// a -> b -> a -> b -> a -> b: the spectrum of what `a` held is in `b`.  The
// caller has synchronised after writing `a`; the last pass is synchronised here.
__device__ __forceinline__ void grad_transform(float2* a, float2* b, int i,
                                               const float2 (&w)[4][3]) {
    grad_pass<0>(a, b, i, w[0]);
    __syncthreads();
    grad_pass<2>(b, a, i, w[0]);
    __syncthreads();
    grad_pass<4>(a, b, i, w[1]);
    __syncthreads();
    grad_pass<6>(b, a, i, w[2]);
    __syncthreads();
    grad_pass<8>(a, b, i, w[3]);
    __syncthreads();
}

// Launch A.  LDS (floats): two transform buffers, the tile's P, the
// magnitudes, q, the basis' runs (3 x 80 ints) and its mel_nnz values.
constexpr int kLdsBufferA = 0;
constexpr int kLdsBufferB = kLdsBufferA + 2 * kBufferComplex;
constexpr int kLdsP = kLdsBufferB + 2 * kBufferComplex;
constexpr int kLdsMag = kLdsP + kTileSpan;
constexpr int kLdsQ = kLdsMag + 516;
constexpr int kLdsRuns = kLdsQ + kMels;
constexpr int kLdsValues = kLdsRuns + 3 * kMels;

__global__ __launch_bounds__(256) void logmel_backward_frames_kernel(
    const float* __restrict__ audio, const int64_t* __restrict__ seg,
    const int32_t* __restrict__ tiles, int first_tile, const float* __restrict__ table,
    const int32_t* __restrict__ mel_start, const int32_t* __restrict__ mel_count,
    const int32_t* __restrict__ mel_offset, const float* __restrict__ mel_values, int mel_nnz,
    const float* __restrict__ dmel, int64_t ld, int mel_row, float* __restrict__ workspace) {
    extern __shared__ __align__(16) float lds[];
    float2* buffer_a = reinterpret_cast<float2*>(lds + kLdsBufferA);
    float2* buffer_b = reinterpret_cast<float2*>(lds + kLdsBufferB);
    float* part = lds + kLdsP;
    float* mag = lds + kLdsMag;
    float* q = lds + kLdsQ;
    int* run_start = reinterpret_cast<int*>(lds + kLdsRuns);
    int* run_count = run_start + kMels;
    int* run_offset = run_count + kMels;
    float* values = lds + kLdsValues;
    const int tid = threadIdx.x;

    const Tile span = load_tile(tiles, first_tile + blockIdx.x);
    const GradChunk chunk = grad_chunk(audio, seg, span.segment);
    const int frame0 = span.first;
    const int valid = min(kGradFrames, chunk.frames - frame0);

    for (int index = tid; index < kTileSpan; index += 256) part[index] = 0.f;
    for (int index = tid; index < mel_nnz; index += 256) values[index] = mel_values[index];
    if (tid < kMels) {
        // a run the kernel can follow blindly: inside the 513 bins and the values
        int start = mel_start[tid], count = mel_count[tid], offset = mel_offset[tid];
        if (start < 0 || count < 0 || start + count > kBins || offset < 0 ||
            offset + count > mel_nnz)
            count = 0;
        run_start[tid] = start;
        run_count[tid] = count;
        run_offset[tid] = offset;
    }

    // ---- per-thread constants: window, twiddles, the rows of its bins
    float window[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)      // the table holds Hann / 2 (an exact halving)
        window[i] = 2.f * table[kGradTabWindow + tid + 256 * i];
    float2 twiddle[4][3];
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int p = 4 << (2 * pass);                     // passes 2, 4, 6, 8
        const int k = tid & (p - 1);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int exponent = (u + 1) * k * (256 / p);  // < 768
            const int at = exponent < 512 ? exponent : exponent - 512;
            const float sign = exponent < 512 ? 1.f : -1.f;
            twiddle[pass][u] = make_float2(sign * table[kGradTabTw + 2 * at],
                                           sign * table[kGradTabTw + 2 * at + 1]);
        }
    }
    __syncthreads();
    // bins tid, tid + 256 and (thread 0) 512: the first and last row whose run
    // holds the bin
    int row_first[3], row_last[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const int k = b < 2 ? tid + 256 * b : 512;
        row_first[b] = kMels;
        row_last[b] = -1;
        for (int r = 0; r < kMels; ++r) {
            if (k >= run_start[r] && k < run_start[r] + run_count[r]) {
                row_first[b] = min(row_first[b], r);
                row_last[b] = r;
            }
        }
    }

    for (int local = 0; local < valid; ++local) {
        const int frame = frame0 + local;
        // ---- the frame, windowed (reflect / zero per sample as the forward's
        // load_edge: emphases/core.py:357-401, mels.py:31-36)
        const int first = frame * kHop - kPad;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = tid + 256 * i;
            int r = first + n;
            if (r < 0) r = -r;
            if (r >= chunk.length) r = 2 * (chunk.length - 1) - r;
            const bool live = r >= chunk.r_lo && r < chunk.r_hi;
            const float value = live ? chunk.origin[r] : 0.f;
            buffer_a[grad_slot(n)] = make_float2(window[i] * value, 0.f);
        }
        __syncthreads();
        grad_transform(buffer_a, buffer_b, tid, twiddle);
        // ---- magnitudes; X / s stays in registers
        float2 unit[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            unit[b] = make_float2(0.f, 0.f);
            if (b == 2 && tid != 0) continue;
            const int k = b < 2 ? tid + 256 * b : 512;
            const float2 x = buffer_b[grad_slot(k)];
            const float s = sqrtf(x.x * x.x + x.y * x.y + 1e-6f);
            mag[k] = s;
            unit[b] = make_float2(x.x / s, x.y / s);
        }
        __syncthreads();
        // ---- m_r and q_r
        if (tid < kMels) {
            const int start = run_start[tid], count = run_count[tid], offset = run_offset[tid];
            float m = 0.f;
            for (int j = 0; j < count; ++j) m = fmaf(values[offset + j], mag[start + j], m);
            const float g = dmel[static_cast<int64_t>(mel_row + tid) * ld + chunk.frame_off + frame];
            q[tid] = m >= 1e-5f ? g / m : 0.f;
        }
        __syncthreads();
        // ---- G_k, conj(D_k) into the transform buffer, zeros above bin 512
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            if (b == 2 && tid != 0) continue;
            const int k = b < 2 ? tid + 256 * b : 512;
            float big = 0.f;
            for (int r = row_first[b]; r <= row_last[b]; ++r) {
                const int at = k - run_start[r];
                if (at >= 0 && at < run_count[r]) big = fmaf(values[run_offset[r] + at], q[r], big);
            }
            buffer_a[grad_slot(k)] = make_float2(big * unit[b].x, -(big * unit[b].y));
        }
#pragma unroll
        for (int i = 2; i < 4; ++i) {
            const int n = tid + 256 * i;
            if (n > 512) buffer_a[grad_slot(n)] = make_float2(0.f, 0.f);
        }
        __syncthreads();
        grad_transform(buffer_a, buffer_b, tid, twiddle);
        // ---- window and overlap-add inside the tile, frames in rising order
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = tid + 256 * i;
            part[local * kHop + n] += window[i] * buffer_b[grad_slot(n)].x;
        }
        // (the next frame's first write of `part` comes after several barriers)
    }
    __syncthreads();
    float* slot = workspace + static_cast<int64_t>(blockIdx.x) * kTileSpan;
    for (int index = tid; index < kTileSpan; index += 256) slot[index] = part[index];
}

// P[j] of the chunk from the workspace: the earlier tile's part + the later's.
// `slots`: the workspace slot of the chunk's tile 0 (may lie before the run's
// first slot: only the owner's neighbours are ever read).
__device__ __forceinline__ float grad_gather(const float* slots, int tiles_of_chunk, int j) {
    const int tile = min(j / kTileStep, tiles_of_chunk - 1);
    const int local = j - tile * kTileStep;
    const float* slot = slots + static_cast<int64_t>(tile) * kTileSpan;
    const float later = local < kTileSpan ? slot[local] : 0.f;
    if (tile >= 1 && local + kTileStep < kTileSpan)
        return slot[local + kTileStep - kTileSpan] + later;
    return later;
}

// Launch B: the samples a tile owns.
__global__ __launch_bounds__(256) void logmel_backward_fold_kernel(
    const int64_t* __restrict__ seg, const int32_t* __restrict__ tiles, int first_tile,
    int first_slot_tile, const float* __restrict__ workspace, float* __restrict__ daudio) {
    const int index = first_tile + blockIdx.x;
    const Tile span = load_tile(tiles, index);
    const GradChunk chunk = grad_chunk(daudio, seg, span.segment);
    const int tile = span.first / kGradFrames;
    const int tiles_of_chunk = (chunk.frames + kGradFrames - 1) / kGradFrames;
    const int samples = chunk.length;
    const int begin = tile * kTileStep;
    const int end = tile == tiles_of_chunk - 1 ? samples : begin + kTileStep;
    const float* slots =
        workspace + (static_cast<int64_t>(index - tile) - first_slot_tile) * kTileSpan;
    float* out = daudio + chunk.shift;
    for (int n = begin + threadIdx.x; n < end; n += 256) {
        if (n < chunk.r_lo || n >= chunk.r_hi) continue;       // the utterance's zero padding
        float value = grad_gather(slots, tiles_of_chunk, n + kPad);
        if (n >= 1 && n <= kPad) value += grad_gather(slots, tiles_of_chunk, kPad - n);
        if (n >= samples - kPad - 1 && n <= samples - 2)
            value += grad_gather(slots, tiles_of_chunk, 2 * (samples - 1) - n + kPad);
        out[n] = value;
    }
}

size_t grad_lds_bytes(int mel_nnz) { return (kLdsValues + mel_nnz) * sizeof(float); }

}  // namespace

}  // namespace emph

using namespace emph;

extern "C" {

int64_t emph_logmel_backward_workspace(int32_t n_tiles) {
    const int64_t slots = n_tiles < 1 ? 1 : (n_tiles > kRunSlots ? kRunSlots : n_tiles);
    return slots * kTileSpan;
}

int emph_logmel_backward(const float* audio, const int64_t* seg, const int32_t* tiles,
                         int32_t n_tiles, const float* table, const int32_t* mel_start,
                         const int32_t* mel_count, const int32_t* mel_offset,
                         const float* mel_values, int32_t mel_nnz, const float* dmel, int64_t ld,
                         int32_t mel_row, float* workspace, float* daudio, void* stream) {
    EMPH_REQUIRE(n_tiles >= 0, EMPH_EINVAL, "emph_logmel_backward: n_tiles %d", n_tiles);
    EMPH_REQUIRE(audio && seg && tiles && table && mel_start && mel_count && mel_offset &&
                     mel_values && dmel && workspace && daudio,
                 EMPH_EINVAL, "emph_logmel_backward: null pointer");
    auto aligned = [](const void* pointer, uintptr_t to) {
        return (reinterpret_cast<uintptr_t>(pointer) & (to - 1)) == 0;
    };
    EMPH_REQUIRE(aligned(audio, 4) && aligned(seg, 8) && aligned(tiles, 16) && aligned(table, 4) &&
                     aligned(mel_start, 4) && aligned(mel_count, 4) && aligned(mel_offset, 4) &&
                     aligned(mel_values, 4) && aligned(dmel, 4) && aligned(workspace, 4) &&
                     aligned(daudio, 4),
                 EMPH_EINVAL, "emph_logmel_backward: misaligned pointer");
    EMPH_REQUIRE(mel_nnz > 0 && mel_nnz <= 8192, EMPH_ERANGE,
                 "emph_logmel_backward: mel_nnz %d out of range", mel_nnz);
    EMPH_REQUIRE(mel_row >= 0 && ld > 0, EMPH_EINVAL, "emph_logmel_backward: bad output rows");
    EMPH_REQUIRE(emph_frontend_table_size() == kGradTabSize && emph_frontend_block() == kGradFrames,
                 EMPH_EINVAL, "emph_logmel_backward: the front-end's table or tile has changed");
    if (n_tiles == 0) return EMPH_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = grad_lds_bytes(mel_nnz);
    static LdsReservation reserved;
    if (int status = reserve_lds(
            reserved, reinterpret_cast<const void*>(logmel_backward_frames_kernel), lds,
            "emph_logmel_backward"))
        return status;
    for (int first = 0; first < n_tiles; first += kRunTiles) {
        const int last = first + kRunTiles < n_tiles ? first + kRunTiles : n_tiles;
        // the run's neighbours are recomputed: launch B reads their parts
        const int low = first > 0 ? first - 1 : 0;
        const int high = last < n_tiles ? last + 1 : n_tiles;
        EMPH_LAUNCH(logmel_backward_frames_kernel, dim3(high - low), dim3(256), lds, s, audio,
                    seg, tiles, low, table, mel_start, mel_count, mel_offset, mel_values,
                    mel_nnz, dmel, ld, mel_row, workspace);
        if (int status = check_launch("emph_logmel_backward")) return status;
        EMPH_LAUNCH(logmel_backward_fold_kernel, dim3(last - first), dim3(256), 0, s, seg, tiles,
                    first, low, workspace, daudio);
        if (int status = check_launch("emph_logmel_backward")) return status;
    }
    return EMPH_OK;
}

}  // extern "C"
