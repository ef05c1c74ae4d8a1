// How many independent Philox chains a thread of emph_dropout's kernel should
// carry: the library's per-quad function (csrc/dropout.hip) in kernels of 1, 2,
// 4 and 8 quads per thread, against the same in-place stream without the
// generator (x *= scale), on one frame-rate activation buffer of the training
// shape [80, 75 744] (warm: the conv launch before it has just written it) and
// on a ring of such buffers larger than the Infinity Cache (cold).
// Build: hipcc -O3 --offload-arch=gfx950 -std=c++17 -Iinclude -Iemphases_amd/csrc \
//            tools/micro/dropout_bench.hip -o tools/micro/bin/dropout_bench
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "dropout.hip"

namespace emph {
void set_error(const char* format, ...) {
    va_list arguments;
    va_start(arguments, format);
    vfprintf(stderr, format, arguments);
    va_end(arguments);
    fputc('\n', stderr);
}
}  // namespace emph

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

// QUADS > 0: dropout_kernel's shape with QUADS quads per thread; QUADS < 0: the
// same loads and stores with -QUADS quads per thread and no generator.
template <int QUADS>
__global__ __launch_bounds__(256) void variant_kernel(float4* __restrict__ x, int64_t quads,
                                                      uint32_t threshold, float scale) {
    constexpr int N = QUADS > 0 ? QUADS : -QUADS;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * (256 * N) + threadIdx.x;
    float4 v[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int64_t i = base + 256 * j;
        v[j] = i < quads ? x[i] : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int64_t i = base + 256 * j;
        if (i >= quads) continue;
        if (QUADS > 0) {
            x[i] = emph::dropout_quad(v[j], static_cast<uint64_t>(i), 3, 7, 20261018u, 0u,
                                      threshold, scale);
        } else {
            x[i] = float4{v[j].x * scale, v[j].y * scale, v[j].z * scale, v[j].w * scale};
        }
    }
}

template <int QUADS>
static float run(float4* ring, int buffers, int64_t quads, int launches) {
    constexpr int N = QUADS > 0 ? QUADS : -QUADS;
    const unsigned grid = static_cast<unsigned>((quads + 256 * N - 1) / (256 * N));
    // scale 1 keeps the values finite over any number of in-place launches
    const uint32_t threshold = emph::dropout_threshold(0.1f);
    hipEvent_t begin, end;
    CHECK(hipEventCreate(&begin)); CHECK(hipEventCreate(&end));
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) CHECK(hipEventRecord(begin, 0));
        for (int i = 0; i < launches; ++i)
            hipLaunchKernelGGL(variant_kernel<QUADS>, dim3(grid), dim3(256), 0, 0,
                               ring + (i % buffers) * quads, quads, threshold, 1.f);
    }
    CHECK(hipEventRecord(end, 0)); CHECK(hipEventSynchronize(end));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, begin, end));
    CHECK(hipGetLastError());
    return ms * 1e3f / launches;
}

int main() {
    const int64_t quads = 80 * 75744 / 4;           // 24.2 MB
    const int buffers = 14;                         // 339 MB > 256 MiB of Infinity Cache
    float4* ring;
    CHECK(hipMalloc(&ring, buffers * quads * sizeof(float4)));
    CHECK(hipMemset(ring, 0x3f, buffers * quads * sizeof(float4)));
    const double bytes = 2. * quads * sizeof(float4);
    for (int cold = 0; cold < 2; ++cold) {
        const int n = cold ? buffers : 1, launches = 280;
        const float us[8] = {
            run<-1>(ring, n, quads, launches), run<-4>(ring, n, quads, launches),
            run<1>(ring, n, quads, launches), run<2>(ring, n, quads, launches),
            run<4>(ring, n, quads, launches), run<8>(ring, n, quads, launches),
            run<4>(ring, n, quads, launches), run<-4>(ring, n, quads, launches)};
        const char* names[8] = {"stream, 1 quad", "stream, 4 quads", "philox, 1 quad",
                                "philox, 2 quads", "philox, 4 quads", "philox, 8 quads",
                                "philox, 4 quads (again)", "stream, 4 quads (again)"};
        for (int k = 0; k < 8; ++k)
            printf("%s %-24s %7.2f us per launch (back to back)  %5.2f TB/s\n",
                   cold ? "cold" : "warm", names[k], us[k], bytes / us[k] * 1e-6);
    }
    CHECK(hipFree(ring));
    return 0;
}
