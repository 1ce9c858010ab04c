// tools/mfma_rate_probe.cpp - issue cost of the fp16 16x16 MFMA forms on gfx950 (diagnostic, not product).
//   hipcc --offload-arch=gfx950 -O2 tools/mfma_rate_probe.cpp -o mfma_rate_probe && ./mfma_rate_probe
// One wave per SIMD (4 waves per workgroup, one workgroup per CU), each wave issuing v_mfma_f32_16x16x16_f16 or
// v_mfma_f32_16x16x32_f16 back to back on 4 independent accumulators, operands in registers.  Prints shader-clock cycles
// (s_memtime) per MFMA per SIMD.  The question it answers: does the K = 16 form cost half of the K = 32 form (then a
// zero-padded half k-step could be issued as a K = 16 MFMA) or the same?
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

typedef _Float16 f16;
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CK(x) do { hipError_t r_ = (x); if (r_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(r_)); exit(2); } } while (0)

constexpr int ITERS = 4096;      // x 4 accumulators x 4 unrolled = 65536 MFMAs per wave

template <int K>
__global__ __launch_bounds__(256) void mfma_loop(float *out, unsigned long long *cyc, float seed) {
    const int lane = threadIdx.x & 63;
    f32x4 acc[4];
    for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const f16 v = (f16)(seed * (float)(lane + 1));
    const f16x8 a8 = {v, v, v, v, v, v, v, v};
    const f16x4 a4 = {v, v, v, v};
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < ITERS; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (K == 32) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, a8, acc[i], 0, 0, 0);
                else acc[i] = __builtin_amdgcn_mfma_f32_16x16x16f16(a4, a4, acc[i], 0, 0, 0);
            }
    }
    __builtin_amdgcn_s_waitcnt(0);
    float s = 0.f;
    for (int i = 0; i < 4; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];   // keeps the chain alive
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (lane == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
}

template <int K>
static void run(int cus) {
    float *out; unsigned long long *cyc;
    CK(hipMalloc(&out, (size_t)cus * 256 * 4));
    CK(hipMalloc(&cyc, (size_t)cus * 4 * 8));
    hipLaunchKernelGGL(mfma_loop<K>, dim3(cus), dim3(256), 0, 0, out, cyc, 1e-3f);   // warm-up
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL(mfma_loop<K>, dim3(cus), dim3(256), 0, 0, out, cyc, 1e-3f);
    CK(hipEventRecord(e1));
    CK(hipDeviceSynchronize());
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    unsigned long long *h = (unsigned long long *)malloc((size_t)cus * 4 * 8);
    CK(hipMemcpy(h, cyc, (size_t)cus * 4 * 8, hipMemcpyDeviceToHost));
    double mean = 0.0;
    for (int i = 0; i < cus * 4; ++i) mean += (double)h[i];
    mean /= cus * 4;
    const double n = (double)ITERS * 16;
    printf("v_mfma_f32_16x16x%d_f16: %.2f cycles per MFMA per SIMD (s_memtime), launch %.3f ms, %.1f TFLOP/s over %d CUs\n",
           K, mean / n, ms, 2.0 * 16 * 16 * K * n * cus * 4 / (ms * 1e-3) / 1e12, cus);
    free(h);
    CK(hipFree(out)); CK(hipFree(cyc));
}

int main() {
    hipDeviceProp_t pr;
    CK(hipGetDeviceProperties(&pr, 0));
    printf("%s, %d CUs\n", pr.gcnArchName, pr.multiProcessorCount);
    run<32>(pr.multiProcessorCount);
    run<16>(pr.multiProcessorCount);
    run<32>(pr.multiProcessorCount);
    run<16>(pr.multiProcessorCount);
    return 0;
}
