// Throughput of v_mfma_f64_16x16x4f64 (the instruction of kl_mfma_kernel, parelagmc_amd/csrc/kl.hip) on the whole device:
// every wave runs `iters` rounds of 8 independent accumulator chains, operands from registers, no memory traffic.
// Prints one line: "f64_mfma_tflops <value> waves <n> ms <t>".  Built and run by scripts/kl_bench.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void rate_kernel(int iters, double seed, double* out) {
    f64x4 acc[8];
    for (int c = 0; c < 8; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    double a = seed + threadIdx.x, b = seed - threadIdx.x;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
    }
    double s = 0.0;
    for (int c = 0; c < 8; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    if (s == 12345.678) out[0] = s;   // keeps the chains alive; never true for the seeds used
}

#define CK(x)                                                                       \
    do {                                                                            \
        hipError_t e = (x);                                                         \
        if (e != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); return 1; } \
    } while (0)

int main() {
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    const int blocks = p.multiProcessorCount * 8, iters = 4096;   // 8 x 4 waves per CU
    double* out = nullptr;
    CK(hipMalloc(&out, sizeof(double)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    rate_kernel<<<blocks, 256>>>(iters, 1e-3, out);   // warm-up
    CK(hipGetLastError());
    CK(hipEventRecord(e0));
    for (int r = 0; r < 5; ++r) rate_kernel<<<blocks, 256>>>(iters, 1e-3, out);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    const double waves = (double)blocks * 4, flops = 5.0 * waves * iters * 8 * 2.0 * 16 * 16 * 4;
    std::printf("f64_mfma_tflops %.3f waves %.0f ms %.4f\n", flops / (ms * 1e-3) / 1e12, waves, ms / 5);
    CK(hipFree(out));
    return 0;
}
