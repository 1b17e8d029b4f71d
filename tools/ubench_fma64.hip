// The double-precision FMA rate a register-only loop reaches on this device: 16 independent v_fma_f64 chains per lane, 512
// lanes per workgroup.  Built as a shared library by tools/bench_stylized.py, which calls fma64_rate in its own process so
// that the floor it states for psh_lagged_moments is measured in the same run.
#include <hip/hip_runtime.h>

#define CHAINS 16

__global__ __launch_bounds__(512) void fma64_loop(double* out, double x, int iters) {
    double a[CHAINS];
    const double b = x + 1e-9 * threadIdx.x, c = 1.0 - 1e-9 * threadIdx.x;
#pragma unroll
    for (int i = 0; i < CHAINS; ++i) a[i] = (double)i;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < CHAINS; ++i) a[i] = fma(a[i], c, b);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < CHAINS; ++i) s += a[i];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// FMAs per second (all lanes), the best of `reps` launches of `blocks` workgroups; 0 on a HIP error
extern "C" double fma64_rate(int blocks, int iters, int reps) {
    double* out = nullptr;
    if (hipMalloc(&out, (size_t)blocks * 512 * sizeof(double)) != hipSuccess) return 0.0;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    float best = 1e30f;
    for (int r = 0; r <= reps; ++r) {                            // launch 0 warms up
        (void)hipEventRecord(e0, 0);
        hipLaunchKernelGGL(fma64_loop, dim3(blocks), dim3(512), 0, 0, out, 0.5, iters);
        (void)hipEventRecord(e1, 0);
        if (hipEventSynchronize(e1) != hipSuccess) { best = 1e30f; break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (r && ms < best) best = ms;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(out);
    return best < 1e29f ? (double)blocks * 512.0 * iters * CHAINS / (best * 1e-3) : 0.0;
}
