// psh_launch.h -- host only: the one way a template kernel is picked and launched.
//
//   pick<20, 0>(a.W == 20 ? 20 : 0, [&](auto WT) {
//       return pick<true, false>(aligned, [&](auto AL) {
//           return launch(scan_mq_kernel<WT(), AL()>, grid, PSH_MQ_THREADS, shmem, s, a); }); });
//
// names the kernel once; the compiler writes the ladder.  Only what a lambda's body names is instantiated: a body that
// narrows with `if constexpr` forms no cross product.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace psh {

// dynamic LDS a kernel may ask for without the attribute being raised first
constexpr size_t PSH_LDS_NO_ATTR = 48 * 1024;

// Raise the kernel's dynamic-LDS cap where the launch needs it, launch, report the launch's error.
template <typename... Params, typename... Args>
inline hipError_t launch(void (*kernel)(Params...), dim3 grid, dim3 threads, size_t shmem, hipStream_t s, Args&&... args) {
    if (shmem > PSH_LDS_NO_ATTR) {
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, grid, threads, shmem, s, std::forward<Args>(args)...);
    return hipGetLastError();
}

// f(std::integral_constant<., V>) for the listed V that equals v; hipErrorInvalidValue when none does.
template <auto... Vs, typename T, typename F>
inline hipError_t pick(T v, F&& f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs && ((e = f(std::integral_constant<decltype(Vs), Vs>{})), true)) || ...);
    return e;
}

// the two axes every scan family has: W == 20 is specialised (WT = 20), every other length runs WT = 0; rows whose
// windows load as aligned 16-byte quads, or not
template <typename F>
inline hipError_t pick_w_aligned(int W, bool aligned, F&& f) {
    return pick<20, 0>(W == 20 ? 20 : 0, [&](auto WT) {
        return pick<true, false>(aligned, [&](auto AL) { return f(WT, AL); }); });
}

}  // namespace psh
