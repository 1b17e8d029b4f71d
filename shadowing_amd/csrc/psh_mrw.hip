// psh_mrw.hip -- an ensemble of log-normal multifractal random walks (Bacry, Delour, Muzy 2001) made in HBM: one
// workgroup per pair of paths, a batched FFT held in LDS, fed by counter-based Philox draws, in double.
// Host twin: shadowing_amd/mrw.py (numpy float64, np.fft.fft on the same draws).
//
// The method (the contract of this kernel and of mrw.py), at unit step, n returns per path:
//   r[t] = sigma * eps[t] * exp(omega[t] - c[0]),  t = 0 .. n-1;   lnx[0] = 0, lnx[t+1] = lnx[t] + r[t].
//   * omega: centred stationary Gaussian, Cov(omega[s], omega[t]) = c[|s-t|], c[j] = lam^2 max(ln(L / (j + 1)), 0), L the
//     integral scale.  E[exp(2 omega)] = exp(2 c[0]), so E[r^2] = sigma^2.
//   * eps: unit-variance fractional Gaussian noise of Hurst exponent H, independent of omega,
//     Cov = (|j+1|^2H - 2 |j|^2H + |j-1|^2H) / 2.  H = 0.5 is white noise and is drawn directly.
//   * Both sequences are made exactly by circulant embedding: M = the smallest power of two >= 2n, the covariance
//     extended evenly, chat[j] = c[min(j, M - j)], s[k] = sum_j chat[j] cos(2 pi j k / M) >= 0 (c is convex, decreasing
//     and non-negative on 0 .. M/2; known for fGn at every H), computed by the host in double and handed over as the
//     device table a[k] = sqrt(max(s[k], 0) / M), k < M.
//   * One transform makes two paths.  For the pair q (paths 2q and 2q + 1): Z[k] = z0 + i z1 is one Box-Muller pair per
//     k < M, Y[t] = sum_k a[k] Z[k] exp(-2 pi i k t / M); omega of path 2q is Re Y[0 .. n), of path 2q + 1 Im Y[0 .. n).
//   * Draws: psh_philox.h, key = (seed lo, seed hi).  Z[k] of pair q takes counter (k, stream, q lo, q hi), stream = 0 for
//     omega and 1 for eps (H != 0.5); for H = 0.5, eps[2m] and eps[2m + 1] of path g are the Box-Muller pair of counter
//     (m, 2, g lo, g hi).  A path's samples depend only on (seed, path, n, the tables), never on R or the launch.
//   * Order of operations (fixed, so two calls give identical bits): the transform below, then
//     r = (sigma * eps) * exp(omega - c0) in double, dlnx = float32(r).  lnx: thread i of the workgroup sums the chunk
//     t in [i ch, (i + 1) ch), ch = ceil(n / PSH_MRW_THREADS), left to right; the chunk totals are scanned inside each wave
//     by doubling steps (x[l] = x[l - d] + x[l], d = 1, 2, .. 32), the wave totals are added left to right, and
//     lnx[t + 1] = ((waves before + chunks before in the wave) + sum inside the chunk up to t).
//
// The transform: in-place radix-2 decimation in frequency over the M complex doubles in LDS (16 M bytes: 128 KiB at
// M = 8192, under the 160 KiB one workgroup may hold), three stages at a time in registers (a radix-8 butterfly: 8
// elements at stride M >> (s + 3)), so M = 8192 crosses LDS five times (8 8 8 8 2) rather than thirteen; the first
// butterfly takes its inputs a[k] Z[k] straight from the generator, so the draws never make a pass of their own.  The
// base twiddle of a butterfly is one sincospi, the twiddles of its second and third stage are its square and fourth
// power, the eighth roots are constants.  Y[t] ends at slot bitrev(t); each lane then finishes sample pairs (t, t + 1):
// two 16-byte reads, exp, the product with eps, the float32 stores.  For H != 0.5 the eps transform runs first in the
// same LDS and each lane keeps its own samples in registers across the omega transform.
//
// LDS layout: slot p (16 bytes) lives at p ^ ((p >> 4) & 15) ^ ((p >> 8) & 15) ^ ((p >> 12) & 15).  A 256-byte bank row
// holds 16 slots; the strides that occur (8 b slots in the late butterflies, M / 64 and its multiples in the
// bit-reversed read) are powers of two, which put a 16-lane group of a 128-bit access on one or two slots of the row.
// The XOR moves the row index into the slot index, so 16 lanes at stride 16 or 256 slots land on 16 different slots,
// and lanes on consecutive slots stay a permutation of the row.  An XOR rather than a padded row: it costs no LDS
// (a pad would add 8 KiB at M = 8192) and is a bijection on every aligned group of 16 slots, whatever M.
//
// PSH_MRW_THREADS = 512 (8 waves, 2 per SIMD): two radix-8 butterflies per thread and pass at M = 8192.  The first
// butterfly keeps 8 Box-Muller pairs in flight per lane; under the 128 registers a lane gets with 1024 threads the
// compiler spills them (44 to 127 VGPRs to scratch), with 512 threads nothing spills.
//
// Measured on MI355X (tools/bench_mrw.py, median ms of 20 calls writing the float32 returns, three alternating rounds;
// R x n = 2048 x 4096 and 32768 x 4096, each with H = 0.5 / H = 0.3), against forms this kernel does not keep:
//   this form                                                          0.177 / 0.264   2.35 / 3.60
//   the draws replaced by arithmetic on the counter (no Philox, log,   0.079 / 0.135   1.01 / 1.79
//     sqrt, sincos): what the transform, exp and the stores cost
//   the butterflies' arithmetic and every pass after the first         0.131 / 0.168   1.70 / 2.21
//     skipped: what the draws, exp and the stores cost
//   1024 threads (the spilling build above)                            0.199 / 0.341   2.59 / 4.57
//   Box-Muller with separate sin and cos calls (two argument           0.206 / 0.301   2.73 / 4.11
//     reductions; the same bits on every sample compared)
// The draws dominate (about 1.3 of the 2.35 ms: three Gaussians per sample, the count the PDV generator regenerates in
// 5.6 to 7.6 ms at this size); the transform is about 0.65 ms, a good quarter.  The numpy twin takes 11 to 15 s for the
// ensemble-sized case (scaled from 2048 paths), some 4000 times longer.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_mrw_lds.h"    // the transform and the prefix sum, shared with psh_smrw.hip

namespace psh {

template <int MMAX, bool FGN>
__global__ __launch_bounds__(PSH_MRW_THREADS) void mrw_kernel(MrwArgs a) {
    constexpr int U = MMAX / 4 / PSH_MRW_THREADS > 0 ? MMAX / 4 / PSH_MRW_THREADS : 1;    // sample pairs per thread
    constexpr int CH = MMAX / 2 / PSH_MRW_THREADS > 0 ? MMAX / 2 / PSH_MRW_THREADS : 1;   // samples per scan chunk
    __shared__ double2 buf[MMAX];
    __shared__ double2 wtot[PSH_MRW_THREADS / 64];
    const int tid = (int)threadIdx.x, n = a.n, logM = a.logM;
    const uint64_t pair = (uint64_t)blockIdx.x;
    const int64_t g0 = 2 * (int64_t)blockIdx.x, g1 = g0 + 1;
    const bool has1 = g1 < a.R;                              // an odd R: the last pair's second path is not stored

    double2 e0[U], e1[U];                                    // eps of samples t0, t0 + 1: .x path g0, .y path g1
    if constexpr (FGN) {
        mrw_transform(buf, logM, a.a_eps, 1u, pair, a.key0, a.key1);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t0 = 2 * (tid + u * PSH_MRW_THREADS);
            if (t0 < n) {
                e0[u] = buf[mrw_slot((int)(__brev((unsigned)t0) >> (32 - logM)))];
                e1[u] = buf[mrw_slot((int)(__brev((unsigned)(t0 + 1)) >> (32 - logM)))];
            }
        }
        __syncthreads();
    }
    mrw_transform(buf, logM, a.a_omega, 0u, pair, a.key0, a.key1);

    double2 ra[U], rb[U];                                    // r of samples t0, t0 + 1
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int p = tid + u * PSH_MRW_THREADS, t0 = 2 * p;
        ra[u] = rb[u] = make_double2(0.0, 0.0);
        if (t0 >= n) continue;
        const double2 y0 = buf[mrw_slot((int)(__brev((unsigned)t0) >> (32 - logM)))];
        const double2 y1 = buf[mrw_slot((int)(__brev((unsigned)(t0 + 1)) >> (32 - logM)))];
        if constexpr (!FGN) {
            philox_normal_pair((uint32_t)p, 2u, (uint64_t)g0, a.key0, a.key1, e0[u].x, e1[u].x);
            e0[u].y = e1[u].y = 0.0;
            if (has1) philox_normal_pair((uint32_t)p, 2u, (uint64_t)g1, a.key0, a.key1, e0[u].y, e1[u].y);
        }
        ra[u] = make_double2((a.sigma * e0[u].x) * exp(y0.x - a.c0), (a.sigma * e0[u].y) * exp(y0.y - a.c0));
        rb[u] = make_double2((a.sigma * e1[u].x) * exp(y1.x - a.c0), (a.sigma * e1[u].y) * exp(y1.y - a.c0));
        mrw_store_samples(a.dlnx, a.dlnx_stride, a.omega, n, g0, has1, t0, ra[u], rb[u], y0, y1);
    }
    if (a.lnx) mrw_store_lnx<U, CH>(buf, wtot, ra, rb, n, a.lnx, g0, has1);
}

hipError_t launch_mrw(const MrwArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.R + 1) / 2)), block(PSH_MRW_THREADS);
    const bool fgn = a.a_eps != nullptr;
    if ((1 << a.logM) <= 2048) {
        if (fgn) hipLaunchKernelGGL((mrw_kernel<2048, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((mrw_kernel<2048, false>), grid, block, 0, s, a);
    } else {
        if (fgn) hipLaunchKernelGGL((mrw_kernel<8192, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((mrw_kernel<8192, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace psh
