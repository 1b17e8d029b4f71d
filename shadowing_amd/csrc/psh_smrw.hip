// psh_smrw.hip -- an ensemble of skewed multifractal random walks (Pochart, Bouchaud 2002, "The skewed multifractal
// random walk with applications to option smiles") made in HBM: the MRW of psh_mrw.hip with a leverage term in the
// log-volatility, a causal power-law kernel applied to past noise.  One workgroup per pair of paths, the transforms of
// psh_mrw_lds.h held in LDS, in double.  Host twin: shadowing_amd/mrw.py (smrw_log_returns, np.fft on the same draws).
//
// The method (the contract of this kernel and of the twin), at unit step, n returns per path, white noise, m lags:
//   K(j) = K0 / j^alpha for 1 <= j <= m;   A[t] = sum_{j=1..m} K(j) eps[t - j];   v = sum_j K(j)^2;
//   lv[t] = omega[t] - A[t];   r[t] = sigma * eps[t] * exp(lv[t] - (c0 + v));   lnx as for the MRW.
//   * omega, c0, sigma and eps[t], t >= 0, are the MRW's, on the MRW's counters (streams 0 and 2).  The pre-history
//     eps[-m .. -1] takes stream 3: eps[-1 - 2i] and eps[-2 - 2i] of path g are the Box-Muller pair of counter
//     (i, 3, g lo, g hi), so a pre-history sample does not depend on m.  Every t sees m full lags: stationary from t = 0.
//   * A is a linear convolution inside the circulant of size M (the MRW's): z = eps_g0 + i eps_g1 of times -m .. n - 1
//     sits at slots 0 .. n + m - 1, zeros above, X = FFT_M(z), and A[t] is sample t + m of IFFT_M(FFT_M(K) X), exact for
//     n + m <= M.  K is real, so the one complex convolution serves both paths.
//   * Two transforms, not three, by linearity: IFFT_M(G)[t + m] = FFT_M(G[-k] exp(-2 pi i k m / M) / M)[t], so
//     lv = FFT_M(a[k] Z[k] - T[k] X[(-k) mod M]),  T[k] = conj(FFT_M(K)[k]) exp(-2 pi i k m / M) / M  (the host's table
//     k_hat): the omega transform's first butterfly takes the generator's value minus one LDS read times one table entry.
//     X lies bit-reversed where that butterfly writes, and reads and writes of different lanes collide: a lane forms
//     the inputs of all its butterflies (16 at M = 8192: the draws first, then the LDS reads, so that no X value waits
//     in a register while a draw is made), meets a barrier, then runs the butterflies and stores.
//   * Draws: a Box-Muller pair is two consecutive samples of ONE path, a slot of z one sample of each of TWO paths, so a
//     lane fills adjacent slots (t0, t0 + 1) from the two pairs of the two paths; the lane that fills samples t0 >= 0 is
//     the one that finishes them, and keeps eps in registers across both transforms.  Four Gaussians per sample at m = n
//     (the MRW draws three), none drawn twice.  Both paths of the last pair are drawn when R is odd: the transform mixes
//     the two, and a path's bits must not depend on R.
//   * Order of operations: fill, the forward transform (every stage from LDS), the folded first pass, the remaining
//     passes, then r = (sigma * eps) * exp(lv - (c0 + v)) in double, dlnx = float32(r), lnx by psh_mrw.hip's prefix sum.
//     With an all-zero k_hat the first pass subtracts a zero from the MRW's inputs.
//
// PSH_MRW_THREADS = 512 as the MRW: eps (32 registers at M = 8192) and the 16 inputs held across the barrier (64) stay
// under the 256 a lane gets with 8 waves per workgroup (205 used).  Reading the X values before the draws, 64 more
// registers live under the Box-Muller pairs, spilled 24.
//
// Measured on MI355X (tools/bench_smrw.py, m = n, median ms of 20 calls writing the float32 returns, three alternating
// rounds with psh_mrw_generate at H = 0.5 in the same process; R x n = 2048 x 4096 and 32768 x 4096):
//   this kernel                      0.254   3.90
//   psh_mrw_generate, the same run   0.160   2.34      ratio 1.59 and 1.67
// Four Gaussians per sample where the MRW draws three, two transforms and a fill pass where it makes one: about what
// that arithmetic predicts.  The three-transform form (forward, multiply, an inverse from bit-reversed input) was not
// built.  The numpy twin takes 17 s for the ensemble-sized case (scaled from 2048 paths), some 4300 times longer.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_mrw_lds.h"

namespace psh {

#define PSH_SMRW_STREAM_WHITE 2u
#define PSH_SMRW_STREAM_PAST 3u

namespace {

// The first G stages of lv = FFT_M(tab * Z - T * Xrev): buf holds X = FFT_M(z) bit-reversed on entry, the DIF
// intermediate on exit.  NB butterflies per lane, all their inputs formed before the barrier that precedes any store.
template <int G, int NB>
__device__ __forceinline__ void smrw_first_pass(double2* buf, int logM, const double* tab, const double2* khat,
                                                uint64_t pair, uint32_t k0, uint32_t k1) {
    constexpr int N = 1 << G;
    const int lst = logM - G, nb = 1 << lst, mask = (1 << logM) - 1;
    const double step = -2.0 / (double)(1 << logM);
    double2 x[NB][N];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int b = (int)threadIdx.x + i * PSH_MRW_THREADS;
        if (b < nb) {
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const int k = b + (q << lst);
                double z0, z1;
                philox_normal_pair((uint32_t)k, 0u, pair, k0, k1, z0, z1);
                const double av = tab[k];
                x[i][q] = make_double2(av * z0, av * z1);
            }
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const int k = b + (q << lst);
                const unsigned kr = (unsigned)((-k) & mask);                           // (-k) mod M
                const double2 c = cmul(khat[k], buf[mrw_slot((int)(__brev(kr) >> (32 - logM)))]);
                x[i][q] = make_double2(x[i][q].x - c.x, x[i][q].y - c.y);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int b = (int)threadIdx.x + i * PSH_MRW_THREADS;
        if (b < nb) {
            double2 W;
            sincospi((double)b * step, &W.y, &W.x);              // exp(-2 pi i b / M)
            mrw_butterfly<G>(x[i], W);
#pragma unroll
            for (int q = 0; q < N; ++q) buf[mrw_slot(b + (q << lst))] = x[i][q];
        }
    }
}

}  // namespace

template <int MMAX>
__global__ __launch_bounds__(PSH_MRW_THREADS) void smrw_kernel(SmrwArgs a) {
    constexpr int U = MMAX / 4 / PSH_MRW_THREADS > 0 ? MMAX / 4 / PSH_MRW_THREADS : 1;    // sample pairs per thread
    constexpr int CH = MMAX / 2 / PSH_MRW_THREADS > 0 ? MMAX / 2 / PSH_MRW_THREADS : 1;   // samples per scan chunk
    constexpr int NB = MMAX / 8 / PSH_MRW_THREADS > 0 ? MMAX / 8 / PSH_MRW_THREADS : 1;   // radix-8 butterflies per thread
    __shared__ double2 buf[MMAX];
    __shared__ double2 wtot[PSH_MRW_THREADS / 64];
    const int tid = (int)threadIdx.x, n = a.n, m = a.m, logM = a.logM;
    const uint64_t pair = (uint64_t)blockIdx.x;
    const int64_t g0 = 2 * (int64_t)blockIdx.x, g1 = g0 + 1;
    const bool has1 = g1 < a.R;                              // an odd R: the last pair's second path is made, not stored

    // ---- z = eps_g0 + i eps_g1 of times -m .. n - 1 at slots 0 .. n + m - 1, zeros above
    double2 e0[U], e1[U];                                    // eps of samples t0, t0 + 1: .x path g0, .y path g1
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int p = tid + u * PSH_MRW_THREADS, t0 = 2 * p;
        e0[u] = e1[u] = make_double2(0.0, 0.0);
        if (t0 >= n) continue;
        philox_normal_pair((uint32_t)p, PSH_SMRW_STREAM_WHITE, (uint64_t)g0, a.key0, a.key1, e0[u].x, e1[u].x);
        philox_normal_pair((uint32_t)p, PSH_SMRW_STREAM_WHITE, (uint64_t)g1, a.key0, a.key1, e0[u].y, e1[u].y);
        buf[mrw_slot(t0 + m)] = e0[u];
        if (t0 + 1 < n) buf[mrw_slot(t0 + 1 + m)] = e1[u];
    }
    for (int i = tid; 2 * i < m; i += PSH_MRW_THREADS) {     // times -1 - 2i (slot m - 1 - 2i >= 0) and -2 - 2i
        double2 za, zb;
        philox_normal_pair((uint32_t)i, PSH_SMRW_STREAM_PAST, (uint64_t)g0, a.key0, a.key1, za.x, zb.x);
        philox_normal_pair((uint32_t)i, PSH_SMRW_STREAM_PAST, (uint64_t)g1, a.key0, a.key1, za.y, zb.y);
        const int p = m - 1 - 2 * i;
        buf[mrw_slot(p)] = za;
        if (p >= 1) buf[mrw_slot(p - 1)] = zb;
    }
    for (int p = n + m + tid; p < (1 << logM); p += PSH_MRW_THREADS) buf[mrw_slot(p)] = make_double2(0.0, 0.0);
    __syncthreads();

    // ---- X = FFT_M(z), then lv = FFT_M(a Z - T Xrev), both left bit-reversed
    mrw_passes(buf, logM, 0);
    int s;
    if (logM >= 3) { smrw_first_pass<3, NB>(buf, logM, a.a_omega, a.k_hat, pair, a.key0, a.key1); s = 3; }
    else { smrw_first_pass<2, 1>(buf, logM, a.a_omega, a.k_hat, pair, a.key0, a.key1); s = 2; }      // M = 4
    __syncthreads();
    mrw_passes(buf, logM, s);

    double2 ra[U], rb[U];                                    // r of samples t0, t0 + 1
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int t0 = 2 * (tid + u * PSH_MRW_THREADS);
        ra[u] = rb[u] = make_double2(0.0, 0.0);
        if (t0 >= n) continue;
        const double2 y0 = buf[mrw_slot((int)(__brev((unsigned)t0) >> (32 - logM)))];
        const double2 y1 = buf[mrw_slot((int)(__brev((unsigned)(t0 + 1)) >> (32 - logM)))];
        ra[u] = make_double2((a.sigma * e0[u].x) * exp(y0.x - a.cv), (a.sigma * e0[u].y) * exp(y0.y - a.cv));
        rb[u] = make_double2((a.sigma * e1[u].x) * exp(y1.x - a.cv), (a.sigma * e1[u].y) * exp(y1.y - a.cv));
        mrw_store_samples(a.dlnx, a.dlnx_stride, a.logvol, n, g0, has1, t0, ra[u], rb[u], y0, y1);
    }
    if (a.lnx) mrw_store_lnx<U, CH>(buf, wtot, ra, rb, n, a.lnx, g0, has1);
}

hipError_t launch_smrw(const SmrwArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.R + 1) / 2)), block(PSH_MRW_THREADS);
    if ((1 << a.logM) <= 2048) hipLaunchKernelGGL((smrw_kernel<2048>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((smrw_kernel<8192>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace psh
