// psh_scat_lds.h -- what psh_scattering.hip and psh_scattering_grad.hip share: the inverse of psh_mrw_lds.h's forward
// transform on the n complex doubles of a row held in LDS (decimation in time FROM bit-reversed input to time order).  The
// method heads psh_scattering.hip; nothing here may change without moving psh_scattering_spectra's bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh_mrw_lds.h"    // mrw_slot, cmul

namespace psh {

#define PSH_SCAT_THREADS PSH_MRW_THREADS
#define PSH_SCAT_WAVES (PSH_SCAT_THREADS / 64)

// d * exp(+2 pi i e / 8), e = 0 .. 3 (a constant after unrolling)
__device__ __forceinline__ double2 scat_root8(double2 d, int e) {
    switch (e) {
        case 1: return make_double2((d.x - d.y) * PSH_MRW_RSQRT2, (d.x + d.y) * PSH_MRW_RSQRT2);
        case 2: return make_double2(-d.y, d.x);
        case 3: return make_double2((-d.x - d.y) * PSH_MRW_RSQRT2, (d.x - d.y) * PSH_MRW_RSQRT2);
        default: return d;
    }
}

// G radix-2 DIT stages of the inverse on the 2^G elements of one butterfly, in registers: element q stands at
// base + q h, the stage of half-length 2^sub h pairs q with q + 2^sub under exp(+2 pi i (j + (q mod 2^sub) h) / (2^(sub+1) h));
// W = exp(+2 pi i j / (2^G h)) is the twiddle of the last stage
template <int G>
__device__ __forceinline__ void scat_inv_butterfly(double2 (&x)[1 << G], double2 W) {
    constexpr int N = 1 << G;
    double2 Wp[G];
    Wp[G - 1] = W;
#pragma unroll
    for (int sub = G - 2; sub >= 0; --sub) Wp[sub] = cmul(Wp[sub + 1], Wp[sub + 1]);
#pragma unroll
    for (int sub = 0; sub < G; ++sub) {
        const int hq = 1 << sub;
#pragma unroll
        for (int h0 = 0; h0 < N; h0 += 2 * hq) {
#pragma unroll
            for (int r = 0; r < hq; ++r) {
                const double2 u = x[h0 + r];
                const double2 v = scat_root8(cmul(x[h0 + r + hq], Wp[sub]), r * (4 / hq));
                x[h0 + r] = make_double2(u.x + v.x, u.y + v.y);
                x[h0 + r + hq] = make_double2(u.x - v.x, u.y - v.y);
            }
        }
    }
}

// The stages of half-length h .. 2^(G-1) h, h = 2^lh, of the in-place radix-2 DIT inverse (exp(+2 pi i / n) the root,
// no 1 / n) of the n = 2^logn slots of buf: butterfly b takes the 2^G elements base + q h of block b / h
template <int G>
__device__ __forceinline__ void scat_inv_pass(double2* buf, int logn, int lh) {
    constexpr int N = 1 << G;
    const int h = 1 << lh;
    const double step = 2.0 / (double)(N << lh);
    for (int b = (int)threadIdx.x; b < (1 << (logn - G)); b += PSH_SCAT_THREADS) {
        const int j = b & (h - 1);
        const int base = ((b >> lh) << (lh + G)) + j;
        double2 x[N];
#pragma unroll
        for (int q = 0; q < N; ++q) x[q] = buf[mrw_slot(base + (q << lh))];
        double2 W;
        sincospi((double)j * step, &W.y, &W.x);              // exp(+2 pi i j / (N h))
        scat_inv_butterfly<G>(x, W);
#pragma unroll
        for (int q = 0; q < N; ++q) buf[mrw_slot(base + (q << lh))] = x[q];
    }
}

// buf holds X[k] at slot bitrev(k); leaves sum_k X[k] exp(+2 pi i k t / n) at slot t; ends on a barrier
__device__ __forceinline__ void scat_inverse(double2* buf, int logn) {
    int lh = logn % 3;
    if (lh == 1) scat_inv_pass<1>(buf, logn, 0);
    else if (lh == 2) scat_inv_pass<2>(buf, logn, 0);
    if (lh) __syncthreads();
    for (; lh < logn; lh += 3) {
        scat_inv_pass<3>(buf, logn, lh);
        __syncthreads();
    }
}

}  // namespace psh
