// psh_mrw_lds.h -- what psh_mrw.hip and psh_smrw.hip share: the batched transform of M complex doubles held in LDS, the
// stores of a lane's samples, and the workgroup-wide prefix sum that turns a pair of paths' returns into log-prices.  The
// method, the LDS layout and the order of operations head psh_mrw.hip; nothing here may change without moving
// psh_mrw_generate's bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh_philox.h"

namespace psh {

#define PSH_MRW_THREADS 512
#define PSH_MRW_RSQRT2 0.7071067811865476

__device__ __forceinline__ int mrw_slot(int p) { return p ^ ((p >> 4) & 15) ^ ((p >> 8) & 15) ^ ((p >> 12) & 15); }

__device__ __forceinline__ double2 cmul(double2 u, double2 w) {
    return make_double2(u.x * w.x - u.y * w.y, u.x * w.y + u.y * w.x);
}

// d * exp(-2 pi i e / 8), e = 0 .. 3 (a constant after unrolling)
__device__ __forceinline__ double2 mul_root8(double2 d, int e) {
    switch (e) {
        case 1: return make_double2((d.x + d.y) * PSH_MRW_RSQRT2, (d.y - d.x) * PSH_MRW_RSQRT2);
        case 2: return make_double2(d.y, -d.x);
        case 3: return make_double2((d.y - d.x) * PSH_MRW_RSQRT2, (-d.x - d.y) * PSH_MRW_RSQRT2);
        default: return d;
    }
}

// G radix-2 DIF stages on the 2^G elements of one butterfly, in registers; W is the base twiddle of its first stage
template <int G>
__device__ __forceinline__ void mrw_butterfly(double2 (&x)[1 << G], double2 W) {
    constexpr int N = 1 << G;
#pragma unroll
    for (int sub = 0; sub < G; ++sub) {
        const int half = N >> (sub + 1);
#pragma unroll
        for (int h = 0; h < N; h += 2 * half) {
#pragma unroll
            for (int r = 0; r < half; ++r) {
                const double2 u = x[h + r], v = x[h + r + half];
                x[h + r] = make_double2(u.x + v.x, u.y + v.y);
                const double2 d = cmul(make_double2(u.x - v.x, u.y - v.y), W);
                x[h + r + half] = mul_root8(d, r * (4 / half));
            }
        }
        if (sub + 1 < G) W = cmul(W, W);
    }
}

// Stages s .. s + G - 1 of the in-place radix-2 DIF transform of the M = 2^logM slots of buf, exp(-2 pi i / M) the root:
// butterfly b takes the 2^G elements base + q * st, st = M >> (s + G), of block b / st.  FIRST (s = 0): the inputs are
// tab[k] * Z[k], Z[k] the Box-Muller pair of counter (k, stream, pair lo, pair hi), and buf is only written.
template <int G, bool FIRST>
__device__ __forceinline__ void mrw_pass(double2* buf, int logM, int s, const double* tab, uint32_t stream, uint64_t pair,
                                         uint32_t k0, uint32_t k1) {
    constexpr int N = 1 << G;
    const int lst = logM - s - G, st = 1 << lst;
    const double step = -2.0 / (double)(1 << logM);
    for (int b = (int)threadIdx.x; b < (1 << (logM - G)); b += PSH_MRW_THREADS) {
        const int j = b & (st - 1);
        const int base = ((b >> lst) << (logM - s)) + j;
        double2 x[N];
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const int k = base + (q << lst);
            if constexpr (FIRST) {
                double z0, z1;
                philox_normal_pair((uint32_t)k, stream, pair, k0, k1, z0, z1);
                const double av = tab[k];
                x[q] = make_double2(av * z0, av * z1);
            } else {
                x[q] = buf[mrw_slot(k)];
            }
        }
        double2 W;
        sincospi((double)(j << s) * step, &W.y, &W.x);       // exp(-2 pi i (j << s) / M)
        mrw_butterfly<G>(x, W);
#pragma unroll
        for (int q = 0; q < N; ++q) buf[mrw_slot(base + (q << lst))] = x[q];
    }
}

// Stages s .. logM - 1 on what buf holds (three at a time, then what is left); ends on a barrier
__device__ __forceinline__ void mrw_passes(double2* buf, int logM, int s) {
    for (; s + 3 <= logM; s += 3) {
        mrw_pass<3, false>(buf, logM, s, nullptr, 0u, 0u, 0u, 0u);
        __syncthreads();
    }
    if (logM - s == 2) mrw_pass<2, false>(buf, logM, s, nullptr, 0u, 0u, 0u, 0u);
    else if (logM - s == 1) mrw_pass<1, false>(buf, logM, s, nullptr, 0u, 0u, 0u, 0u);
    if (s < logM) __syncthreads();
}

// Y = FFT_M(tab * Z) of the pair, left bit-reversed in buf (Y[t] at slot bitrev(t)); ends on a barrier
__device__ __forceinline__ void mrw_transform(double2* buf, int logM, const double* tab, uint32_t stream, uint64_t pair,
                                              uint32_t k0, uint32_t k1) {
    int s;
    if (logM >= 3) { mrw_pass<3, true>(buf, logM, 0, tab, stream, pair, k0, k1); s = 3; }
    else { mrw_pass<2, true>(buf, logM, 0, tab, stream, pair, k0, k1); s = 2; }       // M = 4
    __syncthreads();
    mrw_passes(buf, logM, s);
}

// The returns ra, rb and the log-volatilities y0, y1 of samples t0 and t0 + 1 (.x path g0, .y path g0 + 1) go to the rows
// of dlnx (float32, dlnx_stride apart) and of logvol (n apart); either may be nullptr
__device__ __forceinline__ void mrw_store_samples(float* dlnx, int64_t dlnx_stride, double* logvol, int n, int64_t g0,
                                                  bool has1, int t0, double2 ra, double2 rb, double2 y0, double2 y1) {
    const bool two = t0 + 1 < n;
    if (dlnx) {
        float* row0 = dlnx + g0 * dlnx_stride + t0;
        row0[0] = (float)ra.x;
        if (two) row0[1] = (float)rb.x;
        if (has1) {
            float* row1 = row0 + dlnx_stride;
            row1[0] = (float)ra.y;
            if (two) row1[1] = (float)rb.y;
        }
    }
    if (logvol) {
        double* row0 = logvol + g0 * n + t0;
        row0[0] = y0.x;
        if (two) row0[1] = y1.x;
        if (has1) {
            row0[n] = y0.y;
            if (two) row0[n + 1] = y1.y;
        }
    }
}

// lnx of the pair (g0, g0 + 1) from its returns: ra[u], rb[u] are r of samples t0 = 2 (tid + u PSH_MRW_THREADS) and
// t0 + 1 (.x path g0, .y path g0 + 1; zero where t0 >= n).  The returns go back to LDS in time order, then a
// workgroup-wide prefix sum (its order: the header of psh_mrw.hip).  Every thread of the workgroup calls it.
template <int U, int CH>
__device__ __forceinline__ void mrw_store_lnx(double2* buf, double2* wtot, const double2 (&ra)[U], const double2 (&rb)[U],
                                              int n, double* lnx, int64_t g0, bool has1) {
    const int tid = (int)threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int t0 = 2 * (tid + u * PSH_MRW_THREADS);
        if (t0 < n) {
            buf[mrw_slot(t0)] = ra[u];
            buf[mrw_slot(t0 + 1)] = rb[u];                   // (t0 + 1 <= n < M: a slot nobody reads when t0 + 1 == n)
        }
    }
    __syncthreads();
    const int ch = (n + PSH_MRW_THREADS - 1) / PSH_MRW_THREADS;
    double2 part[CH];
    double2 run = make_double2(0.0, 0.0);
#pragma unroll
    for (int u = 0; u < CH; ++u) {
        const int t = tid * ch + u;
        if (u < ch && t < n) {
            const double2 v = buf[mrw_slot(t)];
            run.x = run.x + v.x;
            run.y = run.y + v.y;
        }
        part[u] = run;
    }
    const int lane = tid & 63, wave = tid >> 6;
    double2 inc = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double yx = __shfl_up(inc.x, d), yy = __shfl_up(inc.y, d);
        if (lane >= d) { inc.x = yx + inc.x; inc.y = yy + inc.y; }
    }
    double2 before = make_double2(__shfl_up(inc.x, 1), __shfl_up(inc.y, 1));
    if (lane == 0) before = make_double2(0.0, 0.0);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    double2 off = make_double2(0.0, 0.0);
    for (int w = 0; w < wave; ++w) { off.x = off.x + wtot[w].x; off.y = off.y + wtot[w].y; }
    off.x = off.x + before.x;
    off.y = off.y + before.y;
    double* l0 = lnx + g0 * (int64_t)(n + 1);
    double* l1 = l0 + (n + 1);
    if (tid == 0) {
        l0[0] = 0.0;
        if (has1) l1[0] = 0.0;
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) {
        const int t = tid * ch + u;
        if (u < ch && t < n) {
            l0[t + 1] = off.x + part[u].x;
            if (has1) l1[t + 1] = off.y + part[u].y;
        }
    }
}

}  // namespace psh
