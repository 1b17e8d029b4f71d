// psh_sort_lds.h -- the in-LDS sort and the fixed-order scan that the kernels over the k shadowing paths of a column share:
// psh_quantiles.hip (psh_weighted_quantiles), psh_scoring.hip (psh_score_ensemble) and psh_weights.hip (psh_softmax_weights,
// on the k distances of a query row, a NaN taking the largest key first).  Path j of a column is the 64-bit
// entry (order-preserving 32-bit key of its float32 value) << 32 | j, -0.0 taking +0.0's key, so entries are unique and
// ties break by path index; the bitonic network runs NB index bits a pass on registers, and entry i lies at i + i / 16 in
// LDS.  The method and the bank arithmetic head psh_quantiles.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace psh {

namespace {

#define PSH_QNT_RUN 16          // threads per run of the scan
#define PSH_QNT_GRP 8           // runs per group

__device__ __forceinline__ int qnt_phys(int i) { return i + (i >> 4); }

__device__ __forceinline__ uint32_t qnt_key(float x) {
    const uint32_t u = __float_as_uint(x == 0.0f ? 0.0f : x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float qnt_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__device__ __forceinline__ void qnt_cmpex(uint64_t& lo, uint64_t& hi, bool desc) {
    const uint64_t a = lo, c = hi;
    const bool sw = (a > c) != desc;
    lo = sw ? c : a;
    hi = sw ? a : c;
}

// phases 1 .. NB of the network on runs of 2^NB consecutive entries, in registers
template <int NB, int THREADS>
__device__ __forceinline__ void qnt_sort_first(uint64_t* ent, int n2, int tid) {
    constexpr int E = 1 << NB;
    for (int g = tid; g < (n2 >> NB); g += THREADS) {
        uint64_t v[E];
#pragma unroll
        for (int r = 0; r < E; ++r) v[r] = ent[qnt_phys((g << NB) + r)];
#pragma unroll
        for (int s = 1; s <= NB; ++s)
#pragma unroll
            for (int b = s - 1; b >= 0; --b)
#pragma unroll
                for (int r = 0; r < E; ++r)
                    if (!(r & (1 << b))) qnt_cmpex(v[r], v[r | (1 << b)], s < NB ? ((r >> s) & 1) != 0 : (g & 1) != 0);
#pragma unroll
        for (int r = 0; r < E; ++r) ent[qnt_phys((g << NB) + r)] = v[r];
    }
}

// the sub-stages of phase s on the index bits lo + N - 1 .. lo
template <int N, int THREADS>
__device__ __forceinline__ void qnt_sort_pass(uint64_t* ent, int n2, int lo, int s, int tid) {
    constexpr int E = 1 << N;
    for (int g = tid; g < (n2 >> N); g += THREADS) {
        const int base = ((g >> lo) << (lo + N)) | (g & ((1 << lo) - 1));
        const bool desc = ((base >> s) & 1) != 0;
        uint64_t v[E];
#pragma unroll
        for (int r = 0; r < E; ++r) v[r] = ent[qnt_phys(base | (r << lo))];
#pragma unroll
        for (int b = N - 1; b >= 0; --b)
#pragma unroll
            for (int r = 0; r < E; ++r)
                if (!(r & (1 << b))) qnt_cmpex(v[r], v[r | (1 << b)], desc);
#pragma unroll
        for (int r = 0; r < E; ++r) ent[qnt_phys(base | (r << lo))] = v[r];
    }
}

// the whole network on n2 entries, a power of two >= 2^NB: a barrier of the caller's stands between the stores of the
// entries and this call, and the sorted order is visible to every thread on return
template <int NB, int THREADS>
__device__ __forceinline__ void qnt_sort(uint64_t* ent, int n2, int tid) {
    qnt_sort_first<NB, THREADS>(ent, n2, tid);
    __syncthreads();
    for (int s = NB + 1; (1 << s) <= n2; ++s) {
        for (int hi = s; hi > 0;) {
            const int nb = hi < NB ? hi : NB, lo = hi - nb;
            if (nb == 1) qnt_sort_pass<1, THREADS>(ent, n2, lo, s, tid);
            else if (nb == 2) qnt_sort_pass<2, THREADS>(ent, n2, lo, s, tid);
            else if (NB >= 3 && nb == 3) qnt_sort_pass<(NB >= 3 ? 3 : 1), THREADS>(ent, n2, lo, s, tid);
            else if (NB >= 4 && nb == 4) qnt_sort_pass<(NB >= 4 ? 4 : 1), THREADS>(ent, n2, lo, s, tid);
            __syncthreads();
            hi = lo;
        }
    }
}

// Exclusive prefix of one value per thread, sum or maximum (of values >= 0), in a fixed order: sequential over the 16 threads
// of a run, the 8 runs of a group and the groups; the total is left in g[GROUPS].  The maximum is exact in any order.
template <int THREADS, bool MAX>
__device__ __forceinline__ double qnt_scan(double* x, double* r, double* g, double mine, int tid) {
    constexpr int RUNS = THREADS / PSH_QNT_RUN, GROUPS = RUNS / PSH_QNT_GRP;
    __syncthreads();                                          // the arrays may still be read from the scan before
    x[tid] = mine;
    __syncthreads();
    if (tid < RUNS) {
        double acc = 0.0;
        for (int u = 0; u < PSH_QNT_RUN; ++u) {
            const int p = tid * PSH_QNT_RUN + u;
            const double v = x[p];
            x[p] = acc;
            acc = MAX ? fmax(acc, v) : acc + v;
        }
        r[tid] = acc;
    }
    __syncthreads();
    if (tid < GROUPS) {
        double acc = 0.0;
        for (int u = 0; u < PSH_QNT_GRP; ++u) {
            const int p = tid * PSH_QNT_GRP + u;
            const double v = r[p];
            r[p] = acc;
            acc = MAX ? fmax(acc, v) : acc + v;
        }
        g[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int u = 0; u < GROUPS; ++u) {
            const double v = g[u];
            g[u] = acc;
            acc = MAX ? fmax(acc, v) : acc + v;
        }
        g[GROUPS] = acc;
    }
    __syncthreads();
    const int run = tid / PSH_QNT_RUN, grp = run / PSH_QNT_GRP;
    return MAX ? fmax(fmax(g[grp], r[run]), x[tid]) : (g[grp] + r[run]) + x[tid];
}

}  // namespace

}  // namespace psh
