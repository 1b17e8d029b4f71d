// psh_wave.h -- the wave-wide and workgroup-wide reductions and scans every kernel of libpsh_hip.so is built from, stated
// once: the order of the additions is part of what the kernels promise ("bitwise repeatable", "bit-equal to the twin").
// Needs nothing of the scans (psh_device.h includes it; the statistics kernels take it alone).  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psh {

// ----------------------------------------------------------------------------------
// wave reductions: the butterfly 32, 16, .. 1 over the 64 lanes, the result in every lane.  Both lanes of a pair combine
// the same two numbers, so a commutative op leaves every lane with the same bits.
// ----------------------------------------------------------------------------------
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}

// The operators.  Floating-point minima and maxima are fminf / fmin / fmaxf / fmax and nothing else: they drop a NaN
// operand, which callers rely on (psh_weights.hip carries a NaN by a flag beside the maximum).  Integers compare as integers.
struct WaveSum { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct WaveOr { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a | b; } };
struct WaveMin {
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
};
struct WaveMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
};

template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, WaveSum{}); }
template <typename T> __device__ __forceinline__ T wave_or(T v) { return wave_reduce(v, WaveOr{}); }
template <typename T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, WaveMin{}); }
template <typename T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, WaveMax{}); }
// the smallest lo and the largest hi of the wave, one butterfly for both
template <typename T>
__device__ __forceinline__ void wave_minmax(T& lo, T& hi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
        lo = WaveMin{}(lo, l2);
        hi = WaveMax{}(hi, h2);
    }
}

// The maximum of a non-negative value over the wave, in every lane (uniform): four DPP steps inside the rows of 16 lanes, then the
// four rows through SGPRs -- no trip through the LDS crossbar (six dependent ds_bpermute are ~100+ cycles each beside a busy LDS).
__device__ __forceinline__ float wave_max_nonneg(float x) {
    // (as integers: non-negative floats order like their bit patterns, and an integer maximum needs no quieting of its operands
    //  -- fmaxf() cost a v_max x, x per operand and kept the DPP move a separate instruction; old = 0 with bound_ctrl lets the
    //  compiler fold the move into the v_max_i32 itself)
    int v = __float_as_int(x);
    auto step = [&](int moved) { v = v > moved ? v : moved; };
    step(__builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));     // quad_perm [1, 0, 3, 2]
    step(__builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));     // quad_perm [2, 3, 0, 1]
    step(__builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true));    // row_half_mirror
    step(__builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true));    // row_mirror
    const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const int r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    const int m01 = r0 > r1 ? r0 : r1, m23 = r2 > r3 ? r2 : r3;
    return __int_as_float(m01 > m23 ? m01 : m23);
}
// The sum of a value over the wave, in every lane (uniform), the same way: pairs, quads, half rows, rows by DPP, the four rows
// through SGPRs.  (The order of the additions is not the lane order: callers that bound a rounding error allow for any order.)
__device__ __forceinline__ float wave_sum_dpp(float x) {
    int v = __float_as_int(x);
    auto step = [&](int moved) { v = __float_as_int(__int_as_float(v) + __int_as_float(moved)); };
    step(__builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));     // quad_perm [1, 0, 3, 2]
    step(__builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));     // quad_perm [2, 3, 0, 1]
    step(__builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true));    // row_half_mirror
    step(__builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true));    // row_mirror
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(v, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(v, 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(v, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(v, 48));
    return (r0 + r1) + (r2 + r3);
}

// ----------------------------------------------------------------------------------
// the workgroup's fixed tree: the butterfly over each wave, lane 0 of wave w writes red[w], one barrier, and every thread
// folds red[0] op red[1] op .. left to right -- the fold STARTS at red[0], not at a zero, so a total of -0.0 stays -0.0.
// Every thread returns the same bits.  TAIL_BARRIER: a second barrier after the fold, for a caller that writes red[] again
// before anything else separates the two uses.  (A caller with a barrier of its own kind between the two halves, or with
// several values behind one barrier, takes the halves.)
// ----------------------------------------------------------------------------------
template <typename T, typename Op>
__device__ __forceinline__ void block_reduce_put(T v, T* red, Op op) {
    v = wave_reduce(v, op);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
}
template <int WAVES, typename T, typename Op>
__device__ __forceinline__ T block_reduce_fold(const T* red, Op op) {
    T s = red[0];
    for (int u = 1; u < WAVES; ++u) s = op(s, red[u]);
    return s;
}
template <int WAVES, bool TAIL_BARRIER = false, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T* red, Op op) {
    block_reduce_put(v, red, op);
    __syncthreads();
    const T s = block_reduce_fold<WAVES>(red, op);
    if (TAIL_BARRIER) __syncthreads();
    return s;
}

// ----------------------------------------------------------------------------------
// wave scans (inclusive sums in lane order; lane: the caller's lane id, which it holds anyway)
// ----------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(T v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}
// the same on the DPP path (no LDS crossbar): row_shr 1, 2, 4, 8 inside the rows of 16 lanes, then row_bcast 15 into rows
// 1 and 3 and row_bcast 31 into rows 2 and 3
__device__ __forceinline__ int wave_scan_inclusive_dpp(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, true);
    return v;
}
// the wave's total, uniform (an SGPR)
__device__ __forceinline__ int wave_total_dpp(int v) { return __builtin_amdgcn_readlane(wave_scan_inclusive_dpp(v), 63); }

// ----------------------------------------------------------------------------------
// which bucket of a histogram holds the rank-th (1-based) entry: called by ONE wave, lane l owning the PER counters
// hist[PER l .. PER l + PER).  The lanes' sums are scanned; exactly one lane finds before < rank <= before + its own sum
// (none when rank exceeds the total), walks its PER counters and calls owner(RankBucket) -- inside the one divergent
// region the walk runs in: handing the answer back to every lane first cost the callers a second region (and two more
// spilled SGPRs in psh_fused.hip and psh_stream.hip).  Every lane returns whether it was the one.
// ----------------------------------------------------------------------------------
struct RankBucket {
    int bucket;
    unsigned before;    // entries in the buckets below `bucket`
    unsigned count;     // entries in `bucket`: before < rank <= before + count
};
// (the lane's counters and their place in the wave's running count: read and scanned once for a caller with two ranks)
template <int PER>
struct RankHist {
    unsigned h[PER], before, upto;
    int first;
    __device__ __forceinline__ RankHist(const unsigned* hist, int lane) : first(PER * lane) {
        unsigned sl = 0;
#pragma unroll
        for (int c = 0; c < PER; ++c) { h[c] = hist[PER * lane + c]; sl += h[c]; }
        upto = wave_scan_inclusive(sl, lane);
        before = upto - sl;
    }
    template <typename F>
    __device__ __forceinline__ bool find(unsigned rank, F owner) const {
        unsigned cum = before;
        const bool mine = cum < rank && upto >= rank;
        if (mine) {
            RankBucket r{first, cum, 0u};
#pragma unroll
            for (int c = 0; c < PER; ++c) {
                if (cum < rank && cum + h[c] >= rank) r = RankBucket{first + c, cum, h[c]};
                cum += h[c];
            }
            owner(r);
        }
        return mine;
    }
};
template <int PER, typename F>
__device__ __forceinline__ bool rank_bucket(const unsigned* hist, int lane, unsigned rank, F owner) {
    return RankHist<PER>(hist, lane).find(rank, owner);
}
// The largest key bucket `bucket` of a histogram over (key - kmin) >> shift can hold, clamped to kmax.  Every entry in the
// buckets <= `bucket` is at or below that edge, and when `bucket` holds the rank-th entry there are >= rank of them: the edge
// is an upper bound of the rank-th smallest key.
__device__ __forceinline__ unsigned bucket_upper_edge(unsigned kmin, unsigned kmax, int bucket, int shift) {
    const unsigned long long e = (unsigned long long)kmin + (((unsigned long long)bucket + 1ull) << shift) - 1ull;
    return e > (unsigned long long)kmax ? kmax : (unsigned)e;
}

}  // namespace psh
