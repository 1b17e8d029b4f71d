// psh_segment.h -- what the scan kernels of libpsh_hip.so share per SEGMENT: its staging from HBM into LDS, the work queue
// of a block (the units it owns, the next one, which row and segment a unit is, its load) and the one-query rejection
// test on the matrix cores for W <= 33 (scan_mx_kernel, scan_fused_kernel, stream_scan_kernel).  Internal; every function
// is forced inline, the kernels keep their names and signatures.  psh_scan.hip has the design overview and the test's
// error bound.
#pragma once
#include "psh_device.h"

namespace psh {

// ----------------------------------------------------------------------------------
// staging a segment
// ----------------------------------------------------------------------------------
struct Stage {  // one segment in flight from HBM, 5 x 16 bytes per lane
    f32x4 v[PSH_NSTAGE];
};

// one of the PSH_NSTAGE 16-byte loads of a segment (q is a compile-time index at every
// call site).  row: first float of the row; floats [seg_start, seg_start + nfloat) are
// wanted, clamped to the row (the clamped tail only feeds inadmissible windows).
template <bool ALIGNED>
__device__ __forceinline__ void stage_load_one(Stage& st, int q, const float* __restrict__ row, int64_t T,
                                               int seg_start, int nfloat, int lane) {
    if (ALIGNED) {
        const f32x4* src = reinterpret_cast<const f32x4*>(row + seg_start);
        const int last = (int)((T - seg_start) >> 2) - 1;  // last float4 inside the row
        const int nq = (nfloat + 3) >> 2;                   // 256 <= nq <= 320
        int m = lane + 64 * q;
        if (q < PSH_NSTAGE - 1 || m < nq) {
            m = m > last ? last : m;
            st.v[q] = __builtin_nontemporal_load(src + m);
        }
    } else {
        const int lastf = (int)(T - seg_start) - 1;
        float e[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            int p = 4 * (lane + 64 * q) + c;
            p = p > lastf ? lastf : p;
            e[c] = (4 * (lane + 64 * q) < nfloat) ? row[seg_start + p] : 0.0f;
        }
        st.v[q] = f32x4{e[0], e[1], e[2], e[3]};
    }
}

template <bool ALIGNED>
__device__ __forceinline__ void stage_load(Stage& st, const float* __restrict__ row, int64_t T,
                                           int seg_start, int nfloat, int lane) {
#pragma unroll
    for (int q = 0; q < PSH_NSTAGE; ++q) stage_load_one<ALIGNED>(st, q, row, T, seg_start, nfloat, lane);
}

template <bool PAD = true>
__device__ __forceinline__ void stage_store(const Stage& st, float* tile, int nfloat, int lane) {
    const int nq = (nfloat + 3) >> 2;
#pragma unroll
    for (int q = 0; q < PSH_NSTAGE; ++q) {
        const int m = lane + 64 * q;
        if (q < PSH_NSTAGE - 1 || m < nq) *reinterpret_cast<f32x4*>(tile + lds_idx<PAD>(4 * m)) = st.v[q];
    }
}

// ----------------------------------------------------------------------------------
// the unit queue of a block
// ----------------------------------------------------------------------------------
// A unit is one segment of one row (times a query group where the kernel has them).  Waves of one SIMD are served oldest
// first, so with a static split the young waves of every SIMD finish up to 2x later than the old ones and the tail of the
// launch runs at a fraction of the occupancy (measured: waves end between 69 and 149 us).  All waves of the block therefore
// pull units from one LDS counter; the block's own share [lo, hi) of the units is static.
struct UnitQueue {
    unsigned lo, hi;
    int* next;                                   // LDS counter: units of this block handed out so far
    // next unit of this block (wave-uniform), >= hi when exhausted
    __device__ __forceinline__ unsigned grab(int lane) const {
        int v = 0;
        if (lane == 0) v = atomicAdd(next, 1);
        return lo + (unsigned)__builtin_amdgcn_readfirstlane(v);
    }
};
// the even share of n units (host guarantees n < 2^31) for this block
__device__ __forceinline__ UnitQueue unit_queue(unsigned n, int* next) {
    return UnitQueue{(unsigned)(((unsigned long long)n * blockIdx.x) / gridDim.x),
                     (unsigned)(((unsigned long long)n * (blockIdx.x + 1)) / gridDim.x), next};
}

struct Unit {
    unsigned qg, rs, ri, sg;                     // query group, (row, segment) index, row index, segment
    __device__ __forceinline__ int seg_start() const { return (int)sg * PSH_SEG; }
    __device__ __forceinline__ int64_t row(const ScanArgs& a) const { return a.row0 + (int64_t)ri * a.row_stride; }
};
// unit -> (row index, segment)
__device__ __forceinline__ Unit unit_decode(const ScanArgs& a, unsigned u) {
    const unsigned ri = fast_div(u, a.magic_nseg, (unsigned)a.nseg);
    return Unit{0u, u, ri, u - ri * (unsigned)a.nseg};
}
// unit -> (query group, row index, segment); n_rs = n_rows * nseg
__device__ __forceinline__ Unit unit_decode(const ScanArgs& a, unsigned u, unsigned n_rs) {
    const unsigned qg = fast_div(u, a.magic_nrs, n_rs);
    Unit c = unit_decode(a, u - qg * n_rs);
    c.qg = qg;
    return c;
}
// the unit's segment into the staging registers; rows row0 + ri * row_stride (the bootstrap samples walk their own rows)
template <bool ALIGNED>
__device__ __forceinline__ void load_unit(Stage& st, const ScanArgs& a, int64_t row0, int64_t row_stride, const Unit& c,
                                          int nfloat, int lane) {
    stage_load<ALIGNED>(st, a.dataset + (row0 + (int64_t)c.ri * row_stride) * a.T, a.T, (int)c.sg * PSH_SEG, nfloat, lane);
}
template <bool ALIGNED>
__device__ __forceinline__ void load_unit(Stage& st, const ScanArgs& a, const Unit& c, int nfloat, int lane) {
    load_unit<ALIGNED>(st, a, a.row0, a.row_stride, c, nfloat, lane);
}

// ----------------------------------------------------------------------------------
// the one-query f16 segment test on the matrix cores, W <= 33 (the bound: psh_scan.hip, above scan_mx_kernel)
// ----------------------------------------------------------------------------------
// the f16 staging layout (also scan_mq_kernel / scan_mq8_kernel / boot_mq_kernel)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define PSH_MX_SLOTS 144                      // 16-byte slots per f16 array: 32*31 + 64 values, whole groups of 16 slots
#define PSH_MX_NHALF (PSH_MX_SLOTS * 8)
#define PSH_MX_PEND 64                        // >= 64: one ballot can admit a whole wave

// logical f16 index -> LDS index.  A-fragment reads of the 32 rows sit 64 bytes apart
// (4 slots): rotating the slot inside its group of 16 by the group number spreads 16
// consecutive rows over 16 distinct slots without any padding.
__device__ __forceinline__ int mx_half(int idx) {
    const int slot = idx >> 3;
    return (((slot & ~15) | ((slot + (slot >> 4)) & 15)) << 3) | (idx & 7);
}

// A wave's two f16 arrays (y^, then (y~^2)^: PSH_MX_NHALF halves each, contiguous) start out as zeros: the tail slots no
// segment ever writes must hold finite values -- the banded product multiplies them by its zero taps, and 0 * NaN
// poisons a row.
__device__ __forceinline__ void mx_zero(_Float16* ah, int lane) {
    unsigned* z = reinterpret_cast<unsigned*>(ah);
    for (int i = lane; i < PSH_MX_NHALF; i += 64) z[i] = 0u;              // 2 arrays x NHALF halves = NHALF dwords
}

// B fragments: lane (n = lane & 31, hk = lane >> 5) holds k = 16 s + 8 hk + i, i < 8.  Column n is the band shifted down
// by n: the band of ones (window energies) ...
__device__ __forceinline__ void mx_band_ones(f16x8 (&bo)[4], int W, int lane) {
    const int n = lane & 31, hk = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = 16 * s + 8 * hk + i - n;
            bo[s][i] = (_Float16)((j >= 0 && j < W) ? 1.0f : 0.0f);
        }
}
// ... and the shifted query, B[k][n] = -2 x^[k - n]
__device__ __forceinline__ void mx_band_query(f16x8 (&bx)[4], const_f32p x, float scale, int W, int lane) {
    const int n = lane & 31, hk = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = 16 * s + 8 * hk + i - n;
            const bool in = j >= 0 && j < W;
            const float xv = x[in ? j : 0];
            bx[s][i] = (_Float16)(in ? -2.0f * (xv * scale) : 0.0f);
        }
}

// the f16 copies of a staged segment: y^ and (y~^2)^, 4 values = one 8-byte store per array and chunk (the partial last
// stage as stage_store has it)
__device__ __forceinline__ void mx_convert(const Stage& st, _Float16* a1, _Float16* a2, float scale, int nfloat, int lane) {
    const int nq = (nfloat + 3) >> 2;
#pragma unroll
    for (int q = 0; q < PSH_NSTAGE; ++q) {
        const int m = lane + 64 * q;
        if (q < PSH_NSTAGE - 1 || m < nq) {
            const f32x4 v = st.v[q] * scale;
            const f32x4 v2 = v * v;
            *reinterpret_cast<f16x4*>(a1 + mx_half(4 * m)) = __builtin_convertvector(v, f16x4);
            *reinterpret_cast<f16x4*>(a2 + mx_half(4 * m)) = __builtin_convertvector(v2, f16x4);
        }
    }
}

// four A fragments per LDS round trip: row m = lane & 31 of A is the 64 consecutive values [32 m, 32 m + 64) of `arr`
__device__ __forceinline__ void mx_load_a(f16x8 (&fa)[4], const _Float16* arr, int lane) {
    const int m = lane & 31, hk = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) fa[s] = *reinterpret_cast<const f16x8*>(arr + mx_half(32 * m + 16 * s + 8 * hk));
}
// c + A B over the four K-steps; b(s): the B fragment of K-step s (registers, or read from LDS per use).  c is the C
// operand of the first MFMA: a product seeded with the window energies needs no copy.
template <typename BFrag>
__device__ __forceinline__ f32x16 mx_mac4(const f16x8 (&fa)[4], BFrag b, const f32x16& c) {
    f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0], b(0), c, 0, 0, 0);
#pragma unroll
    for (int s = 1; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[s], b(s), acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ f32x16 mx_mac4(const f16x8 (&fa)[4], const f16x8 (&b)[4], const f32x16& c) {
    return mx_mac4(fa, [&](int s) { return b[s]; }, c);
}
// the window energies of the segment: A = (y~^2)^, B = the band of ones
__device__ __forceinline__ f32x16 mx_energies(f16x8 (&fa)[4], const _Float16* a2, const f16x8 (&bo)[4], int lane) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    mx_load_a(fa, a2, lane);
    return mx_mac4(fa, bo, acc);
}

// bit r: the window of accumulator r is NOT provably above thr (NaN-safe: !(t^ > thr))
__device__ __forceinline__ unsigned mx_keep_mask(const f32x16& acc, float thr) {
    unsigned hm = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) hm |= !(acc[r] > thr) ? (1u << r) : 0u;
    return hm;
}
// any window of the wave's segment left to look at (about one segment in four)
__device__ __forceinline__ bool mx_any_keep(const f32x16& acc, float thr) {
    bool keep = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) keep = keep || !(acc[r] > thr);
    return __any(keep);
}
// C layout of the 32x32 MFMA: accumulator r of lane (m = lane & 31, hk = lane >> 5) is row (r & 3) + 8 (r >> 2) + 4 hk,
// column m -> the window's index in the segment
__device__ __forceinline__ int mx_window(int r, int lane) {
    const int m = lane & 31, hk = lane >> 5;
    return 32 * ((r & 3) + 8 * (r >> 2) + 4 * hk) + m;
}
// the exact chain of the window at tile index p
template <int WT>
__device__ __forceinline__ float mx_exact(const float* tile, int p, const_f32p x, int W) {
    if constexpr (WT > 0) return exact_one<(WT > 0 ? WT : 20)>(tile, p, x);
    else return exact_one_rt(tile, p, x, W);
}

// The survivors of one query's accumulator tile: the exact chain from the fp32 tile, and what comes out below tau goes
// to the block's front list fl[cap] behind the LDS cursor (one atomic per ballot).  The cursor counts past cap: the
// caller sees the overflow there; overflow(v, t) is called for every entry that found no slot.
template <int WT, typename Overflow>
__device__ __forceinline__ void mx_admit(const f32x16& acc, float thr, float tau, const float* tile, const_f32p x, int W,
                                         int seg_start, int Tp, int r_global, unsigned q, u32x4* fl, int cap, int* cursor,
                                         int lane, Overflow overflow) {
    const unsigned hm = mx_keep_mask(acc, thr);
#pragma unroll 1
    for (int r = 0; r < 16; ++r) {
        const int p = mx_window(r, lane);
        bool hit = (((hm >> r) & 1u) != 0u) && (seg_start + p < Tp);
        if (!__ballot(hit)) continue;
        float v = 0.0f;
        if (hit) v = mx_exact<WT>(tile, p, x, W);
        hit = hit && (v < tau);
        const unsigned long long mask = __ballot(hit);
        if (!mask) continue;
        int base = 0;
        if (lane == 0) base = atomicAdd(cursor, __popcll(mask));
        base = __builtin_amdgcn_readfirstlane(base);
        if (hit) {
            const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
            if (slot < cap) fl[slot] = u32x4{__float_as_uint(v), (unsigned)r_global, (unsigned)(seg_start + p), q};
            else overflow(v, seg_start + p);
        }
    }
}

// A block's list of admitted windows is full (clustered matches: a smooth ensemble -- price levels, not returns -- puts a
// window's neighbours in t next to it in distance too): the entry goes straight to the query's compact list in memory, one
// device-scope atomic per entry (r05; until then such a step gave up -- PSH_STATUS_RETRY -- and the caller ran the separate launches)
__device__ __forceinline__ void spill_candidate(FusedHdr* hdr, void* cand_list, int cand_cap, int q, float xn, float acc, int r_global, int t) {
    const unsigned slot = __hip_atomic_fetch_add((gu32*)&hdr->stream.ncand[q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot < (unsigned)cand_cap)
        reinterpret_cast<u32x4*>(cand_list)[(size_t)q * cand_cap + slot] = u32x4{__float_as_uint(dist_from_acc(acc, xn)), (unsigned)r_global, (unsigned)t, (unsigned)q};
}

// the rejection threshold's constants when the scan streams the resident f16 copy (derivation: psh_stream_copy.hip, above
// copy_scan_kernel): relative part a, absolute part b (up to W = 31; (2 W + 2) / 64 of it beyond, as on the fp32 route)
#define PSH_COPY_A (1.0 / 320.0)
#define PSH_COPY_B (1.0 / 131072.0)

}  // namespace psh
