// psh_long.h -- what the LONG-WINDOW kernels of libpsh_hip.so (34 <= W <= 256 for one to three queries, 26 <= W <= 256 for
// batches) share per SEGMENT, stated once: the geometry of a wave's f16 rows, the segment's staging by buffer loads, the
// tile's C operand from the prefix sums, the minimum of a tile, the upper bound of the sample, a query's tables, the zero
// fill of the rows and the exact chain of a queued window.  Internal; every function is forced inline.
//
// Who calls what:
//                           stream_scan_long_body   stream_sample_long_body   scan_lq_kernel
//                           (psh_stream.hip)        (psh_stream.hip)          (psh_lq.hip)
//   long_stage_row          AUX 2 (nt)              AUX 0                     AUX 0
//   long_energy_operand     lower                   own text (*)              by MODE
//   long_tile_min           --                      own text (*)              BOOT
//   long_upper_bound        --                      yes                       BOOT, main branch
//   long_query_tables       -- (copies bxtab)       yes                       yes
//   long_zero_rows          yes                     yes (twice)               yes
//   long_exact_window       scalar query loads      --                        16-byte query loads
//
// (*) Sites left as they were, because the shared form made the compiler's output worse there (the numbers, kernel by
// kernel: profiles/long_refactor_compare.txt, 4.):
//   * the segment's conversion -- f16 rows, prefix sums of the squares, the carry -- in all three kernels; its error bound
//     stays where it was derived, in stream_scan_long_body (2 to 16 more VGPRs, spills in stream_sample_long_kernel1);
//   * +inf in the C operand for the windows a row does not have, in both scans (14 more VGPRs in stream_scan_long_kernel);
//   * the C operand and the tile's minimum in stream_sample_long_body (spills: the kernel is held to 128 registers).
//
// What stays where it is, on purpose:
//   * kernel names and template signatures (the benchmark and tools/summarize_pmc.py name them);
//   * prefix_store of psh_embed_px.hip: plain sums, a double carry, the |y| sum, one group at a time -- another scan;
//   * copy_scan_kernel's verify_queue: the audit of the f16 copy is interleaved with its chain;
//   * the K-loops (long_chain, the sample's unrolled loop, run_group): their pipelines differ on purpose;
//   * the near-match branch of the upper bound (`loose` in the sample, the estimate in scan_lq_kernel);
//   * stream_sample_finish, the survivors' queues and their publication.
#pragma once
#include "psh_segment.h"

namespace psh {

// ----------------------------------------------------------------------------------
// geometry
// ----------------------------------------------------------------------------------
// A wave's f16 rows: ROWS of 32 consecutive samples y^ of the segment followed by 8 halves of padding -- 40 halves = 80
// bytes = 20 dwords a row: the 16 lanes of a ds_read_b128 group (rows m with all 16 residues mod 16, 4 dwords each) fall on
// 20 m mod 64 = 16 different multiples of 4.  The A fragment of row m, K-step s lies at row m + (s >> 1), halves
// 16 (s & 1) + 8 hk .. + 7 of it: per PAIR of K-steps one pointer moves by one row and every other offset is an immediate
// (the slot-rotation layout of the short kernels, mx_half, cost the K-loop 7 vector instructions per step for the address
// alone, and on this part vector instructions ADD to the matrix cores' time).  There is no row of squares: the window
// energies come from the fp32 prefix sums S[0 .. SEG + W - 1] beside the rows (stream_scan_long_body has the construction and its bound), and enter the product as
// its C operand (long_energy_operand).
#define PSH_LONG_ROW 40
#define PSH_LONG_SFLOATS 1280         // fp32 prefix sums of a segment's squares: entries 0 .. SEG + W - 1 <= 1279; scratch afterwards
#define PSH_LONG_QCAP 64              // deferred survivors a wave keeps before it verifies them (8 bytes an entry)
#define PSH_LONG_GAMMA 7.62939453125e-06f   // 2^-17: what the energies from prefix sums may be off by, per unit of S[p + W] (stream_scan_long_body)
__host__ __device__ constexpr int long_rows(int nks) { return 31 + (nks + 1) / 2; }            // rows the band of row 31 reaches in nks K-steps
__host__ __device__ constexpr int long_nhalf(int nks) { return long_rows(nks) * PSH_LONG_ROW; }  // halves of a wave's rows

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // four floats at any float's address

// ----------------------------------------------------------------------------------
// staging
// ----------------------------------------------------------------------------------
// A segment is staged by BUFFER loads: the row is the resource (base = its first float, records = its bytes), a lane's five
// 16-byte pieces sit at one constant VGPR offset + immediates, the segment's start is the scalar offset -- no address
// arithmetic on the vector ALUs, and what lies beyond the row reads as zero (it only feeds inadmissible windows).  Rows need
// 4-byte alignment only: one code path for aligned and unaligned ensembles.  AUX: the loads' cache policy (0, or 2 = nt).
template <int AUX>
__device__ __forceinline__ void long_stage_row(Stage& st, const float* dataset, int64_t T, int64_t row, int seg_start, int nfloat, int lane) {
    const int64_t bytes = T * 4;
    const __amdgpu_buffer_rsrc_t rs = buffer_rsrc(dataset + row * T, (unsigned)(bytes > 0x7ffffffc ? 0x7ffffffc : bytes));
    const int nq4 = (nfloat + 3) >> 2;
    const int lane16 = lane * 16;
#pragma unroll
    for (int q = 0; q < PSH_NSTAGE; ++q)
        if (q < PSH_NSTAGE - 1 || lane + 64 * q < nq4) {
            const u32x4v w = __builtin_amdgcn_raw_buffer_load_b128(rs, lane16 + 1024 * q, seg_start * 4, AUX);
            st.v[q] = f32x4{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3])};
        }
}

// ----------------------------------------------------------------------------------
// the tile's C operand
// ----------------------------------------------------------------------------------
// What the prefix sums say about the 16 windows of this lane (ps_lo = sp + m + 128 hk, ps_hi = ps_lo + W: slot r is window
// p = mx_window(r, lane)): a LOWER bound of the energies, E^(p) - gamma S^[p + W], or an UPPER one, E^(p) + gamma S^[p + W].
template <bool UPPER>
__device__ __forceinline__ f32x16 long_energy_operand(const float* ps_lo, const float* ps_hi) {
    f32x16 ce;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int off = 32 * (r & 3) + 256 * (r >> 2);
        ce[r] = __builtin_fmaf(ps_hi[off], UPPER ? 1.0f + PSH_LONG_GAMMA : 1.0f - PSH_LONG_GAMMA, -ps_lo[off]);
    }
    return ce;
}

// ----------------------------------------------------------------------------------
// the sample: minimum of a tile, upper bound of the unit's smallest acc
// ----------------------------------------------------------------------------------
// the smallest value of a tile over the windows that exist, in every lane (fminf: a NaN slot is dropped)
__device__ __forceinline__ float long_tile_min(const f32x16& c, int nvalid, int lane) {
    float mn = __uint_as_float(PSH_INF_BITS);
    if (nvalid >= PSH_SEG) {
#pragma unroll
        for (int r = 0; r < 16; ++r) mn = fminf(mn, c[r]);
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mx_window(r, lane);
            mn = p < nvalid ? fminf(mn, c[r]) : mn;
        }
    }
    return wave_min(mn);
}
// An upper bound of the smallest acc of a unit from its estimate est = max(t^ + nx~, 0), back in the data's scale (the
// sample's scale is 2^sexp).  With 2 |c^ - c| <= a (nx~ + E) and E <= 2 (nx~ + acc~) (stream_threshold's model, a = 1 / 900,
// read the other way round):
//     acc~ (1 - 2 a) <= t^ + nx~ (1 + 3 a) + b,     b = long_bound_b(W).
// NaN data: the unit carries no information, +inf.  (A near-match -- est < nx~ / 6, where this bound is the 3 a nx~ term
// alone -- is each caller's own business.)
__device__ __forceinline__ float long_bound_b(int W) { return (float)(2 * W + 2) / 64.0f / 262144.0f; }
__device__ __forceinline__ float long_unscale(float ub, int sexp) {
    const float inv = __uint_as_float((unsigned)(127 - sexp) << 23);
    ub = ub * inv * inv;
    if (!(ub == ub)) ub = __uint_as_float(PSH_INF_BITS);
    return ub;
}
__device__ __forceinline__ float long_upper_bound(float est, float nx, int W, int sexp) {
    return long_unscale((est + nx * (3.0f / 900.0f) + long_bound_b(W)) * (1.0f + 2.0f / 900.0f + 1.0e-5f + 6.0f * PSH_LONG_GAMMA) * (1.0f + 1e-6f), sexp);
}

// ----------------------------------------------------------------------------------
// tables and zero fill
// ----------------------------------------------------------------------------------
// The B fragments of nq queries xs[query][W] (in LDS) as eight shifted copies of -2 x~ each (psh_kernels.h, lq_copy_chunks):
// tab[query][copy c < 8][chunk v < CP][8 halves], copy c, chunk v, half i holds -2 x~[8 (v - 3) + i - c]; zero outside the window.
template <int NKS>
__device__ __forceinline__ void long_query_tables(_Float16* tab, const float* xs, int nq, int W, float scale, int tid, int nthreads) {
    constexpr int CP = lq_copy_chunks(NKS), QS = lq_query_bytes(NKS) / 2;     // chunks a copy, HALVES a query
    for (int e = tid; e < nq * 8 * CP; e += nthreads) {
        const int v = e % CP, c = (e / CP) & 7, q = e / (8 * CP);
        const float* xq = xs + (size_t)q * W;
        f16x8 b;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = 8 * (v - 3) + i - c;
            const bool in = j >= 0 && j < W;
            const float xv = xq[in ? j : 0];
            b[i] = (_Float16)(in ? -2.0f * (xv * scale) : 0.0f);
        }
        *reinterpret_cast<f16x8*>(tab + (size_t)q * QS + ((size_t)c * CP + v) * 8) = b;
    }
}
// every slot of the rows a segment does not write must be finite (the band's zero taps multiply them: 0 * NaN poisons a row)
__device__ __forceinline__ void long_zero_rows(_Float16* a1, int words, int lane) {
    unsigned* z = reinterpret_cast<unsigned*>(a1);
    for (int i = lane; i < words; i += 64) z[i] = 0u;
}

// ----------------------------------------------------------------------------------
// the exact chain of one queued window
// ----------------------------------------------------------------------------------
// A lane per queued window: its W samples straight from memory, 16 bytes a load (64 scattered requests an instruction, all
// of them L2 / MALL hits: the segment was streamed microseconds ago), the chain in the reference's order.  XP: the query
// pointer's type -- const_f32p: scalar loads (a uniform query), const float*: 16-byte vector loads (a query per lane).
__device__ __forceinline__ f32x4u long_load4(const float* p) { return *reinterpret_cast<const f32x4u*>(p); }
__device__ __forceinline__ f32x4u long_load4(const_f32p p) { return f32x4u{p[0], p[1], p[2], p[3]}; }
template <typename XP>
__device__ __forceinline__ float long_exact_window(const float* y, XP x, int W) {
    float v = 0.0f;
    int j = 0;
#pragma unroll 2
    for (; j + 4 <= W; j += 4) {
        const f32x4u yy = long_load4(y + j), xx = long_load4(x + j);
#pragma unroll
        for (int c = 0; c < 4; ++c) { const float D = __fsub_rn(xx[c], yy[c]); v = __builtin_fmaf(D, D, v); }
    }
    for (; j < W; ++j) { const float D = __fsub_rn(x[j], y[j]); v = __builtin_fmaf(D, D, v); }
    return v;
}

}  // namespace psh
