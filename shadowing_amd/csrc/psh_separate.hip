// psh_separate.hip -- time-separated nearest windows (psh_separate_topk): the exclusion zone of subsequence search on the
// (B, K) list a scan returns, so that the k shadowing paths of a date are k draws and not a window and its one-sample
// shifts.  Host twin: shadowing_amd/separation.py.
//
// The definition (shared with the twin, include/psh.h and README "Separated neighbours"):
//   One query has a list of K entries (d_i, r_i, t_i), i = 0 .. K-1, in the order given (the scan hands it over ascending in
//   (d, r, t)).  The rule reads positions and indices only, never d.  Delta >= 0 is an integer number of samples.
//     keep_i  =  r_i >= 0  and  there is no j < i with keep_j, r_j == r_i and |t_j - t_i| <= Delta
//   Row b of the outputs holds the first k kept entries in list order: the bits of d, [r, t], and the position i.
//   out_count[b] is the number kept among all K (it may exceed k); out_count[b] < k sets PSH_SEPARATE_STATUS_SHORT and
//   leaves +inf, (-1, -1), -1 in the slots past the count.
//
// The method: one workgroup per query, the list in LDS, no atomics, no floating-point arithmetic at all.
//   1. Sort (r << 32) | i with the network of psh_sort_lds.h: rows together, each in list order; padding (r < 0, and the
//      fill up to a power of two) takes r = 0xffffffff and sorts last.
//   2. A prefix count of the row heads gives every entry a dense row number s < K; t is gathered from the list by i.
//   3. Sort (s << 45) | (t << 14) | i: every row in time order, each entry carrying its list position (i < 2^14, t < 2^31,
//      s < 2^14: 59 bits; padding keeps every bit above 14 set and matches no row).
//   4. Settle one state byte per list position in rounds.  A thread owns 2^NB consecutive sorted positions.  An undecided
//      entry walks its time-neighbours of the same row, to the left and to the right, while |dt| <= Delta (dt is a
//      difference of two values in [0, 2^31): nothing is ever added to Delta).  It is DROPPED at the first neighbour
//      with a smaller position that is kept, KEPT when every neighbour with a smaller position is dropped (or there is
//      none), and waits otherwise.  A decision is only taken on decisions that are final, so the fixed point is the
//      greedy walk's, whatever the order in which threads see each other's bytes inside a round; a round ends with one
//      barrier that carries "anything changed", and the undecided entry with the smallest position settles in every
//      round, so there are at most K rounds (the loop is bounded by that).  A thread sweeps its positions upwards and
//      then downwards in a round, so a chain that runs along the time axis settles 2^NB links a round.
//   5. An integer prefix count of the kept flags in list order gives the output slots.
//   LDS at K = 16384: 136 KiB of entries (padded as in psh_quantiles.hip: entry i at i + i / 16), 16 KiB of state bytes,
//   64 bytes of wave totals.  Three instantiations by capacity, as the other kernels on this network:
//   K <= 1024 (256 threads, NB = 2), K <= 4096 (512 threads, NB = 3), K <= 16384 (1024 threads, NB = 4).
//   The walk of one entry is linear in its neighbours, a round's work is spread over the workgroup; the worst number of
//   rounds is one row whose positions rise with t at Delta = 1 (K / 2^NB rounds of one barrier each), the longest walks
//   are one row at Delta >= its span (K neighbours an entry, two or three rounds).  README "Separated neighbours" holds
//   the measured times of both (tools/bench_separation.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_sort_lds.h"
#include "psh_wave.h"

namespace psh {

namespace {

#define PSH_SEP_UNDECIDED 0
#define PSH_SEP_KEPT 1
#define PSH_SEP_DROPPED 2

// exclusive prefix sum of one int per thread in thread order; the workgroup's total in `total`
template <int WAVES>
__device__ __forceinline__ int sep_scan(int v, int* wsum, int tid, int& total) {
    const int lane = tid & 63, wave = tid >> 6;
    const int inc = wave_scan_inclusive(v, lane);
    __syncthreads();                                          // wsum may still be read from the scan before
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int u = 0; u < WAVES; ++u) {
        const int w = wsum[u];
        base += u < wave ? w : 0;
        tot += w;
    }
    total = tot;
    return base + inc - v;
}

template <int CAP, int THREADS, int NB>
__global__ __launch_bounds__(THREADS) void separate_kernel(SeparateArgs a) {
    constexpr int E = 1 << NB, WAVES = THREADS / 64;
    static_assert(E * THREADS == CAP && CAP <= (1 << 14), "geometry");
    __shared__ uint64_t ent[CAP + CAP / 16];
    __shared__ uint8_t state[CAP];
    __shared__ int wsum[WAVES];
    const int tid = (int)threadIdx.x, K = a.K, k = a.k;
    const int64_t b = (int64_t)blockIdx.x;
    const int32_t* idx = a.idx + b * K * 2;
    const uint32_t delta = (uint32_t)a.delta;
    const int p0 = tid * E;                                   // my sorted positions, and later my list positions

    int n2 = E;
    while (n2 < K) n2 <<= 1;                                  // K <= CAP: the launcher chose the instantiation

    // ---- 1. rows together, each in list order
    for (int j = tid; j < n2; j += THREADS) {
        const int32_t r = j < K ? idx[2 * j] : -1;
        ent[qnt_phys(j)] = ((uint64_t)(r < 0 ? 0xffffffffu : (uint32_t)r) << 32) | (uint32_t)j;
        state[j] = r < 0 ? PSH_SEP_DROPPED : PSH_SEP_UNDECIDED;
    }
    __syncthreads();
    qnt_sort<NB, THREADS>(ent, n2, tid);

    // ---- 2. dense row numbers
    uint64_t v[E];
    const uint32_t left = p0 > 0 && p0 < n2 ? (uint32_t)(ent[qnt_phys(p0 - 1)] >> 32) : 0xffffffffu;
    int heads = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        v[e] = p0 + e < n2 ? ent[qnt_phys(p0 + e)] : ~0ull;
        const uint32_t r = (uint32_t)(v[e] >> 32), before = e ? (uint32_t)(v[e ? e - 1 : 0] >> 32) : left;
        heads += (p0 + e == 0 || r != before) ? 1 : 0;
    }
    int total;
    int s = sep_scan<WAVES>(heads, wsum, tid, total) - 1;     // (the scan's barriers stand between the reads and the stores)
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (p0 + e >= n2) break;
        const uint32_t r = (uint32_t)(v[e] >> 32), before = e ? (uint32_t)(v[e ? e - 1 : 0] >> 32) : left, i = (uint32_t)v[e];
        s += (p0 + e == 0 || r != before) ? 1 : 0;
        uint64_t key = (~0ull << 14) | i;
        if (r != 0xffffffffu) key = ((uint64_t)s << 45) | ((uint64_t)((uint32_t)idx[2 * i + 1] & 0x7fffffffu) << 14) | i;
        ent[qnt_phys(p0 + e)] = key;
    }
    __syncthreads();

    // ---- 3. every row in time order
    qnt_sort<NB, THREADS>(ent, n2, tid);

    // ---- 4. settle
    unsigned pending = 0;
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (p0 + e < n2 && (ent[qnt_phys(p0 + e)] >> 45) != 0x7ffffull) pending |= 1u << e;

    auto settle = [&](int e) {
        const int p = p0 + e;
        const uint64_t kp = ent[qnt_phys(p)];
        const uint64_t sp = kp >> 45;
        const uint32_t tp = (uint32_t)(kp >> 14) & 0x7fffffffu, ip = (uint32_t)kp & 0x3fffu;
        bool drop = false, blocked = false;
        for (int q = p - 1; q >= 0; --q) {
            const uint64_t kq = ent[qnt_phys(q)];
            if ((kq >> 45) != sp || tp - ((uint32_t)(kq >> 14) & 0x7fffffffu) > delta) break;
            const uint32_t iq = (uint32_t)kq & 0x3fffu;
            if (iq < ip) {
                const uint8_t st = state[iq];
                if (st == PSH_SEP_KEPT) { drop = true; break; }
                blocked |= st == PSH_SEP_UNDECIDED;
            }
        }
        for (int q = p + 1; q < n2 && !drop; ++q) {
            const uint64_t kq = ent[qnt_phys(q)];
            if ((kq >> 45) != sp || ((uint32_t)(kq >> 14) & 0x7fffffffu) - tp > delta) break;
            const uint32_t iq = (uint32_t)kq & 0x3fffu;
            if (iq < ip) {
                const uint8_t st = state[iq];
                if (st == PSH_SEP_KEPT) drop = true;
                blocked |= st == PSH_SEP_UNDECIDED;
            }
        }
        if (!drop && blocked) return 0;
        state[ip] = drop ? PSH_SEP_DROPPED : PSH_SEP_KEPT;
        pending &= ~(1u << e);
        return 1;
    };

    for (int round = 0; round <= n2; ++round) {               // (at most K rounds settle everything: the bound ends a loop
        int changed = 0;                                      //  that a wrong list could not)
        if (pending) {
            for (int e = 0; e < E; ++e)
                if (pending >> e & 1) changed |= settle(e);
            for (int e = E - 1; e >= 0; --e)
                if (pending >> e & 1) changed |= settle(e);
        }
        if (!__syncthreads_or(changed)) break;
    }

    // ---- 5. the first k kept entries, in list order
    int mine = 0;
    unsigned kept = 0;
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (p0 + e < K && state[p0 + e] == PSH_SEP_KEPT) {
            kept |= 1u << e;
            ++mine;
        }
    int slot = sep_scan<WAVES>(mine, wsum, tid, total);
    const uint32_t* d = reinterpret_cast<const uint32_t*>(a.d) + b * K;       // (bits, not numbers: a NaN keeps its payload)
    uint32_t* out_d = reinterpret_cast<uint32_t*>(a.out_d) + b * k;
    int32_t* out_idx = a.out_idx + b * k * 2;
    int32_t* out_pos = a.out_pos + b * k;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        if (!(kept >> e & 1)) continue;
        if (slot < k) {
            const int i = p0 + e;
            out_d[slot] = d[i];
            out_idx[2 * slot] = idx[2 * i];
            out_idx[2 * slot + 1] = idx[2 * i + 1];
            out_pos[slot] = i;
        }
        ++slot;
    }
    for (int j = total + tid; j < k; j += THREADS) {
        out_d[j] = 0x7f800000u;
        out_idx[2 * j] = out_idx[2 * j + 1] = -1;
        out_pos[j] = -1;
    }
    if (tid == 0) {
        a.out_count[b] = total;
        a.out_status[b] = total < k ? PSH_SEPARATE_STATUS_SHORT : PSH_SEPARATE_STATUS_OK;
    }
}

}  // namespace

hipError_t launch_separate(const SeparateArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)a.B);
    if (a.K <= 1024) hipLaunchKernelGGL((separate_kernel<1024, 256, 2>), grid, dim3(256), 0, s, a);
    else if (a.K <= 4096) hipLaunchKernelGGL((separate_kernel<4096, 512, 3>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((separate_kernel<16384, 1024, 4>), grid, dim3(1024), 0, s, a);
    return hipGetLastError();
}

}  // namespace psh
