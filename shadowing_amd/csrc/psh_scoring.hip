// psh_scoring.hip -- the CRPS, the PIT and the mean of weighted predictive ensembles against what happened, for a whole grid
// of weightings at once (psh_score_ensemble): how good the conditional distributions of the k shadowing paths are, and which
// eta and k make them best.  Host twin: shadowing_amd/scoring.py.
//
// The definition (shared with the twin, include/psh.h and README "Scoring the predictions"):
//   One column is one (b, i) of values[B, k, m], float32; y = obs[b, i], float32, is what was realised.  Weight set e of
//   query b is weights[e, b, 0 .. k-1], float64, used as given and never renormalised; weights = NULL means one set of unit
//   weights.  At most PSH_SCORE_MAX_SETS = 64 sets.  Keep the paths with w > 0, order them by (value ascending, path index
//   ascending) and write x_(0..n-1), w_(i) for the sorted values and weights.  All arithmetic is in double:
//     C_i = sum_{l<=i} w_(l)      S_i = sum_{l<=i} w_(l) x_(l)      W = C_{n-1} (as computed)
//     mean   = S_{n-1} / W
//     pit_lo = (sum of w_(i) with x_(i) <  y) / W          F(y-)
//     pit_hi = (sum of w_(i) with x_(i) <= y) / W          F(y)
//     c_i    = min(max(y, x_(i)), x_(i+1))
//     crps   = (x_(0) - y)_+ + (y - x_(n-1))_+
//              + (1 / W^2) sum_{i=0}^{n-2} [ C_i^2 (c_i - x_(i)) + (W - C_i)^2 (x_(i+1) - c_i) ]
//   crps is the integral of (F(z) - 1[z >= y])^2 written gap by gap: every term is non-negative and nothing cancels.  It
//   equals E|X - y| - 1/2 E|X - X'| under p = w / W.
//   A path of weight exactly 0 contributes nothing, whatever its value.  A non-finite value at a positive weight makes that
//   column's four results NaN for that set and sets PSH_SCORE_STATUS_NONFINITE in status[e, b].  A non-finite or negative
//   weight, or W not > 0, makes all of (e, b) NaN and sets PSH_SCORE_STATUS_WEIGHTS (the values are then not looked at).  A
//   non-finite obs[b, i] makes the column NaN for every set and sets PSH_SCORE_STATUS_OBS in every status[e, b] (the values
//   of that column are then not looked at; the weights still are).  -0.0 and +0.0 are one value.
//
// The method: one workgroup per column sorts once, then serves every weight set from the one sorted order.
//   * Load and sort are psh_quantiles.hip's (psh_sort_lds.h): (key, path index) entries in LDS, a bitonic network NB index
//     bits a pass, the same three capacities and thread counts.  The order does not depend on the weights, so a grid of
//     (eta, k') weightings costs one sort: "one sort serves every level", one step further.
//   * Per set, thread t owns the sorted positions [t c, (t + 1) c).  Walk 1 gathers w by path index (a set's k weights are
//     read by the m columns of the query and stay in L2), checks them, adds them and notes the chunk's last weighted position.
//     The fixed-order scan gives the chunk bases of C; the maximum of the chunk ends gives W (exact in any order, and
//     W >= every C_i as computed, so no (W - C_i) is negative and pit_hi = 1 exactly when no path lies above y).
//   * The zero weights: a k' cut-off zeroes most paths, scattered through the value order, so the predecessor of a chunk's
//     first weighted path may lie many chunks back.  A prefix maximum over "my last weighted position + 1" gives it; the
//     thread reads that entry's value from LDS and takes its own chunk base as the predecessor's C.  A gap belongs to the
//     thread that owns its upper path; (x_(0) - y)_+ to the thread whose first weighted path has no predecessor, and
//     (y - x_(n-1))_+ to the thread whose last weighted position is the largest.
//   * Walk 2 adds the gap terms and w x in order and notes C at the chunk's last path below y and at its last path not above
//     y.  The per-thread sums (gap terms, edge term, S) and maxima (the two C) are combined by a fixed tree: a butterfly over
//     the 64 lanes of a wave (both lanes of a pair add the same two numbers), then the waves in order.  No floating-point
//     atomics: two calls give identical bits.  A set's bits depend on nothing but its own weights: not on n_sets, not on the
//     grid.  Scaling a set's weights by a power of two scales C, W, S exactly and cancels, while W^2 stays in range.
//   * LDS: the scans' scratch is the quantiles' (9 KiB at 1024 threads); the tree adds 5 doubles a wave, 640 bytes.  The
//     16384-entry instantiation holds 148936 bytes of the 163840 a workgroup may hold.
//   * Small grids: with fewer columns than compute units, a second grid dimension splits the sets into groups, each group
//     sorting again, as many groups as fill PSH_SMALL_GRID_CUS = 256 units.  Each set is computed by the same code from the same
//     sorted order, so the bits do not depend on the split.
//
// Measured on MI355X (tools/bench_scoring.py: median ms of 20 calls, three alternating rounds, every case in one process,
// Softmax weights on a k' cut; B x k x m = 1 x 8192 x 3, 64 x 8192 x 3, 256 x 1024 x 8):
//                                                     E = 1    4       16   |  E = 1    4       16   |  E = 1    4       16
//   this kernel                                       0.064   0.065   0.066 |  0.071   0.116   0.277 |  0.070   0.111   0.268
//   psh_weighted_quantiles, seven levels (the sort)   0.064                 |  0.069                 |  0.067
//   torch sort once; gather, cumsum, ... per set      1.44    5.28    20.5  |  1.71    6.22    24.3  |  0.56    1.81    6.73
//   copy to the host + the numpy twin                 2.0     2.9     5.5   |  96      165     335   |  108     219     498
//   upload of the (E, B, k) weights                   0.023   0.038   0.10  |  0.090   0.39    1.48  |  0.059   0.20    0.77
// One set costs what the quantile kernel costs: the time is the sort.  Where the grid fills the chip a further set costs
// 0.014 ms: 16 sets take 0.24 of 16 calls with one set.  Two changes to the per-set loop were measured and dropped, each
// leaving 64 x 8192 x 3, E = 16 where it was (0.278 and 0.277 ms): both maxima from one pass of shuffles in place of two
// scans, and the weights gathered eight loads at a time.  So neither the scans' barriers nor the latency of a gather sets
// the 0.014 ms; what is left is the number of gathers, 2 k a column and set, 8 bytes from a line of their own each (the
// same per compute unit at 256 x 1024 x 8, which costs the same).  Holding the chunk's weights in registers for the second
// walk spills at 1024 threads (128 registers a thread) and was not timed.  The set split was measured at 1 x 8192 x 3
// (3 columns, one set a group): 16 sets cost what one costs, 0.066 ms, where the unsplit loop would add 15 x 0.014 ms as
// it does on the full grids; so the split stays.  Other group sizes were not measured.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_sort_lds.h"

namespace psh {

namespace {

// Sums of v[0..2] and maxima (of values >= 0) of v[3..4] over the workgroup, in a fixed tree: a butterfly over a wave's 64
// lanes, then the waves in order.  Every thread returns with the same five numbers.  (The tree of psh_wave.h's block_reduce,
// written out: the five butterflies go step by step here, their shuffles overlapping; as five wave_reduce in a row the
// 1024-thread kernel measured 0.7 % slower at 64 x 8192 x 3 with 16 sets.)
template <int WAVES>
__device__ __forceinline__ void score_reduce(double (*red)[WAVES], double* v, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q] += __shfl_xor(v[q], o);
#pragma unroll
        for (int q = 3; q < 5; ++q) v[q] = fmax(v[q], __shfl_xor(v[q], o));
    }
    if ((tid & 63) == 0)
#pragma unroll
        for (int q = 0; q < 5; ++q) red[q][tid >> 6] = v[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        double acc = red[q][0];
        for (int u = 1; u < WAVES; ++u) acc = q < 3 ? acc + red[q][u] : fmax(acc, red[q][u]);
        v[q] = acc;
    }
}

template <int CAP, int THREADS, int NB>
__global__ __launch_bounds__(THREADS) void score_kernel(ScoreArgs a) {
    constexpr int RUNS = THREADS / PSH_QNT_RUN, GROUPS = RUNS / PSH_QNT_GRP, WAVES = THREADS / 64;
    static_assert(GROUPS >= 1 && GROUPS <= 8 && (1 << NB) * THREADS == CAP, "geometry");
    __shared__ uint64_t ent[CAP + CAP / 16];
    __shared__ double sc[THREADS], rc[RUNS], gc[GROUPS + 1];  // the scans' scratch
    __shared__ double red[5][WAVES];                          // the tree's
    const int tid = (int)threadIdx.x, k = a.k, m = a.m, B = a.B;
    const int64_t col = (int64_t)blockIdx.x, b = col / m, i = col % m;
    const int e0 = (int)blockIdx.y * a.sets_per_group, e1 = e0 + a.sets_per_group < a.n_sets ? e0 + a.sets_per_group : a.n_sets;
    const float* v = a.values + b * k * m + i;
    const double y = (double)a.obs[b * m + i];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    if (!isfinite(y)) {                                       // the column is NaN for every set; the weights still speak
        for (int e = e0; e < e1; ++e) {
            const double* w = a.weights ? a.weights + ((int64_t)e * B + b) * k : nullptr;
            int badw = 0, some = w ? 0 : 1;                   // a bad weight; a positive one
            for (int j = tid; w && j < k; j += THREADS) {
                const double wj = w[j];
                if (!(wj >= 0.0) || isinf(wj)) badw = 1;
                else if (wj > 0.0) some = 1;
            }
            badw = __syncthreads_or(badw);
            some = __syncthreads_or(some);
            if (tid == 0) {
                const int64_t o = ((int64_t)e * B + b) * m + i;
                a.crps[o] = a.pit_lo[o] = a.pit_hi[o] = a.mean[o] = qnan;
                if (a.status) atomicOr(a.status + (int64_t)e * B + b, PSH_SCORE_STATUS_OBS | (badw || !some ? PSH_SCORE_STATUS_WEIGHTS : 0));
            }
        }
        return;
    }

    int n2 = 1 << NB;
    while (n2 < k) n2 <<= 1;                                  // k <= CAP: the launcher chose the instantiation

    // ---- load
    for (int j = tid; j < n2; j += THREADS) {
        uint64_t e = ((uint64_t)0xffffffffu << 32) | (uint32_t)j;
        if (j < k) e = ((uint64_t)qnt_key(v[(int64_t)j * m]) << 32) | (uint32_t)j;
        ent[qnt_phys(j)] = e;
    }
    __syncthreads();

    // ---- sort
    qnt_sort<NB, THREADS>(ent, n2, tid);

    const int chunk = (k + THREADS - 1) / THREADS;
    const int i0 = tid * chunk < k ? tid * chunk : k, i1 = i0 + chunk < k ? i0 + chunk : k;

    for (int e = e0; e < e1; ++e) {
        const double* w = a.weights ? a.weights + ((int64_t)e * B + b) * k : nullptr;
        const int64_t o = ((int64_t)e * B + b) * m + i;

        // ---- walk 1: the chunk's weight, its last weighted position (+ 1; 0: none), and the checks
        double c = 0.0;
        int last = 0, badw = 0, badx = 0;                     // a bad weight; a non-finite value that weighs
        for (int p = i0; p < i1; ++p) {
            const uint64_t en = ent[qnt_phys(p)];
            const double wj = w ? w[(uint32_t)en] : 1.0;
            if (!(wj >= 0.0) || isinf(wj)) badw = 1;
            else if (wj > 0.0) {
                if (!isfinite(qnt_value((uint32_t)(en >> 32)))) badx = 1;
                c += wj;
                last = p + 1;
            }
        }
        badw = __syncthreads_or(badw);
        badx = __syncthreads_or(badx);
        if (badw || badx) {
            if (tid == 0) {
                a.crps[o] = a.pit_lo[o] = a.pit_hi[o] = a.mean[o] = qnan;
                if (a.status) atomicOr(a.status + (int64_t)e * B + b, badw ? PSH_SCORE_STATUS_WEIGHTS : PSH_SCORE_STATUS_NONFINITE);
            }
            continue;
        }

        // ---- the chunk bases of C, W, and the last weighted position before the chunk
        const double bc = qnt_scan<THREADS, false>(sc, rc, gc, c, tid);
        qnt_scan<THREADS, true>(sc, rc, gc, c > 0.0 ? bc + c : 0.0, tid);      // a chunk without weight claims nothing
        const double W = gc[GROUPS];
        const int prev = (int)qnt_scan<THREADS, true>(sc, rc, gc, (double)last, tid);
        const int last_all = (int)gc[GROUPS];
        if (!(W > 0.0)) {
            if (tid == 0) {
                a.crps[o] = a.pit_lo[o] = a.pit_hi[o] = a.mean[o] = qnan;
                if (a.status) atomicOr(a.status + (int64_t)e * B + b, PSH_SCORE_STATUS_WEIGHTS);
            }
            continue;
        }

        // ---- walk 2: the gaps whose upper path is mine, w x, and C at my last path below y / not above y
        bool have = prev > 0;
        double xa = have ? (double)qnt_value((uint32_t)(ent[qnt_phys(prev - 1)] >> 32)) : 0.0, Ca = bc, lc = 0.0;
        double r[5] = {0.0, 0.0, 0.0, 0.0, 0.0};              // gap terms, the edge term, S; C below y, C not above y
        for (int p = i0; p < i1; ++p) {
            const uint64_t en = ent[qnt_phys(p)];
            const double wj = w ? w[(uint32_t)en] : 1.0;
            if (!(wj > 0.0)) continue;
            const double xb = (double)qnt_value((uint32_t)(en >> 32));
            if (have) {
                const double cc = fmin(fmax(y, xa), xb), rest = W - Ca;
                r[0] += Ca * Ca * (cc - xa) + rest * rest * (xb - cc);
            } else {
                r[1] = fmax(xb - y, 0.0);                     // the first weighted path of the column
            }
            lc += wj;
            Ca = bc + lc;
            r[2] += wj * xb;
            if (xb < y) r[3] = Ca;
            if (xb <= y) r[4] = Ca;
            xa = xb;
            have = true;
        }
        if (last > 0 && last == last_all) r[1] += fmax(y - xa, 0.0);   // the last one
        score_reduce<WAVES>(red, r, tid);
        if (tid == 0) {
            a.crps[o] = r[1] + r[0] / (W * W);
            a.pit_lo[o] = r[3] / W;
            a.pit_hi[o] = r[4] / W;
            a.mean[o] = r[2] / W;
        }
    }
}

}  // namespace

hipError_t launch_score(const ScoreArgs& args, hipStream_t s) {
    ScoreArgs a = args;
    const int64_t cols = (int64_t)a.B * a.m;
    int groups = 1;                                           // groups of sets, each sorting again, while units stand idle
    if (cols < PSH_SMALL_GRID_CUS) groups = (int)(PSH_SMALL_GRID_CUS / cols) < a.n_sets ? (int)(PSH_SMALL_GRID_CUS / cols) : a.n_sets;
    a.sets_per_group = (a.n_sets + groups - 1) / groups;
    const dim3 grid((unsigned)cols, (unsigned)((a.n_sets + a.sets_per_group - 1) / a.sets_per_group));
    if (a.k <= 1024) hipLaunchKernelGGL((score_kernel<1024, 256, 2>), grid, dim3(256), 0, s, a);
    else if (a.k <= 4096) hipLaunchKernelGGL((score_kernel<4096, 512, 3>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((score_kernel<16384, 1024, 4>), grid, dim3(1024), 0, s, a);
    return hipGetLastError();
}

}  // namespace psh
