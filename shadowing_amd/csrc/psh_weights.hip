// psh_weights.hip -- the averaging weights of the k shadowing paths of a query, formed where the distances lie, for a whole
// grid of (eta, k') weightings at once (psh_softmax_weights): what psh_weighted_moments, psh_weighted_quantiles,
// psh_score_ensemble and psh_hedged_mc take as given.  Host twin: shadowing_amd/weights.py.
//
// The definition (shared with the twin, include/psh.h and README "Forming the weights on the device"):
//   distances[B, k], float32.  A grid of n_etas widths and n_ks cut-offs 1 <= k' <= k; set e = a * n_ks + c is
//   (etas[a], ks[c]), at most PSH_SCORE_MAX_SETS = 64 sets.  For one query and one set:
//   1. Order the paths by (distance ascending as numbers, path index ascending): -0.0 and +0.0 are equal, a NaN of either
//      sign comes after +inf, NaNs among themselves go by index (numpy's stable argsort).
//   2. The first k' paths are kept; every other path gets weight exactly 0.0.
//   3. With d_j converted to double and s = 2.0 * (eta * eta), computed once on the host in double:
//        z_j = -(d_j * d_j) / s      zmax = max of z over the kept paths (NaN if any kept z is NaN)
//        a_j = z_j - zmax            e_j = exp(a_j)      Z = sum of e_j over the kept paths, in a fixed order
//        w_j = e_j / Z
//      d_j * d_j is exact (a float32 squared in double), so a_j is three IEEE operations -- a negation apart -- and comes out
//      bit-identical here and in the twin: the library is compiled with -ffp-contract=off and nothing here is written as a
//      fused multiply-add.  What differs between the two sides is exp (1 ulp each), the order of the sum and the division.
//   4. eta = +infinity (the twin's eta = None) is w_j = 1.0 / k' for the kept paths, whatever their distances.
//   5. A NaN among the kept distances makes every kept weight of that (e, b) NaN (zmax is NaN), and so do kept distances
//      that are all infinite (-inf - -inf); the paths past the cut-off keep their 0.0, and a NaN or inf there is harmless.
//      The consumers answer a NaN weight with their *_STATUS_WEIGHTS.
//   6. No floating-point atomics: two calls give identical bits, and a set's bits depend on its own (eta, k') alone.
//
// The method: one workgroup per query row, the sort of psh_sort_lds.h, then a loop over the sets of the row.
//   * Load: (key, path index) entries in LDS as the quantile and scoring kernels hold them, a NaN of either sign taking the
//     largest key first (qnt_key alone sends a NaN with the sign bit set to the front).  The padding entries share that key
//     and carry indices >= k, so they still sort behind every path.
//   * Every flow hands over the rows the scan returned ascending.  The load compares each key with its successor's; a row
//     that is already in order (ties included: the indices ascend) skips the network.  Measured on MI355X
//     (tools/bench_weights.py, ms, ascending against shuffled rows of 8192): 0.019 / 0.052 for one row and one set,
//     0.040 / 0.095 for 64 rows and 16 sets, 0.103 / 0.296 for 252 rows and 16 sets (a shuffled row also scatters its
//     writes); so the skip stays.  At 252 rows and 16 sets the (E, B, k) doubles leave at 2.6 TB/s.
//   * Per set, thread t owns the sorted positions t, t + THREADS, ...: a cut-off k' far below k still spreads its k'
//     exponentials over k' threads, and a row that came in ascending is written back in whole lines.  z_j of the thread's
//     kept positions stay in registers (CAP / THREADS of them) from the maximum to the division.
//       1. zmax: a butterfly of fmax over a wave's 64 lanes, the waves through LDS; a NaN is carried by a flag beside it
//          (fmax drops NaN), and the maximum is exact in any order.
//       2. e_j = exp(z_j - zmax) and the thread's sum, positions ascending.
//       3. Z: the same fixed tree with +: both lanes of a pair add the same two numbers, then the waves in order.  (The
//          sequential scan of psh_sort_lds.h gives prefixes, which nothing here needs; its five barriers a set would
//          stand against two.)
//       4. w_j = e_j / Z at the path's own index, 0.0 past k'.
//   * LDS: the entries and 2 doubles a wave; the 16384-entry instantiation holds 139776 bytes of the 163840 a workgroup may
//     hold.
//   * Small grids: with fewer rows than compute units, a second grid dimension splits the sets into groups, each group
//     sorting again, as psh_score_ensemble does.  Each set is computed by the same code from the same order, so the bits
//     do not depend on the split.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_sort_lds.h"
#include "psh_wave.h"

namespace psh {

namespace {

// qnt_key with every NaN behind +inf
__device__ __forceinline__ uint32_t wgt_key(float x) { return x != x ? 0xffffffffu : qnt_key(x); }

template <int CAP, int THREADS, int NB>
__global__ __launch_bounds__(THREADS) void weights_kernel(WeightsArgs a) {
    constexpr int ITEMS = 1 << NB, WAVES = THREADS / 64;
    static_assert(ITEMS * THREADS == CAP, "geometry");
    __shared__ uint64_t ent[CAP + CAP / 16];
    __shared__ double red[2][WAVES];                          // the maxima and the sums of the waves
    const int tid = (int)threadIdx.x, k = a.k;
    const int64_t b = (int64_t)blockIdx.x;
    const int e0 = (int)blockIdx.y * a.sets_per_group, n_sets = a.n_etas * a.n_ks;
    const int e1 = e0 + a.sets_per_group < n_sets ? e0 + a.sets_per_group : n_sets;
    const float* d = a.distances + b * k;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    int n2 = 1 << NB;
    while (n2 < k) n2 <<= 1;                                  // k <= CAP: the launcher chose the instantiation

    // ---- load; is the row in order already?
    int unsorted = 0;
    for (int j = tid; j < n2; j += THREADS) {
        uint64_t e = ((uint64_t)0xffffffffu << 32) | (uint32_t)j;
        if (j < k) {
            const uint32_t key = wgt_key(d[j]);
            e = ((uint64_t)key << 32) | (uint32_t)j;
            if (j + 1 < k && wgt_key(d[j + 1]) < key) unsorted = 1;
        }
        ent[qnt_phys(j)] = e;
    }
    unsorted = __syncthreads_or(unsorted);

    // ---- sort
    if (unsorted) qnt_sort<NB, THREADS>(ent, n2, tid);

    for (int e = e0; e < e1; ++e) {
        const double s = a.s[e / a.n_ks];
        const int kc = a.ks[e % a.n_ks];
        double* out = a.out + ((int64_t)e * a.B + b) * k;

        if (isinf(s)) {                                       // eta = +infinity: 1 / k' whatever the distances
            const double u = 1.0 / (double)kc;
            for (int p = tid; p < k; p += THREADS) out[(uint32_t)ent[qnt_phys(p)]] = p < kc ? u : 0.0;
            continue;
        }

        // ---- z of my kept positions; zmax.  The rounds of THREADS positions that hold kept ones are the same for every
        // thread (a scalar branch); inside a round a thread past the cut-off computes along and is not counted.
        const int rounds = (kc + THREADS - 1) / THREADS;
        double z[ITEMS], m = -INFINITY;
        int has_nan = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) z[i] = 0.0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            if (i >= rounds) break;
            const int p = tid + i * THREADS;
            const bool kept = p < kc;
            const double x = (double)qnt_value((uint32_t)(ent[qnt_phys(kept ? p : 0)] >> 32));
            const double zz = -(x * x) / s;
            z[i] = zz;
            has_nan |= (kept && zz != zz) ? 1 : 0;
            m = kept ? fmax(m, zz) : m;                   // (fmax drops a NaN: the flag carries it)
        }
        block_reduce_put(m, red[0], WaveMax{});
        has_nan = __syncthreads_or(has_nan);              // (the tree's barrier, carrying the flag)
        double zmax = block_reduce_fold<WAVES>(red[0], WaveMax{});
        if (has_nan) zmax = qnan;

        // ---- e = exp(z - zmax); Z
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            if (i >= rounds) break;
            const double arg = z[i] - zmax;
            const double ev = exp(arg);
            z[i] = ev;
            sum = tid + i * THREADS < kc ? sum + ev : sum;
        }
        const double Z = block_reduce<WAVES>(sum, red[1], WaveSum{});

        // ---- w at the path's own index
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int p = tid + i * THREADS;
            if (p < k) out[(uint32_t)ent[qnt_phys(p)]] = p < kc ? z[i] / Z : 0.0;
        }
    }
}

}  // namespace

hipError_t launch_softmax_weights(const WeightsArgs& args, hipStream_t s) {
    WeightsArgs a = args;
    const int n_sets = a.n_etas * a.n_ks;
    int groups = 1;                                           // groups of sets, each sorting again, while units stand idle
    if (a.B < PSH_SMALL_GRID_CUS) groups = PSH_SMALL_GRID_CUS / a.B < n_sets ? PSH_SMALL_GRID_CUS / a.B : n_sets;
    a.sets_per_group = (n_sets + groups - 1) / groups;
    const dim3 grid((unsigned)a.B, (unsigned)((n_sets + a.sets_per_group - 1) / a.sets_per_group));
    if (a.k <= 1024) hipLaunchKernelGGL((weights_kernel<1024, 256, 2>), grid, dim3(256), 0, s, a);
    else if (a.k <= 4096) hipLaunchKernelGGL((weights_kernel<4096, 512, 3>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((weights_kernel<16384, 1024, 4>), grid, dim3(1024), 0, s, a);
    return hipGetLastError();
}

}  // namespace psh
