// psh_quantiles.hip -- weighted quantiles and tail means over the k shadowing paths (psh_weighted_quantiles): the risk
// questions of the conditional ensemble that psh_weighted_moments (psh_predict.hip) cannot answer.  Host twin:
// shadowing_amd/quantiles.py.
//
// The definition (shared with the twin and README "Predictive quantiles"):
//   One column is one (b, i) of values[B, k, m], float32.  Its weights are w[b, 0 .. k-1], float64, used as given and never
//   renormalised; weights = NULL means w_j = 1.  The levels are 0 < p_a < 1, at most PSH_QUANTILE_MAX_LEVELS = 32 of them,
//   in any order.  Order the k paths by (value ascending, path index ascending) and write x_(i), w_(i) for the sorted
//   values and weights.  All arithmetic is in double, float32 values converted exactly:
//     C_i = sum_{l<=i} w_(l)      S_i = sum_{l<=i} w_(l) x_(l)      W = C_{k-1} (as computed)      t = p * W
//     i*  = the first i with C_i >= t
//     q(p)     = x_(i*)                                                   the lower weighted quantile (inverted CDF)
//     lower(p) = ( S_{i*-1} + (t - C_{i*-1}) x_(i*) ) / t                 mean of the lowest p of the mass
//     upper(p) = ( (C_{i*} - t) x_(i*) + (S_{k-1} - S_{i*}) ) / (W - t)   mean of the highest 1 - p of the mass
//   A path whose weight is exactly 0 contributes nothing, even if its value is NaN or inf.  A non-finite value at a
//   positive weight makes that column's three results NaN and sets PSH_QUANTILE_STATUS_NONFINITE for query b.  A
//   non-finite or negative weight, or W not > 0, makes all of query b's results NaN and sets PSH_QUANTILE_STATUS_WEIGHTS
//   (and then the values are not looked at).  -0.0 and +0.0 are equal values; which zero a quantile returns is unspecified.
//
// The method: one workgroup per column, one sort for every level and all three outputs.
//   * Load: path j becomes the 64-bit entry (order-preserving 32-bit key of the value) << 32 | j; -0.0 takes +0.0's key.
//     Entries are unique, so ties break by index for free.  The list is padded to n2, a power of two, with sentinels
//     0xffffffff << 32 | j, j >= k, which sort behind every path and weigh nothing.  Bad weights and non-finite values are
//     found here and the workgroup leaves with NaN and the status bit.
//   * Sort: a bitonic network on the entries in LDS, NB index bits a pass: a thread takes the 2^NB entries that differ in
//     the bits [lo, lo + NB) into registers, runs the NB sub-stages of the phase on them and writes them back, so a phase
//     of s sub-stages costs ceil(s / NB) trips through LDS and barriers instead of s; the first NB phases are one pass.
//     At n2 = 16384, NB = 4 that is 29 passes where the plain network has 105.  Entry i lies at i + i / 16 (one pad entry
//     after every 16): in the pass with lo = 0 a lane's 16 entries are contiguous and the lanes 17 entries apart, and with
//     8-byte entries a stride of 34 dwords puts the 32 lanes of a ds_read_b64 group on 32 different bank pairs; for every
//     other lo the lanes of a group fall on different pairs as well.
//   * Sums: thread t owns the sorted positions [t c, (t + 1) c), c = ceil(k / threads), and adds w and w x over them in
//     order, gathering w by path index (the k weights of a query are read by its m columns and stay in L2).  Unit weights
//     read nothing.  The chunk bases come from a three-level scan in a fixed order (16 threads, 8 runs, the groups), each
//     level a sequential exclusive prefix; inside a chunk C_i = fl(base + the chunk's running sum).  A parallel scan adds
//     the same prefix in two associations, so the chunk ends C_e(t) = fl(base_t + c_t) need not increase with t to the
//     last bit.  The level's owner is therefore found with a prefix MAXIMUM of the chunk ends (exact in any order; a chunk
//     without weight enters as 0): W is the largest chunk end, and the one thread with max_{u<t} C_e(u) < t_a <= C_e(t)
//     walks its chunk again to the first position whose C reaches t_a and writes the three results.
//   * No floating-point atomics: two calls give identical bits.  Scaling every weight by a power of two scales every C, S
//     and t by it exactly and cancels in the three results.
//   * A column is read with stride m.  For the m of real calls (3 to 10 maturities) a 128-byte line holds 32 / m paths of
//     the column and the m workgroups of a query share the lines through L2: HBM sees the statistic once, and the load is
//     a small part of the sort's time (tools/bench_quantiles.py sets the kernel against psh_weighted_moments, one read).
//     So the column is read where it lies and nothing is transposed.
//   * Three instantiations by capacity, so that small k does not pay for PSH_MAX_K = 16384 entries of LDS:
//     k <= 1024 (256 threads, NB = 2), k <= 4096 (512 threads, NB = 3), k <= 16384 (1024 threads, NB = 4).
//
// Measured on MI355X (tools/bench_quantiles.py: median ms of 20 calls, three alternating rounds, every case in one process,
// seven levels, Softmax weights; B x k x m = 1 x 8192 x 3, 64 x 8192 x 3, 256 x 1024 x 8):
//   this kernel                                      0.063   0.074   0.067
//   psh_weighted_moments on the same input (a read)  0.025   0.029   0.017
//   torch.sort + cumsum + searchsorted + gather      2.57    2.67    0.62
//   copy to the host + the numpy twin                2.4     125     137
// The three shapes cost the same: each fills at most one wave of workgroups per compute unit, so the time is one column's
// chain of LDS passes and barriers.  Other thread counts and NB per capacity were not measured.
// The entry, the network and the scan live in psh_sort_lds.h, which psh_scoring.hip shares.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_sort_lds.h"

namespace psh {

namespace {

template <int CAP, int THREADS, int NB>
__global__ __launch_bounds__(THREADS) void quantiles_kernel(QuantileArgs a) {
    constexpr int RUNS = THREADS / PSH_QNT_RUN, GROUPS = RUNS / PSH_QNT_GRP;
    static_assert(GROUPS >= 1 && GROUPS <= 8 && (1 << NB) * THREADS == CAP, "geometry");
    __shared__ uint64_t ent[CAP + CAP / 16];
    __shared__ double sc[THREADS], rc[RUNS], gc[GROUPS + 1];  // the scans' scratch
    const int tid = (int)threadIdx.x, k = a.k, m = a.m, nl = a.n_levels;
    const int64_t col = (int64_t)blockIdx.x, b = col / m, i = col % m;
    const float* v = a.values + b * k * m + i;
    const double* w = a.weights ? a.weights + b * k : nullptr;
    const int64_t out0 = b * nl * m + i;                      // level l goes to out0 + l * m
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    int n2 = 1 << NB;
    while (n2 < k) n2 <<= 1;                                  // k <= CAP: the launcher chose the instantiation

    // ---- load
    int badw = 0, badx = 0;
    for (int j = tid; j < n2; j += THREADS) {
        uint64_t e = ((uint64_t)0xffffffffu << 32) | (uint32_t)j;
        if (j < k) {
            const float x = v[(int64_t)j * m];
            const double wj = w ? w[j] : 1.0;
            if (!(wj >= 0.0) || isinf(wj)) badw = 1;
            else if (wj > 0.0 && !isfinite(x)) badx = 1;
            e = ((uint64_t)qnt_key(x) << 32) | (uint32_t)j;
        }
        ent[qnt_phys(j)] = e;
    }
    badw = __syncthreads_or(badw);
    badx = __syncthreads_or(badx);
    if (badw || badx) {
        for (int l = tid; l < nl; l += THREADS) {
            a.q[out0 + (int64_t)l * m] = qnan;
            a.lower[out0 + (int64_t)l * m] = qnan;
            a.upper[out0 + (int64_t)l * m] = qnan;
        }
        if (tid == 0 && a.status) atomicOr(a.status + b, badw ? PSH_QUANTILE_STATUS_WEIGHTS : PSH_QUANTILE_STATUS_NONFINITE);
        return;
    }

    // ---- sort
    qnt_sort<NB, THREADS>(ent, n2, tid);

    // ---- the chunk's sums
    const int chunk = (k + THREADS - 1) / THREADS;
    const int i0 = tid * chunk < k ? tid * chunk : k, i1 = i0 + chunk < k ? i0 + chunk : k;
    double c = 0.0, s = 0.0;
    for (int p = i0; p < i1; ++p) {
        const uint64_t e = ent[qnt_phys(p)];
        const double wj = w ? w[(uint32_t)e] : 1.0;
        if (wj > 0.0) {
            c += wj;
            s += wj * (double)qnt_value((uint32_t)(e >> 32));
        }
    }

    // ---- the chunk bases, then the first chunk whose end reaches each level
    const double bc = qnt_scan<THREADS, false>(sc, rc, gc, c, tid), bs = qnt_scan<THREADS, false>(sc, rc, gc, s, tid);
    const double S = gc[GROUPS];
    const double ce = c > 0.0 ? bc + c : 0.0;                 // C at the chunk's last path; a chunk without weight claims nothing
    const double before = qnt_scan<THREADS, true>(sc, rc, gc, ce, tid);
    const double W = gc[GROUPS];

    if (!(W > 0.0)) {
        for (int l = tid; l < nl; l += THREADS) {
            a.q[out0 + (int64_t)l * m] = qnan;
            a.lower[out0 + (int64_t)l * m] = qnan;
            a.upper[out0 + (int64_t)l * m] = qnan;
        }
        if (tid == 0 && a.status) atomicOr(a.status + b, PSH_QUANTILE_STATUS_WEIGHTS);
        return;
    }

    for (int l = 0; l < nl; ++l) {
        const double t = a.levels[l] * W;
        if (!(t > 0.0)) {                                     // p W underflowed: no path lies below the level
            if (tid == 0) a.q[out0 + (int64_t)l * m] = a.lower[out0 + (int64_t)l * m] = a.upper[out0 + (int64_t)l * m] = qnan;
            continue;
        }
        if (!(before < t && t <= ce)) continue;
        double lc = 0.0, ls = 0.0, Cp = bc, Sp = bs, Ci = bc, Si = bs, xq = qnan;
        for (int p = i0; p < i1; ++p) {
            const uint64_t e = ent[qnt_phys(p)];
            const double wj = w ? w[(uint32_t)e] : 1.0;
            if (!(wj > 0.0)) continue;
            xq = (double)qnt_value((uint32_t)(e >> 32));
            Cp = bc + lc;
            Sp = bs + ls;
            lc += wj;
            ls += wj * xq;
            Ci = bc + lc;
            Si = bs + ls;
            if (Ci >= t) break;                               // at the chunk's last path at the latest: Ci = ce there
        }
        a.q[out0 + (int64_t)l * m] = xq;
        a.lower[out0 + (int64_t)l * m] = (Sp + (t - Cp) * xq) / t;
        a.upper[out0 + (int64_t)l * m] = ((Ci - t) * xq + (S - Si)) / (W - t);
    }
}

}  // namespace

hipError_t launch_quantiles(const QuantileArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((int64_t)a.B * a.m));
    if (a.k <= 1024) hipLaunchKernelGGL((quantiles_kernel<1024, 256, 2>), grid, dim3(256), 0, s, a);
    else if (a.k <= 4096) hipLaunchKernelGGL((quantiles_kernel<4096, 512, 3>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((quantiles_kernel<16384, 1024, 4>), grid, dim3(1024), 0, s, a);
    return hipGetLastError();
}

}  // namespace psh
