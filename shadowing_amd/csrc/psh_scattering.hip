// psh_scattering.hip -- the wavelet scattering spectra of an ensemble where it lies (psh_scattering_spectra; Morel et al.,
// arXiv 2204.10177, stated in our own terms: parity with scatspectra is not pinned): for R rows of n float32 returns, n a
// power of two, J scales and G groups of rows, the sums over each group's finite rows of
//   S1[j] = mean_t U_j,  S2[j] = mean_t U_j^2,  C3[j1,j2] = mean_t W_j2 conj(V_{j1,j2}),  C4[j1,j1',j2] = mean_t V_{j1,j2}
//   conj(V_{j1',j2}),   W_j = IDFT(F[x] psi_hat[j]),  U_j = |W_j|,  V_{j1,j2} = IDFT(F[U_j1] psi_hat[j2]),
// F the DFT of size n (convolutions are circular over the row), every sample converted to double first, all arithmetic
// in double.  Host twin: shadowing_amd/scattering.py (np.fft on the time-domain sums above).
//
// The method:
//   * One workgroup per row, every n-point transform in LDS; a row's spectra never go to HBM.  A row costs 2 J + 1
//     transforms: F[x], J inverses (W_j) and J forward transforms (F[U_j]).
//   * C3 and C4 need no further inverse.  By Parseval, psi_hat real:
//       C3[j1,j2]     = (1/n^2) sum_k F[x][k]    conj(F[U_j1][k])  psi_hat[j2][k]^2
//       C4[j1,j1',j2] = (1/n^2) sum_k F[U_j1][k] conj(F[U_j1'][k]) psi_hat[j2][k]^2
//     and psi_hat[j2][k] is zero outside n / 2^(j2+2) < k < n / 2^j2 (the table is never read outside that band), so
//     F[U_j1] is needed on the bins k < n / 2^j1 alone.
//   * The forward transform is psh_mrw_lds.h's (radix-2 decimation in frequency, three stages at a time in registers,
//     X[k] left at slot bitrev(k)).  The inverse is its counterpart, built here: decimation in time FROM bit-reversed
//     input to time order (psh_scat_lds.h), the stages of half-length h, 2h, 4h of one pass taken together on the 8 elements base + q h
//     (log2 n mod 3 stages first, at h = 1, where every twiddle is 1).  The twiddle of the pass's last stage is one
//     sincospi, exp(+2 pi i j / 8h); the earlier stages take its square and fourth power, the eighth roots are
//     constants.  n = 4096 crosses LDS four times (8 8 8 8) in either direction.
//   * Order of operations per row (fixed; so are all the sums below: two calls give identical bits):
//       1. x -> buf as (x, 0); a row that holds a NaN or an inf is left here: it adds nothing and is not counted.
//       2. forward; fx[k] = F[x][k] for k < n / 2.
//       3. for j = J down to 1:
//            buf[bitrev(k)] = fx[k] psi_hat[j][k] inside the band, 0 elsewhere; inverse; u = |buf[t]| / n (the 1 / n of
//            the IDFT; exact), S1 += u, S2 += u u, buf[t] = (u, 0); forward: buf holds F[U_j];
//            for j >= 2, keep[n / 2^j + k] = F[U_j][k], k < n / 2^j (F[U_1] is only ever read from buf);
//            the sums over k of C3[j, j2] and C4[j, j', j2], j <= j' <= j2 <= J: F[U_j] from buf, F[U_j'] (j' > j) from
//            keep, F[x] from fx.  Output o of this list belongs to wave o mod 8, whose lane l adds k = lo + l, lo + l
//            + 64, .. in that order; the lanes are added by a butterfly of __shfl_xor (32, 16, .. 1).
//       S1 and S2: thread i adds t = i, i + 512, ..; the lanes by the same butterfly, the 8 waves left to right.
//     Each of a row's NOUT numbers is added once to the workgroup's accumulator in LDS, rows in row order.
//   * Work is cut into units that depend on (R, G) alone, psh_moments.hip's scheme: group g (rows [floor(g R / G),
//     floor((g+1) R / G)), c of them) is cut into ceil(c / RU) runs of RU = ceil(c / 16) rows, one workgroup per unit, on
//     a grid of G * min(16, ceil(R / G)) units (the units a smaller group does not need are empty).  A unit's sums go to
//     the workspace; the second launch adds a group's partials in unit order.  No floating-point atomics, nothing depends
//     on how many workgroups ran, and a group's sums depend on its own rows alone.
//
// LDS layout (NMAX = 1024 or 4096 by n): buf, NMAX complex doubles at psh_mrw_lds.h's XOR-swizzled slots (64 KiB);
// fx, NMAX / 2 (32 KiB); keep, NMAX / 2: F[U_j] of j = 2 .. J at [n / 2^j, 2 n / 2^j), fewer than n / 2 bins together
// (32 KiB); the accumulator (570 doubles at J = 10) and 16 doubles for the wave totals: 132.6 KiB of the 160 KiB a
// workgroup may hold, one workgroup of 512 threads per CU.
//
// Measured on MI355X (tools/bench_scattering.py: median ms of 20 calls, three alternating rounds, every case in one process,
// J = 9, G = 64, a skewed-MRW ensemble made on the device; R x n = 2048 x 4096 and 32768 x 4096):
//   this kernel (19 R transforms of 4096 points)                       1.50     22.5
//   one read of the ensemble (psh_realized_variance, full length)      0.027    0.179
//   psh_mrw_generate, same R, n = 2048 (R / 2 transforms + the draws)  0.091    1.19
//   per transform, this kernel / psh_mrw_generate                      0.44     0.50
// 36 ns per transform chip-wide, the band products and the envelope included; the generator's 72 ns are mostly draws.  The
// numpy twin takes 7.9 and 127 s (one run on 64 rows, scaled): 5300 and 5600 times longer.  Device and twin agree within
// 5e-15 of the largest value of each family (tests/test_gpu_scattering.py asks for 1e-9).
// Forms not built: subsampled inverses for the coarse bands (|W_j| is not band-limited: subsampling it aliases, which
// would change the definition); two rows per workgroup with paired real transforms (two working buffers and two sets of
// kept spectra need 256 KiB of LDS at n = 4096).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_mrw_lds.h"    // mrw_slot, cmul, mrw_butterfly (through mrw_passes): the forward transform
#include "psh_scat_lds.h"   // scat_inverse: its counterpart
#include "psh_wave.h"

namespace psh {

namespace {

// the rows per unit of a group of c rows
__device__ __forceinline__ int64_t scat_rows_per_unit(int64_t c) { return (c + 15) / 16; }

template <int NMAX>
__global__ __launch_bounds__(PSH_SCAT_THREADS) void scat_kernel(ScatArgs a) {
    __shared__ double2 buf[NMAX];
    __shared__ double2 fx[NMAX / 2];
    __shared__ double2 keep[NMAX / 2];
    __shared__ double acc[PSH_SCAT_MAX_NOUT];
    __shared__ double red[2 * PSH_SCAT_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = a.n, logn = a.logn, J = a.J, half = n >> 1;
    const int P3 = J * (J + 1) / 2, P4 = J * (J + 1) * (J + 2) / 6;
    double* const c3re = acc + 2 * J;
    double* const c3im = c3re + P3;
    double* const c4re = c3im + P3;
    double* const c4im = c4re + P4;
    const double inv_n = 1.0 / (double)n, inv_n2 = inv_n * inv_n;

    const int64_t unit = (int64_t)blockIdx.x, g = unit / a.upg, p = unit % a.upg;
    const int64_t g0 = g * a.R / a.G, g1 = (g + 1) * a.R / a.G, ru = scat_rows_per_unit(g1 - g0);
    const int64_t r0 = g0 + p * ru < g1 ? g0 + p * ru : g1, r1 = r0 + ru < g1 ? r0 + ru : g1;

    for (int i = tid; i < a.nout; i += PSH_SCAT_THREADS) acc[i] = 0.0;
    int64_t used = 0;

    for (int64_t r = r0; r < r1; ++r) {
        const float* row = a.x + r * a.stride;
        int bad = 0;
        for (int t = tid; t < n; t += PSH_SCAT_THREADS) {
            const float v = row[t];
            bad |= !isfinite(v);
            buf[mrw_slot(t)] = make_double2((double)v, 0.0);
        }
        if (__syncthreads_or(bad)) continue;                 // (the products of the row before ended on a barrier)
        ++used;
        mrw_passes(buf, logn, 0);
        for (int k = tid; k < half; k += PSH_SCAT_THREADS) fx[k] = buf[mrw_slot((int)(__brev((unsigned)k) >> (32 - logn)))];
        __syncthreads();

        for (int j = J; j >= 1; --j) {
            // ---- W_j: the band of F[x] psi_hat[j], bit-reversed, then the inverse
            {
                const int lo = n >> (j + 2), hi = n >> j;
                const double* ps = a.psi + (int64_t)(j - 1) * half;
                for (int k = tid; k < n; k += PSH_SCAT_THREADS) {
                    double2 v = make_double2(0.0, 0.0);
                    if (k > lo && k < hi) {
                        const double w = ps[k];
                        const double2 f = fx[k];
                        v = make_double2(f.x * w, f.y * w);
                    }
                    buf[mrw_slot((int)(__brev((unsigned)k) >> (32 - logn)))] = v;
                }
            }
            __syncthreads();
            scat_inverse(buf, logn);

            // ---- U_j = |W_j|, its first two moments
            double s1 = 0.0, s2 = 0.0;
            for (int t = tid; t < n; t += PSH_SCAT_THREADS) {
                const double2 w = buf[mrw_slot(t)];
                const double u = sqrt(w.x * w.x + w.y * w.y) * inv_n;
                s1 = s1 + u;
                s2 = s2 + u * u;
                buf[mrw_slot(t)] = make_double2(u, 0.0);
            }
            block_reduce_put(s1, red, WaveSum{});
            block_reduce_put(s2, red + PSH_SCAT_WAVES, WaveSum{});
            __syncthreads();
            if (tid == 0) {
                const double t1 = block_reduce_fold<PSH_SCAT_WAVES>(red, WaveSum{});
                const double t2 = block_reduce_fold<PSH_SCAT_WAVES>(red + PSH_SCAT_WAVES, WaveSum{});
                acc[j - 1] = acc[j - 1] + t1 * inv_n;             // the means over t (1 / n: exact)
                acc[J + j - 1] = acc[J + j - 1] + t2 * inv_n;
            }
            mrw_passes(buf, logn, 0);                        // buf: F[U_j][k] at slot bitrev(k)

            // ---- keep F[U_j] for the coarser j1 to come; C3[j, .] and C4[j, ., .]
            if (j >= 2) {
                const int m = n >> j;
                for (int k = tid; k < m; k += PSH_SCAT_THREADS)
                    keep[m + k] = buf[mrw_slot((int)(__brev((unsigned)k) >> (32 - logn)))];
            }
            int o = 0;
            for (int j2 = j; j2 <= J; ++j2) {
                const int lo = (n >> (j2 + 2)) + 1, hi = n >> j2;
                const double* ps = a.psi + (int64_t)(j2 - 1) * half;
                for (int jp = j - 1; jp <= j2; ++jp, ++o) {   // jp = j - 1: C3[j, j2]; jp >= j: C4[j, jp, j2]
                    if ((o & (PSH_SCAT_WAVES - 1)) != wave) continue;
                    const double2* other = jp > j ? keep + (n >> jp) : nullptr;
                    double re = 0.0, im = 0.0;
                    for (int k = lo + lane; k < hi; k += 64) {
                        const double w = ps[k], w2 = w * w;
                        const double2 cur = buf[mrw_slot((int)(__brev((unsigned)k) >> (32 - logn)))];
                        const double2 u = jp < j ? fx[k] : cur;
                        const double2 v = jp > j ? other[k] : cur;
                        re = re + w2 * (u.x * v.x + u.y * v.y);           // u conj(v)
                        im = im + w2 * (u.y * v.x - u.x * v.y);
                    }
                    re = wave_sum(re);
                    im = wave_sum(im);
                    if (lane == 0) {
                        if (jp < j) {
                            const int p3 = j2 * (j2 - 1) / 2 + (j - 1);
                            c3re[p3] = c3re[p3] + re * inv_n2;
                            c3im[p3] = c3im[p3] + im * inv_n2;
                        } else {
                            const int p4 = (j2 - 1) * j2 * (j2 + 1) / 6 + jp * (jp - 1) / 2 + (j - 1);
                            c4re[p4] = c4re[p4] + re * inv_n2;
                            if (jp > j) c4im[p4] = c4im[p4] + im * inv_n2;     // (j1 = j1': real)
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    double* part = a.partial + unit * (int64_t)a.nout;
    for (int i = tid; i < a.nout; i += PSH_SCAT_THREADS) part[i] = acc[i];
    if (tid == 0) a.unit_rows[unit] = used;
}

// out[g][e] = the partials of group g's units in unit order; rows_used[g]; the status bit
__global__ __launch_bounds__(256) void scat_reduce_kernel(ScatArgs a) {
    const int64_t per = (int64_t)a.nout, total = a.G * per;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        const int64_t g = i / per, e = i % per;
        const int64_t c = (g + 1) * a.R / a.G - g * a.R / a.G, ru = scat_rows_per_unit(c), units = (c + ru - 1) / ru;
        const double* part = a.partial + g * a.upg * per + e;
        double s = 0.0;
        for (int64_t p = 0; p < units; ++p) s = s + part[p * per];
        a.out[i] = s;
    }
    if (i < a.G) {
        int64_t rows = 0;
        for (int64_t p = 0; p < a.upg; ++p) rows += a.unit_rows[i * a.upg + p];
        a.rows_used[i] = rows;
    }
    if (i == 0 && a.status) {
        int64_t rows = 0;
        for (int64_t u = 0; u < a.G * a.upg; ++u) rows += a.unit_rows[u];
        *a.status = rows < a.R ? PSH_SCATTERING_STATUS_ROWS_EXCLUDED : PSH_SCATTERING_STATUS_OK;
    }
}

}  // namespace

void scattering_plan(int64_t R, int64_t G, int J, ScatArgs* a) {
    const int64_t per_group = (R + G - 1) / G;
    a->upg = per_group < 16 ? per_group : 16;
    a->nout = 2 * J + J * (J + 1) + J * (J + 1) * (J + 2) / 3;
}

hipError_t launch_scattering(const ScatArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)(a.G * a.upg)), block(PSH_SCAT_THREADS);
    if (a.n <= 1024) hipLaunchKernelGGL((scat_kernel<1024>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((scat_kernel<4096>), grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t total = a.G * (int64_t)a.nout;
    hipLaunchKernelGGL(scat_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace psh
