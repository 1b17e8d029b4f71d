// psh_moments.hip -- the stylised facts of an ensemble where it lies (psh_lagged_moments): for R rows of n float32 returns,
// G groups of rows and lags tau = 0 .. m, the four sums over the group's rows and t = 0 .. n - 1 - tau of
//   xx = x[t] x[t+tau],  xx2 = x[t] x[t+tau]^2 (leverage),  x2x = x[t]^2 x[t+tau],  x2x2 = x[t]^2 x[t+tau]^2,
// every sample converted to double first, and the rows each group used.  Host twin: shadowing_amd/stylized.py.
//
// The method:
//   * Work is cut into units that depend on (R, G) alone: group g (rows [floor(g R / G), floor((g+1) R / G))) is cut into
//     UPG = ceil(ceil(R / G) / RU) runs of RU = ceil(ceil(R / G) / 16) rows, one workgroup per unit.  A unit's sums stay in
//     registers across its rows and go to the workspace; the second launch adds the UPG partials of a group in unit
//     order.  No floating-point atomics, and nothing depends on how many workgroups ran or in which order.
//   * A row is scanned for NaN / inf before any of it is added: such a row contributes nothing and is not counted.
//   * A row is walked in tiles of PSH_MOM_TILE = 2048 samples.  A tile is staged in LDS as doubles with a halo of the lags
//     that follow it (zeros past the row's end, so the hot loop tests no bound): a pair belongs to the tile of its first
//     end, and its second end lies in that tile or in the halo.
//   * Lags 1 .. m: a lane owns U consecutive lags (U = 1, 2, 4 for m <= 64, <= 128, above), a wave 64 U of them, and the 8
//     waves are C = ceil(m / 64 U) lag chunks times S = floor(8 / C) slices of the tile's t range.  The lane keeps
//     x[t + tau] and its square for its U lags in a register window that slides with t: a step of t costs one broadcast
//     read of x[t], one read of the sample that enters the window, two squares (exact: 24-bit inputs) and 4 U FMAs.
//     Lanes U doubles apart would meet on the LDS banks, so the tile is stored with one pad double after every U (the
//     lane stride becomes U + 1 doubles: odd, no conflict among the 32 lanes of a ds_read_b64 group).
//   * Lag 0 (the second, third and fourth moments) is summed by the thread that stages a sample.
//   * At the end of a unit the slices are added in slice order through LDS, then the lag-0 sums by a fixed tree.
//
// Measured on MI355X (tools/bench_stylized.py: median ms of 20 calls, three alternating rounds, every case in one process,
// G = 64, a skewed-MRW ensemble made on the device; R x n = 2048 x 4096 and 32768 x 4096):
//   m       this kernel        4 R n (m + 1) FMAs at the measured rate     ratio
//   40      0.233    2.41      0.043    0.69                               5.4   3.5
//   256     0.411    5.48      0.269    4.31                               1.52  1.27
//   1024    1.30    20.1       1.07    17.2                                1.21  1.17
// The rate is what a register-only loop of 16 independent v_fma_f64 chains reached in the same run, 3.20e13 FMA/s
// (tools/ubench_fma64.hip).  The other floor, one read of the ensemble (psh_realized_variance over the full length), took
// 0.027 and 0.179 ms and is the smaller one in every case.  At m <= 64 a lane owns one lag: 6 double operations and two
// LDS reads for 4 FMAs, and m of a wave's 64 lanes at work (40 of 64 here), hence the 3.5.  The numpy twin takes 6.0,
// 29 and 100 s for the 32768 rows (one run on 256 rows, scaled): 2500, 5400 and 5000 times longer.
// Only this form of the loop was built: the Toeplitz product on v_mfma_f64_16x16x4_f64 was not.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"

namespace psh {

#define PSH_MOM_THREADS 512
#define PSH_MOM_WAVES (PSH_MOM_THREADS / 64)
#define PSH_MOM_TILE 2048
// the largest padded index: samples 0 .. TILE + 1024 at U = 4 (one pad per 4) -> 3840; the slice exchange takes
// 4 chunks * 4 sums * 256 lags = 4096 doubles
#define PSH_MOM_LDS 4104

namespace {

template <int U>
__device__ __forceinline__ int mom_phys(int i) {
    return U == 1 ? i : i + i / U;
}

// t = ts .. te - 1 (both multiples of U) of the staged tile against the lane's U lags 1 + off + j, off a multiple of U
template <int U>
__device__ __forceinline__ void mom_pass(const double* tile, int ts, int te, int off, double (&acc)[4][U]) {
    double w[U], w2[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
        w[j] = tile[mom_phys<U>(ts + 1 + off + j)];
        w2[j] = w[j] * w[j];
    }
#pragma unroll 2
    for (int t = ts; t < te; t += U) {
        const double* pa = tile + mom_phys<U>(t);                  // t is a multiple of U: sample t + k lies at pa[k]
        const double* pb = tile + mom_phys<U>(t + off + U);        // ... and sample t + off + U + r at pb[r], r < U
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const double a = pa[k], a2 = a * a;
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const double b = w[(j + k) % U], b2 = w2[(j + k) % U];
                acc[0][j] = fma(a, b, acc[0][j]);
                acc[1][j] = fma(a, b2, acc[1][j]);
                acc[2][j] = fma(a2, b, acc[2][j]);
                acc[3][j] = fma(a2, b2, acc[3][j]);
            }
            // x[t + k + 1 + (the lane's last lag)] enters where the first lag's sample leaves
            const double nb = pb[k + 1 + ((U > 1 && k + 1 == U) ? 1 : 0)];
            w[k % U] = nb;
            w2[k % U] = nb * nb;
        }
    }
}

template <int U>
__global__ __launch_bounds__(PSH_MOM_THREADS) void moments_kernel(MomentsLagArgs a) {
    __shared__ double tile[PSH_MOM_LDS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, m = a.m, C = a.chunks, S = PSH_MOM_WAVES / C;
    const bool worker = wave < C * S;
    const int chunk = wave % C, slice = wave / C;
    const int off = chunk * 64 * U + lane * U;                    // the lane's lags: 1 + off + j
    const int halo = C * 64 * U;

    const int64_t unit = (int64_t)blockIdx.x, g = unit / a.upg, p = unit % a.upg;
    const int64_t g0 = g * a.R / a.G, g1 = (g + 1) * a.R / a.G;
    const int64_t r0 = g0 + p * a.ru < g1 ? g0 + p * a.ru : g1, r1 = r0 + a.ru < g1 ? r0 + a.ru : g1;

    double acc[4][U];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < U; ++j) acc[q][j] = 0.0;
    double s2 = 0.0, s3 = 0.0, s4 = 0.0;
    int64_t used = 0;

    for (int64_t r = r0; r < r1; ++r) {
        const float* row = a.x + r * a.stride;
        int bad = 0;
        for (int i = tid; i < n; i += PSH_MOM_THREADS) bad |= !isfinite(row[i]);
        if (__syncthreads_or(bad)) continue;                      // (the barrier also ends the reads of the last tile)
        ++used;
        for (int T0 = 0; T0 < n; T0 += PSH_MOM_TILE) {
            const int V = n - T0 < PSH_MOM_TILE ? n - T0 : PSH_MOM_TILE;
            const int Vr = (V + U - 1) / U * U;
            if (T0) __syncthreads();
            for (int i = tid; i <= Vr + halo; i += PSH_MOM_THREADS) {
                const double v = T0 + i < n ? (double)row[T0 + i] : 0.0;
                tile[mom_phys<U>(i)] = v;
                if (i < V) {
                    const double v2 = v * v;
                    s2 += v2;
                    s3 = fma(v, v2, s3);
                    s4 = fma(v2, v2, s4);
                }
            }
            __syncthreads();
            if (worker) {
                const int q = ((Vr + S - 1) / S + U - 1) / U * U;
                const int ts = slice * q < Vr ? slice * q : Vr, te = ts + q < Vr ? ts + q : Vr;
                mom_pass<U>(tile, ts, te, off, acc);
            }
        }
    }
    __syncthreads();

    // ---- the slices, added in slice order by slice 0, which holds the unit's sums of lags 1 .. m
    double* part = a.partial + unit * 4 * (int64_t)(m + 1);
    for (int s = 1; s < S; ++s) {
        if (worker && slice == s) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < U; ++j) tile[(chunk * 4 + q) * 64 * U + j * 64 + lane] = acc[q][j];
        }
        __syncthreads();
        if (worker && slice == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < U; ++j) acc[q][j] += tile[(chunk * 4 + q) * 64 * U + j * 64 + lane];
        }
        __syncthreads();
    }
    if (worker && slice == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < U; ++j)
                if (1 + off + j <= m) part[(int64_t)q * (m + 1) + 1 + off + j] = acc[q][j];
    }

    // ---- lag 0: a fixed tree over the threads
    double* red = tile;
    red[tid] = s2;
    red[PSH_MOM_THREADS + tid] = s3;
    red[2 * PSH_MOM_THREADS + tid] = s4;
    __syncthreads();
    for (int h = PSH_MOM_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            red[tid] += red[tid + h];
            red[PSH_MOM_THREADS + tid] += red[PSH_MOM_THREADS + tid + h];
            red[2 * PSH_MOM_THREADS + tid] += red[2 * PSH_MOM_THREADS + tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[0] = red[0];
        part[(int64_t)(m + 1)] = red[PSH_MOM_THREADS];
        part[2 * (int64_t)(m + 1)] = red[PSH_MOM_THREADS];
        part[3 * (int64_t)(m + 1)] = red[2 * PSH_MOM_THREADS];
        a.unit_rows[unit] = used;
    }
}

// out[g][q][tau] = the partials of group g's units in unit order; rows_used[g]; the status bit
__global__ __launch_bounds__(256) void moments_reduce_kernel(MomentsLagArgs a) {
    const int64_t per = 4 * (int64_t)(a.m + 1), total = a.G * per;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        const int64_t g = i / per, e = i % per;
        const double* part = a.partial + g * a.upg * per + e;
        double s = 0.0;
        for (int64_t p = 0; p < a.upg; ++p) s += part[p * per];
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
        *a.status = rows < a.R ? PSH_MOMENTS_STATUS_ROWS_EXCLUDED : PSH_MOMENTS_STATUS_OK;
    }
}

}  // namespace

void moments_lag_plan(int64_t R, int64_t G, int m, MomentsLagArgs* a) {
    const int64_t per_group = (R + G - 1) / G;
    a->ru = (per_group + 15) / 16;
    a->upg = (per_group + a->ru - 1) / a->ru;
    a->lanes_u = m <= 64 ? 1 : m <= 128 ? 2 : 4;
    const int per_wave = 64 * a->lanes_u;
    a->chunks = m <= per_wave ? 1 : (m + per_wave - 1) / per_wave;
}

hipError_t launch_lagged_moments(const MomentsLagArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)(a.G * a.upg)), block(PSH_MOM_THREADS);
    if (a.lanes_u == 1) hipLaunchKernelGGL((moments_kernel<1>), grid, block, 0, s, a);
    else if (a.lanes_u == 2) hipLaunchKernelGGL((moments_kernel<2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((moments_kernel<4>), grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t total = a.G * 4 * (int64_t)(a.m + 1);
    hipLaunchKernelGGL(moments_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace psh
