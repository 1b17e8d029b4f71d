// psh_pdv.hip -- path generation of the discrete path-dependent volatility model (Guyon, Lekeufack 2024; the
// reference's PDVModelDiscrete.gen): B * S paths, one lane per path.  Host twin: shadowing_amd/pdv.py (numpy float64).
//
// The method (the contract of this kernel and of pdv.py):
//   Path g = b * S + p (date b, path p) runs n steps in double.
//   * Raw draws z[t], t < n: the caller's (device (B*S) x n float64), or a counter-based Philox4x32-10 keyed by the
//     64-bit seed (key = (seed lo, seed hi)), so the draws of path g at step t depend only on (seed, g, t):
//       - nu == 0, Gaussian: counter (t >> 1, 0, g lo, g hi) gives the 64-bit words a = (x1:x0) >> 11 and
//         b = (x3:x2) >> 11, u1 = (a + 1) 2^-53 in (0, 1], u2 = b 2^-53 in [0, 1); Box-Muller: rad = sqrt(-2 ln u1),
//         z[2m] = rad cos(2 pi u2), z[2m + 1] = rad sin(2 pi u2).
//       - nu > 0, Student-t(nu) by Bailey's polar method: attempt j = 0, 1, ... takes counter (t, j, g lo, g hi),
//         U = a 2^-52 - 1, V = b 2^-52 - 1 (in [-1, 1)), W = U^2 + V^2; the first attempt with 0 < W < 1 gives
//         z = U sqrt(nu (W^(-2/nu) - 1) / W).  Exact for any nu > 0; after PSH_PDV_MAX_ATTEMPTS rejections (probability
//         (1 - pi/4)^64 < 1e-42) z = 0.
//   * Normalisation over the time axis, as numpy's `dw -= mean; dw /= std; dw *= sqrt(dt)`: mean = sum_t z / n,
//     c = z - mean, std = sqrt(sum_t c^2 / n - (sum_t c / n)^2) (numpy takes the std of c, whose mean is ~1e-17),
//     dw[t] = (c[t] / std) * sqrt_dt.  Column 0 enters the mean and the std; the recursion never uses it.
//   * Recursion, R1 = R10[b], R2 = R20[b] (2 factors each), St = S0:
//       sigma(R1, R2) = clip(b0 + b1 r1 + b2 sqrt(r2) [+ b3 ((|r1| + r1) / 2)^2], 0, 1.5),
//         r1 = (1 - th0) R1[0] + th0 R1[1], r2 = (1 - th1) R2[0] + th1 R2[1];
//       t = 0: sigma[0] = sigma(R1, R2), St[0] = S0;
//       t >= 1: sigma[t] = sigma(R1, R2), rt = max(sigma[t] dw[t], -0.999999), St[t] = St[t-1] (1 + rt),
//               R1[i] = decay1[i] R1[i] + lams1[i] rt, R2[i] = decay2[i] R2[i] + lams2[i] rt^2,
//       decay = exp(-lams / 252) as the caller computed it (host and device use the same doubles).
//     clip and max are explicit comparisons that keep a NaN (numpy's clip and maximum propagate it; fmin / fmax would
//     not): a negative r2 gives sqrt(r2) = NaN, and the NaN runs through the rest of the path.
//   * Outputs, each optional: sigma and St (B*S, n) float64; dlnx = float32(log1p(rt)) (B*S, n - 1); the raw draws z
//     and the normalised draws dw (B*S, n) float64.
//
// Decomposition: one lane per path, PSH_PDV_THREADS paths per block, no workspace.  The per-path mean and std need every
// draw before the recursion can start: the draws are generated (or read) three times -- sum, sum of squared deviations,
// recursion -- instead of being stored, so nothing but the outputs touches memory.  Gaussian draws come in Box-Muller
// pairs, so chunks of PSH_PDV_CH (even) steps start at an even t.  Each lane stores its own path's samples.  Measured on
// MI355X (tools/bench_pdv.py, median ms; B = 1 / 64 with S = 8192, n = 75; B = 1, S = 32768, n = 4096), against two
// forms this kernel does not keep:
//   this form                                                                  0.169  0.920  5.59
//   chunks of sigma / St / dlnx staged in LDS and written out as rows          0.187  1.069  6.74
//     (a store then writes 8 consecutive samples of 8 paths, not one sample of 64 paths; the barriers cost more)
//   the draws of chunk c + 1 generated before the recursion of chunk c         0.168  0.922  5.68
//     (independent work for the dependent chain's stalls: no gain, the draws' own cost dominates)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_philox.h"

namespace psh {

#define PSH_PDV_THREADS 256
#define PSH_PDV_CH 8
#define PSH_PDV_MAX_ATTEMPTS 64

namespace {

enum { PDV_GAUSS = 0, PDV_STUDENT = 1, PDV_GIVEN = 2 };

// Philox4x32-10, its 53-bit words and Box-Muller: psh_philox.h (shared with psh_mrw.hip)
__device__ __forceinline__ void normal_pair(uint32_t m, uint64_t g, uint32_t k0, uint32_t k1, double& z0, double& z1) {
    philox_normal_pair(m, 0u, g, k0, k1, z0, z1);
}

__device__ __forceinline__ double student_t(uint32_t t, uint64_t g, uint32_t k0, uint32_t k1, double nu, double nexp) {
    for (uint32_t j = 0; j < PSH_PDV_MAX_ATTEMPTS; ++j) {
        uint64_t a, b;
        philox_words(t, j, g, k0, k1, a, b);
        const double U = (double)a * 0x1p-52 - 1.0, V = (double)b * 0x1p-52 - 1.0;
        const double W = U * U + V * V;
        if (W < 1.0 && W > 0.0) return U * sqrt(nu * (pow(W, nexp) - 1.0) / W);
    }
    return 0.0;
}

// raw draws of steps t0 .. t0 + CH - 1 of path g (steps >= n: Philox values nobody stores, or the path's last given draw)
template <int MODE>
__device__ __forceinline__ void raw_chunk(const PdvArgs& a, uint64_t g, int t0, double (&z)[PSH_PDV_CH]) {
    if constexpr (MODE == PDV_GAUSS) {
#pragma unroll
        for (int j = 0; j < PSH_PDV_CH; j += 2) normal_pair((uint32_t)((t0 + j) >> 1), g, a.key0, a.key1, z[j], z[j + 1]);
    } else if constexpr (MODE == PDV_STUDENT) {
#pragma unroll
        for (int j = 0; j < PSH_PDV_CH; ++j) z[j] = student_t((uint32_t)(t0 + j), g, a.key0, a.key1, a.nu, a.nexp);
    } else {
        const double* row = a.draws + (int64_t)g * a.n;
#pragma unroll
        for (int j = 0; j < PSH_PDV_CH; ++j) z[j] = row[t0 + j < a.n ? t0 + j : a.n - 1];
    }
}

template <bool EXTRA>
__device__ __forceinline__ double pdv_sigma(const PdvArgs& a, double R1a, double R1b, double R2a, double R2b) {
    const double r1 = (1.0 - a.theta[0]) * R1a + a.theta[0] * R1b;
    const double r2 = (1.0 - a.theta[1]) * R2a + a.theta[1] * R2b;
    double s = a.beta[0] + a.beta[1] * r1 + a.beta[2] * sqrt(r2);
    if constexpr (EXTRA) {
        const double h = 0.5 * fabs(r1) + 0.5 * r1;
        s = s + a.beta[3] * (h * h);
    }
    s = (s > 0.0 || s != s) ? s : 0.0;                       // numpy's clip: a NaN stays
    s = (s < 1.5 || s != s) ? s : 1.5;
    return s;
}

}  // namespace

template <int MODE, bool EXTRA>
__global__ __launch_bounds__(PSH_PDV_THREADS) void pdv_kernel(PdvArgs a) {
    constexpr int CH = PSH_PDV_CH;
    const int tid = (int)threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * PSH_PDV_THREADS;
    const bool live = g0 + tid < a.n_paths;
    const int64_t g = live ? g0 + tid : a.n_paths - 1;       // dead lanes shadow the last path and store nothing
    const int n = a.n;
    const double dn = (double)n;

    // ---- pass 1: the mean of the raw draws (and the raw draws, when asked for)
    double sum = 0.0;
    for (int t0 = 0; t0 < n; t0 += CH) {
        double z[CH];
        raw_chunk<MODE>(a, (uint64_t)g, t0, z);
#pragma unroll
        for (int j = 0; j < CH; ++j) sum = t0 + j < n ? sum + z[j] : sum;
        if (a.raw && live) {
#pragma unroll
            for (int j = 0; j < CH; ++j)
                if (t0 + j < n) a.raw[g * n + t0 + j] = z[j];
        }
    }
    const double mean = sum / dn;

    // ---- pass 2: the std of c = z - mean
    double s1 = 0.0, s2 = 0.0;
    for (int t0 = 0; t0 < n; t0 += CH) {
        double z[CH];
        raw_chunk<MODE>(a, (uint64_t)g, t0, z);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const double c = z[j] - mean;
            s1 = t0 + j < n ? s1 + c : s1;
            s2 = t0 + j < n ? s2 + c * c : s2;
        }
    }
    const double m2 = s1 / dn;
    const double sd = sqrt(s2 / dn - m2 * m2);

    // ---- pass 3: the recursion
    const int64_t b = g / a.S;
    double R1a = a.R10[2 * b], R1b = a.R10[2 * b + 1], R2a = a.R20[2 * b], R2b = a.R20[2 * b + 1];
    double st = a.S0;
    for (int t0 = 0; t0 < n; t0 += CH) {
        double z[CH];
        raw_chunk<MODE>(a, (uint64_t)g, t0, z);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int t = t0 + j;
            const double dw = ((z[j] - mean) / sd) * a.sqdt;
            const double sig = pdv_sigma<EXTRA>(a, R1a, R1b, R2a, R2b);
            double rt = sig * dw;
            rt = (rt >= -0.999999 || rt != rt) ? rt : -0.999999;   // numpy's maximum: a NaN stays
            if (t > 0) {
                st = st * (1.0 + rt);
                const double rr = rt * rt;
                R1a = a.decay1[0] * R1a + a.lam1[0] * rt;
                R1b = a.decay1[1] * R1b + a.lam1[1] * rt;
                R2a = a.decay2[0] * R2a + a.lam2[0] * rr;
                R2b = a.decay2[1] * R2b + a.lam2[1] * rr;
            }
            if (live && t < n) {
                if (a.sigma) a.sigma[g * n + t] = sig;
                if (a.St) a.St[g * n + t] = st;
                if (a.dlnx && t > 0) a.dlnx[g * (n - 1) + t - 1] = (float)log1p(rt);
                if (a.dw) a.dw[g * n + t] = dw;
            }
        }
    }
}

hipError_t launch_pdv(const PdvArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.n_paths + PSH_PDV_THREADS - 1) / PSH_PDV_THREADS)), block(PSH_PDV_THREADS);
    const int mode = a.draws ? PDV_GIVEN : (a.nu > 0.0 ? PDV_STUDENT : PDV_GAUSS);
    const bool extra = a.n_betas > 3;
#define PSH_PDV_LAUNCH(M)                                                                \
    if (extra) hipLaunchKernelGGL((pdv_kernel<M, true>), grid, block, 0, s, a);          \
    else hipLaunchKernelGGL((pdv_kernel<M, false>), grid, block, 0, s, a);
    switch (mode) {
        case PDV_GAUSS: PSH_PDV_LAUNCH(PDV_GAUSS) break;
        case PDV_STUDENT: PSH_PDV_LAUNCH(PDV_STUDENT) break;
        default: PSH_PDV_LAUNCH(PDV_GIVEN) break;
    }
#undef PSH_PDV_LAUNCH
    return hipGetLastError();
}

}  // namespace psh
