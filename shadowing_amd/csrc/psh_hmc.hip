// psh_hmc.hip -- hedged Monte Carlo (Potters, Bouchaud, Sestovic 2001) on the k shadowing paths of a date: the option
// pricing use of Path Shadowing Monte Carlo.  Host twin: shadowing_amd/pricing.py (numpy float64, the same method).
//
// The method (the contract of this kernel, of pricing.py and of tests/_hmc_reference.py):
//   For one date: k paths of float32 log-returns r[i, t], t < L, and weights w[i] >= 0, normalised by their sum.  Inputs
//   x_init (spot), rate (annual, continuously compounded), maturities Ts (samples, 1 <= T <= L), rescaled log-moneyness
//   Ms, degree P (1..5).  All arithmetic in double.
//   * S[i, 0] = x_init, S[i, n] = x_init * exp(sum_{t<n} r[i, t]);  rho = rate / 252, tau_T = T / 252.
//   * sigma_T = sqrt(sum_i w[i] * (252 / T) * sum_{t<T} r[i, t]^2).
//   * K = x_init * exp(rate * tau_T) * exp(M * sigma_T * sqrt(tau_T)).
//   * kind OTM: a call for M >= 0, a put for M < 0; CALL / PUT force one kind.
//   * V_T = payoff; for n = T-1 .. 0:
//       y_i = e^-rho V_{n+1}(S[i, n+1]),  D_i = e^-rho S[i, n+1] - S[i, n],
//       basis psi_a(u) = u^a, a = 0..P, u = (S[i, n] - mean_n) / std_n (weighted; the fitted function is a polynomial in
//       S, so the standardisation only matters to rounding); when every weighted path has the same price (always at
//       n = 0) u = 0, i.e. the basis is {1};
//       features f_i = (psi_a(u_i))_a ++ (psi_a(u_i) D_i)_a, unknowns (gamma, beta);
//       G theta = h, G = sum_i w_i f_i f_i^T, h = sum_i w_i f_i y_i, by Cholesky in the order gamma_0..gamma_P,
//       beta_0..beta_P: an unknown whose pivot is <= 1e-10 times its diagonal entry of G (or whose diagonal is 0) is
//       dropped -- set to 0, its row and column removed;
//       V_n = sum_a gamma_a psi_a (the hedge phi_n = sum_a beta_a psi_a).
//   * Ill-conditioned: the maturity's prices and IVs are NaN (its strikes and sigma stay) and the date's status word gets
//     PSH_HMC_STATUS_ILL_CONDITIONED when, at some step n < T, a kept unknown has a pivot below its diagonal times
//       - TAU_SING = 1e-6, for any unknown: the fit is nearly singular (on heavy tails, a few outlying paths decide the
//         top powers of u); or
//       - TAU_ILL = 0.2, for beta_0 at a step n > 0: beta_0's pivot over sum_i w_i D_i^2 is the share of D's weighted
//         second moment that no polynomial of degree P in S_n explains.  A small one means the hedge is almost riskless,
//         V and phi D can barely be told apart, and the split between gamma and beta amplifies rounding step after step.
//         (At n = 0 the fit is the 2 x 2 regression on {1, D}: a drifting first step alone cannot amplify anything.)
//     Evidence (numpy twin against tests/_hmc_reference.py, both float64; "agree" is 1e-9 relative + 1e-9 absolute):
//     - Drift sweep: k = 200, L = 20, Ts 5 / 20, returns c + e N(0, 1), c in {0, +-0.001, 0.003, +-0.01}, e 1e-2 .. 1e-6,
//       degrees 1 / 3 / 5.  Every case with a beta_0 ratio >= 0.35 agrees to 2.6e-13 x_init; every case that does not
//       agree has a ratio <= 0.07 (degree 5: 0.058 .. 0.07; degree 3: <= 8e-3; degree 1: <= 8e-5), and below ~1e-2 prices
//       reach 1e10 .. 1e62 on a spot of 100.  There the minimum pivot ratio over all unknowns is no guide: drifting
//       degree-3 data at 9.2e-4 do not agree, GBM with a spread of vols at degree 5, k = 2000, T = 75, reaches 2.2e-4
//       and agrees (Hermite He_a(u) in place of u^a: 2.6e-3 and 3.3e-4, no better).
//     - Student-t 2.5 (tests/_adversarial.py), 24 dates of k = 1000, T = 75, degrees 3 / 4 / 5: every date that does
//       not agree (8e-8 .. 1e-2 absolute, prices from -4 to 584 where the rest give ~6.4) has a minimum kept pivot ratio
//       <= 7.5e-8 (1.2e-7 on other Student-t draws), while its beta_0 ratio stays >= 0.8; every date at >= 4e-7 agrees.
//       GBM data stay at >= 2e-4 at degree 5.
//     - Not covered: an unknown whose pivot rounds to either side of the 1e-10 drop rule in two implementations.
//   * price = V_0; implied vol: Black-Scholes (spot x_init, strike K, tau_T, rate) inverted by exactly 100 bisection
//     halvings on [1e-4, 5]; NaN when the price lies outside [BS(1e-4), BS(5)].
//   * Non-finite weights, a weight sum that is not > 0, or a non-finite return in [0, max Ts) of a path with non-zero
//     weight: the date's results are NaN and its status word says why.
//
// Decomposition: one block per (date, maturity, group of up to PSH_HMC_SG strikes).  The block keeps ln S of its k paths in
// LDS (k <= PSH_MAX_K doubles, 128 KB) and walks n backwards, rebuilding ln S[i, n] = ln S[i, n+1] - r[i, n] from the one
// forward sum; S[i, 0] is x_init exactly.  Per step: a reduction of the mean / spread of S_n, then one of the moments
// sum w u^m, sum w u^m D, sum w u^m D^2 (m <= 2P: every entry of G) and of h for the block's strikes; per-thread partials in
// double, wave sums by butterfly, the waves added in a fixed order (bitwise repeatable).  Wave 0 factorises G (lane i holds
// row i), lane s of the block then solves for strike s and leaves gamma in LDS for the next step's Horner.  The tail of the
// block inverts Black-Scholes by the same bisection as pricing.py.  No workspace.  The status words are zeroed on the
// stream before the launch and OR-ed by the g == 0 block of each (date, maturity), whichever finishes first.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"

namespace psh {

#define PSH_HMC_THREADS 256
#define PSH_HMC_WAVES (PSH_HMC_THREADS / 64)
#define PSH_HMC_TAU_ILL 0.2
#define PSH_HMC_TAU_SING 1e-6

namespace {

__device__ __forceinline__ double hmc_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double hmc_wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double hmc_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// tot[q] = sum over the block of v[q]: wave butterflies, then the waves in order.  Ends with a barrier.
template <int N>
__device__ __forceinline__ void block_sum(const double (&v)[N], double* red, double* tot) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const double s = hmc_wave_sum(v[q]);
        if (lane == 0) red[wave * N + q] = s;
    }
    __syncthreads();
    for (int q = (int)threadIdx.x; q < N; q += PSH_HMC_THREADS) {
        double s = 0.0;
        for (int w = 0; w < PSH_HMC_WAVES; ++w) s += red[w * N + q];
        tot[q] = s;
    }
    __syncthreads();
}

__device__ double norm_cdf(double x) { return 0.5 * erfc(-x * 0.70710678118654752440); }

__device__ double bs_price(double x0, double K, double tau, double rate, double sig, bool call) {
    const double sd = sig * sqrt(tau);
    const double d1 = (log(x0 / K) + (rate + 0.5 * sig * sig) * tau) / sd;
    const double d2 = d1 - sd;
    const double df = exp(-rate * tau);
    return call ? x0 * norm_cdf(d1) - K * df * norm_cdf(d2) : K * df * norm_cdf(-d2) - x0 * norm_cdf(-d1);
}

__device__ double implied_vol(double price, double x0, double K, double tau, double rate, bool call) {
    double lo = 1e-4, hi = 5.0;
    if (!(bs_price(x0, K, tau, rate, lo, call) <= price && price <= bs_price(x0, K, tau, rate, hi, call))) return NAN;
    for (int it = 0; it < 100; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (bs_price(x0, K, tau, rate, mid, call) < price) lo = mid;
        else hi = mid;
    }
    return 0.5 * (lo + hi);
}

}  // namespace

template <int P>
__global__ __launch_bounds__(PSH_HMC_THREADS) void hmc_kernel(HmcArgs a) {
    constexpr int NB = P + 1, NF = 2 * NB, NMOM = 2 * P + 1, SG = PSH_HMC_SG;
    constexpr int NV = 3 * NMOM + 2 * NB * SG;               // moments of G, then h (gamma rows, beta rows) per strike
    extern __shared__ double lnS[];                          // (k) ln(S[i, n+1] / x_init) of the step being solved
    __shared__ double red[PSH_HMC_WAVES * NV];
    __shared__ double tot[NV];
    __shared__ double Lsh[NF * NF];                          // the Cholesky factor (row-major, dropped columns zero)
    __shared__ double coef[SG * NB];                         // gamma of V_{n+1} per strike, basis u_{n+1}
    __shared__ int bad_sh;

    const int tid = (int)threadIdx.x, lane = tid & 63;
    int blk = (int)blockIdx.x;
    const int g = blk % a.ngroups;
    blk /= a.ngroups;
    const int it = blk % a.nT;
    const int b = blk / a.nT;
    const int T = a.Ts[it];
    int Tmax = 0;
    for (int q = 0; q < a.nT; ++q) Tmax = a.Ts[q] > Tmax ? a.Ts[q] : Tmax;
    const int j0 = g * SG;
    const int ns = (a.nM - j0) < SG ? (a.nM - j0) : SG;
    const int k = a.k;
    const float* xb = a.x + (int64_t)b * k * a.row_stride;
    const double* wb = a.w ? a.w + (int64_t)b * k : nullptr;
    const double x0 = a.x_init;

    // ---- ln S_T by the forward sum, the realized variance to T, the non-finite checks
    if (tid == 0) bad_sh = 0;
    __syncthreads();
    {
        double acc[2] = {0.0, 0.0};                          // sum w, sum w * sum_{t<T} r^2
        int bad = 0;
        for (int i = tid; i < k; i += PSH_HMC_THREADS) {
            const double wi = wb ? wb[i] : 1.0;
            if (!isfinite(wi)) bad |= PSH_HMC_STATUS_WEIGHTS;
            double l = 0.0, q2 = 0.0;
            if (wi != 0.0) {
                const float* row = xb + (int64_t)i * a.row_stride;
#pragma unroll 4
                for (int t = 0; t < Tmax; ++t) {
                    const double r = (double)row[t];
                    if (!isfinite(r)) bad |= PSH_HMC_STATUS_NONFINITE;
                    if (t < T) { l += r; q2 += r * r; }
                }
            }
            lnS[i] = l;
            acc[0] += wi;
            acc[1] += wi * q2;
        }
        if (bad) atomicOr(&bad_sh, bad);
        block_sum<2>(acc, red, tot);
    }
    const double wsum = tot[0];
    int bad = bad_sh;
    if (!(wsum > 0.0) || !isfinite(wsum)) bad |= PSH_HMC_STATUS_WEIGHTS;
    const int64_t obase = ((int64_t)b * a.nT + it) * a.nM + j0;
    if (bad) {
        if (tid < ns) {
            a.price[obase + tid] = NAN;
            a.iv[obase + tid] = NAN;
            a.strike[obase + tid] = NAN;
        }
        if (tid == 0 && g == 0 && a.sigma) a.sigma[(int64_t)b * a.nT + it] = NAN;
        if (tid == 0 && g == 0 && it == 0 && a.status) atomicOr(&a.status[b], bad);
        return;                                              // (block-uniform)
    }
    const double invw = 1.0 / wsum;
    const double tau = (double)T / 252.0;
    const double sigma = sqrt((252.0 / (double)T) * (tot[1] * invw));
    const double disc = exp(-(a.rate / 252.0));
    const double fwd = x0 * exp(a.rate * tau);
    double Kj[SG];
    bool callj[SG];
#pragma unroll
    for (int s = 0; s < SG; ++s) {
        const double M = s < ns ? a.Ms[j0 + s] : 0.0;
        Kj[s] = fwd * exp(M * sigma * sqrt(tau));
        callj[s] = a.kind == PSH_HMC_CALL || (a.kind == PSH_HMC_OTM && M >= 0.0);
    }
    if (tid == 0 && g == 0 && a.sigma) a.sigma[(int64_t)b * a.nT + it] = sigma;

    double mu1 = 0.0, isd1 = 0.0;                            // the standardisation of step n+1 (coef's basis)
    bool ill = false;                                        // (wave 0, lane-uniform) the rule of the header
    for (int n = T - 1; n >= 0; --n) {
        // ---- mean / spread of S_n over the weighted paths (u = 0 when they all share one price: always at n = 0)
        double mu0 = x0, isd0 = 0.0;
        if (n > 0) {
            double acc[2] = {0.0, 0.0};
            double mn = INFINITY, mx = -INFINITY;
#pragma unroll 1
            for (int i = tid; i < k; i += PSH_HMC_THREADS) {
                const double wi = wb ? wb[i] : 1.0;
                if (wi == 0.0) continue;
                const double S = x0 * exp(lnS[i] - (double)xb[(int64_t)i * a.row_stride + n]);
                const double wn = wi * invw, d = S - x0;
                acc[0] += wn * d;
                acc[1] += wn * d * d;
                mn = fmin(mn, S);
                mx = fmax(mx, S);
            }
            mn = hmc_wave_min(mn);
            mx = hmc_wave_max(mx);
            if (lane == 0) {
                red[PSH_HMC_WAVES * 2 + (tid >> 6)] = mn;
                red[PSH_HMC_WAVES * 3 + (tid >> 6)] = mx;
            }
            block_sum<2>(acc, red, tot);
            for (int w = 0; w < PSH_HMC_WAVES; ++w) {
                mn = fmin(mn, red[PSH_HMC_WAVES * 2 + w]);
                mx = fmax(mx, red[PSH_HMC_WAVES * 3 + w]);
            }
            if (mn != mx) {
                const double m1 = tot[0], var = tot[1] - m1 * m1;
                mu0 = x0 + m1;
                isd0 = 1.0 / (var > 0.0 ? sqrt(var) : mx - mn);
            }
            __syncthreads();                                 // (red / tot are reused below)
        }

        // ---- moments of G and h of the block's strikes
        double mom[3 * NMOM], hv[2 * NB * SG];
#pragma unroll
        for (int q = 0; q < 3 * NMOM; ++q) mom[q] = 0.0;
#pragma unroll
        for (int q = 0; q < 2 * NB * SG; ++q) hv[q] = 0.0;
#pragma unroll 1
        for (int i = tid; i < k; i += PSH_HMC_THREADS) {
            const double wi = wb ? wb[i] : 1.0;
            if (wi == 0.0) continue;
            const double l1 = lnS[i];
            const double l0 = n > 0 ? l1 - (double)xb[(int64_t)i * a.row_stride + n] : 0.0;
            lnS[i] = l0;
            const double S1 = x0 * exp(l1), S0 = n > 0 ? x0 * exp(l0) : x0;
            const double wn = wi * invw;
            const double D = disc * S1 - S0;
            const double u0 = (S0 - mu0) * isd0;
            double pw[NMOM];
            pw[0] = 1.0;
#pragma unroll
            for (int m = 1; m < NMOM; ++m) pw[m] = pw[m - 1] * u0;
            const double wd = wn * D, wdd = wd * D;
#pragma unroll
            for (int m = 0; m < NMOM; ++m) {
                mom[m] += wn * pw[m];
                mom[NMOM + m] += wd * pw[m];
                mom[2 * NMOM + m] += wdd * pw[m];
            }
            const double u1 = (S1 - mu1) * isd1;
#pragma unroll
            for (int s = 0; s < SG; ++s) {
                if (s >= ns) break;
                double V;
                if (n == T - 1) {
                    V = callj[s] ? fmax(S1 - Kj[s], 0.0) : fmax(Kj[s] - S1, 0.0);
                } else {
                    V = coef[s * NB + P];
#pragma unroll
                    for (int q = P - 1; q >= 0; --q) V = V * u1 + coef[s * NB + q];
                }
                const double y = disc * V;
                const double wy = wn * y, wdy = wd * y;
#pragma unroll
                for (int q = 0; q < NB; ++q) {
                    hv[s * NF + q] += wy * pw[q];
                    hv[s * NF + NB + q] += wdy * pw[q];
                }
            }
        }
        {
            double v[NV];
#pragma unroll
            for (int q = 0; q < 3 * NMOM; ++q) v[q] = mom[q];
#pragma unroll
            for (int q = 0; q < 2 * NB * SG; ++q) v[3 * NMOM + q] = hv[q];
            block_sum<NV>(v, red, tot);
        }

        // ---- pivoted Cholesky of G: lane i of wave 0 holds row i; right-looking, which subtracts the products of a row
        //      in the same order as the left-looking textbook form of pricing.py
        if (tid < 64) {
            double A[NF];
            const int i = lane < NF ? lane : 0;
            const int ai = i < NB ? i : i - NB, bi = i < NB ? 0 : 1;     // row block: gamma (0) / beta (1)
#pragma unroll
            for (int c = 0; c < NF; ++c) {
                const int ac = c < NB ? c : c - NB, bc = c < NB ? 0 : 1;
                A[c] = lane < NF ? tot[(bi + bc) * NMOM + ai + ac] : 0.0;
            }
            double diag0 = 0.0;
#pragma unroll
            for (int c = 0; c < NF; ++c) diag0 = c == lane ? A[c] : diag0;
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const double dj = __shfl(A[j], j, 64), gj = __shfl(diag0, j, 64);
                const bool keep = gj > 0.0 && dj > 1e-10 * gj;
                ill = ill || (keep && (dj < PSH_HMC_TAU_SING * gj || (j == NB && n > 0 && dj < PSH_HMC_TAU_ILL * gj)));
                const double ljj = keep ? sqrt(dj) : 0.0;
                const double lij = !keep ? 0.0 : (lane == j ? ljj : (lane > j ? A[j] / ljj : 0.0));
                A[j] = lij;
#pragma unroll
                for (int c = j + 1; c < NF; ++c) A[c] -= lij * __shfl(lij, c, 64);
            }
            if (lane < NF) {
#pragma unroll
                for (int c = 0; c < NF; ++c) Lsh[lane * NF + c] = c <= lane ? A[c] : 0.0;
            }
        }
        __syncthreads();
        // ---- strike s: forward and back substitution; gamma -> coef
        if (tid < ns) {
            double z[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                double hj = tot[3 * NMOM + tid * NF + j];
#pragma unroll
                for (int c = 0; c < j; ++c) hj -= Lsh[j * NF + c] * z[c];
                const double ljj = Lsh[j * NF + j];
                z[j] = ljj > 0.0 ? hj / ljj : 0.0;
            }
#pragma unroll
            for (int j = NF - 1; j >= 0; --j) {
                double t = z[j];
#pragma unroll
                for (int c = j + 1; c < NF; ++c) t -= Lsh[c * NF + j] * z[c];
                const double ljj = Lsh[j * NF + j];
                z[j] = ljj > 0.0 ? t / ljj : 0.0;            // (z[c > j] already hold theta)
            }
#pragma unroll
            for (int q = 0; q < NB; ++q) coef[tid * NB + q] = z[q];
        }
        __syncthreads();
        mu1 = mu0;
        isd1 = isd0;
    }

    // ---- V_0 = gamma_0 (u = 0 at n = 0); implied vol.  Lanes 0..ns-1 of wave 0 hold `ill`.
    if (tid == 0 && g == 0 && ill && a.status) atomicOr(&a.status[b], PSH_HMC_STATUS_ILL_CONDITIONED);
    if (tid < ns) {
        double K = Kj[0];
        bool call = callj[0];
#pragma unroll
        for (int s = 1; s < SG; ++s)
            if (s == tid) { K = Kj[s]; call = callj[s]; }
        const double price = ill ? NAN : coef[tid * NB];
        a.price[obase + tid] = price;
        a.strike[obase + tid] = K;
        a.iv[obase + tid] = ill ? NAN : implied_vol(price, x0, K, tau, a.rate, call);
    }
}

hipError_t launch_hedged_mc(const HmcArgs& a, hipStream_t s) {
    const size_t shmem = (size_t)a.k * sizeof(double);
    const dim3 grid((unsigned)((int64_t)a.B * a.nT * a.ngroups)), block(PSH_HMC_THREADS);
    if (a.status) {                                          // the blocks OR their bits in
        const hipError_t e = hipMemsetAsync(a.status, 0, (size_t)a.B * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
#define PSH_HMC_CASE(P)                                                                                          \
    case P: {                                                                                                    \
        hipError_t e = hipFuncSetAttribute((const void*)hmc_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                           (int)shmem);                                                          \
        if (e != hipSuccess) return e;                                                                           \
        hipLaunchKernelGGL(hmc_kernel<P>, grid, block, shmem, s, a);                                             \
        break;                                                                                                   \
    }
    switch (a.degree) {
        PSH_HMC_CASE(1)
        PSH_HMC_CASE(2)
        PSH_HMC_CASE(3)
        PSH_HMC_CASE(4)
        PSH_HMC_CASE(5)
        default: return hipErrorInvalidValue;
    }
#undef PSH_HMC_CASE
    return hipGetLastError();
}

}  // namespace psh
