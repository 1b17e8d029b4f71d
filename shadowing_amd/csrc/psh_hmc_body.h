// psh_hmc_body.h -- the body of the hedged Monte Carlo fit, shared by psh_hmc.hip (psh_hedged_mc: hmc_kernel<P>) and
// psh_hmc_report.hip (psh_hedged_mc_policy: the same fit with its policy kept).  The method and the decomposition head
// psh_hmc.hip; the policy layout heads psh_hmc_report.hip.  hmc_body<P, false> is the kernel of psh_hedged_mc as it was:
// the POLICY branch is the one store of (mu_n, isd_n, gamma_n, beta_n) per step by the lanes that solve for a strike.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_wave.h"

namespace psh {

#define PSH_HMC_THREADS 256
#define PSH_HMC_WAVES (PSH_HMC_THREADS / 64)
#define PSH_HMC_TAU_ILL 0.2
#define PSH_HMC_TAU_SING 1e-6

namespace {

// tot[q] = sum over the block of v[q]: wave butterflies, then the waves in order from 0.0 (block_reduce of psh_wave.h starts
// at the first wave's sum: the two differ in the sign of a zero total).  Ends with a barrier.
template <int N>
__device__ __forceinline__ void block_sum(const double (&v)[N], double* red, double* tot) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const double s = wave_sum(v[q]);
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

// policy: (B, nT, nM, max Ts, 2P + 4) doubles, zeroed by the launcher (POLICY only; rows n >= T stay 0)
template <int P, bool POLICY>
__device__ __forceinline__ void hmc_body(const HmcArgs& a, double* policy) {
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
            mn = wave_min(mn);
            mx = wave_max(mx);
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
            if constexpr (POLICY) {
                double* row = policy + ((obase + tid) * Tmax + n) * (NF + 2);
                row[0] = mu0;
                row[1] = isd0;
#pragma unroll
                for (int q = 0; q < NF; ++q) row[2 + q] = z[q];
            }
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

}  // namespace psh
