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
// The body lives in psh_hmc_body.h, which psh_hmc_report.hip instantiates a second time with the policy kept.
#include "psh_launch.h"
#include "psh_hmc_body.h"

namespace psh {

template <int P>
__global__ __launch_bounds__(PSH_HMC_THREADS) void hmc_kernel(HmcArgs a) {
    hmc_body<P, false>(a, nullptr);
}

hipError_t launch_hedged_mc(const HmcArgs& a, hipStream_t s) {
    const size_t shmem = (size_t)a.k * sizeof(double);
    const dim3 grid((unsigned)((int64_t)a.B * a.nT * a.ngroups)), block(PSH_HMC_THREADS);
    if (a.status) {                                          // the blocks OR their bits in
        const hipError_t e = hipMemsetAsync(a.status, 0, (size_t)a.B * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    return pick<1, 2, 3, 4, 5>(a.degree, [&](auto P) { return launch(hmc_kernel<P()>, grid, block, shmem, s, a); });
}

}  // namespace psh
