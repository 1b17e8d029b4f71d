// psh_hmc_report.hip -- the hedge of a smile: the hedged Monte Carlo fit of psh_hmc.hip with its policy kept
// (psh_hedged_mc_policy), and the replay of a policy on paths (psh_hedge_replay): the hedged P&L of every path, its mean,
// the residual risk and the standard error of the price.  Host twin: shadowing_amd/pricing.py (replay_host).
//
// The definition (the contract of these kernels, of pricing.py and of tests/_hmc_report_reference.py):
//   The POLICY of one (date b, maturity T = Ts[q], strike j) is what the fit of psh_hmc.hip computes at every step
//   n = 0 .. T-1: mu_n, isd_n (the standardisation of S_n), gamma_n[0..P] and beta_n[0..P]; dropped unknowns are 0.
//   Layout, double, row-major:  policy[b][q][j][n][c],  n < Tmax = max Ts,  c < 2P + 4 = [mu, isd, gamma_0..P, beta_0..P];
//   rows n >= T are 0.  delta = beta_0[0], the hedge ratio at inception, where the basis is {1}.  (The rows of a maturity
//   that the fit flagged ill-conditioned are what the fit computed and mean nothing; those of a date with bad inputs are 0.)
//   The REPLAY of a policy runs on k' paths of float32 log-returns r' with weights w' (normalised by their sum; NULL:
//   uniform; the rules of the fit).  All arithmetic in double, rho = rate / 252:
//     l_0 = 0, l_{n+1} = l_n + r'[i, n]          S_n = x_init exp(l_n), S_0 = x_init exactly
//     u_n = (S_n - mu_n) isd_n                    phi_n = Horner of beta_n in u_n, top coefficient first (as the fit's V)
//     D_n = e^-rho S_{n+1} - S_n                  gain_i = sum_{n<T} exp(-rho n) phi_n D_n   (n ascending)
//     pay_i = exp(-rho T) payoff_j(S_T)           K_j and call / put are the FIT's (its strike output, kind, sign of M)
//     pnl_i = pay_i - gain_i
//   With the centre c = the fit's price V_0 (so that nothing cancels), nine sums per (b, q, j):
//     a1 = sum w (pnl - c)   a2 = sum w (pnl - c)^2   b1 = sum w^2 (pnl - c)   b2 = sum w^2 (pnl - c)^2
//     p1, p2, q1, q2: the same four of pay         s2 = sum w^2
//     mean = c + a1          risk = sqrt(max(a2 - a1^2, 0))          se = sqrt(max(b2 - 2 a1 b1 + a1^2 s2, 0))
//     mc   = c + p1          risk_unhedged, se_unhedged likewise      n_eff = 1 / s2
//   se treats the policy as fixed: honest on paths the policy was not fitted on, optimistic in-sample.
//   A path of weight 0 contributes nothing, its returns are not read and its pnl is NaN.  A non-finite return in
//   [0, max Ts) of a weighted path, or bad weights, makes all the date's sums and pnl NaN and sets the status bits of
//   psh_hedged_mc.  A maturity whose centre is not finite (the fit flagged it) gives NaN sums and NaN pnl.
//   By construction: in-sample a1 = 0 to rounding (gamma_0 is never dropped, so every step's residual has zero weighted
//   mean); mc - mean = sum w gain; pnl_call,i - pnl_put,i = x_init - K exp(-rho T) for every path at one strike, in or out
//   of sample (the fit is linear in the payoff and S_T - K is hedged exactly by phi = 1); on a full binomial tree with
//   T <= P + 1 every weighted path's pnl is the CRR price, risk = 0 and delta is the CRR delta.
//
// Decomposition of the replay: one block per (date, maturity, group of up to PSH_HMC_SG strikes, tile of PSH_HEDGE_TILE
// paths).  The block stages (mu, isd, beta) of its strikes' policy rows and exp(-rho n) in LDS -- the replay never needs
// gamma -- T (P + 3) doubles a strike; a lane walks its paths forward once and serves all the group's strikes from the same
// S_n (the LDS reads are wave-uniform: broadcasts).  No per-path state in LDS, so k' is not limited by PSH_MAX_K.  A tile's
// sums are taken with the raw weights, as block_sum takes them (per-thread partials over the lane's paths in order, wave
// butterflies, waves in order), and go with sum w and the tile's status bits to the workspace; hedge_finish_kernel adds
// the tiles in tile order and normalises by sum w.  No floating-point atomics: two calls give identical bits, and the
// tile size is a constant, so the result does not depend on the grid.
//
// Device times (tools/bench_smile_report.py on an MI355X: k = 8192, 9 strikes, degree 3, ms per call, median of 20, one
// process; fit = psh_hedged_mc, policy = psh_hedged_mc_policy, replay in-sample without / with pnl):
//   README case (L = 20, Ts 5/10/20)      B = 1: fit 1.12  policy 1.10  replay 0.053 / 0.055;  B = 64: 2.13  2.12  0.349 / 0.345
//   tutorial case (L = 252, Ts 7/25/75)   B = 1: fit 4.00  policy 3.89  replay 0.099 / 0.100;  B = 64: 8.43  8.43  1.399 / 1.409
// The policy variant costs nothing this measurement can see (one store of 2P + 4 doubles per step by <= 3 lanes, and a
// memset); the replay is 3 % to 17 % of the fit.
#include "psh_launch.h"
#include "psh_hmc_body.h"

namespace psh {

template <int P>
__global__ __launch_bounds__(PSH_HMC_THREADS) void hmc_policy_kernel(HmcArgs a, double* policy) {
    hmc_body<P, true>(a, policy);
}

hipError_t launch_hedged_mc_policy(const HmcArgs& a, double* policy, hipStream_t s) {
    const size_t shmem = (size_t)a.k * sizeof(double);
    const dim3 grid((unsigned)((int64_t)a.B * a.nT * a.ngroups)), block(PSH_HMC_THREADS);
    int Tmax = 0;
    for (int q = 0; q < a.nT; ++q) Tmax = a.Ts[q] > Tmax ? a.Ts[q] : Tmax;
    hipError_t e = hipMemsetAsync(policy, 0, (size_t)a.B * a.nT * a.nM * Tmax * (2 * a.degree + 4) * sizeof(double), s);
    if (e != hipSuccess) return e;
    if (a.status) {                                          // the blocks OR their bits in
        e = hipMemsetAsync(a.status, 0, (size_t)a.B * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    return pick<1, 2, 3, 4, 5>(a.degree, [&](auto P) { return launch(hmc_policy_kernel<P()>, grid, block, shmem, s, a, policy); });
}

namespace {
constexpr int even(int n) { return (n + 1) & ~1; }           // LDS carves stay 16-byte aligned
constexpr int HEDGE_NV = 8 * PSH_HMC_SG + 2;                 // per strike a1 a2 b1 b2 p1 p2 q1 q2, then sum w, sum w^2
}  // namespace

size_t hedge_replay_lds_bytes(int T, int degree) {
    return sizeof(double) * ((size_t)even(PSH_HMC_SG * T * (degree + 3)) + even(T) + PSH_HMC_WAVES * HEDGE_NV + HEDGE_NV + 2);
}

template <int P>
__global__ __launch_bounds__(PSH_HMC_THREADS) void hedge_replay_kernel(HedgeReplayArgs a) {
    constexpr int NB = P + 1, NC = 2 * P + 4, NR = P + 3, SG = PSH_HMC_SG, NV = HEDGE_NV;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = (int)threadIdx.x;
    int64_t blk = (int64_t)blockIdx.x;
    const int tile = (int)(blk % a.ntiles);
    blk /= a.ntiles;
    const int g = (int)(blk % a.ngroups);
    blk /= a.ngroups;
    const int it = (int)(blk % a.nT);
    const int b = (int)(blk / a.nT);
    const int T = a.Ts[it], Tmax = a.Tmax;
    const int j0 = g * SG;
    const int ns = (a.nM - j0) < SG ? (a.nM - j0) : SG;
    const int64_t obase = ((int64_t)b * a.nT + it) * a.nM + j0;

    double* pol = lds;                                       // [s][n][mu, isd, beta_0..P]
    double* dn = pol + even(SG * T * NR);                    // exp(-rho n)
    double* red = dn + even(T);
    double* tot = red + PSH_HMC_WAVES * NV;
    int* bad_sh = (int*)(tot + NV);

    const double x0 = a.x_init, rho = a.rate / 252.0;
    for (int e = tid; e < ns * T * NR; e += PSH_HMC_THREADS) {
        const int s = e / (T * NR), rem = e - s * (T * NR), n = rem / NR, c = rem - n * NR;
        pol[e] = a.policy[((obase + s) * Tmax + n) * NC + (c < 2 ? c : c + NB)];
    }
    for (int n = tid; n < T; n += PSH_HMC_THREADS) dn[n] = exp(-rho * (double)n);
    if (tid == 0) *bad_sh = 0;
    __syncthreads();

    const double disc = exp(-rho), discT = exp(-rho * (double)T);
    double Kj[SG], cj[SG];
    bool callj[SG];
#pragma unroll
    for (int s = 0; s < SG; ++s) {
        const double M = s < ns ? a.Ms[j0 + s] : 0.0;
        Kj[s] = s < ns ? a.strike[obase + s] : 0.0;
        cj[s] = s < ns ? a.centre[obase + s] : 0.0;
        callj[s] = a.kind == PSH_HMC_CALL || (a.kind == PSH_HMC_OTM && M >= 0.0);
    }

    double v[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = 0.0;
    int bad = 0;
    const int64_t i1 = ((int64_t)tile + 1) * PSH_HEDGE_TILE < (int64_t)a.k ? ((int64_t)tile + 1) * PSH_HEDGE_TILE : (int64_t)a.k;
#pragma unroll 1
    for (int64_t i = (int64_t)tile * PSH_HEDGE_TILE + tid; i < i1; i += PSH_HMC_THREADS) {
        const double wi = a.w ? a.w[(int64_t)b * a.k + i] : 1.0;
        if (!isfinite(wi)) bad |= PSH_HMC_STATUS_WEIGHTS;
        double pay[SG], gain[SG];
#pragma unroll
        for (int s = 0; s < SG; ++s) pay[s] = gain[s] = 0.0;
        if (wi != 0.0) {
            const float* row = a.x + ((int64_t)b * a.k + i) * a.row_stride;
            double l = 0.0, S0 = x0;
#pragma unroll 1
            for (int n = 0; n < Tmax; ++n) {
                const double r = (double)row[n];
                if (!isfinite(r)) bad |= PSH_HMC_STATUS_NONFINITE;
                if (n >= T) continue;
                l += r;
                const double S1 = x0 * exp(l);
                const double dD = dn[n] * (disc * S1 - S0);
#pragma unroll
                for (int s = 0; s < SG; ++s) {
                    if (s >= ns) break;
                    const double* pr = pol + (s * T + n) * NR;
                    const double u = (S0 - pr[0]) * pr[1];
                    double phi = pr[2 + P];
#pragma unroll
                    for (int q = P - 1; q >= 0; --q) phi = phi * u + pr[2 + q];
                    gain[s] += phi * dD;
                }
                S0 = S1;
            }
#pragma unroll
            for (int s = 0; s < SG; ++s) pay[s] = discT * (callj[s] ? fmax(S0 - Kj[s], 0.0) : fmax(Kj[s] - S0, 0.0));
            const double w2 = wi * wi;
            v[8 * SG] += wi;
            v[8 * SG + 1] += w2;
#pragma unroll
            for (int s = 0; s < SG; ++s) {
                const double dp = (pay[s] - gain[s]) - cj[s], dq = pay[s] - cj[s];
                v[8 * s + 0] += wi * dp;
                v[8 * s + 1] += wi * dp * dp;
                v[8 * s + 2] += w2 * dp;
                v[8 * s + 3] += w2 * dp * dp;
                v[8 * s + 4] += wi * dq;
                v[8 * s + 5] += wi * dq * dq;
                v[8 * s + 6] += w2 * dq;
                v[8 * s + 7] += w2 * dq * dq;
            }
        }
        if (a.pnl) {
#pragma unroll
            for (int s = 0; s < SG; ++s)
                if (s < ns) a.pnl[(obase + s) * a.k + i] = (wi != 0.0 && isfinite(cj[s])) ? pay[s] - gain[s] : NAN;
        }
    }
    if (bad) atomicOr(bad_sh, bad);
    block_sum<NV>(v, red, tot);                              // (its first barrier also publishes bad_sh)
    if (tid < ns) {
        double* out = a.part + ((obase + tid) * a.ntiles + tile) * PSH_HEDGE_NPART;
        out[0] = tot[8 * SG];
#pragma unroll
        for (int q = 0; q < 8; ++q) out[1 + q] = tot[8 * tid + q];
        out[9] = tot[8 * SG + 1];
        out[10] = (double)*bad_sh;
    }
}

// one block per (date, maturity, strike): the tiles in tile order, the normalisation, the NaN rules, the status word
__global__ __launch_bounds__(64) void hedge_finish_kernel(HedgeReplayArgs a) {
    const int64_t o = (int64_t)blockIdx.x;
    const int b = (int)(o / ((int64_t)a.nT * a.nM));
    const double* part = a.part + o * a.ntiles * PSH_HEDGE_NPART;
    double t[PSH_HEDGE_NPART - 1];
#pragma unroll
    for (int q = 0; q < PSH_HEDGE_NPART - 1; ++q) t[q] = 0.0;
    int bad = 0;
    for (int tile = 0; tile < a.ntiles; ++tile) {            // (every lane reads the same words)
#pragma unroll
        for (int q = 0; q < PSH_HEDGE_NPART - 1; ++q) t[q] += part[tile * PSH_HEDGE_NPART + q];
        bad |= (int)part[tile * PSH_HEDGE_NPART + PSH_HEDGE_NPART - 1];
    }
    const double W = t[0];
    if (!(W > 0.0) || !isfinite(W)) bad |= PSH_HMC_STATUS_WEIGHTS;
    const bool nan = bad || !isfinite(a.centre[o]);
    if (threadIdx.x == 0) {
        const double iw = 1.0 / W, iw2 = iw * iw;
        double* out = a.sums + o * PSH_HEDGE_NSUM;
#pragma unroll
        for (int q = 0; q < 8; ++q) out[q] = nan ? NAN : t[1 + q] * ((q & 2) ? iw2 : iw);
        out[8] = nan ? NAN : t[9] * iw2;
        if (bad && a.status) atomicOr(&a.status[b], bad);
    }
    if (bad && a.pnl)
        for (int64_t i = (int64_t)threadIdx.x; i < (int64_t)a.k; i += 64) a.pnl[o * a.k + i] = NAN;
}

hipError_t launch_hedge_replay(const HedgeReplayArgs& a, hipStream_t s) {
    int Tm = 0;
    for (int q = 0; q < a.nT; ++q) Tm = a.Ts[q] > Tm ? a.Ts[q] : Tm;
    const size_t shmem = hedge_replay_lds_bytes(Tm, a.degree);
    const dim3 grid((unsigned)((int64_t)a.B * a.nT * a.ngroups * a.ntiles)), block(PSH_HMC_THREADS);
    hipError_t e;
    if (a.status) {
        e = hipMemsetAsync(a.status, 0, (size_t)a.B * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    e = pick<1, 2, 3, 4, 5>(a.degree, [&](auto P) { return launch(hedge_replay_kernel<P()>, grid, block, shmem, s, a); });
    if (e != hipSuccess) return e;
    return launch(hedge_finish_kernel, (unsigned)((int64_t)a.B * a.nT * a.nM), 64, 0, s, a);
}

}  // namespace psh
