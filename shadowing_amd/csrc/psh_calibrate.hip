// psh_calibrate.hip -- the weights of the k shadowing paths of a date, moved as little as possible in relative entropy from
// their prior until the weighted paths reprice quoted vanillas (psh_calibrate_weights): the weighted Monte Carlo of
// Avellaneda, Buff, Friedman, Grandchamp, Kruk and Newman (2001).  What comes out is a (B, k) float64 weight array, which
// psh_hedged_mc, psh_hedge_replay, psh_weighted_quantiles, psh_weighted_moments and psh_score_ensemble take as given.
// Host twin: shadowing_amd/calibration.py (calibrate_host).
//
// The definition (shared with the twin, include/psh.h and README "Calibrating to market quotes"), for one date b, all in
// double:
//   r[i, 0..len) float32 log-returns of path i (any row stride), p_i >= 0 the prior weights (NULL: 1), rho = rate / 252,
//   Ts[0..nT) maturities in samples, strike[q, m] and target[q, m] the quotes (a NaN target: not quoted).
//     l_0 = 0, l_{n+1} = l_n + r[i, n]  (sequential)      S_{T,i} = x_init exp(l_T)
//     g_ij = exp(-rho T_j) payoff_j(S_{T_j, i})            payoff: max(S - K, 0) call, max(K - S, 0) put;
//                                                          PSH_HMC_OTM: a call iff K >= x_init exp(rho T)
//     the forward of maturity q (martingale != 0): g = exp(-rho T) S_T, target c = x_init
//     h_ij = (g_ij - c_j) / x_init                         instrument j = q * nM + m;  forwards: nT * nM + q
//     J = nT * nM + (martingale ? nT : 0) <= PSH_CAL_MAX_INSTRUMENTS = 32
//   exp(-rho T) and x_init exp(rho T) are formed once on the host, in double.  The weights are
//     a_i = sum_j lambda_j h_ij (quoted j, ascending)      amax = max of a over the paths with p_i > 0
//     e_i = p_i exp(a_i - amax)      Z = sum e_i      P = sum p_i  (fixed order)      q_i = e_i / Z
//   and lambda minimises   Phi = amax + ln(Z / P) + (eps / 2) |lambda|^2 :
//     grad_j = mu_j + eps lambda_j,  mu_j = sum_i q_i h_ij,   H_jl = sum_i q_i h_ij h_il - mu_j mu_l + eps delta_jl.
//   The iteration: lambda = 0; stop with success when max_j |grad_j| <= tol; else solve H d = -grad by Cholesky in
//   instrument order, dropping an unknown whose diagonal is not > 0 or whose pivot is <= 1e-10 of its diagonal (step 0;
//   psh_hmc's rule and constant; an unquoted instrument is never an unknown); backtrack t = 1, 1/2, ..., 2^-40 until
//   Phi(lambda + t d) <= Phi(lambda) + 1e-4 t grad.d; at most max_iter steps.  Every unknown dropped above tol, a failed
//   line search or max_iter steps taken above tol: the last iterate with PSH_CAL_STATUS_NOT_CONVERGED.
//   Outputs: weights q (exactly 0 where p_i = 0), lambda (0 for unquoted and dropped unknowns), model_j = sum q_i g_ij
//   (every instrument, quoted or not), info = [kl = sum q_i (a_i - amax) - ln(Z / P), n_eff = 1 / sum q_i^2, steps taken,
//   max_j |grad_j|], status.  NONFINITE (a non-finite return in [0, max Ts) of a path with p_i > 0), WEIGHTS (a prior
//   weight that is negative or not finite, or P not > 0) and QUOTES (a strike that is not finite and > 0, an infinite
//   target): every output of the date is NaN.  A path with p_i = 0 is never read for its value.  p enters only through
//   p_i exp(.), Z and Z / P, so scaling the prior by a power of two changes no bit.  No floating-point atomics; a date is
//   one workgroup's work and its bits depend on nothing else.
//
// The method, two launches:
//   1. cal_terminal_kernel: the only large read.  A workgroup of 256 threads takes 256 paths; 32 lanes read 128 consecutive
//      bytes of a row into an LDS tile (256 rows x 32 returns, a row 33 floats apart), then each thread walks its own row
//      in the tile, sequentially in double as the definition asks, and writes S_T of every maturity to the workspace,
//      (B, k, nT) doubles -- a path's maturities side by side, so the second launch finds them in one cache line.  A path
//      with a non-finite return before max Ts gets NaN at every maturity, which is how the second launch learns of it.
//      (With max_iter = 0 -- this launch, the checks, one Phi and one Hessian pass -- a 252 x 8192 x 75 call took 3.36 ms
//      while one thread read one row straight from memory, and 1.28 ms with the tile, the reciprocal below and the KL sum
//      folded into Phi, which came together.)
//   2. cal_newton_kernel: one workgroup of 512 threads per date does the whole iteration; thread t owns the paths t,
//      t + 512, ...  The k x J matrix h is never stored: its columns are recomputed from S_T (L2-resident between passes).
//      Here h is formed as (g - c) * (1 / x_init), the reciprocal rounded once on the host: one rounding more per h than
//      the definition's division, inside the consistency bound of the README (its (J + 5) |h| term), and it spares a
//      double division per path and instrument in every pass.
//        * Phi at a trial lambda: a_i of the thread's paths go to a workspace row (each thread reads back only what it
//          wrote, so no register array lives across the Hessian pass), amax, Z and sum e_i (a_i - amax) by a fixed tree:
//          a butterfly over a wave's 64 lanes, then the 8 waves in order through LDS.  Every thread adds the same numbers
//          in the same order, so all hold the same Phi and take the line search's decision alike -- nothing is broadcast.
//        * An accepted lambda writes q to out_weights, which is also where the Hessian pass reads it from.
//        * mu and H: the rows of the lower triangle are dealt to the waves two adjacent rows at a time, longest first, there
//          and back, so every wave carries about the same number of entries (J = 32: two passes).  Per pass and tile of 512
//          paths, thread t fills column t of the tile of h in LDS (128 KiB), then each wave accumulates its two rows over
//          the tile, a lane per path: one LDS read of h_il feeds acc0[l] = fma(q_i h_ij, h_il, acc0[l]) and the same for the
//          row below -- explicit fmas; the library is compiled with -ffp-contract=off -- in blocks of eight l behind a
//          scalar branch; at the end the J + 1 sums of a row are reduced by the butterfly.  Each entry of H has one
//          wave's fixed order, so the bits do not depend on anything but the date.
//        * The Cholesky factor is built column by column, thread i < J computing entry (i, j) with its sum in ascending
//          order, a barrier a column; thread 0 runs the two triangular solves.
//      LDS: 128 KiB tile + 4 KiB of q + two 32 x 33 matrices + the vectors: 154832 bytes of the 163840 a workgroup may
//      hold; 243 VGPRs of the 256 that 512 threads leave, no scratch.
//   Measured on MI355X (tools/bench_calibration.py, k = 8192, J = 30, eps = 1e-6, ms a call): 3.76 for one date (5 steps),
//   4.55 for 64 (6 steps), 5.72 for 252 (7 steps); the first form of the Hessian pass (a tile of 256 paths filled by all
//   threads, one row a wave and pass, so four passes) took 6.47 / 8.24 / 11.83.  That is 25 to 30 times the arithmetic
//   floor of k J^2 / 2 FMAs a step: the README says what the rest is.  The Hessian on v_mfma_f64_16x16x4_f64 was not
//   built, so only the vector-ALU form has a number.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "psh.h"
#include "psh_kernels.h"
#include "psh_wave.h"

namespace psh {

namespace {

#define CAL_THREADS 512
#define CAL_WAVES (CAL_THREADS / 64)
#define CAL_CH CAL_THREADS               // paths of a tile of h: a thread fills one path's column
#define CAL_LD (PSH_CAL_MAX_INSTRUMENTS + 1)

__global__ __launch_bounds__(256) void cal_terminal_kernel(CalArgs a) {
    __shared__ float tile[256 * 33];                          // 256 rows x 32 returns, a row 33 floats apart: no bank conflict
    const int nblk = (a.k + 255) / 256, tid = (int)threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x / nblk;
    const int i0 = (int)(blockIdx.x % nblk) * 256, i = i0 + tid;
    const int col = tid & 31, sub = tid >> 5;
    double l = 0.0;
    bool bad = false;
    for (int n0 = 0; n0 < a.Tmax; n0 += 32) {
        __syncthreads();
        for (int rr = sub; rr < 256; rr += 8) {               // 32 lanes read 128 consecutive bytes of a row
            float v = 0.0f;
            if (i0 + rr < a.k && n0 + col < a.Tmax) v = a.x[(b * a.k + i0 + rr) * a.row_stride + n0 + col];
            tile[rr * 33 + col] = v;
        }
        __syncthreads();
        if (i < a.k) {
            double* st = a.st + (b * a.k + i) * a.nT;
            for (int c = 0; c < 32 && n0 + c < a.Tmax; ++c) {
                const float r = tile[tid * 33 + c];
                bad |= !isfinite(r);
                l = l + (double)r;
                for (int q = 0; q < a.nT; ++q)
                    if (a.Ts[q] == n0 + c + 1) st[q] = a.x_init * exp(l);
            }
        }
    }
    if (i < a.k && bad) {
        double* st = a.st + (b * a.k + i) * a.nT;
        for (int q = 0; q < a.nT; ++q) st[q] = __longlong_as_double(0x7ff8000000000000ll);
    }
}

// the discounted payoff of an instrument: sgn > 0 a call, < 0 a put, 0 the forward
__device__ __forceinline__ double cal_g(double S, double K, double disc, int sgn) {
    const double pay = sgn == 0 ? S : fmax(sgn > 0 ? S - K : K - S, 0.0);
    return disc * pay;
}

struct CalShared {
    double hs[PSH_CAL_MAX_INSTRUMENTS * CAL_CH];   // the tile of h: hs[j * CAL_CH + path of the tile]
    double qs[CAL_CH];                             // q of the tile's paths
    double Hs[PSH_CAL_MAX_INSTRUMENTS * CAL_LD];   // sum q h_j h_l (lower triangle)
    double Ls[PSH_CAL_MAX_INSTRUMENTS * CAL_LD];   // its Cholesky factor; L_jj = 0: j is not an unknown
    double mu[PSH_CAL_MAX_INSTRUMENTS], lam[PSH_CAL_MAX_INSTRUMENTS], trial[PSH_CAL_MAX_INSTRUMENTS];
    double step[PSH_CAL_MAX_INSTRUMENTS], grad[PSH_CAL_MAX_INSTRUMENTS];
    double K[PSH_CAL_MAX_INSTRUMENTS], c[PSH_CAL_MAX_INSTRUMENTS], disc[PSH_CAL_MAX_INSTRUMENTS];
    int q[PSH_CAL_MAX_INSTRUMENTS], sgn[PSH_CAL_MAX_INSTRUMENTS], act[PSH_CAL_MAX_INSTRUMENTS];
    double red[CAL_WAVES];
    int dropped;
};

// a_i of the thread's live paths at sh.trial, left in ab[] (each thread reads back only what it wrote); amax returned
__device__ __forceinline__ double cal_args(const CalArgs& a, CalShared& sh, const double* st, const double* prior, double* ab) {
    const int J = a.J, k = a.k, nT = a.nT;
    double m = -INFINITY;
    for (int i = (int)threadIdx.x; i < k; i += CAL_THREADS) {
        if (!((prior ? prior[i] : 1.0) > 0.0)) continue;
        double s = 0.0, S = 0.0;
        int qs = -1;                                          // (S_T is loaded when the maturity changes, not per instrument)
        for (int j = 0; j < J; ++j) {
            if (!sh.act[j]) continue;
            if (sh.q[j] != qs) { qs = sh.q[j]; S = st[(int64_t)i * nT + qs]; }
            const double h = (cal_g(S, sh.K[j], sh.disc[j], sh.sgn[j]) - sh.c[j]) * a.inv_x;
            s = s + sh.trial[j] * h;
        }
        m = fmax(m, s);
        ab[i] = s;
    }
    return block_reduce<CAL_WAVES, true>(m, sh.red, WaveMax{});
}

__global__ __launch_bounds__(CAL_THREADS) void cal_newton_kernel(CalArgs a) {
    __shared__ CalShared sh;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), k = a.k, J = a.J, nQ = a.nT * a.nM;
    const int64_t b = (int64_t)blockIdx.x;
    const double* st = a.st + b * a.nT * k;
    const double* prior = a.prior ? a.prior + b * k : nullptr;
    double* outw = a.w + b * k;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    double* ab = a.st + (int64_t)a.B * a.nT * k + b * k;     // a_i, then e_i, of the trial lambda

    // ---- the instruments; are the quotes usable?
    int bad_quotes = 0;
    if (tid < J) {
        const int j = tid;
        if (j < nQ) {
            const int q = j / a.nM;
            const double K = a.strike[b * nQ + j], c = a.target[b * nQ + j];
            if (!(isfinite(K) && K > 0.0) || isinf(c)) bad_quotes = 1;
            sh.q[j] = q; sh.K[j] = K; sh.disc[j] = a.disc[q];
            sh.act[j] = c == c ? 1 : 0;
            sh.c[j] = c == c ? c : 0.0;
            sh.sgn[j] = a.kind == PSH_HMC_CALL ? 1 : a.kind == PSH_HMC_PUT ? -1 : (K >= a.fwd[q] ? 1 : -1);
        } else {
            const int q = j - nQ;
            sh.q[j] = q; sh.K[j] = 0.0; sh.disc[j] = a.disc[q]; sh.act[j] = 1; sh.c[j] = a.x_init; sh.sgn[j] = 0;
        }
        sh.lam[j] = 0.0; sh.trial[j] = 0.0; sh.step[j] = 0.0; sh.grad[j] = 0.0; sh.mu[j] = 0.0;
    }
    if (tid == 0) sh.dropped = 0;

    // ---- the prior: which of my paths are live, P, and what is wrong with the inputs
    int bad_w = 0, bad_r = 0;
    double psum = 0.0;
    for (int i = tid; i < k; i += CAL_THREADS) {
        const double p = prior ? prior[i] : 1.0;
        if (!isfinite(p) || p < 0.0) bad_w = 1;
        psum = psum + p;
        if (p > 0.0) {
            const double s0 = st[(int64_t)i * a.nT];
            if (s0 != s0) bad_r = 1;
        }
    }
    const double P = block_reduce<CAL_WAVES, true>(psum, sh.red, WaveSum{});          // (its barriers also publish the instruments)
    if (!(P > 0.0) || !isfinite(P)) bad_w = 1;
    int status = (__syncthreads_or(bad_r) ? PSH_CAL_STATUS_NONFINITE : 0);
    status |= (__syncthreads_or(bad_w) ? PSH_CAL_STATUS_WEIGHTS : 0);
    status |= (__syncthreads_or(bad_quotes) ? PSH_CAL_STATUS_QUOTES : 0);
    if (status) {
        for (int i = tid; i < k; i += CAL_THREADS) outw[i] = qnan;
        if (tid < J) { a.lam[b * J + tid] = qnan; a.model[b * J + tid] = qnan; }
        if (tid < 4) a.info[b * 4 + tid] = qnan;
        if (tid == 0) a.status[b] = status;
        return;
    }

    // Phi at sh.trial; leaves e_i in ab[] and returns Z through zout, ln(Z / P) through lout, sum e_i (a_i - amax) through kout
    auto phi_at = [&](double& zout, double& lout, double& kout) -> double {
        const double amax = cal_args(a, sh, st, prior, ab);
        double zs = 0.0, ks = 0.0;
        for (int i = tid; i < k; i += CAL_THREADS) {
            const double p = prior ? prior[i] : 1.0;
            double e = 0.0;
            if (p > 0.0) {
                const double d = ab[i] - amax;
                e = p * exp(d);
                ks = ks + e * d;
            }
            ab[i] = e;
            zs = zs + e;
        }
        const double Z = block_reduce<CAL_WAVES, true>(zs, sh.red, WaveSum{});
        kout = block_reduce<CAL_WAVES, true>(ks, sh.red, WaveSum{});
        double l2 = 0.0;
        for (int j = 0; j < J; ++j) l2 = l2 + sh.trial[j] * sh.trial[j];
        zout = Z;
        lout = log(Z / P);
        return (amax + lout) + (0.5 * a.eps) * l2;
    };

    double Z = 0.0, lnzp = 0.0, ksum = 0.0;
    double phi = phi_at(Z, lnzp, ksum);                    // lambda = 0
    int steps = 0, dropped_last = 0;
    double gmax = 0.0;

    for (;;) {
        // ---- q of the accepted lambda, where the passes below and the caller read it
        for (int i = tid; i < k; i += CAL_THREADS) outw[i] = ab[i] / Z;
        __threadfence_block();
        __syncthreads();

        // ---- mu and the lower triangle of sum q h h: two adjacent rows a wave and pass, longest first, there and back
        for (int pass = 0; 2 * pass * CAL_WAVES < J; ++pass) {
            const int slot = pass * CAL_WAVES + ((pass & 1) ? CAL_WAVES - 1 - wave : wave);
            const int r0 = J - 1 - 2 * slot, r1 = r0 - 1;       // (r1 = -1: a last row on its own)
            const bool mine = r0 >= 0;
            double acc0[PSH_CAL_MAX_INSTRUMENTS], acc1[PSH_CAL_MAX_INSTRUMENTS], mu0 = 0.0, mu1 = 0.0;
#pragma unroll
            for (int l = 0; l < PSH_CAL_MAX_INSTRUMENTS; ++l) acc0[l] = acc1[l] = 0.0;
            for (int c0 = 0; c0 < k; c0 += CAL_CH) {
                __syncthreads();
                {
                    const int i = c0 + tid;
                    const bool in = i < k, lv = in && (prior ? prior[i] : 1.0) > 0.0;
                    double S = a.x_init;
                    int qs = -1;
                    for (int j = 0; j < J; ++j) {
                        if (sh.q[j] != qs) { qs = sh.q[j]; S = lv ? st[(int64_t)i * a.nT + qs] : a.x_init; }
                        sh.hs[j * CAL_CH + tid] = in ? (cal_g(S, sh.K[j], sh.disc[j], sh.sgn[j]) - sh.c[j]) * a.inv_x : 0.0;
                    }
                    sh.qs[tid] = in ? outw[i] : 0.0;
                }
                __syncthreads();
                if (mine) {
#pragma unroll 1
                    for (int u = 0; u < CAL_CH / 64; ++u) {
                        const int ii = lane + 64 * u;
                        const double q = sh.qs[ii];
                        const double qh0 = q * sh.hs[r0 * CAL_CH + ii];
                        const double qh1 = r1 >= 0 ? q * sh.hs[r1 * CAL_CH + ii] : 0.0;
                        mu0 = mu0 + qh0;
                        mu1 = mu1 + qh1;
#pragma unroll
                        for (int l = 0; l < PSH_CAL_MAX_INSTRUMENTS; ++l)       // (in eights: a scalar branch each; entries past the row are not used)
                            if ((l & ~7) <= r0) {
                                const double hl = sh.hs[l * CAL_CH + ii];
                                acc0[l] = fma(qh0, hl, acc0[l]);
                                acc1[l] = fma(qh1, hl, acc1[l]);
                            }
                    }
                }
            }
            if (mine) {
                mu0 = wave_sum(mu0);
                mu1 = wave_sum(mu1);
                if (lane == 0 && sh.act[r0]) sh.mu[r0] = mu0;
                if (lane == 0 && r1 >= 0 && sh.act[r1]) sh.mu[r1] = mu1;
#pragma unroll
                for (int l = 0; l < PSH_CAL_MAX_INSTRUMENTS; ++l) {
                    if (l > r0) continue;
                    const double v0 = wave_sum(acc0[l]), v1 = wave_sum(acc1[l]);
                    if (lane == 0) sh.Hs[r0 * CAL_LD + l] = v0;
                    if (lane == 0 && l <= r1) sh.Hs[r1 * CAL_LD + l] = v1;
                }
            }
        }
        __syncthreads();

        // ---- the gradient; done?
        if (tid < J) sh.grad[tid] = sh.act[tid] ? sh.mu[tid] + a.eps * sh.lam[tid] : 0.0;
        __syncthreads();
        gmax = 0.0;
        for (int j = 0; j < J; ++j) gmax = fmax(gmax, fabs(sh.grad[j]));
        if (gmax <= a.tol) break;
        if (!(gmax == gmax)) { status |= PSH_CAL_STATUS_NOT_CONVERGED; break; }
        if (steps >= a.max_iter) { status |= PSH_CAL_STATUS_NOT_CONVERGED; break; }

        // ---- H d = -grad: the factor column by column, thread i the entry (i, j)
        if (tid == 0) sh.dropped = 0;
        int kept = 0;
        for (int j = 0; j < J; ++j) {
            const double hjj = (sh.Hs[j * CAL_LD + j] - sh.mu[j] * sh.mu[j]) + a.eps;
            double d = hjj;
            for (int c = 0; c < j; ++c) d = d - sh.Ls[j * CAL_LD + c] * sh.Ls[j * CAL_LD + c];
            const bool keep = sh.act[j] && hjj > 0.0 && d > 1e-10 * hjj;
            kept += keep ? 1 : 0;
            if (!keep) {
                if (tid >= j && tid < J) sh.Ls[tid * CAL_LD + j] = 0.0;
                if (tid == 0 && sh.act[j]) sh.dropped = 1;
            } else {
                const double ljj = sqrt(d);
                if (tid == j) sh.Ls[j * CAL_LD + j] = ljj;
                if (tid > j && tid < J) {
                    double v = 0.0;                           // (the row of an unquoted instrument was not summed)
                    if (sh.act[tid]) {
                        v = sh.Hs[tid * CAL_LD + j] - sh.mu[tid] * sh.mu[j];
                        for (int c = 0; c < j; ++c) v = v - sh.Ls[tid * CAL_LD + c] * sh.Ls[j * CAL_LD + c];
                        v = v / ljj;
                    }
                    sh.Ls[tid * CAL_LD + j] = v;
                }
            }
            __syncthreads();
        }
        dropped_last = sh.dropped;
        if (kept == 0) { status |= PSH_CAL_STATUS_NOT_CONVERGED; break; }
        if (tid == 0) {
            for (int j = 0; j < J; ++j) {
                double v = -sh.grad[j];
                for (int c = 0; c < j; ++c) v = v - sh.Ls[j * CAL_LD + c] * sh.step[c];
                const double ljj = sh.Ls[j * CAL_LD + j];
                sh.step[j] = ljj > 0.0 ? v / ljj : 0.0;
            }
            for (int j = J - 1; j >= 0; --j) {
                double v = sh.step[j];
                for (int c = j + 1; c < J; ++c) v = v - sh.Ls[c * CAL_LD + j] * sh.step[c];
                const double ljj = sh.Ls[j * CAL_LD + j];
                sh.step[j] = ljj > 0.0 ? v / ljj : 0.0;
            }
        }
        __syncthreads();
        double gd = 0.0;
        for (int j = 0; j < J; ++j) gd = gd + sh.grad[j] * sh.step[j];

        // ---- backtrack
        bool accepted = false;
        double t = 1.0;
        for (int halving = 0; halving <= 40; ++halving, t = 0.5 * t) {
            __syncthreads();                                  // (the last trial has been read)
            if (tid < J) sh.trial[tid] = sh.lam[tid] + t * sh.step[tid];
            __syncthreads();
            double zt, lt, kt;
            const double pt = phi_at(zt, lt, kt);
            if (pt <= phi + (1e-4 * t) * gd) {
                accepted = true;
                phi = pt; Z = zt; lnzp = lt; ksum = kt;
                break;
            }
        }
        if (!accepted) { status |= PSH_CAL_STATUS_NOT_CONVERGED; break; }
        if (tid < J) sh.lam[tid] = sh.trial[tid];
        ++steps;
        __syncthreads();
    }
    if (dropped_last) status |= PSH_CAL_STATUS_DROPPED;

    // ---- the results at the last accepted lambda (q is in out_weights already)
    __syncthreads();
    double q2 = 0.0;
    for (int i = tid; i < k; i += CAL_THREADS) {
        const double q = outw[i];
        q2 = q2 + q * q;
    }
    const double kl = ksum / Z - lnzp;
    const double s2 = block_reduce<CAL_WAVES, true>(q2, sh.red, WaveSum{});
    for (int j = wave; j < J; j += CAL_WAVES) {
        double m = 0.0;
#pragma unroll 4
        for (int i = lane; i < k; i += 64) {
            const double p = prior ? prior[i] : 1.0;
            const double S = p > 0.0 ? st[(int64_t)i * a.nT + sh.q[j]] : a.x_init;
            m = m + outw[i] * cal_g(S, sh.K[j], sh.disc[j], sh.sgn[j]);
        }
        m = wave_sum(m);
        if (lane == 0) a.model[b * J + j] = m;
    }
    if (tid < J) a.lam[b * J + tid] = sh.lam[tid];
    if (tid == 0) {
        a.info[b * 4 + 0] = kl;
        a.info[b * 4 + 1] = 1.0 / s2;
        a.info[b * 4 + 2] = (double)steps;
        a.info[b * 4 + 3] = gmax;
        a.status[b] = status;
    }
}

}  // namespace

hipError_t launch_calibrate(const CalArgs& a, hipStream_t s) {
    const int nblk = (a.k + 255) / 256;
    hipLaunchKernelGGL(cal_terminal_kernel, dim3((unsigned)((int64_t)a.B * nblk)), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cal_newton_kernel, dim3((unsigned)a.B), dim3(CAL_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace psh
