"""An independent float64 restatement of the hedged Monte Carlo method (README "Option pricing"), written from the
method's definition and not from shadowing_amd/pricing.py: plain loops over dates, maturities, strikes and steps, the
Gram matrix built as sum_i w_i f_i f_i^T from explicit features, the weighted mean / std in two passes, and a small
Cholesky with the pivot rule.  Also the known answers of tests/test_hmc_cpu.py and tests/test_gpu_hmc_exact.py."""
from __future__ import annotations

import math

import numpy as np


def norm_cdf(x: float) -> float:
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def bs(x0: float, K: float, tau: float, rate: float, sig: float, call: bool) -> float:
    sd = sig * math.sqrt(tau)
    d1 = (math.log(x0 / K) + (rate + 0.5 * sig * sig) * tau) / sd
    d2 = d1 - sd
    if call:
        return x0 * norm_cdf(d1) - K * math.exp(-rate * tau) * norm_cdf(d2)
    return K * math.exp(-rate * tau) * norm_cdf(-d2) - x0 * norm_cdf(-d1)


def implied_vol(p: float, x0: float, K: float, tau: float, rate: float, call: bool) -> float:
    lo, hi = 1e-4, 5.0
    if not (bs(x0, K, tau, rate, lo, call) <= p <= bs(x0, K, tau, rate, hi, call)):
        return math.nan
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        if bs(x0, K, tau, rate, mid, call) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


TAU_ILL = 0.2
TAU_SING = 1e-6
ILL = 4


def cholesky_solve(G: np.ndarray, h: np.ndarray, first_step: bool = False):
    """Cholesky in the fixed order of the unknowns; an unknown whose pivot <= 1e-10 * G[j, j] (or G[j, j] == 0) is
    dropped (theta_j = 0, its row and column removed).  Returns (theta, ill): ill when a kept unknown has a pivot
    < TAU_SING * G[j, j] (nearly singular), or when beta_0, the first hedge unknown, is kept with a pivot
    < TAU_ILL * G[j, j] at a step other than the first (the hedge is almost a function of today's price)."""
    n = len(h)
    L = np.zeros((n, n))
    kept = []
    ill = False
    for j in range(n):
        piv = G[j, j] - sum(L[j, c] ** 2 for c in kept)
        if G[j, j] == 0.0 or piv <= 1e-10 * G[j, j]:
            continue
        if piv < TAU_SING * G[j, j] or (j == n // 2 and not first_step and piv < TAU_ILL * G[j, j]):
            ill = True
        kept.append(j)
        L[j, j] = math.sqrt(piv)
        for i in range(j + 1, n):
            L[i, j] = (G[i, j] - sum(L[i, c] * L[j, c] for c in kept[:-1])) / L[j, j]
    z = np.zeros(n)
    for j in kept:
        z[j] = (h[j] - sum(L[j, c] * z[c] for c in kept if c < j)) / L[j, j]
    theta = np.zeros(n)
    for j in reversed(kept):
        theta[j] = (z[j] - sum(L[i, j] * theta[i] for i in kept if i > j)) / L[j, j]
    return theta, ill


def hmc_date(r: np.ndarray, w, x0: float, rate: float, Ts, Ms, degree: int = 3, kind: str = "otm"):
    """r (k, L) float32 log-returns, w (k,) or None.  Returns dict of (nT, nM) price / iv / strike and (nT,) sigma, or
    all-NaN results and a non-zero status for bad inputs; an ill-conditioned maturity has NaN prices / ivs and sets
    status bit ILL."""
    k = r.shape[0]
    nT, nM = len(Ts), len(Ms)
    nan = {"price": np.full((nT, nM), np.nan), "iv": np.full((nT, nM), np.nan), "strike": np.full((nT, nM), np.nan),
           "sigma": np.full(nT, np.nan)}
    w = np.ones(k) if w is None else np.asarray(w, dtype=np.float64)
    status = 0
    if not np.all(np.isfinite(w)):
        status |= 2
    elif not w.sum() > 0:
        status |= 2
    for i in range(k):
        if w[i] != 0 and not np.all(np.isfinite(r[i, :max(Ts)])):
            status |= 1
    if status:
        return dict(nan, status=status)
    w = w / w.sum()
    idx = [i for i in range(k) if w[i] != 0]
    rr = r[idx].astype(np.float64)
    ww = w[idx]
    m = len(idx)
    S = np.empty((m, r.shape[1] + 1))
    S[:, 0] = x0
    for i in range(m):
        acc = 0.0
        for t in range(r.shape[1]):
            acc += rr[i, t]
            S[i, t + 1] = x0 * math.exp(acc)
    rho = rate / 252.0
    out = {"price": np.empty((nT, nM)), "iv": np.empty((nT, nM)), "strike": np.empty((nT, nM)), "sigma": np.empty(nT)}
    status = 0
    for q, T in enumerate(Ts):
        tau = T / 252.0
        sig = math.sqrt(sum(ww[i] * (252.0 / T) * float(np.sum(rr[i, :T] ** 2)) for i in range(m)))
        out["sigma"][q] = sig
        for j, M in enumerate(Ms):
            K = x0 * math.exp(rate * tau) * math.exp(M * sig * math.sqrt(tau))
            call = kind == "call" or (kind == "otm" and M >= 0)
            V = np.maximum(S[:, T] - K, 0.0) if call else np.maximum(K - S[:, T], 0.0)
            ill = False
            for n in range(T - 1, -1, -1):
                y = math.exp(-rho) * V
                D = math.exp(-rho) * S[:, n + 1] - S[:, n]
                if np.all(S[:, n] == S[0, n]):
                    u = np.zeros(m)
                else:
                    mean = float(np.sum(ww * S[:, n]))
                    std = math.sqrt(float(np.sum(ww * (S[:, n] - mean) ** 2)))
                    u = (S[:, n] - mean) / std
                psi = np.stack([u ** a for a in range(degree + 1)], axis=1)
                f = np.concatenate([psi, psi * D[:, None]], axis=1)
                G = (f * ww[:, None]).T @ f
                h = (f * ww[:, None]).T @ y
                theta, ill_n = cholesky_solve(G, h, n == 0)
                ill = ill or ill_n
                V = psi @ theta[:degree + 1]
            out["strike"][q, j] = K
            if ill:
                status |= ILL
                out["price"][q, j] = out["iv"][q, j] = math.nan
                continue
            out["price"][q, j] = V[0]
            out["iv"][q, j] = implied_vol(V[0], x0, K, tau, rate, call)
    return dict(out, status=status)


# ---- known answers, computed without the method
def binomial_tree(T: int, reps: int, a: float, rng) -> np.ndarray:
    """(reps * 2^T, T) float32 log-returns: every sequence of +-a, `reps` times, rows shuffled."""
    seq = np.array([[a if (s >> t) & 1 else -a for t in range(T)] for s in range(2 ** T)])
    r = np.tile(seq, (reps, 1))
    return r[rng.permutation(r.shape[0])].astype(np.float32)


def crr_price(x0: float, K: float, a: float, rate: float, T: int, call: bool) -> float:
    """Cox-Ross-Rubinstein: e^{-rho T} E_q[payoff(x0 e^{(2j - T) a})], q = (e^rho - e^-a) / (e^a - e^-a), rho = rate / 252."""
    rho = rate / 252.0
    q = (math.exp(rho) - math.exp(-a)) / (math.exp(a) - math.exp(-a))
    tot = 0.0
    for j in range(T + 1):
        ST = x0 * math.exp((2 * j - T) * a)
        tot += math.comb(T, j) * q ** j * (1.0 - q) ** (T - j) * (max(ST - K, 0.0) if call else max(K - ST, 0.0))
    return math.exp(-rho * T) * tot


def drift_returns(c: float, e: float, k: int = 200, L: int = 20, seed: int = 0):
    """Paths with a common drift c and a spread e between them, float32, and softmax-like weights: the ill-conditioned
    regime of the hedge when |c| >> e."""
    g = np.random.default_rng(seed)
    r = (c + e * g.standard_normal((k, L))).astype(np.float32)
    d = g.random(k)
    w = np.exp(-(d - d.min()) / 0.3)
    return r, w / w.sum()


A = 2.0 ** -6                                  # sums of +-A are exact in double
MS = [-1.5, -0.5, 0.0, 0.5, 1.5]


def binomial_case(P, T, reps, rate, kind, seed, zero_half=False, x0=100.0):
    """A full binomial tree of depth T (every sequence `reps` times, shuffled), random positive weights, and the expected
    strikes and CRR prices (nT = 1)."""
    rng = np.random.default_rng(seed)
    r = binomial_tree(T, reps, A, rng)
    w = rng.uniform(0.25, 1.0, r.shape[0])
    if zero_half:                              # every other copy of each sequence (reps is even): the tree stays full
        seen = {}
        for i, row in enumerate(map(tuple, r)):
            seen[row] = seen.get(row, 0) + 1
            w[i] = 0.0 if seen[row] % 2 else w[i]
        assert (w == 0).sum() == r.shape[0] // 2 and len({tuple(row) for row in r[w > 0]}) == 2 ** T
    tau = T / 252.0
    sig = A * math.sqrt(252.0)
    K = np.array([x0 * math.exp(rate * tau) * math.exp(M * sig * math.sqrt(tau)) for M in MS])
    call = [kind == "call" or (kind == "otm" and M >= 0) for M in MS]
    crr = np.array([crr_price(x0, K[j], A, rate, T, call[j]) for j in range(len(MS))])
    return r, w, K, sig, crr


SWEEP_E = [1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 1e-5, 1e-6]


def check_sweep_case(res, rf, Ts, Ms, x0=100.0):
    """Both flag the same maturities (NaN prices and IVs, finite strikes and sigma), or both agree and stay bounded."""
    assert res["status"] == rf["status"], (res["status"], rf["status"])
    assert res["status"] in (0, ILL)
    np.testing.assert_allclose(res["strike"], rf["strike"], rtol=1e-12)
    np.testing.assert_allclose(res["sigma"], rf["sigma"], rtol=1e-12)
    nan = np.isnan(res["price"])
    np.testing.assert_array_equal(nan, np.isnan(rf["price"]))
    assert (nan.all(axis=1) | ~nan.any(axis=1)).all()                   # whole maturities
    assert np.isnan(res["iv"][nan]).all() and np.isnan(rf["iv"][nan]).all()
    assert nan.any() == bool(res["status"] & ILL)
    ok = ~nan
    np.testing.assert_allclose(res["price"][ok], rf["price"][ok], rtol=1e-9, atol=1e-9)
    assert (np.abs(res["price"][ok]) <= 2 * (x0 + res["strike"][ok])).all()
    return nan


def student_t_dates(seed: int, B: int = 8, k: int = 1000, L: int = 75):
    """(B, k, L) float32 Student-t (2.5) returns of tests/_adversarial.py ("student_t") and (B, k) softmax-like weights:
    heavy tails, where a few outlying paths can make the fit nearly singular."""
    import _adversarial as adv
    ds, _ = adv.make("student_t", B * k, L + 40, 1, 20, 20, seed)
    d = np.random.default_rng(seed).random((B, k))
    w = np.exp(-(d - d.min(axis=1, keepdims=True)) / 0.3)
    return np.ascontiguousarray(ds[:, :L].reshape(B, k, L)), w


def assert_iv_close(iv, want, price, strike, Ts, x0: float, rate: float):
    """IVs to 1e-8, plus the move that a price error of 1e-9 (relative and absolute) allows where vega is tiny; NaN where
    `want` is NaN.  iv, want, price, strike: (nT, nM)."""
    tau = (np.asarray(Ts, dtype=np.float64) / 252.0)[:, None]
    sig = np.where(np.isfinite(want), want, 1.0)
    d1 = (np.log(x0 / strike) + (rate + 0.5 * sig ** 2) * tau) / (sig * np.sqrt(tau))
    vega = x0 * np.exp(-0.5 * d1 ** 2) / math.sqrt(2 * math.pi) * np.sqrt(tau)
    tol = 1e-8 + (1e-9 * np.abs(price) + 1e-9) / np.maximum(vega, 1e-300)
    np.testing.assert_array_equal(np.isnan(iv), np.isnan(want))
    ok = np.isfinite(want)
    assert (np.abs(iv[ok] - want[ok]) <= tol[ok]).all(), np.argwhere(ok & ~(np.abs(iv - want) <= tol))
