"""An independent float64 restatement of the hedged Monte Carlo method (README "Option pricing"), written from the
method's definition and not from shadowing_amd/pricing.py: plain loops over dates, maturities, strikes and steps, the
Gram matrix built as sum_i w_i f_i f_i^T from explicit features, the weighted mean / std in two passes, and a small
Cholesky with the pivot rule."""
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


def cholesky_solve(G: np.ndarray, h: np.ndarray) -> np.ndarray:
    """Cholesky in the fixed order of the unknowns; an unknown whose pivot <= 1e-10 * G[j, j] (or G[j, j] == 0) is
    dropped (theta_j = 0, its row and column removed)."""
    n = len(h)
    L = np.zeros((n, n))
    kept = []
    for j in range(n):
        piv = G[j, j] - sum(L[j, c] ** 2 for c in kept)
        if G[j, j] == 0.0 or piv <= 1e-10 * G[j, j]:
            continue
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
    return theta


def hmc_date(r: np.ndarray, w, x0: float, rate: float, Ts, Ms, degree: int = 3, kind: str = "otm"):
    """r (k, L) float32 log-returns, w (k,) or None.  Returns dict of (nT, nM) price / iv / strike and (nT,) sigma, or
    all-NaN results and a non-zero status for bad inputs."""
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
    for q, T in enumerate(Ts):
        tau = T / 252.0
        sig = math.sqrt(sum(ww[i] * (252.0 / T) * float(np.sum(rr[i, :T] ** 2)) for i in range(m)))
        out["sigma"][q] = sig
        for j, M in enumerate(Ms):
            K = x0 * math.exp(rate * tau) * math.exp(M * sig * math.sqrt(tau))
            call = kind == "call" or (kind == "otm" and M >= 0)
            V = np.maximum(S[:, T] - K, 0.0) if call else np.maximum(K - S[:, T], 0.0)
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
                theta = cholesky_solve(G, h)
                V = psi @ theta[:degree + 1]
            out["price"][q, j] = V[0]
            out["strike"][q, j] = K
            out["iv"][q, j] = implied_vol(V[0], x0, K, tau, rate, call)
    return dict(out, status=0)
