"""An independent float64 restatement of the hedge report (README "Option pricing": the policy and its replay), written
from the definition and not from shadowing_amd/pricing.py: plain loops over maturities, strikes, steps and paths.  The
fit is the one of tests/_hmc_reference.py (explicit features, two-pass mean / std, its small Cholesky) with the
coefficients kept; the replay walks one path at a time.  Also the CRR delta of tests on full binomial trees."""
from __future__ import annotations

import math

import numpy as np

import _hmc_reference as ref


def fit_policy(r: np.ndarray, w, x0: float, rate: float, Ts, Ms, degree: int = 3, kind: str = "otm"):
    """r (k, L) float32 log-returns, w (k,) or None (valid inputs only).  Returns (policy (nT, nM, max Ts, 2 degree + 4),
    price (nT, nM), strike (nT, nM)); a flagged maturity has a NaN price."""
    k = r.shape[0]
    nT, nM, P = len(Ts), len(Ms), degree
    w = np.ones(k) if w is None else np.asarray(w, dtype=np.float64)
    w = w / w.sum()
    idx = [i for i in range(k) if w[i] != 0]
    rr, ww, m = r[idx].astype(np.float64), w[idx], len(idx)
    S = np.empty((m, max(Ts) + 1))
    S[:, 0] = x0
    for i in range(m):
        acc = 0.0
        for t in range(max(Ts)):
            acc += rr[i, t]
            S[i, t + 1] = x0 * math.exp(acc)
    rho = rate / 252.0
    policy = np.zeros((nT, nM, max(Ts), 2 * P + 4))
    price, strike = np.empty((nT, nM)), np.empty((nT, nM))
    for q, T in enumerate(Ts):
        tau = T / 252.0
        sig = math.sqrt(sum(ww[i] * (252.0 / T) * float(np.sum(rr[i, :T] ** 2)) for i in range(m)))
        for j, M in enumerate(Ms):
            K = x0 * math.exp(rate * tau) * math.exp(M * sig * math.sqrt(tau))
            call = kind == "call" or (kind == "otm" and M >= 0)
            V = np.maximum(S[:, T] - K, 0.0) if call else np.maximum(K - S[:, T], 0.0)
            ill = False
            for n in range(T - 1, -1, -1):
                y = math.exp(-rho) * V
                D = math.exp(-rho) * S[:, n + 1] - S[:, n]
                if np.all(S[:, n] == S[0, n]):
                    mean, isd = x0, 0.0
                else:
                    mean = float(np.sum(ww * S[:, n]))
                    isd = 1.0 / math.sqrt(float(np.sum(ww * (S[:, n] - mean) ** 2)))
                u = (S[:, n] - mean) * isd
                psi = np.stack([u ** a for a in range(P + 1)], axis=1)
                f = np.concatenate([psi, psi * D[:, None]], axis=1)
                theta, ill_n = ref.cholesky_solve((f * ww[:, None]).T @ f, (f * ww[:, None]).T @ y, n == 0)
                ill = ill or ill_n
                policy[q, j, n, 0], policy[q, j, n, 1], policy[q, j, n, 2:] = mean, isd, theta
                V = psi @ theta[:P + 1]
            strike[q, j] = K
            price[q, j] = math.nan if ill else V[0]
    return policy, price, strike


def replay(r: np.ndarray, w, x0: float, rate: float, Ts, Ms, degree: int, kind: str, policy: np.ndarray,
           strike: np.ndarray, centre: np.ndarray):
    """The replay of one date's policy on r (k', L) with weights w (k',) or None, path by path.  Returns (sums
    (nT, nM, 9), pnl (nT, nM, k'), status)."""
    k = r.shape[0]
    nT, nM, P = len(Ts), len(Ms), degree
    sums, pnl = np.full((nT, nM, 9), math.nan), np.full((nT, nM, k), math.nan)
    w = np.ones(k) if w is None else np.asarray(w, dtype=np.float64)
    status = 0
    if not np.all(np.isfinite(w)) or not w.sum() > 0:
        status |= 2
    for i in range(k):
        if w[i] != 0 and not np.all(np.isfinite(r[i, :max(Ts)])):
            status |= 1
    if status:
        return sums, pnl, status
    w = w / w.sum()
    rho = rate / 252.0
    for q, T in enumerate(Ts):
        for j, M in enumerate(Ms):
            c = centre[q, j]
            if not math.isfinite(c):
                continue
            call = kind == "call" or (kind == "otm" and M >= 0)
            acc = [0.0] * 9
            for i in range(k):
                if w[i] == 0:
                    continue
                l, S, gain = 0.0, x0, 0.0
                for n in range(T):
                    l += float(r[i, n])
                    S1 = x0 * math.exp(l)
                    row = policy[q, j, n]
                    u = (S - row[0]) * row[1]
                    phi = sum(row[2 + P + 1 + a] * u ** a for a in range(P + 1))
                    gain += math.exp(-rho * n) * phi * (math.exp(-rho) * S1 - S)
                    S = S1
                pay = math.exp(-rho * T) * (max(S - strike[q, j], 0.0) if call else max(strike[q, j] - S, 0.0))
                pnl[q, j, i] = pay - gain
                dp, dq = pay - gain - c, pay - c
                for z, v in enumerate((w[i] * dp, w[i] * dp * dp, w[i] ** 2 * dp, w[i] ** 2 * dp * dp, w[i] * dq,
                                       w[i] * dq * dq, w[i] ** 2 * dq, w[i] ** 2 * dq * dq, w[i] ** 2)):
                    acc[z] += v
            sums[q, j] = acc
    return sums, pnl, status


def results(sums: np.ndarray, centre: np.ndarray) -> dict:
    a1, a2, b1, b2, p1, p2, q1, q2, s2 = (sums[..., z] for z in range(9))
    pos = lambda v: np.sqrt(np.where(v > 0, v, np.where(np.isnan(v), np.nan, 0.0)))   # noqa: E731
    return {"mean": centre + a1, "mc": centre + p1, "risk": pos(a2 - a1 ** 2), "risk_unhedged": pos(p2 - p1 ** 2),
            "se": pos(b2 - 2 * a1 * b1 + a1 ** 2 * s2), "se_unhedged": pos(q2 - 2 * p1 * q1 + p1 ** 2 * s2), "n_eff": 1 / s2}


def crr_delta(x0: float, K: float, a: float, rate: float, T: int, call: bool) -> float:
    """(V_u - V_d) / (S_u - S_d), V_u and V_d the CRR prices of the two children of the root (T - 1 steps left)."""
    up, dn = x0 * math.exp(a), x0 * math.exp(-a)
    if T == 1:
        pay = (lambda s: max(s - K, 0.0)) if call else (lambda s: max(K - s, 0.0))
        return (pay(up) - pay(dn)) / (up - dn)
    return (ref.crr_price(up, K, a, rate, T - 1, call) - ref.crr_price(dn, K, a, rate, T - 1, call)) / (up - dn)


def mrw_like_returns(seed: int, B: int, k: int, L: int, sigma: float = 0.2):
    """(B, k, L) float32 returns with a spread of vols (a real smile) and (B, k) softmax-like weights with some zeros."""
    g = np.random.default_rng(seed)
    sig = sigma * (0.5 + g.random((B, k, 1)))
    r = (sig * math.sqrt(1 / 252) * g.standard_normal((B, k, L)) - 0.5 * sig ** 2 / 252).astype(np.float32)
    d = g.random((B, k))
    w = np.exp(-(d - d.min(axis=1, keepdims=True)) / 0.3)
    w[g.random((B, k)) < 0.1] = 0.0
    w[:, 0] = 1.0                                            # (never all zero)
    return r, w
