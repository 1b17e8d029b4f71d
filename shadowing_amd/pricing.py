"""Option pricing on shadowing paths: hedged Monte Carlo (Potters, Bouchaud, Sestovic 2001) and the implied-volatility
smile, the second use of Path Shadowing Monte Carlo that the reference README names ("Option pricing").

In the reference, `PriceData` and `compute_smile` come from the un-vendored dependency `scatspectra`.  The definitions
below are this project's own (PARITY UNPINNED, as for the averaging stand-ins of averaging.py): the method is written out
in the header of shadowing_amd/csrc/psh_hmc.hip and in README "Option pricing".  `compute_smile(..., cuda=True)` runs it
as one launch of psh_hedged_mc; `cuda=False` is the numpy float64 twin below, which follows the kernel operation for
operation except for the order of its sums.

The hedge of a smile (`report=True`, `hedge_pnl`): the fit's POLICY -- for every step n < T of a (date, maturity, strike)
the row [mu_n, isd_n, gamma_n[0..P], beta_n[0..P]], dropped unknowns 0, rows n >= T zero, `coef[b][q][j][n][c]` with
n < max Ts and c < 2P + 4 -- and its REPLAY on k' paths r' with weights w' (normalised by their sum), in double,
rho = rate / 252:
    l_0 = 0, l_{n+1} = l_n + r'[i, n]          S_n = x_init exp(l_n), S_0 = x_init exactly
    u_n = (S_n - mu_n) isd_n                    phi_n = Horner of beta_n in u_n, top coefficient first
    D_n = e^-rho S_{n+1} - S_n                  gain_i = sum_{n<T} exp(-rho n) phi_n D_n
    pay_i = exp(-rho T) payoff_j(S_T)           (K_j and call / put are the fit's)
    pnl_i = pay_i - gain_i
With the centre c = the fit's price V_0, nine sums per (b, q, j):
    a1 = sum w (pnl - c)   a2 = sum w (pnl - c)^2   b1 = sum w^2 (pnl - c)   b2 = sum w^2 (pnl - c)^2
    p1, p2, q1, q2: the same four of pay         s2 = sum w^2
    mean = c + a1          risk = sqrt(max(a2 - a1^2, 0))          se = sqrt(max(b2 - 2 a1 b1 + a1^2 s2, 0))
    mc   = c + p1          risk_unhedged, se_unhedged likewise      n_eff = 1 / s2
delta = beta_0[0], the hedge ratio at inception.  `se` treats the policy as fixed: it is honest on paths the policy was
not fitted on and optimistic in-sample.  A path of weight 0 contributes nothing and its pnl is NaN; bad inputs make the
date's results NaN (the status bits of the fit); a maturity the fit flagged gives NaN.  The full statement heads
shadowing_amd/csrc/psh_hmc_report.hip; psh_hedged_mc_policy and psh_hedge_replay run it on the device, `replay_host`
below is the numpy twin.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields

import numpy as np
import torch

KINDS = {"otm": 0, "call": 1, "put": 2}
STATUS_OK, STATUS_NONFINITE, STATUS_WEIGHTS, STATUS_ILL_CONDITIONED = 0, 1, 2, 4
MAX_DEGREE = 5
TAU_ILL = 0.2          # beta_0 kept at a step n > 0 with a pivot below TAU_ILL * its diagonal: ill-conditioned
TAU_SING = 1e-6       # any unknown kept with a pivot below TAU_SING * its diagonal: ill-conditioned


class PriceData:
    """Prices from log-returns, log-prices or prices (our convention):
      dlnx given: x = x_init * exp([0, cumsum(dlnx)]) along the last axis (length T + 1; x_init defaults to 1);
      lnx given:  x = x_init * exp(lnx - lnx[..., :1]), or exp(lnx) without x_init;
      x given:    x as is, or rescaled to start at x_init.
    `.x`, `.lnx`, `.dx`, `.dlnx` are numpy float64 arrays."""

    def __init__(self, dlnx=None, lnx=None, x=None, x_init: float | None = None):
        if sum(v is not None for v in (dlnx, lnx, x)) != 1:
            raise ValueError("PriceData takes exactly one of dlnx, lnx, x")
        if dlnx is not None:
            d = _as_numpy(dlnx)
            zero = np.zeros(d.shape[:-1] + (1,))
            self._x = (1.0 if x_init is None else float(x_init)) * np.exp(np.concatenate([zero, np.cumsum(d, axis=-1)], -1))
        elif lnx is not None:
            ln = _as_numpy(lnx)
            self._x = np.exp(ln) if x_init is None else float(x_init) * np.exp(ln - ln[..., :1])
        else:
            xx = _as_numpy(x)
            self._x = xx if x_init is None else float(x_init) * xx / xx[..., :1]

    @property
    def x(self) -> np.ndarray:
        return self._x

    @property
    def lnx(self) -> np.ndarray:
        return np.log(self._x)

    @property
    def dx(self) -> np.ndarray:
        return np.diff(self._x, axis=-1)

    @property
    def dlnx(self) -> np.ndarray:
        return np.diff(np.log(self._x), axis=-1)


def _as_numpy(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


@dataclass
class Smile:
    """Hedged Monte Carlo prices and Black-Scholes implied vols: `prices`, `ivs`, `strikes` (B, nT, nM) -- (nT, nM) when
    compute_smile got a single date -- `sigma` (B, nT) the scale of the strikes, `status` (B,) PSH_HMC_STATUS_* bits."""
    prices: np.ndarray
    ivs: np.ndarray
    strikes: np.ndarray
    sigma: np.ndarray
    Ts: np.ndarray
    Ms: np.ndarray
    kind: str
    status: np.ndarray
    x_init: float = 100.0
    r: float = 0.0
    # report=True (None otherwise): the hedge of the smile on the fit's own paths, shaped as `prices` -- `delta` the hedge
    # ratio at inception, `price_mc` the unhedged Monte Carlo price, `risk` / `risk_unhedged` the weighted standard
    # deviation of the hedged / unhedged discounted P&L, `price_se` / `price_se_unhedged` the standard errors of `prices`
    # / `price_mc` (in-sample: the policy is taken as fixed, so `price_se` is optimistic), `iv_se` = price_se over the
    # Black-Scholes vega at `ivs`, `n_eff` = 1 / sum w^2, and `policy`, the HedgePolicy that hedge_pnl() replays.
    delta: np.ndarray | None = None
    price_mc: np.ndarray | None = None
    risk: np.ndarray | None = None
    risk_unhedged: np.ndarray | None = None
    price_se: np.ndarray | None = None
    price_se_unhedged: np.ndarray | None = None
    iv_se: np.ndarray | None = None
    n_eff: np.ndarray | None = None
    policy: "HedgePolicy | None" = None
    # calibrate_to=MarketQuotes (None otherwise): the calibration.Calibration whose weights the smile was priced under
    calibration: object = None

    def plot(self, ax=None, rescale: bool = True, legend: bool = True, color=None, errorbars: bool = False, **kw):
        """Implied vol against M (rescale=True) or against log(K / F), F the forward (rescale=False): one line per
        maturity, of the first date when there are several.  errorbars=True draws +- `iv_se` (a report=True smile)."""
        import matplotlib.pyplot as plt
        if ax is None:
            ax = plt.gca()
        ivs = self.ivs if self.ivs.ndim == 2 else self.ivs[0]
        strikes = self.strikes if self.strikes.ndim == 2 else self.strikes[0]
        if errorbars and self.iv_se is None:
            raise ValueError("errorbars=True needs a smile computed with report=True")
        for q, T in enumerate(self.Ts):
            fwd = self.x_init * math.exp(self.r * T / 252.0)
            xs = self.Ms if rescale else np.log(strikes[q] / fwd)
            if errorbars:
                se = self.iv_se if self.iv_se.ndim == 2 else self.iv_se[0]
                ax.errorbar(xs, ivs[q], yerr=se[q], color=color, label=f"T={int(T)}", marker="o", capsize=3, **kw)
                continue
            ax.plot(xs, ivs[q], color=color, label=f"T={int(T)}", marker="o", **kw)
        ax.set_xlabel("M (rescaled log-moneyness)" if rescale else "log(K / F)")
        ax.set_ylabel("implied vol")
        if legend:
            ax.legend()
        return ax


@dataclass
class HedgePolicy:
    """The policy of a fit: `coef` (B, nT, nM, max Ts, 2 degree + 4) float64, numpy or a HIP tensor, rows
    [mu_n, isd_n, gamma_n[0..P], beta_n[0..P]] (module docstring); `strikes` and `prices` (B, nT, nM) the fit's (numpy);
    `status` (B,) the fit's.  Always batched: a single date is B = 1."""
    coef: object
    strikes: np.ndarray
    prices: np.ndarray
    Ts: np.ndarray
    Ms: np.ndarray
    kind: str
    degree: int
    x_init: float
    r: float
    status: np.ndarray


@dataclass
class HedgedPnL:
    """The replay of a policy: per (B, nT, nM) -- (nT, nM) for one set of paths -- `mean` of the hedged discounted P&L,
    `mc` of the unhedged payoff, their weighted standard deviations `risk` / `risk_unhedged`, the standard errors `se` /
    `se_unhedged` of `mean` / `mc` (the policy taken as fixed), `n_eff` = 1 / sum w^2, the nine `sums` (..., 9) of the
    module docstring, `status` (B,), and `pnl` (..., k') per path (numpy; NaN for a path of weight 0) when asked for."""
    mean: np.ndarray
    mc: np.ndarray
    risk: np.ndarray
    risk_unhedged: np.ndarray
    se: np.ndarray
    se_unhedged: np.ndarray
    n_eff: np.ndarray
    sums: np.ndarray
    status: np.ndarray
    pnl: np.ndarray | None = None


def report_from_sums(sums: np.ndarray, centre: np.ndarray) -> dict:
    """The results of the nine sums (..., 9) about the centre (...): what the device and the host path both report."""
    a1, a2, b1, b2, p1, p2, q1, q2, s2 = np.moveaxis(np.asarray(sums, dtype=np.float64), -1, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"mean": centre + a1, "mc": centre + p1,
                "risk": np.sqrt(np.maximum(a2 - a1 * a1, 0.0)), "risk_unhedged": np.sqrt(np.maximum(p2 - p1 * p1, 0.0)),
                "se": np.sqrt(np.maximum(b2 - 2.0 * a1 * b1 + a1 * a1 * s2, 0.0)),
                "se_unhedged": np.sqrt(np.maximum(q2 - 2.0 * p1 * q1 + p1 * p1 * s2, 0.0)), "n_eff": 1.0 / s2}


def bs_vega(x0: float, K, tau, rate: float, sig):
    """Black-Scholes vega x0 pdf(d1) sqrt(tau), elementwise (NaN where sig is NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d1 = (np.log(x0 / K) + (rate + 0.5 * sig * sig) * tau) / (sig * np.sqrt(tau))
        return x0 * np.exp(-0.5 * d1 * d1) / math.sqrt(2.0 * math.pi) * np.sqrt(tau)


# ---- Black-Scholes and its inversion (the kernel's implied_vol, operation for operation)
def _norm_cdf(x: float) -> float:
    return 0.5 * math.erfc(-x * 0.70710678118654752440)


def bs_price(x0: float, K: float, tau: float, rate: float, sig: float, call: bool) -> float:
    sd = sig * math.sqrt(tau)
    d1 = (math.log(x0 / K) + (rate + 0.5 * sig * sig) * tau) / sd
    d2 = d1 - sd
    df = math.exp(-rate * tau)
    return x0 * _norm_cdf(d1) - K * df * _norm_cdf(d2) if call else K * df * _norm_cdf(-d2) - x0 * _norm_cdf(-d1)


def implied_vol(price: float, x0: float, K: float, tau: float, rate: float, call: bool) -> float:
    """100 bisection halvings on [1e-4, 5]; NaN when the price is outside [BS(1e-4), BS(5)] (no root in the bracket)."""
    lo, hi = 1e-4, 5.0
    if not (bs_price(x0, K, tau, rate, lo, call) <= price <= bs_price(x0, K, tau, rate, hi, call)):
        return math.nan
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        if bs_price(x0, K, tau, rate, mid, call) < price:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _solve_dropping(G: np.ndarray, H: np.ndarray, first_step: bool) -> tuple[np.ndarray, bool]:
    """(theta (NF, nM), ill) of G theta = H by Cholesky in the fixed order of the unknowns; an unknown whose pivot is
    <= 1e-10 times its diagonal (or whose diagonal is 0) is dropped: theta = 0, its row and column removed.  ill: an
    unknown is kept with a pivot below TAU_SING times its diagonal, or (not at the first step, n = 0) beta_0 (unknown
    NF / 2) is kept with a pivot below TAU_ILL times its diagonal."""
    nf = G.shape[0]
    L = np.zeros_like(G)
    ill = False
    for j in range(nf):
        d = G[j, j]
        for c in range(j):
            d -= L[j, c] * L[j, c]
        if not (G[j, j] > 0.0 and d > 1e-10 * G[j, j]):
            continue                                          # dropped: column j of L stays 0
        if d < TAU_SING * G[j, j] or (j == nf // 2 and not first_step and d < TAU_ILL * G[j, j]):
            ill = True
        ljj = math.sqrt(d)
        L[j, j] = ljj
        for i in range(j + 1, nf):
            s = G[i, j]
            for c in range(j):
                s -= L[i, c] * L[j, c]
            L[i, j] = s / ljj
    z = np.zeros_like(H)
    for j in range(nf):
        hj = H[j].copy()
        for c in range(j):
            hj -= L[j, c] * z[c]
        z[j] = hj / L[j, j] if L[j, j] > 0.0 else 0.0
    for j in range(nf - 1, -1, -1):
        t = z[j].copy()
        for c in range(j + 1, nf):
            t -= L[c, j] * z[c]
        z[j] = t / L[j, j] if L[j, j] > 0.0 else 0.0
    return z, ill


def _hmc_date(r: np.ndarray, w: np.ndarray | None, x0: float, rate: float, Ts, Ms, degree: int, kind: int,
              keep_policy: bool = False):
    """One date on the host: r (k, L) float32 log-returns, w (k,) raw weights or None.  Returns (price, iv, strike
    (nT, nM), sigma (nT,), status), and with keep_policy the policy (nT, nM, max Ts, 2 degree + 4) as a sixth."""
    nT, nM = len(Ts), len(Ms)
    policy = np.zeros((nT, nM, max(Ts), 2 * degree + 4)) if keep_policy else None
    price, iv, strike = (np.full((nT, nM), np.nan) for _ in range(3))
    sigma_out = np.full(nT, np.nan)
    k = r.shape[0]
    wr = np.ones(k) if w is None else np.asarray(w, dtype=np.float64)
    status = 0
    if not np.isfinite(wr).all():
        status |= STATUS_WEIGHTS
    wsum = float(wr.sum())
    if not (wsum > 0.0 and math.isfinite(wsum)):
        status |= STATUS_WEIGHTS
    live = wr != 0.0
    Tmax = max(Ts)
    if not np.isfinite(r[live, :Tmax]).all():
        status |= STATUS_NONFINITE
    if status:
        return (price, iv, strike, sigma_out, status) + ((policy,) if keep_policy else ())
    invw = 1.0 / wsum
    wl = wr[live] * invw
    rl = r[live].astype(np.float64)
    lnS = np.concatenate([np.zeros((rl.shape[0], 1)), np.cumsum(rl, axis=1)], axis=1)
    P = degree
    NB, NMOM = P + 1, 2 * P + 1
    disc = math.exp(-(rate / 252.0))
    Ms = np.asarray(Ms, dtype=np.float64)
    for q, T in enumerate(Ts):
        tau = T / 252.0
        sigma = math.sqrt((252.0 / T) * (float(wr[live] @ (rl[:, :T] ** 2).sum(axis=1)) * invw))
        sigma_out[q] = sigma
        fwd = x0 * math.exp(rate * tau)
        K = fwd * np.exp(Ms * sigma * math.sqrt(tau))
        call = np.full(nM, kind == KINDS["call"]) | ((kind == KINDS["otm"]) & (Ms >= 0.0))
        S = x0 * np.exp(lnS[:, :T + 1])
        S[:, 0] = x0
        S1 = S[:, T]
        V = np.where(call[None, :], np.maximum(S1[:, None] - K[None, :], 0.0), np.maximum(K[None, :] - S1[:, None], 0.0))
        gamma, ill = None, False
        for n in range(T - 1, -1, -1):
            S0, S1 = S[:, n], S[:, n + 1]
            mu, isd = x0, 0.0
            if n > 0:
                d = S0 - x0
                m1, m2 = float(wl @ d), float(wl @ (d * d))
                mn, mx = S0.min(), S0.max()
                if mn != mx:
                    var = m2 - m1 * m1
                    mu = x0 + m1
                    isd = 1.0 / (math.sqrt(var) if var > 0.0 else mx - mn)
            u0 = (S0 - mu) * isd
            D = disc * S1 - S0
            pw = np.empty((u0.shape[0], NMOM))
            pw[:, 0] = 1.0
            for m in range(1, NMOM):
                pw[:, m] = pw[:, m - 1] * u0
            wd = wl * D
            mom = np.stack([wl @ pw, wd @ pw, (wd * D) @ pw])          # (3, NMOM)
            y = disc * V
            H = np.concatenate([pw[:, :NB].T @ (wl[:, None] * y), pw[:, :NB].T @ (wd[:, None] * y)])   # (2 NB, nM)
            a = np.arange(NB)
            G = np.block([[mom[0][a[:, None] + a[None, :]], mom[1][a[:, None] + a[None, :]]],
                          [mom[1][a[:, None] + a[None, :]], mom[2][a[:, None] + a[None, :]]]])
            theta, ill_n = _solve_dropping(G, H, n == 0)
            gamma, ill = theta[:NB], ill or ill_n                     # gamma (NB, nM)
            if keep_policy:
                policy[q, :, n, 0], policy[q, :, n, 1], policy[q, :, n, 2:] = mu, isd, theta.T
            V = np.broadcast_to(gamma[P], (u0.shape[0], nM)).copy()
            for c in range(P - 1, -1, -1):
                V = V * u0[:, None] + gamma[c]
        strike[q] = K
        if ill:                                                         # price and iv stay NaN
            status |= STATUS_ILL_CONDITIONED
            continue
        price[q] = gamma[0]
        iv[q] = [implied_vol(float(price[q, j]), x0, float(K[j]), tau, rate, bool(call[j])) for j in range(nM)]
    return (price, iv, strike, sigma_out, status) + ((policy,) if keep_policy else ())


def hedged_mc_host(dlnx: np.ndarray, weights: np.ndarray | None, Ts, Ms, x_init: float = 100.0, rate: float = 0.0,
                   degree: int = 3, kind: int = 0, policy: bool = False) -> dict:
    """The numpy float64 twin of psh_hedged_mc: dlnx (B, k, L) float32, weights (B, k) or None; any k.  policy=True: of
    psh_hedged_mc_policy, with "policy" (B, nT, nM, max Ts, 2 degree + 4)."""
    B = dlnx.shape[0]
    res = [_hmc_date(dlnx[b], None if weights is None else weights[b], x_init, rate, Ts, Ms, degree, kind, policy)
           for b in range(B)]
    out = {"price": np.stack([x[0] for x in res]), "iv": np.stack([x[1] for x in res]),
           "strike": np.stack([x[2] for x in res]), "sigma": np.stack([x[3] for x in res]),
           "status": np.array([x[4] for x in res], dtype=np.int32)}
    if policy:
        out["policy"] = np.stack([x[5] for x in res])
    return out


def replay_host(dlnx: np.ndarray, weights: np.ndarray | None, Ts, Ms, policy: np.ndarray, strike: np.ndarray,
                centre: np.ndarray, x_init: float = 100.0, rate: float = 0.0, degree: int = 3, kind: int = 0,
                return_pnl: bool = False) -> dict:
    """The numpy float64 twin of psh_hedge_replay (the module docstring's replay): dlnx (B, k', L) float32, weights
    (B, k') or None, policy (B, nT, nM, max Ts, 2 degree + 4), strike and centre (B, nT, nM) the fit's.  Returns "sums"
    (B, nT, nM, 9), "status" (B,) and, when asked for, "pnl" (B, nT, nM, k')."""
    B, k = dlnx.shape[0], dlnx.shape[1]
    nT, nM, P = len(Ts), len(Ms), degree
    Tmax = max(Ts)
    sums = np.full((B, nT, nM, 9), np.nan)
    pnl_out = np.full((B, nT, nM, k), np.nan) if return_pnl else None
    status = np.zeros(B, dtype=np.int32)
    rho = rate / 252.0
    disc = math.exp(-rho)
    Ms = np.asarray(Ms, dtype=np.float64)
    call = np.full(nM, kind == KINDS["call"]) | ((kind == KINDS["otm"]) & (Ms >= 0.0))
    for b in range(B):
        wr = np.ones(k) if weights is None else np.asarray(weights[b], dtype=np.float64)
        st = 0
        if not np.isfinite(wr).all():
            st |= STATUS_WEIGHTS
        wsum = float(wr.sum())
        if not (wsum > 0.0 and math.isfinite(wsum)):
            st |= STATUS_WEIGHTS
        live = wr != 0.0
        if not np.isfinite(dlnx[b][live, :Tmax]).all():
            st |= STATUS_NONFINITE
        status[b] = st
        if st:
            continue
        wl = wr[live] * (1.0 / wsum)
        wl2 = wl * wl
        rl = dlnx[b][live].astype(np.float64)
        lnS = np.concatenate([np.zeros((rl.shape[0], 1)), np.cumsum(rl, axis=1)], axis=1)
        for q, T in enumerate(Ts):
            S = x_init * np.exp(lnS[:, :T + 1])
            S[:, 0] = x_init
            gain = np.zeros((rl.shape[0], nM))
            for n in range(T):
                row = policy[b, q, :, n, :]                               # (nM, 2P + 4)
                u = (S[:, n, None] - row[None, :, 0]) * row[None, :, 1]
                phi = np.broadcast_to(row[:, 2 + P + 1 + P], u.shape).copy()
                for c in range(P - 1, -1, -1):
                    phi = phi * u + row[None, :, 2 + P + 1 + c]
                gain += phi * (math.exp(-rho * n) * (disc * S[:, n + 1] - S[:, n]))[:, None]
            ST, K = S[:, T, None], strike[b, q][None, :]
            pay = math.exp(-rho * T) * np.where(call[None, :], np.maximum(ST - K, 0.0), np.maximum(K - ST, 0.0))
            pnl = pay - gain
            c = centre[b, q]
            flagged = ~np.isfinite(c)
            dp, dq = pnl - c[None, :], pay - c[None, :]
            res = np.stack([wl @ dp, wl @ (dp * dp), wl2 @ dp, wl2 @ (dp * dp), wl @ dq, wl @ (dq * dq), wl2 @ dq,
                            wl2 @ (dq * dq), np.full(nM, float(wl2.sum()))], axis=-1)
            res[flagged] = np.nan
            sums[b, q] = res
            if return_pnl:
                pnl_out[b, q][:, live] = np.where(flagged[:, None], np.nan, pnl.T)
    out = {"sums": sums, "status": status}
    if return_pnl:
        out["pnl"] = pnl_out
    return out


def _check_args(Ts, Ms, L: int, degree: int, kind: str):
    Ts = [int(T) for T in np.atleast_1d(Ts)]
    Ms = [float(M) for M in np.atleast_1d(Ms)]
    if not Ts or not Ms:
        raise ValueError("Ts and Ms must not be empty")
    if min(Ts) < 1 or max(Ts) > L:
        raise ValueError(f"maturities must lie in [1, {L}] samples, got {Ts}")
    if not all(math.isfinite(M) for M in Ms):
        raise ValueError("Ms must be finite")
    if not 1 <= int(degree) <= MAX_DEGREE:
        raise ValueError(f"degree must be in 1..{MAX_DEGREE}, got {degree}")
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    return Ts, Ms


def _replay(x, w, Ts, Ms, coef, strike, centre, x_init, r, degree, kind, return_pnl, cuda):
    """psh_hedge_replay (cuda) or replay_host on (B, k', L) float32 log-returns x; strike / centre numpy (B, nT, nM).
    Returns a dict of numpy arrays."""
    if cuda:
        from . import _native
        dev = x.device
        up = lambda a: a.to(dev) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
        out = _native.hedge_replay(x, w, Ts, Ms, up(coef).contiguous(), up(strike), up(centre), x_init, r, degree,
                                   KINDS[kind], return_pnl)
        return {name: t.cpu().numpy() for name, t in out.items()}
    coef = coef.detach().cpu().numpy() if isinstance(coef, torch.Tensor) else np.asarray(coef)
    return replay_host(x, w, Ts, Ms, coef, strike, centre, x_init, r, degree, KINDS[kind], return_pnl)


def _returns_and_weights(dlnx, weights, cuda: bool):
    """The (B, k, L) float32 log-returns and (B, k) float64 weights (or None) where the pricing runs: HIP tensors for
    cuda=True, numpy otherwise."""
    if cuda:
        x = dlnx if isinstance(dlnx, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dlnx, dtype=np.float32))
        dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
        x = x.to(dev, torch.float32)
        w = None
        if weights is not None:
            w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64))
            w = w.to(dev, torch.float64).contiguous()
        return x, w
    x = dlnx.detach().cpu().numpy() if isinstance(dlnx, torch.Tensor) else np.asarray(dlnx)
    w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else weights
    return x.astype(np.float32, copy=False), None if w is None else np.asarray(w, dtype=np.float64)


def smile_from_log_returns(dlnx, weights, Ts, Ms, x_init: float = 100.0, r: float = 0.0, *, degree: int = 3,
                           kind: str = "otm", cuda: bool = False, report: bool = False) -> Smile:
    """The hedged Monte Carlo smile of (B, k, L) float32 log-returns (numpy, or a HIP tensor -- any row stride, e.g. the
    out-context view of gathered paths) with (B, k) weights or None.  cuda=True: one psh_hedged_mc launch (k <= PSH_MAX_K,
    nT, nM <= 64); cuda=False: the numpy twin.  report=True: the fit keeps its policy (psh_hedged_mc_policy) and replays
    it on its own paths (psh_hedge_replay): the Smile's report fields; on the device the paths and the policy stay there."""
    L = dlnx.shape[-1]
    Ts, Ms = _check_args(Ts, Ms, L, degree, kind)
    x, w = _returns_and_weights(dlnx, weights, cuda)
    if cuda:
        from . import _native
        out = _native.hedged_mc(x, w, Ts, Ms, x_init, r, degree, KINDS[kind], policy=report)
        host = {name: t.cpu().numpy() for name, t in out.items() if name != "policy"}
    else:
        out = host = hedged_mc_host(x, w, Ts, Ms, x_init, r, degree, KINDS[kind], policy=report)
    sm = Smile(host["price"], host["iv"], host["strike"], host["sigma"], np.asarray(Ts), np.asarray(Ms), kind,
               host["status"], float(x_init), float(r))
    if report:
        rep = _replay(x, w, Ts, Ms, out["policy"], host["strike"], host["price"], x_init, r, degree, kind, False, cuda)
        res = report_from_sums(rep["sums"], sm.prices)
        coef = out["policy"]
        with np.errstate(invalid="ignore", divide="ignore"):
            beta00 = (coef[:, :, :, 0, degree + 3].cpu().numpy() if isinstance(coef, torch.Tensor) else coef[:, :, :, 0, degree + 3])
            sm.delta = np.where(np.isfinite(sm.prices), beta00, np.nan)
            tau = (np.asarray(Ts, dtype=np.float64) / 252.0)[None, :, None]
            sm.iv_se = res["se"] / bs_vega(float(x_init), sm.strikes, tau, float(r), sm.ivs)
        sm.price_mc, sm.risk, sm.risk_unhedged = res["mc"], res["risk"], res["risk_unhedged"]
        sm.price_se, sm.price_se_unhedged, sm.n_eff = res["se"], res["se_unhedged"], res["n_eff"]
        sm.policy = HedgePolicy(coef, sm.strikes, sm.prices, sm.Ts, sm.Ms, kind, int(degree), float(x_init), float(r), sm.status)
    return sm


REPORT_FIELDS = ("delta", "price_mc", "risk", "risk_unhedged", "price_se", "price_se_unhedged", "iv_se", "n_eff")


def concat_smiles(parts: list) -> Smile:
    """One Smile of several batches of dates (the same Ts, Ms, kind, x_init, r), report fields and policy included."""
    cat = lambda name: np.concatenate([getattr(p, name) for p in parts])   # noqa: E731
    p0 = parts[0]
    sm = Smile(cat("prices"), cat("ivs"), cat("strikes"), cat("sigma"), p0.Ts, p0.Ms, p0.kind, cat("status"), p0.x_init, p0.r)
    if p0.policy is not None:
        for name in REPORT_FIELDS:
            setattr(sm, name, cat(name))
        coefs = [p.policy.coef for p in parts]
        coef = torch.cat(coefs) if isinstance(coefs[0], torch.Tensor) else np.concatenate(coefs)
        sm.policy = HedgePolicy(coef, sm.strikes, sm.prices, sm.Ts, sm.Ms, p0.kind, p0.policy.degree, p0.x_init, p0.r, sm.status)
    if p0.calibration is not None:
        from .calibration import concat_calibrations
        sm.calibration = concat_calibrations([p.calibration for p in parts])
    return sm


def _paths_to_returns(x, cuda: bool | None):
    """(dlnx (B, k, N) float32 -- a torch tensor when cuda, numpy otherwise -- x_init, single, cuda) of price paths
    x (k, N+1) or (B, k, N+1) that all start at the same price."""
    single = x.dim() == 2 if isinstance(x, torch.Tensor) else np.ndim(x) == 2
    if cuda is None:
        cuda = isinstance(x, torch.Tensor) and x.is_cuda
    if isinstance(x, torch.Tensor):
        xt = x[None] if single else x
        if xt.dim() != 3:
            raise ValueError("x must be (k, N+1) or (B, k, N+1)")
        x0t = xt[..., 0]
        if not bool((x0t == x0t.reshape(-1)[0]).all()):
            raise ValueError("every path must start at the same price x[..., 0]")
        x_init = float(x0t.reshape(-1)[0])
        dlnx = torch.diff(torch.log(xt.to(torch.float64)), dim=-1).to(torch.float32)
        if not cuda:
            dlnx = dlnx.cpu().numpy()
    else:
        xn = np.asarray(x, dtype=np.float64)
        xn = xn[None] if single else xn
        if xn.ndim != 3:
            raise ValueError("x must be (k, N+1) or (B, k, N+1)")
        if not (xn[..., 0] == xn.reshape(-1)[0]).all():
            raise ValueError("every path must start at the same price x[..., 0]")
        x_init = float(xn.reshape(-1)[0])
        dlnx = np.diff(np.log(xn), axis=-1).astype(np.float32)
    if not (x_init > 0.0 and math.isfinite(x_init)):
        raise ValueError(f"the spot x[..., 0] must be positive and finite, got {x_init}")
    return dlnx, x_init, single, bool(cuda)


def _ave_weights(ave, B: int, k: int):
    """(B, k) float64 weights of a DiscreteProba-like `ave`, or None (uniform)."""
    w = None if ave is None else getattr(ave, "weights", None)
    if w is not None:
        w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w, dtype=np.float64)
        while w.ndim > 2 and w.shape[-1] == 1:
            w = w[..., 0]
        if w.ndim == 1:
            w = np.broadcast_to(w, (B, k))
        if w.shape != (B, k):
            raise ValueError(f"ave.weights must be (k,) or (B, k) = ({B}, {k}), got {w.shape}")
        w = np.ascontiguousarray(w, dtype=np.float64)
    return w


def compute_smile(x, Ts, Ms, r: float = 0.0, ave=None, *, degree: int = 3, kind: str = "otm", cuda: bool | None = None,
                  report: bool = False) -> Smile:
    """Hedged Monte Carlo smile of price paths x (k, N+1) or (B, k, N+1) (numpy or torch; every path starts at the same
    x[..., 0], the spot).  `ave`: a DiscreteProba whose `weights` are (k,) / (B, k), or None (uniform).  Ts: maturities in
    samples (1 <= T <= N); Ms: rescaled log-moneyness, K = F exp(M sigma_T sqrt(T / 252)).  Log-returns are rounded to
    float32 on both paths, so cuda=True (the psh_hedged_mc kernel) and cuda=False (numpy) answer the same question.
    cuda=None: the device when x is a HIP tensor.  report=True fills the Smile's report fields (delta, price_mc, risk,
    risk_unhedged, price_se, price_se_unhedged, iv_se, n_eff, policy): the hedge on the fit's own paths; hedge_pnl()
    replays `policy` on others."""
    dlnx, x_init, single, cuda = _paths_to_returns(x, cuda)
    w = _ave_weights(ave, dlnx.shape[0], dlnx.shape[1])
    sm = smile_from_log_returns(dlnx, w, Ts, Ms, x_init, r, degree=degree, kind=kind, cuda=cuda, report=report)
    if single:
        sm.prices, sm.ivs, sm.strikes, sm.sigma, sm.status = sm.prices[0], sm.ivs[0], sm.strikes[0], sm.sigma[0], sm.status[0]
        if report:                                                        # (the policy stays batched, B = 1)
            for name in REPORT_FIELDS:
                setattr(sm, name, getattr(sm, name)[0])
    return sm


def hedge_pnl(policy: HedgePolicy, x, ave=None, return_paths: bool = False, cuda: bool | None = None) -> HedgedPnL:
    """Replay `policy` (Smile.policy of a report=True smile) on price paths x (k', N+1) or (B, k', N+1), N >= max Ts, that
    start at the policy's x_init (ValueError otherwise); B is the policy's number of dates.  `ave`: the paths' weights as
    in compute_smile.  On paths the policy was not fitted on this is the out-of-sample check of the hedge: `risk` is what
    the hedge really leaves, `se` the honest standard error of `mean`.  return_paths=True also returns `pnl` per path
    (weighted_quantiles(pnl, ...) gives the VaR of the hedged position).  cuda=None: the device when the policy's
    coefficients are a HIP tensor."""
    on_dev = isinstance(policy.coef, torch.Tensor) and policy.coef.is_cuda
    dlnx, x_init, single, cuda = _paths_to_returns(x, on_dev if cuda is None else cuda)
    if x_init != policy.x_init:
        raise ValueError(f"the paths start at {x_init}, the policy was fitted at x_init = {policy.x_init}")
    B = policy.prices.shape[0]
    if dlnx.shape[0] != B:
        raise ValueError(f"the policy holds {B} date(s), x holds {dlnx.shape[0]}")
    Ts, Ms = [int(T) for T in policy.Ts], [float(M) for M in policy.Ms]
    if max(Ts) > dlnx.shape[-1]:
        raise ValueError(f"the paths have {dlnx.shape[-1]} steps, the policy's longest maturity is {max(Ts)}")
    xw, w = _returns_and_weights(dlnx, _ave_weights(ave, B, dlnx.shape[1]), cuda)
    rep = _replay(xw, w, Ts, Ms, policy.coef, policy.strikes, policy.prices, policy.x_init, policy.r, policy.degree,
                  policy.kind, return_paths, cuda)
    res = report_from_sums(rep["sums"], policy.prices)
    out = HedgedPnL(res["mean"], res["mc"], res["risk"], res["risk_unhedged"], res["se"], res["se_unhedged"], res["n_eff"],
                    rep["sums"], rep["status"], rep.get("pnl"))
    if single:
        for f in fields(out):
            v = getattr(out, f.name)
            if v is not None:
                setattr(out, f.name, v[0])
    return out
