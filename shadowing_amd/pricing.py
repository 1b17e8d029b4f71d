"""Option pricing on shadowing paths: hedged Monte Carlo (Potters, Bouchaud, Sestovic 2001) and the implied-volatility
smile, the second use of Path Shadowing Monte Carlo that the reference README names ("Option pricing").

In the reference, `PriceData` and `compute_smile` come from the un-vendored dependency `scatspectra`.  The definitions
below are this project's own (PARITY UNPINNED, as for the averaging stand-ins of averaging.py): the method is written out
in the header of shadowing_amd/csrc/psh_hmc.hip and in README "Option pricing".  `compute_smile(..., cuda=True)` runs it
as one launch of psh_hedged_mc; `cuda=False` is the numpy float64 twin below, which follows the kernel operation for
operation except for the order of its sums.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

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

    def plot(self, ax=None, rescale: bool = True, legend: bool = True, color=None, **kw):
        """Implied vol against M (rescale=True) or against log(K / F), F the forward (rescale=False): one line per
        maturity, of the first date when there are several."""
        import matplotlib.pyplot as plt
        if ax is None:
            ax = plt.gca()
        ivs = self.ivs if self.ivs.ndim == 2 else self.ivs[0]
        strikes = self.strikes if self.strikes.ndim == 2 else self.strikes[0]
        for q, T in enumerate(self.Ts):
            fwd = self.x_init * math.exp(self.r * T / 252.0)
            xs = self.Ms if rescale else np.log(strikes[q] / fwd)
            ax.plot(xs, ivs[q], color=color, label=f"T={int(T)}", marker="o", **kw)
        ax.set_xlabel("M (rescaled log-moneyness)" if rescale else "log(K / F)")
        ax.set_ylabel("implied vol")
        if legend:
            ax.legend()
        return ax


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


def _hmc_date(r: np.ndarray, w: np.ndarray | None, x0: float, rate: float, Ts, Ms, degree: int, kind: int):
    """One date on the host: r (k, L) float32 log-returns, w (k,) raw weights or None.  Returns (price, iv, strike
    (nT, nM), sigma (nT,), status)."""
    nT, nM = len(Ts), len(Ms)
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
        return price, iv, strike, sigma_out, status
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
            V = np.broadcast_to(gamma[P], (u0.shape[0], nM)).copy()
            for c in range(P - 1, -1, -1):
                V = V * u0[:, None] + gamma[c]
        strike[q] = K
        if ill:                                                         # price and iv stay NaN
            status |= STATUS_ILL_CONDITIONED
            continue
        price[q] = gamma[0]
        iv[q] = [implied_vol(float(price[q, j]), x0, float(K[j]), tau, rate, bool(call[j])) for j in range(nM)]
    return price, iv, strike, sigma_out, status


def hedged_mc_host(dlnx: np.ndarray, weights: np.ndarray | None, Ts, Ms, x_init: float = 100.0, rate: float = 0.0,
                   degree: int = 3, kind: int = 0) -> dict:
    """The numpy float64 twin of psh_hedged_mc: dlnx (B, k, L) float32, weights (B, k) or None; any k."""
    B = dlnx.shape[0]
    res = [_hmc_date(dlnx[b], None if weights is None else weights[b], x_init, rate, Ts, Ms, degree, kind) for b in range(B)]
    return {"price": np.stack([x[0] for x in res]), "iv": np.stack([x[1] for x in res]),
            "strike": np.stack([x[2] for x in res]), "sigma": np.stack([x[3] for x in res]),
            "status": np.array([x[4] for x in res], dtype=np.int32)}


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


def smile_from_log_returns(dlnx, weights, Ts, Ms, x_init: float = 100.0, r: float = 0.0, *, degree: int = 3,
                           kind: str = "otm", cuda: bool = False) -> Smile:
    """The hedged Monte Carlo smile of (B, k, L) float32 log-returns (numpy, or a HIP tensor -- any row stride, e.g. the
    out-context view of gathered paths) with (B, k) weights or None.  cuda=True: one psh_hedged_mc launch (k <= PSH_MAX_K,
    nT, nM <= 64); cuda=False: the numpy twin."""
    L = dlnx.shape[-1]
    Ts, Ms = _check_args(Ts, Ms, L, degree, kind)
    if cuda:
        from . import _native
        x = dlnx if isinstance(dlnx, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dlnx, dtype=np.float32))
        dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
        x = x.to(dev, torch.float32)
        w = None
        if weights is not None:
            w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64))
            w = w.to(dev, torch.float64).contiguous()
        out = _native.hedged_mc(x, w, Ts, Ms, x_init, r, degree, KINDS[kind])
        host = {name: t.cpu().numpy() for name, t in out.items()}
    else:
        x = dlnx.detach().cpu().numpy() if isinstance(dlnx, torch.Tensor) else np.asarray(dlnx)
        w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else weights
        host = hedged_mc_host(x.astype(np.float32, copy=False), None if w is None else np.asarray(w, dtype=np.float64),
                              Ts, Ms, x_init, r, degree, KINDS[kind])
    return Smile(host["price"], host["iv"], host["strike"], host["sigma"], np.asarray(Ts), np.asarray(Ms), kind,
                 host["status"], float(x_init), float(r))


def compute_smile(x, Ts, Ms, r: float = 0.0, ave=None, *, degree: int = 3, kind: str = "otm", cuda: bool | None = None) -> Smile:
    """Hedged Monte Carlo smile of price paths x (k, N+1) or (B, k, N+1) (numpy or torch; every path starts at the same
    x[..., 0], the spot).  `ave`: a DiscreteProba whose `weights` are (k,) / (B, k), or None (uniform).  Ts: maturities in
    samples (1 <= T <= N); Ms: rescaled log-moneyness, K = F exp(M sigma_T sqrt(T / 252)).  Log-returns are rounded to
    float32 on both paths, so cuda=True (the psh_hedged_mc kernel) and cuda=False (numpy) answer the same question.
    cuda=None: the device when x is a HIP tensor."""
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
    B, k = dlnx.shape[0], dlnx.shape[1]
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
    sm = smile_from_log_returns(dlnx, w, Ts, Ms, x_init, r, degree=degree, kind=kind, cuda=bool(cuda))
    if single:
        sm.prices, sm.ivs, sm.strikes, sm.sigma, sm.status = sm.prices[0], sm.ivs[0], sm.strikes[0], sm.sigma[0], sm.status[0]
    return sm
