"""Calibrating the shadowing paths' weights to market option quotes: the weighted Monte Carlo of Avellaneda, Buff,
Friedman, Grandchamp, Kruk and Newman (2001).  The paths stay; their weights move as little as possible, in relative
entropy, from the prior (the averaging weights) until the weighted paths reprice the quotes.  The result is a (B, k)
float64 weight array, which compute_smile, hedge_pnl, weighted_quantiles, score_ensemble and the weighted moments take
as given: a `Calibration` can be passed wherever an `ave` is accepted.

The definition, for one date (README "Calibrating to market quotes"; include/psh.h; the header of
shadowing_amd/csrc/psh_calibrate.hip), all in double, rho = r / 252:
    l_0 = 0, l_{n+1} = l_n + dlnx[i, n]  (sequential)   S_{T,i} = x_init exp(l_T)
    g_ij = exp(-rho T_j) payoff_j(S_{T_j, i})            forward: g = exp(-rho T) S_T, target x_init
    h_ij = (g_ij - c_j) / x_init                         instrument j = q * nM + m;  forwards: nT * nM + q
    a_i = sum_j lambda_j h_ij     amax = max of a over p_i > 0     e_i = p_i exp(a_i - amax)     Z = sum e_i
    q_i = e_i / Z                 P = sum p_i
    Phi(lambda) = amax + ln(Z / P) + (eps / 2) |lambda|^2
    grad_j = mu_j + eps lambda_j,  mu_j = sum_i q_i h_ij,   H_jl = sum_i q_i h_ij h_il - mu_j mu_l + eps delta_jl
Newton steps from lambda = 0: success when max_j |grad_j| <= tol; else H d = -grad by Cholesky in instrument order (an
unknown whose diagonal is not > 0 or whose pivot is <= 1e-10 of it is dropped: step 0; an unquoted instrument, target NaN,
is never an unknown); t = 1, 1/2, ..., 2^-40 until Phi(lambda + t d) <= Phi(lambda) + 1e-4 t grad.d; at most max_iter
steps.  Every unknown dropped above tol, a failed line search or max_iter steps: the last iterate with NOT_CONVERGED.
At the minimum the model reprices quote j with error -eps lambda_j x_init; eps = 0 is the hard constraint.

`calibrate_host` is the numpy float64 twin of psh_calibrate_weights, line for line but for the order of its sums, its exp
and the kernel's h, which multiplies by 1 / x_init where the twin divides; `calibrate_weights(..., cuda=True)` runs the kernel.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from .pricing import KINDS, _ave_weights, _paths_to_returns, _returns_and_weights, bs_price

STATUS_OK, STATUS_NONFINITE, STATUS_WEIGHTS, STATUS_QUOTES, STATUS_NOT_CONVERGED, STATUS_DROPPED = 0, 1, 2, 4, 8, 16
MAX_INSTRUMENTS = 32          # on the device (PSH_CAL_MAX_INSTRUMENTS); the twin takes any number
PIVOT_TOL = 1e-10             # psh_hmc's dropping rule
ARMIJO = 1e-4
MAX_HALVINGS = 40


def instruments(x_init: float, rate: float, Ts, strike: np.ndarray, target: np.ndarray, kind: int, martingale: bool):
    """The J instruments of one date as arrays (q, K, c, disc, sgn, act): maturity index, strike, target (0 where not
    quoted), discount factor, +1 call / -1 put / 0 forward, quoted."""
    nT, nM = strike.shape
    rho = rate / 252.0
    q, K, c, disc, sgn, act = [], [], [], [], [], []
    for iq, T in enumerate(Ts):
        df, fwd = math.exp(-(rho * float(T))), x_init * math.exp(rho * float(T))
        for m in range(nM):
            Kj, cj = float(strike[iq, m]), float(target[iq, m])
            q.append(iq); K.append(Kj); disc.append(df)
            act.append(not math.isnan(cj)); c.append(0.0 if math.isnan(cj) else cj)
            sgn.append(1 if kind == KINDS["call"] else -1 if kind == KINDS["put"] else (1 if Kj >= fwd else -1))
    if martingale:
        for iq, T in enumerate(Ts):
            q.append(iq); K.append(0.0); disc.append(math.exp(-(rho * float(T)))); act.append(True); c.append(x_init); sgn.append(0)
    return (np.array(q), np.array(K), np.array(c), np.array(disc), np.array(sgn), np.array(act, dtype=bool))


def payoffs(S: np.ndarray, inst, dtype=np.float64) -> np.ndarray:
    """g (n, J) of terminal prices S (n, nT): the discounted payoffs of the instruments."""
    q, K, _, disc, sgn, _ = inst
    Sj = S[:, q].astype(dtype)
    K, disc = K.astype(dtype), disc.astype(dtype)
    zero = dtype(0.0)
    pay = np.where(sgn[None, :] == 0, Sj, np.maximum(np.where(sgn[None, :] > 0, Sj - K[None, :], K[None, :] - Sj), zero))
    return disc[None, :] * pay


def terminal_prices(r: np.ndarray, Ts, x_init: float) -> np.ndarray:
    """S (n, nT) of float32 log-returns r (n, L): the sequential double sum of the first T returns, exponentiated."""
    l = np.cumsum(r[:, :max(Ts)].astype(np.float64), axis=1)
    return x_init * np.exp(l[:, [int(T) - 1 for T in Ts]])


def _solve(H: np.ndarray, rhs: np.ndarray, act: np.ndarray):
    """(d, dropped, kept) of H d = rhs by Cholesky in order, with the dropping rule of the definition."""
    J = H.shape[0]
    L = np.zeros_like(H)
    dropped, kept = False, 0
    for j in range(J):
        d = H[j, j]
        for c in range(j):
            d = d - L[j, c] * L[j, c]
        if not (act[j] and H[j, j] > 0.0 and d > PIVOT_TOL * H[j, j]):
            dropped = dropped or bool(act[j])
            continue
        kept += 1
        ljj = math.sqrt(d)
        L[j, j] = ljj
        for i in range(j + 1, J):
            if not act[i]:
                continue
            s = H[i, j]
            for c in range(j):
                s = s - L[i, c] * L[j, c]
            L[i, j] = s / ljj
    z = np.zeros(J)
    for j in range(J):
        v = rhs[j]
        for c in range(j):
            v = v - L[j, c] * z[c]
        z[j] = v / L[j, j] if L[j, j] > 0.0 else 0.0
    for j in range(J - 1, -1, -1):
        v = z[j]
        for c in range(j + 1, J):
            v = v - L[c, j] * z[c]
        z[j] = v / L[j, j] if L[j, j] > 0.0 else 0.0
    return z, dropped, kept


def _cal_date(r, prior, x_init, rate, Ts, strike, target, kind, martingale, eps, tol, max_iter):
    """One date on the host: r (k, L) float32, prior (k,) or None.  Returns (weights (k,), lam (J,), model (J,), info (4,),
    status)."""
    k = r.shape[0]
    nT, nM = strike.shape
    J = nT * nM + (nT if martingale else 0)
    nan = lambda n: np.full(n, np.nan)   # noqa: E731
    p = np.ones(k) if prior is None else np.asarray(prior, dtype=np.float64)
    status = 0
    with np.errstate(invalid="ignore", over="ignore"):
        P = float(np.sum(p))
    if not np.isfinite(p).all() or (p < 0.0).any() or not (P > 0.0 and math.isfinite(P)):
        status |= STATUS_WEIGHTS
    live = p > 0.0
    if not np.isfinite(r[live, :max(Ts)]).all():
        status |= STATUS_NONFINITE
    if not (np.isfinite(strike) & (strike > 0.0)).all() or np.isinf(target).any():
        status |= STATUS_QUOTES
    if status:
        return nan(k), nan(J), nan(J), nan(4), status
    inst = instruments(x_init, rate, Ts, strike, target, kind, martingale)
    c, act = inst[2], inst[5]
    pl = p[live]
    g = payoffs(terminal_prices(r[live], Ts, x_init), inst)
    h = (g - c[None, :]) / x_init

    def phi_at(lam):
        a = np.zeros(pl.shape[0])
        for j in range(J):
            if act[j]:
                a = a + lam[j] * h[:, j]
        amax = float(a.max())
        e = pl * np.exp(a - amax)
        Z = float(np.sum(e))
        l2 = 0.0
        for j in range(J):
            l2 = l2 + lam[j] * lam[j]
        with np.errstate(all="ignore"):
            lnzp = float(np.log(Z / P))
        return (amax + lnzp) + (0.5 * eps) * l2, e, Z, lnzp, a - amax

    lam = np.zeros(J)
    phi, e, Z, lnzp, arg = phi_at(lam)
    steps, dropped_last, gmax = 0, False, 0.0
    while True:
        qw = e / Z
        hq = qw[:, None] * h
        mu = np.where(act, hq.sum(axis=0), 0.0)
        H = hq.T @ h - np.outer(mu, mu) + eps * np.eye(J)
        grad = np.where(act, mu + eps * lam, 0.0)
        gmax = float(np.max(np.abs(grad))) if J else 0.0
        if gmax <= tol:
            break
        if math.isnan(gmax) or steps >= max_iter:
            status |= STATUS_NOT_CONVERGED
            break
        d, dropped_last, kept = _solve(H, -grad, act)
        if kept == 0:
            status |= STATUS_NOT_CONVERGED
            break
        gd = 0.0
        for j in range(J):
            gd = gd + grad[j] * d[j]
        t, accepted = 1.0, False
        for _ in range(MAX_HALVINGS + 1):
            trial = lam + t * d
            with np.errstate(invalid="ignore", over="ignore"):
                res = phi_at(trial)
            if res[0] <= phi + (ARMIJO * t) * gd:
                accepted = True
                break
            t = 0.5 * t
        if not accepted:
            status |= STATUS_NOT_CONVERGED
            break
        lam = trial
        phi, e, Z, lnzp, arg = res
        steps += 1
    if dropped_last:
        status |= STATUS_DROPPED
    qw = e / Z
    weights = np.zeros(k)
    weights[live] = qw
    model = (qw[:, None] * g).sum(axis=0)
    info = np.array([float(np.sum(qw * arg)) - lnzp, 1.0 / float(np.sum(qw * qw)), float(steps), gmax])
    return weights, lam, model, info, status


def _check_cal_args(Ts, L: int, eps: float, tol: float, max_iter: int, kind):
    Ts = [int(T) for T in np.atleast_1d(Ts)]
    if not Ts or min(Ts) < 1 or max(Ts) > L:
        raise ValueError(f"maturities must lie in [1, {L}] samples, got {Ts}")
    if not (float(eps) >= 0.0 and math.isfinite(float(eps))):
        raise ValueError(f"eps must be >= 0 and finite, got {eps}")
    if not float(tol) > 0.0:
        raise ValueError(f"tol must be > 0, got {tol}")
    if int(max_iter) < 0:
        raise ValueError(f"max_iter must be >= 0, got {max_iter}")
    if kind not in KINDS.values():
        raise ValueError(f"kind must be one of {sorted(KINDS.values())}, got {kind!r}")
    return Ts


def calibrate_host(dlnx: np.ndarray, prior: np.ndarray | None, Ts, strike: np.ndarray, target: np.ndarray,
                   x_init: float = 100.0, rate: float = 0.0, kind: int = 0, martingale: bool = True, eps: float = 1e-6,
                   tol: float = 1e-8, max_iter: int = 100) -> dict:
    """The numpy float64 twin of psh_calibrate_weights: dlnx (B, k, L) float32, prior (B, k) or None, strike and target
    (B, nT, nM); any k and any number of instruments.  Returns "weights" (B, k), "lam" and "model" (B, J), "info" (B, 4) =
    [kl, n_eff, steps, max |grad|] and "status" (B,) int32."""
    dlnx = np.asarray(dlnx)
    if dlnx.ndim != 3:
        raise ValueError("dlnx must be (B, k, L)")
    B, k, L = dlnx.shape
    Ts = _check_cal_args(Ts, L, eps, tol, max_iter, kind)
    strike, target = np.asarray(strike, dtype=np.float64), np.asarray(target, dtype=np.float64)
    if strike.ndim != 3 or strike.shape != target.shape or strike.shape[:2] != (B, len(Ts)) or strike.shape[2] < 1:
        raise ValueError(f"strike and target must be (B, nT, nM) = ({B}, {len(Ts)}, nM), got {strike.shape} and {target.shape}")
    if prior is not None and np.shape(prior) != (B, k):
        raise ValueError(f"prior must be (B, k) = ({B}, {k}), got {np.shape(prior)}")
    res = [_cal_date(dlnx[b].astype(np.float32, copy=False), None if prior is None else prior[b], float(x_init), float(rate), Ts,
                     strike[b], target[b], int(kind), bool(martingale), float(eps), float(tol), int(max_iter)) for b in range(B)]
    return {"weights": np.stack([x[0] for x in res]), "lam": np.stack([x[1] for x in res]),
            "model": np.stack([x[2] for x in res]), "info": np.stack([x[3] for x in res]),
            "status": np.array([x[4] for x in res], dtype=np.int32)}


class MarketQuotes:
    """Quoted vanillas: `Ts` (nT,) maturities in samples, `strikes` (nT, nM) or (B, nT, nM), and either `prices` or
    `ivs` (Black-Scholes implied vols, turned into prices by pricing.bs_price once the spot and the rate are known), shaped
    as the strikes; NaN: not quoted.  kind: "otm" (a call iff K >= x_init exp(r T / 252)), "call" or "put"."""

    def __init__(self, Ts, strikes, prices=None, ivs=None, kind: str = "otm"):
        if (prices is None) == (ivs is None):
            raise ValueError("MarketQuotes takes exactly one of prices, ivs")
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
        self.Ts = np.asarray([int(T) for T in np.atleast_1d(Ts)])
        self.strikes = np.asarray(strikes, dtype=np.float64)
        self.prices = None if prices is None else np.asarray(prices, dtype=np.float64)
        self.ivs = None if ivs is None else np.asarray(ivs, dtype=np.float64)
        self.kind = kind
        given = self.prices if self.prices is not None else self.ivs
        if self.strikes.ndim not in (2, 3) or self.strikes.shape != given.shape or self.strikes.shape[-2] != len(self.Ts):
            raise ValueError(f"strikes and prices / ivs must both be (nT, nM) or (B, nT, nM) with nT = {len(self.Ts)}, got "
                             f"{self.strikes.shape} and {given.shape}")

    @classmethod
    def from_smile(cls, smile, use: str = "price_mc") -> "MarketQuotes":
        """The quotes a Smile states: its strikes with its `prices` (hedged) or `price_mc` (plain weighted Monte Carlo, a
        report=True smile)."""
        prices = getattr(smile, use, None)
        if use not in ("prices", "price_mc") or prices is None:
            raise ValueError(f"from_smile: the smile holds no {use!r} (price_mc needs report=True)")
        return cls(smile.Ts, smile.strikes, prices=prices, kind=smile.kind)

    def arrays(self, B: int, x_init: float, r: float):
        """(strike, target) as (B, nT, nM) float64 C-contiguous arrays for B dates at this spot and rate."""
        K = self.strikes
        if self.prices is not None:
            c = self.prices
        else:
            c = np.full(K.shape, np.nan)
            Tq = np.broadcast_to(self.Ts[:, None], K.shape)
            for ix in np.ndindex(K.shape):
                sig, Kj, T = float(self.ivs[ix]), float(K[ix]), float(Tq[ix])
                if math.isnan(sig) or not (Kj > 0.0 and math.isfinite(Kj)):
                    continue
                call = self.kind == "call" or (self.kind == "otm" and Kj >= x_init * math.exp(r / 252.0 * T))
                c[ix] = bs_price(x_init, Kj, T / 252.0, r, sig, call) if sig > 0.0 else math.inf
        if K.ndim == 3 and K.shape[0] not in (1, B):
            raise ValueError(f"the quotes hold {K.shape[0]} date(s), the paths {B}")
        shape = (B,) + K.shape[-2:]
        return (np.ascontiguousarray(np.broadcast_to(K, shape)), np.ascontiguousarray(np.broadcast_to(c, shape)))

    def rows(self, idx) -> "MarketQuotes":
        """The quotes of the dates `idx` (quotes shared by every date stay shared)."""
        if self.strikes.ndim == 2 or self.strikes.shape[0] == 1:
            return self
        cut = lambda a: None if a is None else a[idx]   # noqa: E731
        return MarketQuotes(self.Ts, self.strikes[idx], cut(self.prices), cut(self.ivs), self.kind)


@dataclass
class Calibration:
    """Calibrated weights and how far the paths had to be bent: `weights` (B, k) float64 -- numpy, or a HIP tensor from the
    device route -- `lam` and `model` (B, J) the multipliers and the model prices sum_i q_i g_ij, instrument
    j = q * nM + m, then the nT forwards; `residual` = model - target (NaN where not quoted); `kl` the relative entropy to
    the prior, `n_eff` = 1 / sum q^2, `iterations` the Newton steps, `grad` = max_j |grad_j| at the end, `status` (B,)
    PSH_CAL_STATUS_* bits; `quotes` what it was calibrated to.  A single set of paths drops the leading axis."""
    weights: object
    lam: np.ndarray
    model: np.ndarray
    residual: np.ndarray
    kl: np.ndarray
    n_eff: np.ndarray
    iterations: np.ndarray
    grad: np.ndarray
    status: np.ndarray
    quotes: MarketQuotes | None = None


def calibrate_from_log_returns(dlnx, weights, quotes: MarketQuotes, x_init: float = 100.0, r: float = 0.0, *, eps: float = 1e-6,
                               tol: float = 1e-8, max_iter: int = 100, martingale: bool = True, cuda: bool = False) -> Calibration:
    """Calibrate the weights of (B, k, L) float32 log-returns (numpy, or a HIP tensor of any row stride) with (B, k) prior
    weights or None to `quotes`.  cuda=True: psh_calibrate_weights (k <= PSH_MAX_K, at most 32 instruments), the weights
    stay on the device; cuda=False: the numpy twin."""
    if not isinstance(quotes, MarketQuotes):
        raise TypeError(f"quotes must be MarketQuotes, got {type(quotes).__name__}")
    B, _, L = dlnx.shape
    Ts = _check_cal_args(quotes.Ts, L, eps, tol, max_iter, KINDS[quotes.kind])
    if not (math.isfinite(float(x_init)) and float(x_init) > 0.0 and math.isfinite(float(r))):
        raise ValueError(f"x_init must be positive and finite and r finite, got {x_init}, {r}")
    strike, target = quotes.arrays(B, float(x_init), float(r))
    x, w = _returns_and_weights(dlnx, weights, cuda)
    if cuda:
        from . import _native
        dev = x.device
        out = _native.calibrate_weights(x, w, Ts, torch.from_numpy(strike).to(dev), torch.from_numpy(target).to(dev), x_init, r,
                                        KINDS[quotes.kind], martingale, eps, tol, max_iter)
        host = {name: t.cpu().numpy() for name, t in out.items() if name != "weights"}
        wq = out["weights"]
    else:
        host = calibrate_host(x, w, Ts, strike, target, x_init, r, KINDS[quotes.kind], martingale, eps, tol, max_iter)
        wq = host["weights"]
    J = host["lam"].shape[1]
    c = np.full((B, J), float(x_init))
    c[:, :target.shape[1] * target.shape[2]] = target.reshape(B, -1)
    info = host["info"]
    with np.errstate(invalid="ignore"):
        iters = np.where(np.isnan(info[:, 2]), -1, info[:, 2]).astype(np.int64)
    return Calibration(wq, host["lam"], host["model"], host["model"] - c, info[:, 0], info[:, 1], iters, info[:, 3],
                       host["status"], quotes)


CALIBRATION_FIELDS = ("weights", "lam", "model", "residual", "kl", "n_eff", "iterations", "grad", "status")


def concat_calibrations(parts: list) -> Calibration:
    """One Calibration of several batches of dates."""
    def cat(name):
        vals = [getattr(p, name) for p in parts]
        return torch.cat(vals) if isinstance(vals[0], torch.Tensor) else np.concatenate(vals)
    return Calibration(*(cat(name) for name in CALIBRATION_FIELDS), parts[0].quotes)


def calibrate_weights(x, quotes: MarketQuotes, r: float = 0.0, ave=None, eps: float = 1e-6, tol: float = 1e-8,
                      max_iter: int = 100, martingale: bool = True, cuda: bool | None = None) -> Calibration:
    """Calibrate the weights of price paths x (k, N+1) or (B, k, N+1) (numpy or torch; every path starts at the same
    x[..., 0], the spot) to `quotes`.  `ave`: the prior, a DiscreteProba (or a Calibration) whose `weights` are (k,) /
    (B, k), or None (uniform).  martingale=True adds the forward of every quoted maturity as an instrument.  Log-returns
    are rounded to float32 on both routes.  cuda=None: the device when x is a HIP tensor; cuda=True never falls back.
    ValueError for whatever psh_calibrate_weights rejects."""
    dlnx, x_init, single, cuda = _paths_to_returns(x, cuda)
    w = _ave_weights(ave, dlnx.shape[0], dlnx.shape[1])
    cal = calibrate_from_log_returns(dlnx, w, quotes, x_init, r, eps=eps, tol=tol, max_iter=max_iter, martingale=martingale,
                                     cuda=cuda)
    if single:
        for name in CALIBRATION_FIELDS:
            setattr(cal, name, getattr(cal, name)[0])
    return cal
