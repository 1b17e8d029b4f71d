"""The stylised facts of an ensemble, measured where it lies, and the skewed MRW fitted to them.

`lagged_moments` gives, for R rows of n returns and lags tau = 0 .. m, the means over rows and over t = 0 .. n - 1 - tau of
    xx = x[t] x[t+tau],  xx2 = x[t] x[t+tau]^2 (leverage),  x2x = x[t]^2 x[t+tau] (its time reverse),
    x2x2 = x[t]^2 x[t+tau]^2 (volatility clustering; the fourth moment at tau = 0),
every sample converted to double first, pairs never crossing a row, a row that holds a NaN or an inf left out whole.  The
rows are cut into G groups (group g holds rows [floor(g R / G), floor((g+1) R / G))), and the scatter of the group means
gives each mean its standard error.  On a HIP float32 tensor the sums are psh_lagged_moments' (the method heads
shadowing_amd/csrc/psh_moments.hip): the ensemble is read in place and only the (G, 4, m + 1) sums come to the host.
`cuda=False` is the numpy float64 twin: the same definition on float32-rounded inputs.

`fit_smrw` chooses (sigma, lam, K0, alpha) of the skewed MRW (mrw.smrw_log_returns) for a measured ensemble: sigma^2 is the
variance, the other three a Levenberg-Marquardt fit of the closed forms mrw.smrw_leverage and mrw.smrw_sq_moment to the
measured xx2 and x2x2 at lags 1 .. max_lag, each residual divided by its standard error.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from . import mrw

MAX_LAG = 1024                                       # PSH_MOMENTS_MAX_LAG; the twin keeps it: both accept the same calls
DEFAULT_GROUPS = 64
MIN_FIT_GROUPS = 8


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


@dataclass(frozen=True)
class LaggedMoments:
    """The means of the four lagged products at lags 0 .. m, their standard errors from the scatter of the group means
    (NaN with fewer than two non-empty groups), and what they were made from."""
    n: int                                           # samples per row
    lags: np.ndarray                                 # (m + 1,) int64: 0 .. m
    n_pairs: np.ndarray                              # (m + 1,) int64: rows_used * (n - tau)
    xx: np.ndarray
    xx2: np.ndarray
    x2x: np.ndarray
    x2x2: np.ndarray
    xx_se: np.ndarray
    xx2_se: np.ndarray
    x2x_se: np.ndarray
    x2x2_se: np.ndarray
    rows_used: int
    rows_excluded: int
    group_sums: np.ndarray = field(repr=False)       # (G, 4, m + 1) float64: the sums as measured (they add across ranks)
    group_rows: np.ndarray = field(repr=False)       # (G,) int64

    @property
    def variance(self) -> float:
        return float(self.xx[0])

    @property
    def kurtosis(self) -> float:
        return float(self.x2x2[0] / self.xx[0] ** 2)

    def leverage(self) -> np.ndarray:
        """(m,) E[r_t r_{t+tau}^2] / E[r^2]^2 at tau = 1 .. m: Bouchaud's normalisation of the leverage curve."""
        return self.xx2[1:] / self.xx[0] ** 2


def group_bounds(R: int, G: int) -> np.ndarray:
    """(G + 1,) int64: group g holds rows [bounds[g], bounds[g + 1]) = [floor(g R / G), floor((g+1) R / G))."""
    return (np.arange(G + 1, dtype=np.int64) * R) // G


def _host_sums(X: np.ndarray, m: int, G: int):
    """The numpy twin of psh_lagged_moments on (R, n) float32: (sums (G, 4, m + 1) float64, rows_used (G,) int64)."""
    R, n = X.shape
    ok = np.isfinite(X).all(axis=1)
    x = np.where(ok[:, None], X, np.float32(0.0)).astype(np.float64)     # an excluded row adds zeros
    sq = x * x                                                           # exact: 24-bit inputs
    starts = group_bounds(R, G)[:-1]
    sums = np.empty((G, 4, m + 1))
    for tau in range(m + 1):
        a, a2, b, b2 = x[:, :n - tau], sq[:, :n - tau], x[:, tau:], sq[:, tau:]
        for q, (u, w) in enumerate(((a, b), (a, b2), (a2, b), (a2, b2))):
            sums[:, q, tau] = np.add.reduceat(np.einsum("rt,rt->r", u, w), starts)
    return sums, np.add.reduceat(ok.astype(np.int64), starts)


def _summarise(sums: np.ndarray, rows: np.ndarray, R: int, n: int) -> LaggedMoments:
    G, _, m1 = sums.shape
    lags = np.arange(m1, dtype=np.int64)
    used = int(rows.sum())
    span = (n - lags).astype(np.float64)
    live = rows > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = sums.sum(axis=0) / (used * span)                          # (4, m + 1); 0 / 0 = NaN with no row left
        if int(live.sum()) >= 2:
            gmean = sums[live] / (rows[live, None, None] * span)
            wgt = rows[live] / float(used)
            se = np.sqrt(np.einsum("g,gqt->qt", wgt, (gmean - mean) ** 2) / (int(live.sum()) - 1))
        else:
            se = np.full_like(mean, np.nan)
    return LaggedMoments(n=n, lags=lags, n_pairs=used * (n - lags), xx=mean[0], xx2=mean[1], x2x=mean[2], x2x2=mean[3],
                         xx_se=se[0], xx2_se=se[1], x2x_se=se[2], x2x2_se=se[3], rows_used=used, rows_excluded=R - used,
                         group_sums=sums, group_rows=rows)


def lagged_moments(x, max_lag: int, groups: int | None = None, cuda: bool | None = None) -> LaggedMoments:
    """The lagged cross-moments of (x, x^2) of an ensemble x, (n,), (R, n) or (R, 1, n), numpy or torch, at lags
    0 .. max_lag <= min(n - 1, 1024), with standard errors from `groups` row groups (default min(R, 64)).
    cuda=None: psh_lagged_moments when x is a HIP float32 tensor (read in place), the numpy twin otherwise; cuda=True:
    the device (x is rounded to float32 and uploaded if it is not there; no host fallback); cuda=False: the twin."""
    on_device = _is_torch(x) and x.is_cuda
    if not _is_torch(x):
        x = np.asarray(x)
    if x.ndim == 1:
        x = x[None, :]
    elif x.ndim == 3 and x.shape[1] == 1:
        x = x[:, 0, :]
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"x must be (n,), (R, n) or (R, 1, n) and not empty, got shape {tuple(x.shape)}")
    R, n = int(x.shape[0]), int(x.shape[1])
    if isinstance(max_lag, bool) or int(max_lag) != max_lag or not 0 <= max_lag < n:
        raise ValueError(f"max_lag must be an integer with 0 <= max_lag <= n - 1 = {n - 1}, got {max_lag!r}")
    if max_lag > MAX_LAG:
        raise ValueError(f"max_lag must be <= {MAX_LAG} (what psh_lagged_moments takes; the twin keeps the limit), "
                         f"got {max_lag}")
    G = min(R, DEFAULT_GROUPS) if groups is None else groups
    if isinstance(G, bool) or int(G) != G or not 1 <= G <= R:
        raise ValueError(f"groups must be an integer with 1 <= groups <= R = {R}, got {groups!r}")
    m, G = int(max_lag), int(G)
    if cuda is None:
        cuda = bool(on_device and str(x.dtype) == "torch.float32")
    if cuda:
        import torch
        from . import _native
        if not on_device:
            if not torch.cuda.is_available():
                raise _native.NativeLibraryError("cuda=True needs a HIP device, and there is no host fallback under it")
            x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32) if not _is_torch(x) else x).to("cuda")
        if x.dtype != torch.float32:
            x = x.to(torch.float32)
        sums, rows, _ = _native.lagged_moments(x, m, G)
        return _summarise(sums.cpu().numpy(), rows.cpu().numpy(), R, n)
    X = x.detach().cpu().numpy() if _is_torch(x) else x
    sums, rows = _host_sums(np.ascontiguousarray(X, dtype=np.float32), m, G)
    return _summarise(sums, rows, R, n)


# ---- the fit

def _curves(taus, n, sigma, lam, K0, alpha, L, memory) -> np.ndarray:
    """The closed forms the fit compares with: smrw_leverage at taus, then smrw_sq_moment at taus."""
    kw = dict(lam=lam, L=L, memory=memory, sigma=sigma)
    return np.array([mrw.smrw_leverage(int(t), n, K0, alpha, **kw) for t in taus] +
                    [mrw.smrw_sq_moment(int(t), n, K0, alpha, **kw) for t in taus])


_LO = np.array([0.0, 0.0, 0.05])                     # lam, K0, alpha
_HI = np.array([np.inf, np.inf, 3.0])


def _levenberg_marquardt(resid, p0: np.ndarray, max_iter: int = 200, xtol: float = 1e-11):
    """Minimise |resid(p)|^2 inside the box [_LO, _HI]: forward-difference Jacobian, Marquardt's scaling of the damping,
    steps clipped to the box.  Returns (p, resid(p), jacobian at p, iterations)."""
    def jac(p, r):
        J = np.empty((r.size, p.size))
        for i in range(p.size):
            h = 1e-6 * max(abs(p[i]), 1e-3)
            if p[i] + h > _HI[i]:
                h = -h
            q = p.copy()
            q[i] += h
            J[:, i] = (resid(q) - r) / h
        return J

    p = np.clip(np.asarray(p0, dtype=np.float64), _LO, _HI)
    r = resid(p)
    cost, mu, it = float(r @ r), 1e-3, 0
    J = jac(p, r)
    for it in range(1, max_iter + 1):
        A, g = J.T @ J, J.T @ r
        d = np.diag(A) + 1e-12 * max(float(np.diag(A).max()), 1e-300)
        try:
            step = np.linalg.solve(A + mu * np.diag(d), -g)
        except np.linalg.LinAlgError:
            mu *= 4.0
            continue
        q = np.clip(p + step, _LO, _HI)
        small = bool(np.all(np.abs(q - p) <= xtol * np.maximum(np.abs(p), 1e-3)))
        rq = resid(q)
        cq = float(rq @ rq)
        if cq < cost:
            p, r, cost, mu = q, rq, cq, max(mu / 3.0, 1e-12)
            J = jac(p, r)
        else:
            mu = min(mu * 4.0, 1e12)
        if small:
            break
    return p, r, J, it


def fit_smrw(x, max_lag: int = 40, L: float | None = None, memory: int | None = None, groups: int | None = None,
             cuda: bool | None = None) -> dict:
    """Fit the skewed MRW to an ensemble x (as lagged_moments takes it).  sigma^2 = xx[0]; (lam, K0, alpha) minimise
    chi2 = sum over tau = 1 .. max_lag of ((xx2[tau] - smrw_leverage) / xx2_se[tau])^2 + ((x2x2[tau] - smrw_sq_moment) /
    x2x2_se[tau])^2 inside lam >= 0, K0 >= 0, 0.05 <= alpha <= 3.  L and memory are the caller's and default to n.
    Returns sigma, lam, K0, alpha; `cov`, (4, 4) in that order: of (lam, K0, alpha) from the Jacobian J of the residuals,
    (J^T J)^-1 B (J^T J)^-1 with B the covariance of J^T residuals over the row groups (the lags of one ensemble are
    correlated; a pseudo-inverse: at K0 = 0 alpha has no bearing and gets variance 0), of sigma (xx_se[0] / 2 sigma)^2,
    no cross terms; `stderr`, the square roots of its diagonal by name; chi2, dof, iterations; `params`, the keywords that make
    such an ensemble (`smrw_log_returns(R, n, **fit["params"], cuda=True)`); and `moments`, the LaggedMoments used.
    Needs at least 8 row groups (the standard errors are the weights) and raises ValueError otherwise."""
    mom = lagged_moments(x, max_lag, groups=groups, cuda=cuda)
    n, G = mom.n, int(mom.group_rows.size)
    if G < MIN_FIT_GROUPS or int((mom.group_rows > 0).sum()) < MIN_FIT_GROUPS:
        raise ValueError(f"fit_smrw needs at least {MIN_FIT_GROUPS} non-empty row groups for its standard errors, got {G} "
                         f"({int((mom.group_rows > 0).sum())} non-empty)")
    if max_lag < 2:
        raise ValueError(f"fit_smrw needs max_lag >= 2 (three parameters are fitted), got {max_lag}")
    L = float(n if L is None else L)
    memory = n if memory is None else int(memory)
    if max_lag > memory:
        raise ValueError(f"max_lag must be <= memory = {memory} (smrw_leverage is defined up to the memory), got {max_lag}")
    var = mom.variance
    if not (math.isfinite(var) and var > 0.0):
        raise ValueError(f"the ensemble's variance is {var}: nothing to fit")
    sigma = math.sqrt(var)
    taus = np.arange(1, int(max_lag) + 1)
    data = np.concatenate([mom.xx2[1:], mom.x2x2[1:]])
    se = np.concatenate([mom.xx2_se[1:], mom.x2x2_se[1:]])
    if not (np.all(np.isfinite(se)) and np.all(se > 0.0)):
        raise ValueError("a standard error is zero or not finite: the groups do not scatter (identical rows?)")

    def resid(p):
        return (data - _curves(taus, n, sigma, p[0], p[1], p[2], L, memory)) / se

    # a start from the first lag: x2x2[1] = sigma^4 exp(4 lam^2 ln(L / 2)) and xx2[1] = -2 K0 sigma^3 to first order
    ratio = mom.x2x2[1] / var ** 2
    lam0 = math.sqrt(max(math.log(ratio), 0.0) / (4.0 * max(math.log(L / 2.0), 1e-3))) if ratio > 0.0 else 0.0
    K00 = max(-mom.xx2[1] / (2.0 * sigma ** 3), 1e-3)
    p, r, J, it = _levenberg_marquardt(resid, np.array([min(max(lam0, 0.02), 1.0), min(K00, 1.0), 0.5]))
    cov = np.zeros((4, 4))
    cov[0, 0] = (float(mom.xx_se[0]) / (2.0 * sigma)) ** 2
    # the residuals of one ensemble are correlated across lags, so (J^T J)^-1 alone understates the scatter: the
    # sandwich A^-1 B A^-1, A = J^T J, B the covariance of J^T (data / se) estimated from the group means as the
    # standard errors are
    live = mom.group_rows > 0
    rows = mom.group_rows[live].astype(np.float64)
    gmean = mom.group_sums[live][:, (1, 3), 1:] / (rows[:, None, None] * (n - taus))
    proj = ((gmean.reshape(rows.size, -1) - data) / se) @ J                # (groups, 3)
    B = np.einsum("g,gi,gj->ij", rows / rows.sum(), proj, proj) / (rows.size - 1)
    Ainv = np.linalg.pinv(J.T @ J, rcond=1e-12, hermitian=True)
    cov[1:, 1:] = Ainv @ B @ Ainv
    sd = np.sqrt(np.diag(cov))
    lam, K0, alpha = (float(v) for v in p)
    return dict(sigma=sigma, lam=lam, K0=K0, alpha=alpha, cov=cov,
                stderr=dict(sigma=float(sd[0]), lam=float(sd[1]), K0=float(sd[2]), alpha=float(sd[3])),
                chi2=float(r @ r), dof=int(data.size - 3), iterations=it,
                params=dict(K0=K0, alpha=alpha, lam=lam, L=L, memory=memory, sigma=sigma), moments=mom)


__all__ = ["LaggedMoments", "lagged_moments", "fit_smrw", "group_bounds", "MAX_LAG"]
