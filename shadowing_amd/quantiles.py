"""Predictive quantiles and tail means of a weighted ensemble: VaR and expected shortfall over the k shadowing paths.

One column is one (b, i) of values (B, k, m), rounded to float32; its weights are w[b, :], float64, used as given and never
renormalised (None: w_j = 1).  With the k paths ordered by (value ascending, path index ascending), x_(i) and w_(i) the
sorted values and weights, and all arithmetic in double:

    C_i = sum_{l<=i} w_(l)      S_i = sum_{l<=i} w_(l) x_(l)      W = C_{k-1} (as computed)      t = p W
    i*  = the first i with C_i >= t
    q(p)     = x_(i*)                                                   the lower weighted quantile (inverted CDF)
    lower(p) = ( S_{i*-1} + (t - C_{i*-1}) x_(i*) ) / t                 mean of the lowest p of the mass
    upper(p) = ( (C_{i*} - t) x_(i*) + (S_{k-1} - S_{i*}) ) / (W - t)   mean of the highest 1 - p of the mass

A path of weight exactly 0 contributes nothing, whatever its value.  A non-finite value at a positive weight makes its
column's results NaN and sets STATUS_NONFINITE for the query; a non-finite or negative weight, or W not > 0, makes all the
query's results NaN and sets STATUS_WEIGHTS (the values are then not looked at).  -0.0 and +0.0 are equal values.

On a HIP float32 tensor the work is psh_weighted_quantiles' (the method heads shadowing_amd/csrc/psh_quantiles.hip): one
in-LDS sort per column serves every level, and only the three (B, Q, m) results come to the host.  Everywhere else the numpy
twin below computes the same definition (cumulative sums in sorted order, one after the other).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MAX_LEVELS = 32
STATUS_OK, STATUS_NONFINITE, STATUS_WEIGHTS = 0, 1, 2


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


@dataclass
class PredictiveQuantiles:
    """levels (Q,); q, lower, upper (B, Q, ...) float64 with the trailing dimensions of the statistic; status (B,) int32."""
    levels: np.ndarray
    q: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    status: np.ndarray


def _host_quantiles(values: np.ndarray, weights: np.ndarray | None, levels: np.ndarray, detail: bool = False):
    """The numpy twin on (B, k, m) float32, (B, k) float64 or None, (Q,): q, lower, upper (B, Q, m) and status (B,).
    detail=True adds what a comparison against another summation order needs, each (B, Q, m): `edge` (a cumulative weight
    next to the crossing lies within 4 k 2^-53 W of t, so rounding may move i* by one), `q_prev` / `q_next` (the
    neighbouring order statistics of positive weight) and `bound_lower` / `bound_upper`,
    2 (k + 2) 2^-53 (sum_j w_j |x_j| + W |q|) / t and the same over (W - t)."""
    B, k, m = values.shape
    Q = len(levels)
    out = {n: np.full((B, Q, m), np.nan) for n in ("q", "lower", "upper")}
    names = ("q_prev", "q_next", "bound_lower", "bound_upper")
    det = {n: np.full((B, Q, m), np.nan) for n in names}
    det["edge"] = np.zeros((B, Q, m), dtype=bool)
    status = np.zeros(B, dtype=np.int32)
    cols = np.arange(m)
    eps = 2.0 ** -53
    for b in range(B):
        w = np.ones(k) if weights is None else weights[b]
        if not np.isfinite(w).all() or (w < 0).any() or not (w > 0).any():
            status[b] = STATUS_WEIGHTS
            continue
        keep = w > 0
        x = values[b][keep].astype(np.float64) + 0.0           # (-0.0 + 0.0 = +0.0: the zeros are one value)
        wk = w[keep]
        bad = ~np.isfinite(x).all(axis=0)
        if bad.any():
            status[b] |= STATUS_NONFINITE
            x[:, bad] = 0.0
        order = np.argsort(x, axis=0, kind="stable")            # ties by path index
        xs = np.take_along_axis(x, order, axis=0)
        ws = wk[order]
        Cc = np.cumsum(ws, axis=0)
        Sc = np.cumsum(ws * xs, axis=0)
        W, S = Cc[-1], Sc[-1]
        if not (W > 0).all():
            status[b] = STATUS_WEIGHTS
            continue
        A = (ws * np.abs(xs)).sum(axis=0)
        for a, p in enumerate(levels):
            t = p * W
            i = np.argmax(Cc >= t, axis=0)                     # the first i with C_i >= t (C_{k-1} = W >= t)
            xq, Ci, Si = xs[i, cols], Cc[i, cols], Sc[i, cols]
            ip = np.maximum(i - 1, 0)
            Cp = np.where(i > 0, Cc[ip, cols], 0.0)
            Sp = np.where(i > 0, Sc[ip, cols], 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                lo = (Sp + (t - Cp) * xq) / t
                up = ((Ci - t) * xq + (S - Si)) / (W - t)
            ok = ~bad
            out["q"][b, a, ok], out["lower"][b, a, ok], out["upper"][b, a, ok] = xq[ok], lo[ok], up[ok]
            if detail:
                tol = 4.0 * k * eps * W
                det["edge"][b, a] = ok & ((np.abs(Ci - t) <= tol) | (np.abs(Cp - t) <= tol))
                det["q_prev"][b, a, ok] = xs[ip, cols][ok]
                det["q_next"][b, a, ok] = xs[np.minimum(i + 1, xs.shape[0] - 1), cols][ok]
                scale = 2.0 * (k + 2) * eps * (A + W * np.abs(xq))
                det["bound_lower"][b, a, ok] = (scale / t)[ok]
                det["bound_upper"][b, a, ok] = (scale / (W - t))[ok]
    res = (out["q"], out["lower"], out["upper"], status)
    return res + (det,) if detail else res


def _check_levels(levels) -> np.ndarray:
    lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if lv.ndim != 1 or not 1 <= lv.size <= MAX_LEVELS:
        raise ValueError(f"levels must be 1 to {MAX_LEVELS} numbers, got shape {lv.shape}")
    if not ((lv > 0.0) & (lv < 1.0)).all():
        raise ValueError(f"every level must lie inside (0, 1), got {lv.tolist()}")
    return lv


def weighted_quantiles(values, weights, levels, cuda: bool | None = None) -> PredictiveQuantiles:
    """Quantiles and tail means over axis 1 of a statistic `values` (B, k, ...), numpy or torch, with `weights` (B, k) or
    None (unit weights), at the levels 0 < p < 1 (at most 32, in any order): the definition at the head of this module.
    cuda=None: psh_weighted_quantiles when values is a HIP float32 tensor (read where it lies), the numpy twin otherwise;
    cuda=True: the device (values are rounded to float32 and uploaded if they are not there; no host fallback, and
    k > 16384 raises); cuda=False: the twin, which takes any k."""
    lv = _check_levels(levels)
    on_device = _is_torch(values) and values.is_cuda
    if not _is_torch(values):
        values = np.asarray(values)
    if values.ndim < 2 or min(values.shape) < 1:
        raise ValueError(f"values must be (B, k, ...) and not empty, got shape {tuple(values.shape)}")
    B, k = int(values.shape[0]), int(values.shape[1])
    tail = tuple(int(n) for n in values.shape[2:])
    if weights is not None and tuple(weights.shape) != (B, k):
        raise ValueError(f"weights must be (B, k) = ({B}, {k}), got {tuple(weights.shape)}")
    if cuda is None:
        cuda = bool(on_device and str(values.dtype) == "torch.float32")
    if cuda:
        import torch
        from . import _native
        if k > _native.PSH_MAX_K:
            raise _native.NativeLibraryError(f"psh_weighted_quantiles takes k <= {_native.PSH_MAX_K} paths, got {k} "
                                             "(cuda=False sorts any k on the host)")
        if not on_device:
            if not torch.cuda.is_available():
                raise _native.NativeLibraryError("cuda=True needs a HIP device, and there is no host fallback under it")
            values = torch.as_tensor(np.ascontiguousarray(values, dtype=np.float32) if not _is_torch(values) else values).to("cuda")
        v = values.to(torch.float32).contiguous()
        w = None
        if weights is not None:
            w = weights if _is_torch(weights) else torch.from_numpy(np.array(weights, dtype=np.float64))
            w = w.to(device=v.device, dtype=torch.float64).contiguous()
        q, lo, up, st = _native.weighted_quantiles(v, w, lv)
        return PredictiveQuantiles(lv, q.cpu().numpy(), lo.cpu().numpy(), up.cpu().numpy(), st.cpu().numpy())
    V = values.detach().cpu().numpy() if _is_torch(values) else values
    V = np.ascontiguousarray(V, dtype=np.float32).reshape(B, k, -1)
    Wt = None
    if weights is not None:
        Wt = weights.detach().cpu().numpy() if _is_torch(weights) else np.asarray(weights)
        Wt = np.ascontiguousarray(Wt, dtype=np.float64)
    q, lo, up, st = _host_quantiles(V, Wt, lv)
    shape = (B, lv.size) + tail
    return PredictiveQuantiles(lv, q.reshape(shape), lo.reshape(shape), up.reshape(shape), st)
