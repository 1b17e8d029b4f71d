"""Scores of weighted predictive ensembles against what happened: the CRPS (continuous ranked probability score), the PIT
(probability integral transform) and the mean, for a whole grid of weightings at once -- what says whether the conditional
distributions of the k shadowing paths are any good, and which eta and k make them best.

One column is one (b, i) of values (B, k, m), rounded to float32; y = obs[b, i], float32, is the realised statistic.  Weight
set e of query b is weights[e, b, :], float64, used as given and never renormalised (None: one set, w_j = 1); at most
MAX_SETS = 64 sets.  For one column and one set, keep the paths with w > 0, order them by (value ascending, path index
ascending), write x_(0..n-1), w_(i) for the sorted values and weights, all arithmetic in double:

    C_i = sum_{l<=i} w_(l)      S_i = sum_{l<=i} w_(l) x_(l)      W = C_{n-1} (as computed)
    mean   = S_{n-1} / W
    pit_lo = (sum of w_(i) with x_(i) <  y) / W          F(y-)
    pit_hi = (sum of w_(i) with x_(i) <= y) / W          F(y)
    c_i    = min(max(y, x_(i)), x_(i+1))
    crps   = (x_(0) - y)_+ + (y - x_(n-1))_+
             + (1 / W^2) sum_{i=0}^{n-2} [ C_i^2 (c_i - x_(i)) + (W - C_i)^2 (x_(i+1) - c_i) ]

crps is the integral of (F(z) - 1[z >= y])^2 written gap by gap: every term is non-negative, so nothing cancels.  It equals
E|X - y| - 1/2 E|X - X'| under p = w / W.  It is a proper score: its mean over dates is lowest, in expectation, for the
weighting the outcomes are drawn from.  The PIT is uniform over dates exactly when the forecasts are calibrated.

A path of weight exactly 0 contributes nothing, whatever its value.  A non-finite value at a positive weight makes its
column's four results NaN for that set and sets STATUS_NONFINITE in status[e, b]; a non-finite or negative weight, or W not
> 0, makes all of (e, b) NaN and sets STATUS_WEIGHTS (the values are then not looked at); a non-finite obs[b, i] makes the
column NaN for every set and sets STATUS_OBS in every status[e, b].  -0.0 and +0.0 are one value.  So crps >= 0, n = 1 gives
|x - y|, pit_lo <= pit_hi with equality unless a weighted path equals y, scaling a set's weights by a power of two changes
no bit, and a set's results do not depend on which other sets ride the call.

On a HIP float32 tensor the work is psh_score_ensemble's (the method heads shadowing_amd/csrc/psh_scoring.hip): one in-LDS
sort per column serves every weight set, and only the four (E, B, m) results come to the host.  Everywhere else the numpy
twin below computes the same definition (cumulative sums in sorted order, one after the other).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .quantiles import _is_torch

MAX_SETS = 64
STATUS_OK, STATUS_NONFINITE, STATUS_WEIGHTS, STATUS_OBS = 0, 1, 2, 4


@dataclass
class EnsembleScore:
    """crps, pit_lo, pit_hi, mean: float64, the set axes first, then the queries, then the trailing dimensions of the
    statistic -- (E, B, ...), (B, ...) when the weights had no set axis, (len(etas), len(ks), B, ...) from
    PathShadowing.score(), which also fills `etas` and `ks`; status: int32, the set axes and the queries."""
    crps: np.ndarray
    pit_lo: np.ndarray
    pit_hi: np.ndarray
    mean: np.ndarray
    status: np.ndarray
    etas: tuple | None = None
    ks: tuple | None = None

    @property
    def _set_ndim(self) -> int:
        return self.status.ndim - 1

    def mean_crps(self) -> np.ndarray:
        """The mean CRPS over the queries whose column is finite: the set axes, then the statistic's dimensions (NaN where
        no query is finite)."""
        ok = np.isfinite(self.crps)
        n = ok.sum(axis=self._set_ndim)
        total = np.where(ok, self.crps, 0.0).sum(axis=self._set_ndim)
        return np.where(n > 0, total / np.maximum(n, 1), np.nan)

    def best(self):
        """The set with the lowest mean_crps() for every column of the statistic: an index array shaped like the statistic's
        dimensions, or the pair (index into etas, index into ks) of such arrays when the set axis is (len(etas), len(ks))."""
        nd = self._set_ndim
        if nd == 0:
            raise ValueError("best(): the weights had no set axis")
        mc = self.mean_crps()
        sets = mc.shape[:nd]
        flat = np.where(np.isnan(mc), np.inf, mc).reshape((-1,) + mc.shape[nd:]).argmin(axis=0)
        return flat if nd == 1 else tuple(np.unravel_index(flat, sets))

    def pit(self, u=None) -> np.ndarray:
        """pit_lo + u (pit_hi - pit_lo): the middle of the jump for u = 0.5 (the default); the randomised PIT, uniform for
        calibrated forecasts whatever the ties, for an array of uniforms that broadcasts against pit_lo."""
        u = 0.5 if u is None else np.asarray(u, dtype=np.float64)
        return self.pit_lo + u * (self.pit_hi - self.pit_lo)


def _host_scores(values: np.ndarray, weights: np.ndarray | None, obs: np.ndarray):
    """The numpy twin on (B, k, m) float32, (E, B, k) float64 or None, (B, m) float32: crps, pit_lo, pit_hi, mean (E, B, m)
    and status (E, B)."""
    B, k, m = values.shape
    E = 1 if weights is None else weights.shape[0]
    out = {n: np.full((E, B, m), np.nan) for n in ("crps", "pit_lo", "pit_hi", "mean")}
    status = np.zeros((E, B), dtype=np.int32)
    cols = np.arange(m)
    for b in range(B):
        y = obs[b].astype(np.float64) + 0.0                     # (-0.0 + 0.0 = +0.0: the zeros are one value)
        y_ok = np.isfinite(y)
        if not y_ok.all():
            status[:, b] |= STATUS_OBS
        x_all = values[b].astype(np.float64) + 0.0
        order_all = np.argsort(x_all, axis=0, kind="stable")    # ties by path index; one sort serves every set
        xs_all = np.take_along_axis(x_all, order_all, axis=0)
        for e in range(E):
            w = np.ones(k) if weights is None else weights[e, b]
            if not np.isfinite(w).all() or (w < 0).any() or not (w > 0).any():
                status[e, b] |= STATUS_WEIGHTS
                continue
            keep = (w > 0)[order_all]                           # (k, m): the same n paths in every column
            n = int(keep[:, 0].sum())
            xs = xs_all.T[keep.T].reshape(m, n).T
            ws = w[order_all].T[keep.T].reshape(m, n).T
            bad = ~np.isfinite(xs).all(axis=0)
            if (bad & y_ok).any():
                status[e, b] |= STATUS_NONFINITE
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                Cc = np.cumsum(ws, axis=0)
                Sc = np.cumsum(ws * xs, axis=0)
                W = Cc[-1]
                if not (W > 0).all():
                    status[e, b] |= STATUS_WEIGHTS
                    continue
                xa, xb, Ci = xs[:-1], xs[1:], Cc[:-1]
                c = np.minimum(np.maximum(y, xa), xb)
                terms = Ci * Ci * (c - xa) + (W - Ci) * (W - Ci) * (xb - c)
                G = np.cumsum(terms, axis=0)[-1] if n > 1 else np.zeros(m)
                crps = np.maximum(xs[0] - y, 0.0) + np.maximum(y - xs[-1], 0.0) + G / (W * W)
                n_lo, n_hi = (xs < y).sum(axis=0), (xs <= y).sum(axis=0)
                lo = np.where(n_lo > 0, Cc[np.maximum(n_lo - 1, 0), cols], 0.0) / W
                hi = np.where(n_hi > 0, Cc[np.maximum(n_hi - 1, 0), cols], 0.0) / W
                mean = Sc[-1] / W
            ok = ~bad & y_ok
            out["crps"][e, b, ok], out["pit_lo"][e, b, ok] = crps[ok], lo[ok]
            out["pit_hi"][e, b, ok], out["mean"][e, b, ok] = hi[ok], mean[ok]
    return out["crps"], out["pit_lo"], out["pit_hi"], out["mean"], status


def _host(a, dtype):
    a = a.detach().cpu().numpy() if _is_torch(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=dtype)


def score_ensemble(values, weights, obs, cuda: bool | None = None) -> EnsembleScore:
    """CRPS, PIT and mean over axis 1 of a statistic `values` (B, k, ...), numpy or torch, against `obs` (B, ...), under
    `weights` None (unit weights), (B, k) or (E, B, k) with E <= 64 weight sets: the definition at the head of this module.
    cuda=None: psh_score_ensemble when values is a HIP float32 tensor (read where it lies), the numpy twin otherwise;
    cuda=True: the device (values are rounded to float32 and uploaded if they are not there; no host fallback, and
    k > 16384 raises); cuda=False: the twin, which takes any k."""
    on_device = _is_torch(values) and values.is_cuda
    if not _is_torch(values):
        values = np.asarray(values)
    if values.ndim < 2 or min(values.shape) < 1:
        raise ValueError(f"values must be (B, k, ...) and not empty, got shape {tuple(values.shape)}")
    B, k = int(values.shape[0]), int(values.shape[1])
    tail = tuple(int(n) for n in values.shape[2:])
    if tuple(obs.shape) != (B,) + tail:
        raise ValueError(f"obs must be (B, ...) = {(B,) + tail}, got {tuple(obs.shape)}")
    set_axis = weights is not None and len(weights.shape) == 3
    if weights is not None:
        if tuple(weights.shape)[-2:] != (B, k) or len(weights.shape) not in (2, 3):
            raise ValueError(f"weights must be (B, k) or (E, B, k) with (B, k) = ({B}, {k}), got {tuple(weights.shape)}")
        if set_axis and not 1 <= weights.shape[0] <= MAX_SETS:
            raise ValueError(f"1 to {MAX_SETS} weight sets, got {weights.shape[0]}")
    E = int(weights.shape[0]) if set_axis else 1
    if cuda is None:
        cuda = bool(on_device and str(values.dtype) == "torch.float32")
    if cuda:
        import torch
        from . import _native
        if k > _native.PSH_MAX_K:
            raise _native.NativeLibraryError(f"psh_score_ensemble takes k <= {_native.PSH_MAX_K} paths, got {k} "
                                             "(cuda=False sorts any k on the host)")
        if not on_device:
            if not torch.cuda.is_available():
                raise _native.NativeLibraryError("cuda=True needs a HIP device, and there is no host fallback under it")
            values = torch.as_tensor(np.ascontiguousarray(values, dtype=np.float32) if not _is_torch(values) else values).to("cuda")
        v = values.to(torch.float32).contiguous()
        y = (obs if _is_torch(obs) else torch.from_numpy(np.array(obs, dtype=np.float32)))
        y = y.to(device=v.device, dtype=torch.float32).contiguous()
        w = None
        if weights is not None:
            w = weights if _is_torch(weights) else torch.from_numpy(np.array(weights, dtype=np.float64))
            w = w.to(device=v.device, dtype=torch.float64).reshape(E, B, k).contiguous()
        res = [t.cpu().numpy() for t in _native.score_ensemble(v, w, y)]
    else:
        Wt = None if weights is None else _host(weights, np.float64).reshape(E, B, k)
        res = list(_host_scores(_host(values, np.float32).reshape(B, k, -1), Wt, _host(obs, np.float32).reshape(B, -1)))
    lead = (E, B) if set_axis else (B,)
    return EnsembleScore(*(r.reshape(lead + tail) for r in res[:4]), res[4].reshape(lead))
