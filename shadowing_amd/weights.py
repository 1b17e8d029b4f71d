"""The averaging weights of the k shadowing paths of a query, formed from their distances for a whole grid of (eta, k')
weightings at once: what weighted_moments, weighted_quantiles, score_ensemble and the hedged Monte Carlo take as given.

The definition (shared with shadowing_amd/csrc/psh_weights.hip and include/psh.h).  distances (B, k), float32; a grid of
widths `etas` and cut-offs 1 <= k' <= k `ks`; the result is (len(etas), len(ks), B, k) float64.  For one query and one set:

 1. Order the paths by (distance ascending as numbers, path index ascending): -0.0 and +0.0 are equal, a NaN of either sign
    comes after +inf, NaNs among themselves go by index.  This is np.argsort(kind="stable").
 2. The first k' paths are kept.  Every other path gets weight exactly 0.0.
 3. With d_j converted to double and s = 2.0 * (eta * eta) in double:
        z_j = -(d_j * d_j) / s        zmax = max of z over the kept paths (NaN if any kept z is NaN)
        a_j = z_j - zmax              e_j = exp(a_j)        Z = sum of e_j over the kept paths, in a fixed order
        w_j = e_j / Z
    d_j * d_j is exact (a float32 squared in double), so a_j is three IEEE operations and comes out bit-identical here and
    on the device; the two sides differ by exp (1 ulp each), the order of the sum and the division, which bounds
    |w_device - w_twin| by (2 k' + 16) 2^-53 w_twin + 2^-1070.
 4. eta = None is w_j = 1.0 / k' for the kept paths, whatever their distances.
 5. A NaN among the kept distances makes every kept weight of that set and query NaN, and so do kept distances that are
    all infinite; the consumers answer a NaN weight with their STATUS_WEIGHTS.  A NaN or inf past the cut-off is harmless.
 6. Two calls give identical bits, and a set's bits do not depend on which other sets ride the call.

For eta not None this is, bit for bit, what the stand-in `averaging.Softmax` gives on ascending float32 distances.

On a HIP float32 tensor the work is psh_softmax_weights' (the method heads psh_weights.hip): one workgroup per query sorts the
(key, index) entries in LDS -- or finds them in order, as every scan returns them -- and serves every set from that order.
"""
from __future__ import annotations

import numpy as np

__all__ = ["softmax_weights", "MAX_SETS"]

MAX_SETS = 64                   # PSH_SCORE_MAX_SETS: what one psh_score_ensemble call takes


def _is_torch(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def _grid(k: int, etas, ks):
    """(etas, ks) as tuples, checked as psh_softmax_weights checks them: ValueError for what the C entry rejects."""
    etas = tuple(None if eta is None else float(eta) for eta in etas)
    ks = (k,) if ks is None else tuple(int(n) for n in ks)
    if not etas or not ks:
        raise ValueError("softmax_weights: etas and ks must not be empty")
    if len(etas) * len(ks) > MAX_SETS:
        raise ValueError(f"softmax_weights: {len(etas)} etas x {len(ks)} ks = {len(etas) * len(ks)} weight sets, "
                         f"at most {MAX_SETS} a call")
    for eta in etas:
        if eta is not None and not eta > 0.0:                   # (NaN fails it too)
            raise ValueError(f"softmax_weights: every eta must be None or > 0, got {eta}")
    if min(ks) < 1 or max(ks) > k:
        raise ValueError(f"softmax_weights: every k' must lie in 1 .. k = {k}, got {list(ks)}")
    return etas, ks


def _host_weights(d32: np.ndarray, etas, ks) -> np.ndarray:
    """The numpy twin on (B, k) float32 distances and a checked grid: (len(etas), len(ks), B, k) float64."""
    B, k = d32.shape
    d = d32.astype(np.float64)
    order = np.argsort(d32, axis=1, kind="stable")
    w = np.zeros((len(etas), len(ks), B, k))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c, kc in enumerate(ks):
            near = order[:, :kc]
            dk = np.take_along_axis(d, near, axis=1)
            for a, eta in enumerate(etas):
                if eta is None or np.isinf(eta):
                    wk = np.full((B, kc), 1.0 / kc)
                else:
                    s = 2.0 * (eta * eta)
                    z = -(dk * dk) / s
                    e = np.exp(z - z.max(axis=1, keepdims=True))
                    wk = e / e.sum(axis=1, keepdims=True)
                np.put_along_axis(w[a, c], near, wk, axis=1)
    return w


def softmax_weights(distances, etas, ks=None, cuda: bool | None = None):
    """The (len(etas), len(ks), B, k) float64 weights of `distances` (B, k), numpy or torch, for every pair of a width in
    `etas` (None: the uniform weighting 1 / k') and a cut-off k' in `ks` (default [k]): the definition at the head of this
    module.  Anything that is not float32 is rounded to float32 first.
    cuda=None: psh_softmax_weights when distances is a HIP float32 tensor (read where it lies), the numpy twin otherwise;
    cuda=True: the device (distances are uploaded if they are not there; no host fallback, and k > 16384 raises);
    cuda=False: the twin, which takes any k.  The device gives a HIP tensor, the twin a numpy array."""
    on_device = _is_torch(distances) and distances.is_cuda
    if not _is_torch(distances):
        distances = np.asarray(distances)
    if len(distances.shape) != 2 or min(distances.shape) < 1:
        raise ValueError(f"distances must be (B, k) and not empty, got shape {tuple(distances.shape)}")
    B, k = int(distances.shape[0]), int(distances.shape[1])
    etas, ks = _grid(k, etas, ks)
    if cuda is None:
        cuda = bool(on_device and str(distances.dtype) == "torch.float32")
    if cuda:
        import torch
        from . import _native
        if k > _native.PSH_MAX_K:
            raise _native.NativeLibraryError(f"psh_softmax_weights takes k <= {_native.PSH_MAX_K} paths, got {k} "
                                             "(cuda=False sorts any k on the host)")
        if not on_device:
            if not torch.cuda.is_available():
                raise _native.NativeLibraryError("cuda=True needs a HIP device, and there is no host fallback under it")
            distances = torch.as_tensor(distances if _is_torch(distances) else np.ascontiguousarray(distances, dtype=np.float32)).to("cuda")
        d = distances.to(torch.float32).contiguous()
        return _native.softmax_weights(d, etas, ks).reshape(len(etas), len(ks), B, k)
    d = distances.detach().cpu().numpy() if _is_torch(distances) else distances
    return _host_weights(np.ascontiguousarray(d, dtype=np.float32), etas, ks)
