"""Time-separated nearest windows: the exclusion zone of subsequence search on the list a scan returns (README "Separated
neighbours").  The numpy twin of psh_separate_topk (shadowing_amd/csrc/psh_separate.hip) and the one function that routes
between the two.

The definition (shared with the kernel and include/psh.h).  One query has a list of K entries (d_i, r_i, t_i), i = 0 .. K-1,
in the order given; the scans hand it over ascending in (d, r, t).  The rule reads positions and indices only, never d.
delta >= 0 is an integer number of samples:

    keep_i  =  r_i >= 0  and  there is no j < i with keep_j, r_j == r_i and |t_j - t_i| <= delta

Row b of the result holds the first k kept entries in list order: `distances` (the input's bits, NaN included), `indices`
[r, t], `positions` (int32, the position i in the input list).  `count[b]` is the number kept among all K (it may exceed k);
`status[b]` is STATUS_SHORT when count[b] < k, and the slots past the count then hold +inf, (-1, -1), -1.

Whether entry i is kept depends on the entries before i only (prefix exactness): the kept entries of an exact top-K list are
the first kept entries of the greedy walk over ALL windows, so count >= k makes the answer exact whatever K was.  An entry
with r < 0 is padding: never kept, suppressing nothing.  Integers only: two calls give identical bits, on either route.
"""
from __future__ import annotations

from bisect import bisect_left, insort
from dataclasses import dataclass

import numpy as np

__all__ = ["separate_topk", "Separated", "STATUS_OK", "STATUS_SHORT"]

STATUS_OK, STATUS_SHORT = 0, 1


@dataclass
class Separated:
    """What separate_topk returns: numpy arrays from the twin, HIP tensors from the device."""
    distances: object     # (B, k) float32
    indices: object       # (B, k, 2) int32
    positions: object     # (B, k) int32
    count: object         # (B,) int32
    status: object        # (B,) int32


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _kept_positions(r, t, delta: int) -> list:
    """The positions the rule keeps in one list, ascending: the greedy walk, the kept times of every row held sorted."""
    rows: dict = {}
    kept = []
    for i, (ri, ti) in enumerate(zip(r, t)):
        if ri < 0:
            continue
        times = rows.get(ri)
        if times is None:
            rows[ri] = [ti]
            kept.append(i)
            continue
        p = bisect_left(times, ti)
        if (p < len(times) and times[p] - ti <= delta) or (p > 0 and ti - times[p - 1] <= delta):
            continue
        insort(times, ti)
        kept.append(i)
    return kept


def _host_separate(d32: np.ndarray, idx: np.ndarray, k: int, delta: int) -> Separated:
    B, K = d32.shape
    out_d = np.full((B, k), np.inf, dtype=np.float32)
    out_i = np.full((B, k, 2), -1, dtype=np.int32)
    out_p = np.full((B, k), -1, dtype=np.int32)
    count = np.zeros(B, dtype=np.int32)
    for b in range(B):
        kept = _kept_positions(idx[b, :, 0].tolist(), idx[b, :, 1].tolist(), delta)
        count[b] = len(kept)
        pos = np.asarray(kept[:k], dtype=np.int64)
        n = len(pos)
        out_d[b, :n].view(np.int32)[...] = d32[b, pos].view(np.int32)      # (bits, not numbers: a NaN keeps its payload)
        out_i[b, :n] = idx[b, pos]
        out_p[b, :n] = pos
    return Separated(out_d, out_i, out_p, count, np.where(count < k, STATUS_SHORT, STATUS_OK).astype(np.int32))


def separate_topk(distances, indices, k: int, delta: int, cuda: bool | None = None) -> Separated:
    """The first `k` entries of every query's list that an exclusion zone of `delta` samples keeps: the definition at the
    head of this module.  distances (B, K) float32 and indices (B, K, 2) int32 = [r, t], numpy or torch.
    cuda=None: psh_separate_topk when distances is a HIP tensor (read where it lies), the numpy twin otherwise;
    cuda=True: the device (the list is uploaded if it is not there; no host fallback, and K > 16384 raises);
    cuda=False: the twin, which takes any K.  The device gives HIP tensors, the twin numpy arrays."""
    on_device = _is_torch(distances) and distances.is_cuda
    if not _is_torch(distances):
        distances = np.asarray(distances)
    if not _is_torch(indices):
        indices = np.asarray(indices)
    if len(distances.shape) != 2 or min(distances.shape) < 1 or tuple(indices.shape) != tuple(distances.shape) + (2,):
        raise ValueError(f"distances must be (B, K) and not empty, indices (B, K, 2); got shapes {tuple(distances.shape)} "
                         f"and {tuple(indices.shape)}")
    K = int(distances.shape[1])
    if isinstance(k, bool) or isinstance(delta, bool) or int(k) != k or int(delta) != delta:
        raise ValueError(f"separate_topk: k and delta must be integers, got {k!r} and {delta!r}")
    k, delta = int(k), int(delta)
    if not 1 <= k <= K:
        raise ValueError(f"separate_topk: k must lie in 1 .. K = {K}, got {k}")
    if not 0 <= delta < 2 ** 31:
        raise ValueError(f"separate_topk: delta must lie in 0 .. 2^31 - 1, got {delta}")
    if cuda is None:
        cuda = bool(on_device)
    if cuda:
        import torch
        from . import _native
        if K > _native.PSH_MAX_K:
            raise _native.NativeLibraryError(f"psh_separate_topk takes lists of K <= {_native.PSH_MAX_K} entries, got {K} "
                                             "(cuda=False walks any K on the host)")
        if not on_device and not torch.cuda.is_available():
            raise _native.NativeLibraryError("cuda=True needs a HIP device, and there is no host fallback under it")
        dev = distances.device if on_device else torch.device("cuda", torch.cuda.current_device())
        d = torch.as_tensor(distances).to(dev).to(torch.float32).contiguous()
        i = torch.as_tensor(indices).to(dev).to(torch.int32).contiguous()
        return Separated(*_native.separate_topk(d, i, k, delta))
    d = distances.detach().cpu().numpy() if _is_torch(distances) else distances
    i = indices.detach().cpu().numpy() if _is_torch(indices) else indices
    return _host_separate(np.ascontiguousarray(d, dtype=np.float32), np.ascontiguousarray(i, dtype=np.int32), k, delta)
