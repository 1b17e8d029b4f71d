"""Numpy twins of the device primitives of psh_wave.h and psh_sort_lds.h (and fast_div, unit_queue), written from the
headers' own words: the ORDER of every operation is the header's, so a result is comparable bit for bit.

Conventions.  A "wave array" has 64 lanes on its last axis.  Floating-point arithmetic is numpy's on arrays of the
operand's own dtype: one IEEE-754 rounding per operation, nothing fused.  Two things IEEE leaves open are fixed here
so that bits can be compared:

* the bits of a NaN result (inf + -inf gives another sign on the host than on the device): `bits()` maps every NaN
  to the canonical quiet NaN before a comparison -- WHICH values are NaN is compared exactly;
* the sign of min(+0, -0): fmin_ / fmax_ order -0 below +0 (IEEE 754-2019 minimumNumber / maximumNumber), which is
  what the device's v_min / v_max instructions do.  Both still drop a NaN operand, as fminf / fmaxf.
"""
from __future__ import annotations

import numpy as np

WAVE = 64
RUN, GRP = 16, 8                     # PSH_QNT_RUN, PSH_QNT_GRP


# ------------------------------------------------------------------------------------------ bits
def bits(a: np.ndarray) -> np.ndarray:
    """The raw words of `a` (uint32 / uint64), every NaN as the canonical quiet NaN."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))
    if a.dtype == np.float64:
        return np.where(np.isnan(a), np.uint64(0x7ff8000000000000), a.view(np.uint64))
    if a.dtype.itemsize == 4:
        return a.view(np.uint32)
    return a.view(np.uint64)


# ------------------------------------------------------------------------------------------ the operators
def op_sum(a, b):
    with np.errstate(all="ignore"):
        return a + b                                  # integers wrap, floats round once


def op_or(a, b):
    return a | b


def fmin_(a, b):
    if a.dtype.kind != "f":
        return np.minimum(a, b)
    with np.errstate(invalid="ignore"):
        take_a = np.isnan(b) | (a < b) | ((a == b) & np.signbit(a))
    return np.where(take_a & ~np.isnan(a), a, np.where(np.isnan(b), a, b))


def fmax_(a, b):
    if a.dtype.kind != "f":
        return np.maximum(a, b)
    with np.errstate(invalid="ignore"):
        take_a = np.isnan(b) | (a > b) | ((a == b) & ~np.signbit(a))
    return np.where(take_a & ~np.isnan(a), a, np.where(np.isnan(b), a, b))


OPS = {"sum": op_sum, "or": op_or, "min": fmin_, "max": fmax_}


# ------------------------------------------------------------------------------------------ wave reductions
def wave_reduce(v: np.ndarray, op) -> np.ndarray:
    """The butterfly v[i] = op(v[i], v[i ^ off]), off = 32, 16, .. 1; every lane's own result."""
    v = np.array(v)
    lanes = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., lanes ^ off])
    return v


def wave_minmax(lo: np.ndarray, hi: np.ndarray):
    lanes = np.arange(WAVE)
    lo, hi = np.array(lo), np.array(hi)
    for off in (32, 16, 8, 4, 2, 1):
        lo, hi = fmin_(lo, lo[..., lanes ^ off]), fmax_(hi, hi[..., lanes ^ off])
    return lo, hi


def wave_sum_dpp(x: np.ndarray) -> np.ndarray:
    """Pairs, quads, half rows, rows of 16 -- within each stage both partners hold the same bits, so this is the binary
    tree over adjacent lanes --, then (r0 + r1) + (r2 + r3) over the four rows.  One float32 per wave."""
    v = np.array(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        while v.shape[-1] > 4:
            v = v[..., 0::2] + v[..., 1::2]
        return (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])


def wave_max_nonneg(x: np.ndarray) -> np.ndarray:
    """The numeric maximum of inputs from {+0, denormals, normals, +inf} (the contract excludes negatives and NaN)."""
    x = np.asarray(x, dtype=np.float32)
    assert not np.isnan(x).any() and not np.signbit(x).any()
    return x.max(axis=-1)


# ------------------------------------------------------------------------------------------ wave scans
def wave_scan_inclusive(v: np.ndarray) -> np.ndarray:
    """Hillis-Steele: v[i] += v[i - off] for i >= off, off = 1, 2, .. 32, in the operand's own arithmetic."""
    v = np.array(v)
    with np.errstate(all="ignore"):
        for off in (1, 2, 4, 8, 16, 32):
            t = v.copy()
            t[..., off:] = v[..., off:] + v[..., :-off]
            v = t
    return v


def wave_scan_inclusive_dpp(v: np.ndarray) -> np.ndarray:
    """The int32 cumulative sum in lane order, wrapping."""
    w = np.asarray(v).view(np.uint32).astype(np.uint64)
    return (np.cumsum(w, axis=-1) & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)


def wave_total_dpp(v: np.ndarray) -> np.ndarray:
    return wave_scan_inclusive_dpp(v)[..., 63]


def pack16(c: np.ndarray) -> np.ndarray:
    """The callers' packed counters: c | c << 16."""
    c = np.asarray(c, dtype=np.uint32)
    return (c | (c << np.uint32(16))).view(np.int32)


# ------------------------------------------------------------------------------------------ the workgroup tree
def block_reduce(v: np.ndarray, op) -> np.ndarray:
    """v: [.., WAVES, 64].  The butterfly per wave, red[w] = lane 0's result, then red[0] op red[1] op .. left to right,
    starting AT red[0]."""
    red = np.asarray(v)                  # lane 0 of the butterfly: lane i < off holds v[i] op v[i + off] after each step
    for off in (32, 16, 8, 4, 2, 1):
        red = op(red[..., :off], red[..., off:2 * off])
    red = red[..., 0]
    s = red[..., 0]
    for u in range(1, red.shape[-1]):
        s = op(s, red[..., u])
    return s


# ------------------------------------------------------------------------------------------ the rank search
def rank_find(hist: np.ndarray, rank: int):
    """(bucket, before, count) of the bucket holding the rank-th (1-based) entry, or None: an owner exists iff
    1 <= rank <= total."""
    cum = np.cumsum(np.asarray(hist, dtype=np.uint64))
    if rank < 1 or rank > int(cum[-1]):
        return None
    b = int(np.searchsorted(cum, np.uint64(rank), side="left"))       # first index with cum >= rank
    return b, int(cum[b]) - int(hist[b]), int(hist[b])


def bucket_upper_edge(kmin: int, kmax: int, bucket: int, shift: int) -> int:
    e = int(kmin) + ((int(bucket) + 1) << int(shift)) - 1
    return int(kmax) if e > int(kmax) else e


# ------------------------------------------------------------------------------------------ keys
def qnt_key(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    u = np.where(x == 0.0, np.float32(0.0), x).astype(np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def qnt_value(key: np.ndarray) -> np.ndarray:
    key = np.asarray(key, dtype=np.uint32)
    return np.where(key & np.uint32(0x80000000), key & np.uint32(0x7fffffff), ~key).astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------ the sort network
def qnt_phys(i):
    return i + (i >> 4)


def _cmpex(v, r0, r1, desc):
    a, c = v[:, r0], v[:, r1]
    sw = (a > c) != desc
    v[:, r0], v[:, r1] = np.where(sw, c, a), np.where(sw, a, c)


def _sort_first(ent, n2, NB):
    E = 1 << NB
    g = np.arange(n2 >> NB)
    idx = qnt_phys((g[:, None] << NB) + np.arange(E)[None, :])
    v = ent[idx]                                                   # [group, r, batch]
    for s in range(1, NB + 1):
        for b in range(s - 1, -1, -1):
            for r in range(E):
                if not r & (1 << b):
                    desc = np.full(g.shape, ((r >> s) & 1) != 0) if s < NB else (g & 1) != 0
                    _cmpex(v, r, r | (1 << b), desc[:, None])
    ent[idx] = v


def _sort_pass(ent, n2, N, lo, s):
    E = 1 << N
    g = np.arange(n2 >> N)
    base = ((g >> lo) << (lo + N)) | (g & ((1 << lo) - 1))
    desc = ((base >> s) & 1) != 0
    idx = qnt_phys(base[:, None] | (np.arange(E)[None, :] << lo))
    v = ent[idx]
    for b in range(N - 1, -1, -1):
        for r in range(E):
            if not r & (1 << b):
                _cmpex(v, r, r | (1 << b), desc[:, None])
    ent[idx] = v


def qnt_sort(entries: np.ndarray, NB: int) -> np.ndarray:
    """The network of qnt_sort<NB, THREADS> on `entries` [batch, n2] (any ordered dtype), n2 a power of two >= 2^NB: runs
    of 2^NB in registers (qnt_sort_first), then for each phase s passes of nb <= NB index bits, descending where bit s of
    the group's base index is set; entry i lies at i + i / 16 throughout.  (THREADS only says which thread takes which
    group of a pass: the groups of a pass are disjoint, so it does not enter the result.)"""
    entries = np.asarray(entries)
    batch, n2 = entries.shape
    assert n2 >= (1 << NB) and n2 & (n2 - 1) == 0
    ent = np.zeros((qnt_phys(n2 - 1) + 1, batch), dtype=entries.dtype)
    ent[qnt_phys(np.arange(n2))] = entries.T
    _sort_first(ent, n2, NB)
    s = NB + 1
    while (1 << s) <= n2:
        hi = s
        while hi > 0:
            nb = min(hi, NB)
            lo = hi - nb
            _sort_pass(ent, n2, nb, lo, s)
            hi = lo
        s += 1
    return np.ascontiguousarray(ent[qnt_phys(np.arange(n2))].T)


# ------------------------------------------------------------------------------------------ the fixed-order scan
def _seq_exclusive(v: np.ndarray, is_max: bool):
    """v: [n, m] float64: the exclusive prefix along axis 1 accumulated sequentially from 0.0, and the totals."""
    acc = np.zeros(v.shape[0], dtype=np.float64)
    ex = np.empty_like(v)
    with np.errstate(all="ignore"):
        for u in range(v.shape[1]):
            ex[:, u] = acc
            acc = np.fmax(acc, v[:, u]) if is_max else acc + v[:, u]
    return ex, acc


def qnt_scan(mine: np.ndarray, is_max: bool):
    """qnt_scan<THREADS, MAX> of one value per thread (THREADS = len(mine)): sequential over the 16 threads of a run, the
    8 runs of a group, then the groups; returns ((g[grp] + r[run]) + x[tid] per thread, the total g[GROUPS])."""
    mine = np.asarray(mine, dtype=np.float64)
    threads = mine.shape[0]
    runs, groups = threads // RUN, threads // RUN // GRP
    x, r = _seq_exclusive(mine.reshape(runs, RUN), is_max)
    r, g = _seq_exclusive(r.reshape(groups, GRP), is_max)
    g, total = _seq_exclusive(g.reshape(1, groups), is_max)
    x, r, g = x.reshape(-1), r.reshape(-1), g.reshape(-1)
    tid = np.arange(threads)
    run, grp = tid // RUN, tid // RUN // GRP
    with np.errstate(all="ignore"):
        if is_max:
            return np.fmax(np.fmax(g[grp], r[run]), x), total[0]
        return (g[grp] + r[run]) + x, total[0]


# ------------------------------------------------------------------------------------------ divide and queue
def fast_div_magic(d: int) -> int:
    """floor(2^32 / d) as the host computes it (0 for d = 1, which fast_div never multiplies by)."""
    return (1 << 32) // int(d) if int(d) > 1 else 0


def fast_div(u: int, d: int) -> int:
    return int(u) // int(d)


def unit_queue(n: int, grid: int):
    """The blocks' shares [lo, hi) of n units."""
    b = np.arange(grid, dtype=object)
    return np.array([int(n) * int(i) // grid for i in b], dtype=np.uint64), np.array([int(n) * (int(i) + 1) // grid for i in b], dtype=np.uint64)
