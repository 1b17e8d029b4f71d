"""Inputs the CPU tests of the twins and the GPU tests of the primitives share: the float list of the key map and the
histograms and ranks of the rank search."""
from __future__ import annotations

import numpy as np


def key_floats() -> np.ndarray:
    """Distinct float32 values in strictly increasing order, -inf .. +inf with both signs' denormals, +0 in the middle
    (-0 is the caller's to add: it shares +0's key)."""
    pos = np.array([0x00000001, 0x00000002, 0x007fffff, 0x00800000, 0x00800001, 0x33800000, 0x3f7fffff, 0x3f800000, 0x3f800001,
                    0x40490fdb, 0x4cbebc20, 0x7f7ffffe, 0x7f7fffff, 0x7f800000], dtype=np.uint32)      # smallest denormal .. FLT_MAX, +inf
    neg = (pos | np.uint32(0x80000000))[::-1]
    x = np.concatenate([neg, np.zeros(1, dtype=np.uint32), pos]).view(np.float32)
    assert np.all(np.diff(x.astype(np.float64)) > 0)
    return x


def rank_histograms(per: int, seed: int = 0) -> list[np.ndarray]:
    """Histograms of 64 per counters: the shapes at which a lane scan, a boundary or an empty counter can go wrong."""
    g = np.random.default_rng(seed)
    nb = 64 * per
    out = []

    def one(pairs):
        h = np.zeros(nb, dtype=np.uint32)
        for b, c in pairs:
            h[b] = c
        return h
    out.append(one([(0, 7)]))                                             # all mass in the first bucket
    out.append(one([(nb // 2 + per // 3, 5)]))                            # ... a middle one
    out.append(one([(nb - 1, 3)]))                                        # ... the last
    h = np.zeros(nb, dtype=np.uint32)                                     # one counter per lane
    h[per * np.arange(64) + g.integers(0, per, 64)] = g.integers(1, 9, 64)
    out.append(h)
    h = np.zeros(nb, dtype=np.uint32)                                     # runs of empty lanes between occupied ones
    for lane in (3, 4, 15, 16, 31, 32, 47, 48, 63):
        h[per * lane + g.integers(0, per, 2)] = g.integers(1, 5, 2)
    out.append(h)
    out.append(np.zeros(nb, dtype=np.uint32))                             # all zero
    h = np.zeros(nb, dtype=np.uint32)                                     # random sparse
    idx = g.choice(nb, size=max(4, nb // 10), replace=False)
    h[idx] = g.integers(1, 1000, idx.size)
    out.append(h)
    out.append(g.integers(0, 3, nb).astype(np.uint32))                    # dense, with zeros and ties
    h = np.zeros(nb, dtype=np.uint32)                                     # a total above 2^31 (below 2^32)
    h[[0, nb // 3, nb - 1]] = [1 << 30, (1 << 30) + 5, (1 << 30) - 1]
    h[nb // 2] = 17
    out.append(h)
    return out


def rank_list(hist: np.ndarray, limit: int = 160) -> np.ndarray:
    """0, 1, every cumulative boundary c and c + 1, total, total + 1 and 0xffffffff (a dense histogram's boundaries thinned
    to `limit`, the first and last kept)."""
    cum = np.unique(np.cumsum(hist.astype(np.uint64)))
    if cum.size > limit:
        cum = np.unique(np.concatenate([cum[:8], cum[-8:], cum[:: cum.size // (limit - 16) + 1]]))
    total = int(hist.astype(np.uint64).sum())
    r = np.concatenate([[0, 1, total, total + 1, 0xffffffff], cum, cum + 1]).astype(np.uint64)
    return np.unique(r[r <= 0xffffffff]).astype(np.uint32)


# ---------------------------------------------------------------------------------- the long-window front end (psh_long.h)
LONG_NVALID = (1, 31, 32, 33, 512, 1023, 1024)
LONG_OPERAND_W = (26, 126, 256)
LONG_TABLE_CASES = tuple((nq, W) for nq in (1, 3) for W in (26, 64, 126, 256))        # the buckets 6, 6, 10, 18 ...
LONG_TABLE_W14 = 190                                                                   # ... and 14
LONG_EXACT_W = (26, 33, 34, 127, 256)
LONG_BOUND_SEXP = (-60, 0, 3, 60)


def long_stage_cases():
    """(ensemble [R, T], T, [(row, seg_start, nfloat)]) lists: rows at odd float offsets (T odd), a row shorter than the
    segment, a last segment of five floats with the next row behind it in memory, a first and a later row.  The ensemble is
    followed by a margin of a whole segment, so that no load leaves the allocation whatever the range check does."""
    g = np.random.default_rng(11)
    out = []
    for T, cases in ((1029, [(0, 0, 1023 + 34), (3, 0, 1023 + 256), (0, 1024, 1023 + 64), (2, 1024, 1023 + 256)]),
                     (700, [(0, 0, 1023 + 126), (4, 0, 1023 + 33)]),
                     (2301, [(1, 1024, 1023 + 126), (3, 2048, 1023 + 255)])):
        ds = g.standard_normal((6, T)).astype(np.float32)
        out.append((ds, T, cases))
    return out


def long_prefix_sums(seed: int) -> np.ndarray:
    """1280 float32 prefix sums of squares at the scale the kernels see (samples of a few units), not exact in float32"""
    g = np.random.default_rng(seed)
    return np.concatenate([[0.0], np.cumsum(g.standard_normal(1279) ** 2 * 9.0)]).astype(np.float32)


def long_tiles():
    """[(tile [64, 16], nvalid)]: random tiles, a NaN in a slot that exists and in one that does not, per nvalid"""
    g = np.random.default_rng(12)
    out = []
    for nv in LONG_NVALID:
        t = (g.standard_normal((64, 16)) * 100.0).astype(np.float32)
        t[0, 0] = np.nan                                   # window 0: exists for every nvalid
        t[63, 15] = np.nan                                 # window 1023: exists only when nvalid = 1024
        t[40, 9] = -1.0e6                                  # window 680, below everything: counts only when nvalid > 680
        out.append((t, nv))
    return out


def long_bound_inputs():
    """(est [64], nx [64]): est / nx around 1 / 6, a zero, an inf and a NaN estimate"""
    nx = np.float32(37.5) * (np.float32(1.0) + np.arange(64, dtype=np.float32) / np.float32(64.0))
    est = (nx * (np.float32(1.0 / 6.0) + (np.arange(64, dtype=np.float32) - 32) * np.float32(2.0 ** -20))).astype(np.float32)
    est[0], est[1], est[2] = 0.0, np.inf, np.nan
    return est, nx.astype(np.float32)
