"""Matches planted at every row, segment and horizon edge of a scan (shared by tests/test_boundaries_cpu.py and
tests/test_gpu_boundaries.py; plant() and check() are numpy only).

Window t of a row is admissible when 0 <= t <= T - W - h, Tp = T - W - h + 1 windows a row.  plant() writes, for a few
queries, near-copies of the raw query at the admissible windows where a kernel's own bookkeeping changes -- the first and
last window of a lane's PSH_L = 16, of a wave-segment's PSH_SEG = 1024, of the row, of the ragged last segment -- and EXACT
copies (distance 0) where no window may be returned from: the start positions whose horizon is short, and one copy that
lies across two rows of the flat ensemble.  check() then turns a dropped edge window, an admitted inadmissible one or a
window read across rows into a certain failure that names the plant.

A unit of the scans' work queue is one segment of ONE row (psh_segment.h), so rows are not grouped and the first and last
unit are the plants (0, 0) and (R - 1, Tp - 1); only rows_kernel (one-window rows, T == W + h) takes a row per lane, and
there the edges are rows: ONE_WINDOW_ROWS."""
from __future__ import annotations

import numpy as np

from shadowing_amd import synthetic as syn

SEG, LANE = 1024, 16                 # PSH_SEG windows a (row, segment) unit, PSH_L windows a lane (psh_device.h)
ONE_WINDOW_ROWS = (0, 1, 15, 16, 17, 63, 64, 1023, 1024, 1025)      # ... and R - 2, R - 1: a row per lane, 64 lanes a wave

# geometry -> (Tp - base, h or None for W + 3); base: the multiple of 1024 (of 256 for rows shorter than half a segment)
# nearest to the route's own Tp
GEOMETRIES = {"full": (0, 0), "one": (1, 5), "short": (-1, None)}


def edge_windows(Tp: int) -> list:
    ts = {0, 1, LANE - 1, LANE, LANE + 1, SEG - 1, SEG, SEG + 1, Tp - SEG - 1, Tp - SEG, Tp - LANE - 1, Tp - LANE, Tp - 2, Tp - 1}
    return sorted(t for t in ts if 0 <= t < Tp)


def queries_of(B: int, extra=()) -> list:
    return sorted({0, B // 2, B - 1, *extra})


# A geometry that leaves its route returns to it with the least change of R (the residue of Tp stays).
# emb_dense_mx_B260, full and short: one segment a row (Tp = 1024, 1023) instead of the table's two, so all 512 x 1024 windows
# fit the 526 272 candidate slots a chunk of 130 queries has and the call goes exhaustive (path 1); from 514 rows on they do
# not (514 x 1024 + k = 526 436).
KEEP_ROUTE = {("emb_dense_mx_B260", "full"): dict(R=514), ("emb_dense_mx_B260", "short"): dict(R=514)}


def geometry(c: dict, geom: str) -> dict:
    """The route-table case `c` (R, T, W, h, k, B, flags, hint, emb) at one of GEOMETRIES: its T and h replaced."""
    c = dict(c)
    W = c["emb"][2] if c["emb"] else c["W"]
    off, h = GEOMETRIES[geom]
    h = W + 3 if h is None else h
    if c["T"] == W + c["h"]:                     # one-window rows stay one-window rows
        c["T"], c["h"] = W + h, h
        return c
    Tp0 = c["T"] - W - c["h"] + 1
    base = 256 if Tp0 < 512 else 1024 * int(round(Tp0 / 1024))
    c["T"], c["h"] = base + off + W + h - 1, h
    return c


def route_case(name: str, geom: str) -> dict:
    """The case `name` of the route table (tests/test_gpu_routes.py) at a geometry."""
    from test_gpu_routes import CASES, DEFAULT
    return dict(geometry(dict(DEFAULT, **CASES[name]), geom), **KEEP_ROUTE.get((name, geom), {}))


def identity_inputs(c):
    """(ds (R, T) planted, q (B, W), good, bad) of an Identity case at its geometry."""
    ds = syn.dataset(c["R"], c["T"], 9100 + c["R"])[:, 0, :].copy()
    q = syn.gbm_log_returns((c["B"], c["W"]), 9200 + c["W"])
    good, bad = plant(ds, q, c["h"], planted_queries(c))
    return ds, q, good, bad


def embedded_inputs(c):
    """(ds (R, T) planted, kernel (d, K), raw x (B, K), embedded queries hx (B, d), good, bad): the kernels and the queries of
    test_gpu_embedded._case_inputs, whose raw windows x it does not return."""
    from test_gpu_embedded import _case_inputs
    kind, d, K = c["emb"]
    seed = 9000 + c["R"] + K
    ds, ker, hx = _case_inputs(c["R"], c["T"], d, K, c["B"], kind, seed)
    x = syn.gbm_log_returns((c["B"], K), seed + 1)
    ds = np.ascontiguousarray(ds[:, 0, :]).copy()
    good, bad = plant(ds, x, c["h"], planted_queries(c))
    return ds, ker, x, hx, good, bad


def planted_queries(c):
    W = c["emb"][2] if c["emb"] else c["W"]
    if c["T"] == W + c["h"]:
        return [0]
    return queries_of(c["B"], (129, 130) if c["B"] == 260 else ())      # 260: the two sides of the chunk boundary


class _Rows:
    """Rows in the order 0, R - 1, 1, 2, ...: a plant gets a row of its own."""

    def __init__(self, R, taken=()):
        self.R, self.i, self.taken = R, 0, set(taken)

    def take(self, pair=False):
        while True:
            assert self.i < self.R, "the ensemble has too few rows for the plants"
            r = (0, self.R - 1)[self.i] if self.i < 2 else self.i - 1
            self.i += 1
            if r in self.taken or (pair and (r + 1 >= self.R or r + 1 in self.taken)):
                continue
            self.taken.update((r, r + 1) if pair else (r,))
            return r


def _straddle(ds, x, rows):
    """An exact copy across two rows of the flat ensemble: the first a = W // 2 samples end row r, the rest begin row r + 1."""
    T, W = ds.shape[1], x.shape[0]
    a = W // 2
    r = rows.take(pair=True)
    ds[r, T - a:] = x[:a]
    ds[r + 1, :W - a] = x[a:]
    return (r, T - a)


def plant(ds: np.ndarray, raw_q: np.ndarray, h: int, queries) -> tuple:
    """Edits ds (R, T) float32 in place; (good, bad): lists of (b, r, t).  good[b]'s plant number j (in ascending t; in
    ascending row for one-window rows) is raw_q[b] * (1 + 2^-(6 + j)): relative distance 2^-(6 + j) to float32 rounding, so
    the plants of a query rank in descending j.  bad: exact copies of raw_q[b] at inadmissible start positions."""
    assert ds.dtype == np.float32 and ds.ndim == 2 and ds.flags.c_contiguous
    raw_q = np.asarray(raw_q, dtype=np.float32)
    R, T = ds.shape
    W = raw_q.shape[1]
    Tp = T - W - h + 1
    assert Tp >= 1
    good, bad = [], []

    def near(j):
        return np.float32(1.0 + 2.0 ** -(6 + j))

    if Tp == 1:                                  # one-window rows: the edges are rows
        rs = sorted(r for r in {*ONE_WINDOW_ROWS, R - 2, R - 1} if 0 <= r < R)
        assert len(queries) == 1, "one-window rows: one planted query (the good plants name their rows)"
        b = queries[0]
        for j, r in enumerate(rs):
            ds[r, :W] = raw_q[b] * near(j)
            good.append((b, r, 0))
        rows = _Rows(R, rs)
        for off in sorted({1, h} if h > 0 else ()):
            r = rows.take()
            ds[r, off:off + W] = raw_q[b]
            bad.append((b, r, off))
        bad.append((b, *_straddle(ds, raw_q[b], rows)))
        return good, bad

    ts = edge_windows(Tp)
    order = [ts[0], ts[-1]] + ts[1:-1] if len(ts) > 1 else ts       # (0, 0) and (R - 1, Tp - 1): the first and last unit
    rows = _Rows(R)
    for b in queries:
        at = {}
        for t in order:
            at[t] = rows.take()
        for j, t in enumerate(ts):
            ds[at[t], t:t + W] = raw_q[b] * near(j)
            good.append((b, at[t], t))
        inadmissible = sorted({Tp, Tp + h // 2, T - W}) if h > 0 else []
        for t in inadmissible:
            r = rows.take()
            ds[r, t:t + W] = raw_q[b]
            bad.append((b, r, t))
        bad.append((b, *_straddle(ds, raw_q[b], rows)))
    return good, bad


def check(d, idx, good, bad, T, W, h, what, gap=None):
    """Conditions on a top-k result d (B, k), idx (B, k, 2) of a planted ensemble:
      (a) the first ranks of every planted query are its good plants, in descending plant number;
      (b) no returned window starts past T - W - h, and none is a bad plant (the straddling copy's start lies past it too);
      (c) with gap: the first unplanted distance exceeds gap x the largest planted one.
    Raises AssertionError naming the plant."""
    last = T - W - h
    badset = {(b, r, t) for b, r, t in bad}
    for b in range(idx.shape[0]):
        for rank, (r, t) in enumerate(idx[b].tolist()):
            assert (b, r, t) not in badset, f"{what}: inadmissible (b={b}, r={r}, t={t}) returned at rank {rank}"
            assert 0 <= t <= last, f"{what}: window (b={b}, r={r}, t={t}) past the last admissible t={last} returned at rank {rank}"
    for b in sorted({b for b, _, _ in good}):
        mine = [(r, t) for bb, r, t in good if bb == b][::-1]
        assert len(mine) <= idx.shape[1], f"{what}: k={idx.shape[1]} is less than the {len(mine)} plants of query {b}"
        for rank, (r, t) in enumerate(mine):
            got = tuple(idx[b, rank].tolist())
            where = [i for i, v in enumerate(idx[b].tolist()) if tuple(v) == (r, t)]
            assert got == (r, t), (f"{what}: admissible plant (b={b}, r={r}, t={t}) expected at rank {rank}, "
                                   f"{'found at rank %d' % where[0] if where else 'not returned'}; (r={got[0]}, t={got[1]}) is there")
        if gap is not None:
            n = len(mine)
            assert n < idx.shape[1], f"{what}: no unplanted window among the k={idx.shape[1]} of query {b}"
            assert d[b, n] > gap * d[b, n - 1], (f"{what}: query {b}: the first unplanted distance {d[b, n]:.3g} is within "
                                                 f"{gap} x the largest planted one {d[b, n - 1]:.3g}")
