"""Inputs and the comparison rule shared by the quantile tests (test_quantiles_cpu.py, test_gpu_quantiles.py)."""
import numpy as np

from shadowing_amd import Softmax
from shadowing_amd.quantiles import _host_quantiles

LEVELS = np.array([0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99])
LEVELS32 = np.array([(2 * a + 1) / 64.0 for a in range(32)])[::-1].copy()      # 32 levels, descending: any order is allowed


def values(B, k, m, seed):
    """Gaussian values, a third of them rounded to quarters so that ties occur."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, k, m)).astype(np.float32)
    tie = g.random((B, k, m)) < 1.0 / 3.0
    x[tie] = np.round(x[tie] * 4.0) / 4.0
    return x


def softmax_weights(B, k, seed, eta=0.2):
    """The averaging class's own weights for distances like a scan's: (B, k) float64, normalised."""
    g = np.random.default_rng(seed + 1000)
    d = 0.3 + 0.2 * g.random((B, k))
    return np.ascontiguousarray(Softmax(d, eta).weights, dtype=np.float64)


def twin(v, w, levels):
    """(q, lower, upper, status, detail) of the numpy twin on (B, k, m) float32."""
    return _host_quantiles(np.ascontiguousarray(v, dtype=np.float32), w, np.asarray(levels, dtype=np.float64), detail=True)


def assert_matches_twin(got, v, w, levels, max_edges=None):
    """The comparison rule, device against twin: q equal with == except on an edge the twin reports, where either
    neighbouring order statistic is accepted; at most 1 % of the (column, level) pairs may be on an edge (`max_edges`
    overrides the count: 0 for the inputs known to have none); lower / upper within the twin's bound.  `got` = (q, lower,
    upper, status) as numpy arrays shaped like the twin's."""
    q, lo, up, st, det = twin(v, w, levels)
    gq, glo, gup, gst = (np.asarray(a) for a in got)
    gq, glo, gup = (a.reshape(q.shape) for a in (gq, glo, gup))
    assert np.array_equal(gst, st), (gst, st)
    n_edges = int(det["edge"].sum())
    allowed = q.size // 100 if max_edges is None else max_edges
    assert n_edges <= allowed, f"{n_edges} (column, level) pairs on an edge, {allowed} allowed"
    nan = np.isnan(q)
    assert np.array_equal(np.isnan(gq), nan) and np.array_equal(np.isnan(glo), nan) and np.array_equal(np.isnan(gup), nan)
    ok = ~nan
    same = gq == q
    near = det["edge"] & ((gq == det["q_prev"]) | (gq == det["q_next"]))
    assert (same | near)[ok].all(), f"{int((~(same | near))[ok].sum())} quantiles differ from the twin off the edges"
    # (the tail means are continuous in p: on an edge they are held to the same bound)
    err_lo, err_up = np.abs(glo - lo)[ok], np.abs(gup - up)[ok]
    b_lo, b_up = det["bound_lower"][ok], det["bound_upper"][ok]
    share = max(float((err_lo[b_lo > 0] / b_lo[b_lo > 0]).max(initial=0.0)), float((err_up[b_up > 0] / b_up[b_up > 0]).max(initial=0.0)))
    print(f"largest share of the error bound: {share:.3f} ({n_edges} edges)")
    assert (err_lo <= b_lo).all() and (err_up <= b_up).all(), share
    return share
