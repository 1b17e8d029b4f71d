"""References, bounds and the comparison rule shared by the scoring tests (test_scoring_cpu.py, test_gpu_scoring.py).  The two
references here are independent of the twin's gap form: the O(k^2) pair form E|X - y| - 1/2 E|X - X'| in long double, and
the same in exact rational arithmetic for small k."""
from fractions import Fraction

import numpy as np

from shadowing_amd.scoring import _host_scores

EPS = 2.0 ** -53


def pair_form(x, w, y):
    """(crps, pit_lo, pit_hi, mean) of one column in np.longdouble: x (k,), w (k,) >= 0, y a number; the paths with w = 0
    are dropped first."""
    keep = np.asarray(w) > 0
    x = np.asarray(x, dtype=np.float64)[keep].astype(np.longdouble)
    p = np.asarray(w, dtype=np.float64)[keep].astype(np.longdouble)
    p = p / p.sum()
    y = np.longdouble(y)
    crps = (p * np.abs(x - y)).sum() - np.longdouble(0.5) * (p[:, None] * p[None, :] * np.abs(x[:, None] - x[None, :])).sum()
    return crps, p[x < y].sum(), p[x <= y].sum(), (p * x).sum()


def exact_form(x, w, y):
    """The same four numbers as fractions.Fraction (floats are rationals): exact, for small k."""
    pairs = [(Fraction(float(a)), Fraction(float(b))) for a, b in zip(x, w) if b > 0]
    y = Fraction(float(y))
    W = sum(b for _, b in pairs)
    e1 = sum(b * abs(a - y) for a, b in pairs) / W
    e2 = sum(b * d * abs(a - c) for a, b in pairs for c, d in pairs) / (W * W)
    return (e1 - e2 / 2, sum(b for a, b in pairs if a < y) / W, sum(b for a, b in pairs if a <= y) / W,
            sum(a * b for a, b in pairs) / W)


def bounds(v, w, y):
    """The tolerances of a comparison between two summation orders, each (E, B, m), from v (B, k, m), w (E, B, k) or None and
    y (B, m): crps 8 (k + 4) 2^-53 span with span = max(x_(n-1), y) - min(x_(0), y) over the weighted paths; pit
    2 (k + 2) 2^-53; mean 2 (k + 2) 2^-53 (sum w |x|) / W.  Each side adds at most k non-negative weights in some order: the
    relative error of C_i is at most k 2^-53, the absolute error of W - C_i at most 2 k 2^-53 W, and the gap lengths sum to
    at most span."""
    B, k, m = v.shape
    w = np.ones((1, B, k)) if w is None else np.asarray(w, dtype=np.float64)
    pos = (w > 0)[:, :, :, None]
    x = v.astype(np.float64)[None]
    with np.errstate(invalid="ignore"):
        hi = np.maximum(np.where(pos, x, -np.inf).max(axis=2), y[None])
        lo = np.minimum(np.where(pos, x, np.inf).min(axis=2), y[None])
        A = (np.where(pos, np.abs(x), 0.0) * np.where(pos, w[:, :, :, None], 0.0)).sum(axis=2)
        W = np.where(pos, w[:, :, :, None], 0.0).sum(axis=2)
        return {"crps": 8.0 * (k + 4) * EPS * (hi - lo), "pit": np.full(A.shape, 2.0 * (k + 2) * EPS),
                "mean": 2.0 * (k + 2) * EPS * A / W}


def twin(v, w, y):
    return _host_scores(np.ascontiguousarray(v, dtype=np.float32), None if w is None else np.ascontiguousarray(w, dtype=np.float64),
                        np.ascontiguousarray(y, dtype=np.float32))


def assert_within_bounds(got, ref, v, w, y):
    """`got` and `ref` = (crps, pit_lo, pit_hi, mean, status), arrays shaped (E, B, m) and (E, B): equal status, NaN in the
    same places, every finite result within the bound of `bounds`, and exactly 0 on both sides where span = 0.  Returns the
    largest share of each bound as a dict."""
    g = [np.asarray(a, dtype=np.float64).reshape(np.asarray(r).shape) for a, r in zip(got[:4], ref[:4])]
    r = [np.asarray(a, dtype=np.float64) for a in ref[:4]]
    assert np.array_equal(np.asarray(got[4]).reshape(np.asarray(ref[4]).shape), ref[4]), (got[4], ref[4])
    nan = np.isnan(r[0])
    for a, c in zip(g, r):
        assert np.array_equal(np.isnan(a), nan) and np.array_equal(np.isnan(c), nan)
    ok = ~nan
    bd = bounds(np.asarray(v, dtype=np.float32), w, np.asarray(y, dtype=np.float32).astype(np.float64))
    share = {}
    for name, idx, key in (("crps", 0, "crps"), ("pit_lo", 1, "pit"), ("pit_hi", 2, "pit"), ("mean", 3, "mean")):
        err, b = np.abs(g[idx] - r[idx])[ok], bd[key][ok]
        assert (err <= b).all(), (name, float((err / np.where(b > 0, b, 1.0)).max()))
        share[name] = float((err[b > 0] / b[b > 0]).max(initial=0.0))
    flat = ok & (bd["crps"] == 0.0)
    assert (g[0][flat] == 0.0).all() and (r[0][flat] == 0.0).all()
    assert (g[0][ok] >= 0.0).all() and (g[1][ok] <= g[2][ok]).all() and (g[2][ok] <= 1.0).all()
    print("largest share of the bounds:", {n: round(s, 4) for n, s in share.items()})
    return share


def values(B, k, m, seed, decimals=None):
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, k, m)).astype(np.float32)
    return x if decimals is None else np.round(x, decimals).astype(np.float32)
