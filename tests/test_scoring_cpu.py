"""The numpy twin of psh_score_ensemble (shadowing_amd/scoring.py) and the host API, no GPU: the twin against exact rational
arithmetic and against the O(k^2) pair form in long double (tests/_scoring.py), the consequences the definition states,
propriety and calibration on drawn outcomes, and PathShadowing.score_from_paths on a host shadow() result."""
import math

import numpy as np
import pytest

import _scoring as sc
import shadowing_amd as sa
from shadowing_amd import scoring, synthetic as syn


def column(k, seed, scale=1.0, ties=True, zero_half=True):
    g = np.random.default_rng(seed)
    x = (scale * g.standard_normal(k)).astype(np.float32)
    if ties:
        x = (np.round(x / scale * 4.0) / 4.0 * scale).astype(np.float32)
    w = g.random(k)
    if zero_half and k > 1:
        w[g.random(k) < 0.5] = 0.0
        w[g.integers(k)] = 0.5
    xs = np.sort(x[w > 0])
    ys = [xs[0] - 1.0, xs[-1] + 1.0, xs[len(xs) // 2], 0.5 * (float(xs[0]) + float(xs[-1])) + 1e-3]
    return x, w, [np.float32(y) for y in ys]


def one(x, w, y):
    """The twin on one column: (crps, pit_lo, pit_hi, mean)."""
    r = sa.score_ensemble(x[None, :], None if w is None else w[None, :], np.array([y], dtype=np.float32), cuda=False)
    assert r.status.tolist() == [0]
    return float(r.crps[0]), float(r.pit_lo[0]), float(r.pit_hi[0]), float(r.mean[0])


def check_column(x, w, y, ref):
    k = len(x)
    v = x[None, :, None]
    bd = sc.bounds(v, w[None, None, :], np.array([[float(y)]]))
    got = one(x, w, y)
    err = [abs(float(got[n] - ref[n])) for n in range(4)]
    assert err[0] <= bd["crps"][0, 0, 0] and err[1] <= bd["pit"][0, 0, 0] and err[2] <= bd["pit"][0, 0, 0], (k, err)
    assert err[3] <= bd["mean"][0, 0, 0], (k, err)
    return err[0] / bd["crps"][0, 0, 0] if bd["crps"][0, 0, 0] > 0 else 0.0


@pytest.mark.parametrize("k", (1, 2, 3, 7, 33, 64))
def test_twin_against_exact_rational_arithmetic(k):
    for scale in (1e-3, 1.0, 50.0):
        x, w, ys = column(k, 10 * k + int(scale), scale)
        for y in ys:
            ref = sc.exact_form(x, w, y)
            check_column(x, w, y, [float(r) for r in ref])


@pytest.mark.parametrize("k", (100, 511, 1024))
def test_twin_against_the_pair_form_in_long_double(k):
    worst = 0.0
    for scale, half in ((1e-3, True), (1.0, False), (50.0, True)):
        x, w, ys = column(k, k + int(scale), scale, zero_half=half)
        for y in ys:
            worst = max(worst, check_column(x, w, y, sc.pair_form(x, w, y)))
    print(f"k = {k}: the twin's largest share of the crps bound {worst:.4f}")
    assert worst < 0.25             # the bound does not hide a wrong formula: the twin alone stays well inside it


def test_stated_consequences():
    g = np.random.default_rng(5)
    # n = 1: |x - y|, however many weightless paths surround it
    x = g.standard_normal(9).astype(np.float32)
    w = np.zeros(9)
    w[4] = 0.3
    for y in (np.float32(-2.0), np.float32(2.5), x[4]):
        crps, lo, hi, mean = one(x, w, y)
        assert crps == abs(float(x[4]) - float(y)) and mean == float(x[4])
        assert (lo, hi) == ((1.0, 1.0) if y > x[4] else (0.0, 1.0) if y == x[4] else (0.0, 0.0))
    # crps >= 0, pit_lo <= pit_hi with equality off the samples
    v = sc.values(6, 40, 3, 1, decimals=1)
    wt = g.random((4, 6, 40))
    y_on, y_off = v[:, 7, :].copy(), (v[:, 7, :] + np.float32(0.013)).astype(np.float32)
    r_on, r_off = sa.score_ensemble(v, wt, y_on, cuda=False), sa.score_ensemble(v, wt, y_off, cuda=False)
    assert (r_on.crps >= 0).all() and (r_off.crps >= 0).all()
    assert (r_on.pit_lo < r_on.pit_hi).all() and np.array_equal(r_off.pit_lo, r_off.pit_hi)
    assert r_on.crps.shape == (4, 6, 3) and r_on.status.shape == (4, 6) and not r_on.status.any()
    # a power of two scales nothing
    r2 = sa.score_ensemble(v, wt * 2.0 ** -7, y_on, cuda=False)
    for name in ("crps", "pit_lo", "pit_hi", "mean"):
        assert np.array_equal(getattr(r_on, name).view(np.uint64), getattr(r2, name).view(np.uint64)), name
    # a set's results are the same alone or among others; (B, k) weights drop the set axis
    alone = sa.score_ensemble(v, wt[2], y_on, cuda=False)
    assert alone.crps.shape == (6, 3) and alone.status.shape == (6,)
    for name in ("crps", "pit_lo", "pit_hi", "mean"):
        assert np.array_equal(getattr(alone, name), getattr(r_on, name)[2]), name
    # unit weights are weights of 1
    unit, ones = sa.score_ensemble(v, None, y_on, cuda=False), sa.score_ensemble(v, np.ones((6, 40)), y_on, cuda=False)
    assert np.array_equal(unit.crps, ones.crps) and np.array_equal(unit.mean, ones.mean)
    # all values equal to y: exactly 0
    flat = np.full((2, 30, 2), 0.375, dtype=np.float32)
    r = sa.score_ensemble(flat, g.random((2, 30)), flat[:, 0, :], cuda=False)
    assert (r.crps == 0.0).all() and (r.pit_lo == 0.0).all() and (r.pit_hi == 1.0).all()
    assert (np.abs(r.mean - 0.375) <= 2 * 32 * sc.EPS * 0.375).all()


def test_zero_weight_paths_are_absent_and_the_zeros_are_one_value():
    g = np.random.default_rng(6)
    v = sc.values(3, 20, 2, 2)
    w = g.random((2, 3, 20))
    w[:, :, 5] = w[:, :, 11] = w[:, :, 12] = 0.0
    y = g.standard_normal((3, 2)).astype(np.float32)
    ref = sa.score_ensemble(v, w, y, cuda=False)
    v2 = v.copy()
    v2[:, 5, :], v2[:, 11, :], v2[:, 12, 0], v2[:, 12, 1] = np.nan, np.inf, -np.inf, 1e30
    got = sa.score_ensemble(v2, w, y, cuda=False)
    assert not got.status.any()
    for name in ("crps", "pit_lo", "pit_hi", "mean"):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), name
    # -0.0 and +0.0: one value, in the ensemble and in the observation
    x = np.array([-1.0, -0.0, 0.0, 2.0], dtype=np.float32)
    for y0 in (np.float32(0.0), np.float32(-0.0)):
        crps, lo, hi, mean = one(x, np.ones(4), y0)
        assert (lo, hi) == (0.25, 0.75)
        assert crps == one(np.abs(x) * np.sign(x + 0.0), np.ones(4), np.float32(0.0))[0]


def test_status_bits_and_what_each_turns_nan():
    g = np.random.default_rng(7)
    v = sc.values(3, 16, 3, 3)
    w = g.random((3, 3, 16))
    y = g.standard_normal((3, 3)).astype(np.float32)
    clean = sa.score_ensemble(v, w, y, cuda=False)
    fields = ("crps", "pit_lo", "pit_hi", "mean")

    def same_except(r, mask):
        for name in fields:
            a, c = getattr(r, name), getattr(clean, name)
            assert np.isnan(a[mask]).all() and np.array_equal(a[~mask], c[~mask]), name

    for bad in (np.nan, np.inf, -np.inf):                        # a non-finite value at a positive weight: its column, every set
        v1 = v.copy()
        v1[1, 4, 2] = bad
        w1 = w.copy()
        w1[2, 1, 4] = 0.0                                        # ... that weighs it: set 2 does not
        r = sa.score_ensemble(v1, w1, y, cuda=False)
        base = sa.score_ensemble(v, w1, y, cuda=False)
        assert r.status.tolist() == [[0, scoring.STATUS_NONFINITE, 0]] * 2 + [[0, 0, 0]]
        mask = np.zeros((3, 3, 3), dtype=bool)
        mask[:2, 1, 2] = True
        for name in fields:
            assert np.isnan(getattr(r, name)[mask]).all() and np.array_equal(getattr(r, name)[~mask], getattr(base, name)[~mask])
    for bad in (np.nan, np.inf, -1e-3):                          # a bad weight: all of (e, b)
        w1 = w.copy()
        w1[1, 2, 9] = bad
        r = sa.score_ensemble(v, w1, y, cuda=False)
        assert r.status.tolist() == [[0, 0, 0], [0, 0, scoring.STATUS_WEIGHTS], [0, 0, 0]]
        mask = np.zeros((3, 3, 3), dtype=bool)
        mask[1, 2, :] = True
        same_except(r, mask)
    w1 = w.copy()
    w1[0, 0, :] = 0.0                                            # W = 0
    r = sa.score_ensemble(v, w1, y, cuda=False)
    assert r.status[0, 0] == scoring.STATUS_WEIGHTS and np.isnan(r.crps[0, 0]).all() and r.status.sum() == scoring.STATUS_WEIGHTS
    for bad in (np.nan, np.inf):                                 # a non-finite observation: its column, every set
        y1 = y.copy()
        y1[2, 0] = bad
        r = sa.score_ensemble(v, w, y1, cuda=False)
        assert r.status.tolist() == [[0, 0, scoring.STATUS_OBS]] * 3
        mask = np.zeros((3, 3, 3), dtype=bool)
        mask[:, 2, 0] = True
        same_except(r, mask)
    # mean_crps() averages the finite queries, best() ranks the sets by it, pit() interpolates
    assert np.allclose(r.mean_crps()[:, 0], clean.crps[:, :2, 0].mean(axis=1)) and r.mean_crps().shape == (3, 3)
    assert np.array_equal(clean.best(), clean.mean_crps().argmin(axis=0))
    assert np.array_equal(clean.pit(), 0.5 * (clean.pit_lo + clean.pit_hi)) and np.array_equal(clean.pit(1.0), clean.pit_hi)
    with pytest.raises(ValueError):
        sa.score_ensemble(v, np.ones((65, 3, 16)), y, cuda=False)
    with pytest.raises(ValueError):
        sa.score_ensemble(v, w[0], y[:, :2], cuda=False)


def test_unit_weights_on_normal_draws_meet_the_closed_form():
    x = np.random.default_rng(0).standard_normal(16384).astype(np.float32)
    z = 0.3
    Phi, phi = 0.5 * (1.0 + math.erf(z / math.sqrt(2.0))), math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    closed = z * (2.0 * Phi - 1.0) + 2.0 * phi - 1.0 / math.sqrt(math.pi)
    crps, lo, hi, mean = one(x, None, np.float32(z))
    print(f"crps {crps:.5f} against the closed form {closed:.5f}")
    assert abs(crps - closed) <= 0.02 * closed and abs(lo - Phi) < 0.02 and lo == hi and abs(mean) < 0.03


PROPRIETY_SEED = 7


def test_crps_is_proper_the_true_weighting_scores_best():
    """B = 512 queries of k = 256 values, three Gaussian weightings (widths 0.05, 0.15, 0.45) of random distances in (0, 1),
    each y_b drawn from the categorical distribution of set 1 over the values.  The mean CRPS must be lowest at set 1 (so
    that best() means something).  The seed is chosen, among 0 .. 7, so that the twin's margin over the runner-up is at least
    three standard errors of the per-query difference.  Measured with it: mean CRPS 0.5736, 0.5491, 0.5907; margin of set 1
    over set 0 (the runner-up) 0.02457 = 4.3 standard errors, over set 2 0.04169 = 4.0 standard errors."""
    g = np.random.default_rng(PROPRIETY_SEED)
    B, k = 512, 256
    d = g.random((B, k))
    v = (g.standard_normal((B, k)) + 2.0 * d).astype(np.float32)          # the values depend on the distance: widths matter
    w = np.stack([np.exp(-0.5 * (d / eta) ** 2) for eta in (0.05, 0.15, 0.45)])
    p = w[1] / w[1].sum(axis=1, keepdims=True)
    pick = (p.cumsum(axis=1) > g.random((B, 1))).argmax(axis=1)
    y = v[np.arange(B), pick]
    r = sa.score_ensemble(v, w, y, cuda=False)
    mc = r.mean_crps()
    assert mc.shape == (3,) and int(r.best()) == 1
    for other in (0, 2):
        diff = r.crps[other] - r.crps[1]
        se = diff.std(ddof=1) / math.sqrt(B)
        print(f"set {other}: margin {diff.mean():.5f} = {diff.mean() / se:.1f} standard errors")
        assert diff.mean() >= 3.0 * se


def test_randomised_pit_of_calibrated_forecasts_is_uniform():
    g = np.random.default_rng(11)
    B, k = 2000, 256
    draws = np.round(g.standard_normal((B, k + 1)), 1).astype(np.float32)   # values and y from one law, with ties
    r = sa.score_ensemble(draws[:, :k], None, draws[:, k], cuda=False)
    u = np.sort(r.pit(g.random(B)))
    ks = max(np.abs(u - np.arange(1, B + 1) / B).max(), np.abs(u - np.arange(B) / B).max())
    print(f"Kolmogorov distance {ks:.4f} against {1.63 / math.sqrt(B):.4f}")
    assert ks < 1.63 / math.sqrt(B)
    assert (r.pit_lo < r.pit_hi).any()                                      # (the ties are there: the randomisation matters)


def test_score_from_paths_on_a_host_shadow_result():
    ds = syn.dataset(64, 256, 0)
    q = syn.rolling_queries(5, 20, 1)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20))
    stat = lambda x: sa.realized_variance(x[:, :, 0, :], [5, 20])          # noqa: E731
    d, paths, _ = obj.shadow(q, 128)
    x_real = (0.01 * np.random.default_rng(3).standard_normal((5, 1, 20))).astype(np.float32)
    etas, ks = [0.05, None, 0.5], [32, 128]
    got = obj.score_from_paths(d, paths, x_real, stat, etas, ks)
    assert got.crps.shape == (3, 2, 5, 2) and got.status.shape == (3, 2, 5) and not got.status.any()
    assert got.etas == (0.05, None, 0.5) and got.ks == (32, 128)
    values = stat(obj.context.select_out_context(paths))
    obs = stat(x_real[:, None])[:, 0]
    assert obs.shape == (5, 2)
    order = np.argsort(d, axis=1, kind="stable")
    for a, eta in enumerate(etas):
        for c, kc in enumerate(ks):
            near = order[:, :kc]
            w = np.asarray(obj.init_averaging_proba("softmax", np.take_along_axis(d, near, axis=1), eta).weights, dtype=np.float64)
            ref = sa.score_ensemble(np.take_along_axis(values, near[:, :, None], axis=1), w.reshape(5, kc), obs, cuda=False)
            for name in ("crps", "pit_lo", "pit_hi", "mean"):
                assert np.array_equal(getattr(got, name)[a, c], getattr(ref, name)), (name, eta, kc)
    i_eta, i_k = got.best()
    assert i_eta.shape == i_k.shape == (2,)
    flat = got.mean_crps().reshape(6, 2).argmin(axis=0)
    assert np.array_equal(i_eta * 2 + i_k, flat)
    whole = obj.score(q, x_real, 128, stat, etas, ks)
    split = obj.score(q, x_real, 128, stat, etas, ks, n_context_splits=2)
    assert obj.last_score_reduction == "host"
    assert np.array_equal(whole.crps, got.crps) and np.array_equal(split.crps, got.crps) and split.status.shape == (3, 2, 5)
    with pytest.raises(ValueError):
        obj.score_from_paths(d, paths, x_real, stat, [0.01 * (n + 1) for n in range(33)], [64, 128])    # 66 sets
    with pytest.raises(ValueError):
        obj.score_from_paths(d, paths, x_real, stat, [0.1], [129])
