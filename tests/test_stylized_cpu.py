"""shadowing_amd.stylized without a GPU: the numpy twin of psh_lagged_moments against the literal loops, the group
partition, the rows left out, mrw.smrw_sq_moment against its sums written as loops and against the twin's estimate, and
fit_smrw on the twin's ensembles."""
import functools
import math

import numpy as np
import pytest

import shadowing_amd as sa
from shadowing_amd import mrw, stylized
from test_smrw_cpu import LEVERAGE_SETS

NAMES = ("xx", "xx2", "x2x", "x2x2")


def _loops(x, m, bounds):
    """The definition, literally: for each group, lag, row and t."""
    G = len(bounds) - 1
    sums = np.zeros((G, 4, m + 1))
    rows = np.zeros(G, dtype=np.int64)
    for g in range(G):
        for r in range(bounds[g], bounds[g + 1]):
            if not all(math.isfinite(float(v)) for v in x[r]):
                continue
            rows[g] += 1
            for tau in range(m + 1):
                for t in range(len(x[r]) - tau):
                    a, b = float(x[r][t]), float(x[r][t + tau])
                    sums[g, 0, tau] += a * b
                    sums[g, 1, tau] += a * b * b
                    sums[g, 2, tau] += a * a * b
                    sums[g, 3, tau] += a * a * b * b
    return sums, rows


@functools.lru_cache(maxsize=None)
def _ensemble(lam, K0, alpha, seed):
    """(8192, 1, 512) float32 returns of the twin at sigma = 1: made once, shared, read-only."""
    x = mrw.smrw_log_returns(8192, 512, K0, alpha, lam=lam, sigma=1.0, seed=seed)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("R,n,m,G", [(3, 7, 6, 1), (3, 7, 6, 3), (1, 1, 0, 1), (10, 5, 2, 3)])
def test_twin_against_the_literal_loops(R, n, m, G):
    x = np.random.default_rng(R * 100 + n).standard_normal((R, n)).astype(np.float32)
    mom = sa.lagged_moments(x, m, groups=G, cuda=False)
    sums, rows = _loops(x, m, stylized.group_bounds(R, G))
    np.testing.assert_allclose(mom.group_sums, sums, rtol=1e-13, atol=1e-300)
    assert np.array_equal(mom.group_rows, rows) and mom.rows_used == R and mom.rows_excluded == 0
    assert np.array_equal(mom.lags, np.arange(m + 1)) and np.array_equal(mom.n_pairs, R * (n - np.arange(m + 1)))
    for q, name in enumerate(NAMES):
        np.testing.assert_allclose(getattr(mom, name), sums[:, q].sum(axis=0) / mom.n_pairs, rtol=1e-13, atol=1e-300)
        assert getattr(mom, name).shape == getattr(mom, name + "_se").shape == (m + 1,)
        assert np.all(np.isnan(getattr(mom, name + "_se"))) == (G == 1)
    assert mom.variance == mom.xx[0] and mom.kurtosis == mom.x2x2[0] / mom.xx[0] ** 2
    assert np.array_equal(mom.leverage(), mom.xx2[1:] / mom.xx[0] ** 2) and mom.leverage().shape == (m,)
    # the same numbers from every layout, numpy or torch, and from float64 input (rounded to float32 first)
    import torch
    for other in (x[:, None, :], torch.from_numpy(x.copy()), x.astype(np.float64)):
        assert np.array_equal(sa.lagged_moments(other, m, groups=G).group_sums, mom.group_sums)
    if R == 1:
        assert np.array_equal(sa.lagged_moments(x[0], m).group_sums, mom.group_sums)


def test_the_group_partition_and_the_standard_error():
    assert stylized.group_bounds(10, 3).tolist() == [0, 3, 6, 10]
    assert stylized.group_bounds(7, 7).tolist() == list(range(8))
    x = np.random.default_rng(1).standard_normal((10, 9)).astype(np.float32)
    mom = sa.lagged_moments(x, 2, groups=3, cuda=False)
    assert mom.group_rows.tolist() == [3, 3, 4]
    assert sa.lagged_moments(x, 2, groups=10, cuda=False).group_rows.tolist() == [1] * 10
    assert sa.lagged_moments(x, 2, cuda=False).group_rows.size == 10           # the default: min(R, 64)
    # the standard error: the scatter of the group means about the mean, weighted by group size, over G - 1
    x64 = x.astype(np.float64)
    gm = np.array([np.mean(x64[a:b, :8] * x64[a:b, 1:] ** 2) for a, b in ((0, 3), (3, 6), (6, 10))])
    w = np.array([0.3, 0.3, 0.4])
    assert mom.xx2[1] == pytest.approx(float(w @ gm), rel=1e-13)
    assert mom.xx2_se[1] == pytest.approx(math.sqrt(float(w @ (gm - w @ gm) ** 2) / 2.0), rel=1e-12)


def test_rows_with_nan_or_inf_are_left_out_and_counted():
    x = np.random.default_rng(2).standard_normal((6, 8)).astype(np.float32)
    bad = x.copy()
    bad[1, 0], bad[4, 7] = np.nan, np.inf
    mom = sa.lagged_moments(bad, 3, groups=2, cuda=False)
    sums, rows = _loops(bad, 3, [0, 3, 6])
    assert rows.tolist() == [2, 2] and np.array_equal(mom.group_rows, rows)
    assert mom.rows_used == 4 and mom.rows_excluded == 2 and np.array_equal(mom.n_pairs, 4 * (8 - np.arange(4)))
    np.testing.assert_allclose(mom.group_sums, sums, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(mom.group_sums, sa.lagged_moments(x[[0, 2, 3, 5]], 3, groups=2, cuda=False).group_sums,
                               rtol=1e-13, atol=1e-300)
    bad[:] = np.nan
    bad[3] = -np.inf
    none = sa.lagged_moments(bad, 3, groups=2, cuda=False)
    assert np.all(none.group_sums == 0.0) and none.group_rows.tolist() == [0, 0] and none.rows_used == 0
    assert all(np.all(np.isnan(getattr(none, name))) for name in NAMES) and np.all(none.n_pairs == 0)


def test_sq_moment_closed_form_spelt_out():
    """smrw_sq_moment against the sums written as loops, its sigma^4 scaling and its K0 = 0 limit."""
    n, m, K0, alpha, lam = 64, 40, 0.07, 0.7, 0.15
    K = lambda j: K0 / j ** alpha if 1 <= j <= m else 0.0        # noqa: E731
    v = sum(K(j) ** 2 for j in range(1, m + 1))
    for tau in (1, 3, 40, 50):                                   # 50: past the memory, K(tau) = 0
        ct = lam * lam * max(math.log(n / (tau + 1.0)), 0.0)
        expo = (4 * ct + 2 * K(tau) ** 2 + 2 * sum((K(j) + K(j + tau)) ** 2 for j in range(1, m + 1)) +
                2 * sum(K(j) ** 2 for j in range(1, tau)) - 4 * v)
        want = (1 + 4 * K(tau) ** 2) * math.exp(expo)
        assert mrw.smrw_sq_moment(tau, n, K0, alpha, lam=lam, memory=m, sigma=1.0) == pytest.approx(want, rel=1e-13)
        assert mrw.smrw_sq_moment(tau, n, K0, alpha, lam=lam, memory=m, sigma=2.0) == pytest.approx(16.0 * want, rel=1e-13)
        assert mrw.smrw_sq_moment(tau, n, 0.0, alpha, lam=lam, memory=m, sigma=1.5) == pytest.approx(
            1.5 ** 4 * math.exp(4 * ct), rel=1e-13)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            mrw.smrw_sq_moment(bad, n, K0, alpha, memory=m)


@pytest.mark.parametrize("lam,K0,alpha", LEVERAGE_SETS)
def test_closed_forms_against_the_twins_estimate(lam, K0, alpha):
    """R = 8192, n = 512, seed 11: x2x2 (and xx2) within 6 of the standard errors lagged_moments reports; xx2 is the
    per-lag numpy expression of tests/test_smrw_cpu.py on the float32-rounded returns to 1e-12."""
    R, n = 8192, 512
    x = _ensemble(lam, K0, alpha, 11)
    mom = sa.lagged_moments(x, 20, groups=64, cuda=False)
    r = x[:, 0].astype(np.float64)
    for tau in (1, 2, 5, 20):
        sq, lev = mrw.smrw_sq_moment(tau, n, K0, alpha, lam=lam, sigma=1.0), mrw.smrw_leverage(tau, n, K0, alpha, lam=lam, sigma=1.0)
        z_sq, z_lev = (mom.x2x2[tau] - sq) / mom.x2x2_se[tau], (mom.xx2[tau] - lev) / mom.xx2_se[tau]
        print(f"lam={lam} K0={K0} alpha={alpha} tau={tau}: x2x2 {mom.x2x2[tau]:.4f} closed form {sq:.4f} z {z_sq:+.2f}; "
              f"xx2 {mom.xx2[tau]:+.5f} closed form {lev:+.5f} z {z_lev:+.2f}")
        assert abs(z_sq) <= 6.0 and abs(z_lev) <= 6.0
        per_path = (r[:, :n - tau] * r[:, tau:] ** 2).mean(axis=1)
        assert mom.xx2[tau] == pytest.approx(float(per_path.mean()), rel=1e-12)
        assert abs(mom.x2x[tau]) <= 6.0 * mom.x2x_se[tau]                       # the time-reversed leverage: zero in law
    assert mom.variance == pytest.approx(float(np.mean(r * r)), rel=1e-12)


# three times the worst error of the eight seeds below
FIT_SETS = [((0.2, 0.1, 0.6), (3 * 0.0109, 3 * 0.0015, 3 * 0.0311)), ((0.1, 0.05, 0.75), (3 * 0.0008, 3 * 0.0009, 3 * 0.0369))]


@pytest.mark.parametrize("truth,tol", FIT_SETS)
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_fit_recovers_the_parameters(truth, tol, seed):
    """fit_smrw(max_lag=40) on the twin's ensembles, R = 8192, n = 512, sigma = 1.  Eight seeds, run before the bounds were
    written, gave (lam, K0, alpha), each with the standard deviation the fit reported:
      (0.2, 0.1, 0.6)    11: .1991+-.0032 .0985+-.0015 .5922+-.0142    12: .1979+-.0032 .0998+-.0015 .5988+-.0159
                         13: .1974+-.0028 .1003+-.0014 .6201+-.0153    14: .1997+-.0029 .1014+-.0013 .6305+-.0120
                         15: .2109+-.0111 .1005+-.0027 .6311+-.0175    16: .2015+-.0033 .0997+-.0018 .6038+-.0133
                         17: .2013+-.0031 .0998+-.0017 .6124+-.0151    18: .1990+-.0029 .1015+-.0014 .6007+-.0146
      (0.1, 0.05, 0.75)  11: .1002+-.0022 .0499+-.0005 .7610+-.0171    12: .0998+-.0025 .0505+-.0005 .7519+-.0190
                         13: .0992+-.0022 .0504+-.0005 .7526+-.0192    14: .1001+-.0022 .0503+-.0005 .7869+-.0191
                         15: .1008+-.0022 .0498+-.0005 .7827+-.0211    16: .1007+-.0024 .0499+-.0005 .7562+-.0177
                         17: .1004+-.0022 .0507+-.0005 .7728+-.0182    18: .0994+-.0020 .0509+-.0004 .7466+-.0155
    in 6 to 23 iterations.  Worst errors: lam .0109 and .0008, K0 .0015 and .0009, alpha .0311 and .0369; the largest error
    in reported standard deviations was 2.5 (alpha, seed 14 of the first set).  With (J^T J)^-1 alone as the covariance
    (no account of the correlation between lags) lam of seed 15 stood 5.2 and alpha of seed 14 4.5 reported deviations
    off, which is why the covariance is the sandwich.  The test runs seeds 11 to 13: each parameter within three times the
    worst error seen, and within 4 reported standard deviations of the truth."""
    lam, K0, alpha = truth
    fit = sa.fit_smrw(_ensemble(lam, K0, alpha, seed), max_lag=40, cuda=False)
    sd = fit["stderr"]
    print(f"truth {truth} seed {seed}: sigma {fit['sigma']:.4f}+-{sd['sigma']:.4f} lam {fit['lam']:.4f}+-{sd['lam']:.4f} "
          f"K0 {fit['K0']:.4f}+-{sd['K0']:.4f} alpha {fit['alpha']:.4f}+-{sd['alpha']:.4f} chi2 {fit['chi2']:.1f} / {fit['dof']} "
          f"in {fit['iterations']} iterations")
    for name, want, t in zip(("lam", "K0", "alpha"), truth, tol):
        assert abs(fit[name] - want) <= t, name
        assert abs(fit[name] - want) <= 4.0 * sd[name], name
    assert abs(fit["sigma"] - 1.0) <= 4.0 * sd["sigma"]
    assert fit["cov"].shape == (4, 4) and np.allclose(np.sqrt(np.diag(fit["cov"])), [sd[k] for k in ("sigma", "lam", "K0", "alpha")])
    assert fit["dof"] == 77 and isinstance(fit["moments"], sa.LaggedMoments) and fit["moments"].lags[-1] == 40
    assert fit["params"] == dict(K0=fit["K0"], alpha=fit["alpha"], lam=fit["lam"], sigma=fit["sigma"], L=512.0, memory=512)
    assert mrw.smrw_log_returns(2, 512, seed=1, **fit["params"]).shape == (2, 1, 512)     # the result feeds the generator


def test_fit_of_an_ensemble_without_leverage_gives_k0_zero():
    fit = sa.fit_smrw(_ensemble(0.2, 0.0, 0.6, 11), max_lag=40, cuda=False)
    print(f"lam {fit['lam']:.4f}+-{fit['stderr']['lam']:.4f} K0 {fit['K0']:.5f}+-{fit['stderr']['K0']:.5f} alpha {fit['alpha']:.3f}")
    assert 0.0 <= fit["K0"] <= 4.0 * fit["stderr"]["K0"] and fit["stderr"]["K0"] < 0.01
    assert abs(fit["lam"] - 0.2) <= 4.0 * fit["stderr"]["lam"] and 0.05 <= fit["alpha"] <= 3.0


def test_argument_errors():
    x = np.zeros((16, 2000), dtype=np.float32)
    with pytest.raises(ValueError, match="max_lag"):
        sa.lagged_moments(x[:, :30], 30, cuda=False)             # max_lag >= n
    with pytest.raises(ValueError, match="max_lag"):
        sa.lagged_moments(x, -1, cuda=False)
    # max_lag > 1024: the kernel's limit (psh_lagged_moments itself returns PSH_ERR_UNSUPPORTED); the Python surface raises
    # ValueError before any dispatch, under cuda=True, cuda=None and cuda=False alike, so the twin accepts what the device does
    for cuda in (True, None, False):
        with pytest.raises(ValueError, match="1024"):
            sa.lagged_moments(x, 1025, cuda=cuda)
    assert sa.lagged_moments(x, 1024, groups=1, cuda=False).lags.size == 1025
    for G in (17, 0, 2.5):
        with pytest.raises(ValueError, match="groups"):
            sa.lagged_moments(x, 4, groups=G, cuda=False)
    for shape in ((2, 2, 8), (2, 3, 4, 5), (0, 8), (4, 0)):
        with pytest.raises(ValueError, match="shape"):
            sa.lagged_moments(np.zeros(shape, dtype=np.float32), 0, cuda=False)
    r = np.random.default_rng(3).standard_normal((16, 64)).astype(np.float32)
    with pytest.raises(ValueError, match="8"):
        sa.fit_smrw(r, max_lag=10, groups=7, cuda=False)
    with pytest.raises(ValueError, match="8"):
        sa.fit_smrw(r[:7], max_lag=10, cuda=False)               # the default: min(R, 64) = 7 groups
    with pytest.raises(ValueError, match="memory"):
        sa.fit_smrw(r, max_lag=10, memory=5, cuda=False)


def test_the_public_names():
    import shadowing
    for name in ("lagged_moments", "fit_smrw", "LaggedMoments", "smrw_sq_moment"):
        assert getattr(shadowing, name) is getattr(sa, name) and name in sa.__all__
    assert sa.lagged_moments is stylized.lagged_moments and sa.fit_smrw is stylized.fit_smrw
    assert sa.LaggedMoments is stylized.LaggedMoments and sa.smrw_sq_moment is mrw.smrw_sq_moment


# ---- integer ensembles: the twin equals an int64 reference exactly, on every plan of the device's kernel ----
import _moments_exact as mx                                                     # noqa: E402


def test_the_plan_helper_covers_every_plan_and_both_sides_of_every_boundary():
    plans = {m: mx.lag_plan(m) for m in mx.CENSUS_M}
    assert {p[0] for p in plans.values()} == {1, 2, 4} and {p[1] for p in plans.values()} == {1, 2, 3, 4}
    for lo, hi in mx.BOUNDARIES:
        assert lo in plans and hi in plans and plans[lo] != plans[hi] and mx.lag_plan(lo + 1) == plans[hi]
    assert [mx.lag_plan(m) for m in (1, 64, 65, 128, 129, 256, 257, 512, 513, 768, 769, 1024)] == [
        (1, 1, 8), (1, 1, 8), (2, 1, 8), (2, 1, 8), (4, 1, 8), (4, 1, 8), (4, 2, 4), (4, 2, 4), (4, 3, 2), (4, 3, 2), (4, 4, 2), (4, 4, 2)]
    assert {mx.lag_plan(m)[:2] for m in mx.CENSUS_M} == {mx.lag_plan(m)[:2] for m in range(1, 1025)}       # all six (U, C)
    assert {mx.lag_plan(m)[:2] for m in mx.PLANT_M} == {mx.lag_plan(m)[:2] for m in range(1, 1025)}
    assert mx.lag_plan(600)[1] * mx.lag_plan(600)[2] == 6 < mx.WAVES           # C = 3: waves 6 and 7 are not workers
    assert [mx.slice_len(m) for m in mx.PLANT_M] == [256, 256, 256, 512, 1024, 1024]
    for R, n, m, G in mx.census_shapes():
        assert m < n and n - mx.LT in (m + 3, m + 1 - mx.LT)
    # the second tile's m + 3 samples are no multiple of U = 4 (the staging rounds them up) except where m = 1 mod 4
    assert {m for m in mx.CENSUS_M if m > 128 and (m + 3) % 4 == 0} == {129, 257, 513, 769}


@pytest.mark.parametrize("shape", mx.census_shapes(), ids=mx.census_id)
def test_twin_equals_the_int64_reference_on_integer_samples(shape):
    R, n, m, G = shape
    x = mx.int_ensemble(R, n, 7)
    sums, rows = stylized._host_sums(x, m, G)
    want = mx.int_sums(x, m, G)
    assert np.abs(want).max() < 2 ** 40 and np.array_equal(sums, want.astype(np.float64))
    assert np.array_equal(rows, np.diff(stylized.group_bounds(R, G))) and np.array_equal(sums[:, 1, 0], sums[:, 2, 0])
    assert np.any(want[:, :, m] != 0)                                            # the largest lag is not trivially zero


@pytest.mark.parametrize("m", mx.PLANT_M)
def test_twin_finds_every_impulse_plant_exactly(m):
    x, want = mx.plants(m)
    assert len(x) == 7 + 4 * (mx.lag_plan(m)[2] - 1)
    sums, rows = stylized._host_sums(x, m, len(x))
    assert np.array_equal(sums, want.astype(np.float64)) and np.array_equal(rows, np.ones(len(x), np.int64))
    assert np.array_equal(mx.int_sums(x, m, len(x)), want)


def test_one_dropped_pair_is_noticed():
    """A reference that leaves out ONE pair differs from the twin at that (group, lag), in every sum whose summand is
    not zero there, and nowhere else."""
    R, n, m, G = 3, mx.LT + 603, 600, 3
    x = mx.int_ensemble(R, n, 7)
    sums, _ = stylized._host_sums(x, m, G)
    for row, tau in ((0, 600), (1, 1), (2, 257)):
        assert x[row, n - 1 - tau] != 0 and x[row, n - 1] != 0
        bad = sums != mx.int_sums(x, m, G, drop=(row, tau)).astype(np.float64)
        assert bad.any() and np.array_equal(np.argwhere(bad)[:, [0, 2]], np.array([[row, tau]] * 4))


def test_partition_invariance_is_exact_on_integers():
    x = mx.int_ensemble(37, 300, 11)
    total = mx.int_sums(x, 70, 1)[0]
    for G in (1, 2, 5, 37):
        sums, rows = stylized._host_sums(x, 70, G)
        assert np.array_equal(sums, mx.int_sums(x, 70, G).astype(np.float64))
        assert np.array_equal(sums.sum(axis=0), total.astype(np.float64)) and rows.sum() == 37
