"""Hedged Monte Carlo smile on the host (shadowing_amd.pricing; no GPU): against the independent restatement of
tests/_hmc_reference.py, put-call parity, known answers on GBM paths, the role of the weights and of the hedge, non-finite
inputs, PriceData and the README snippet."""
import math

import numpy as np
import pytest

import shadowing_amd as sa
from shadowing_amd import pricing
import _hmc_reference as ref

DT = 1.0 / 252.0


def gbm_returns(rng, k, L, sigma, rate=0.0):
    """Log-returns of martingale (discounted) GBM paths, float32."""
    z = rng.standard_normal((k, L))
    return (sigma * math.sqrt(DT) * z + (rate - 0.5 * sigma ** 2) * DT).astype(np.float32)


def prices_of(r, x0=100.0):
    return sa.PriceData(dlnx=r, x_init=x0).x


def check_against_reference(r, w, Ts, Ms, degree=3, kind="otm", rate=0.0, x0=100.0):
    ave = None if w is None else sa.DiscreteProba(w)
    sm = sa.compute_smile(prices_of(r, x0), Ts, Ms, r=rate, ave=ave, degree=degree, kind=kind, cuda=False)
    rf = ref.hmc_date(r, w, x0, rate, Ts, Ms, degree, kind)
    np.testing.assert_allclose(sm.strikes, rf["strike"], rtol=1e-12)
    np.testing.assert_allclose(sm.sigma, rf["sigma"], rtol=1e-12)
    np.testing.assert_allclose(sm.prices, rf["price"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(sm.ivs, rf["iv"], rtol=0, atol=1e-8)
    assert sm.status == 0
    return sm


@pytest.mark.parametrize("degree", [1, 2, 3, 4, 5])
def test_host_matches_restatement_all_degrees(degree):
    rng = np.random.default_rng(degree)
    r = gbm_returns(rng, 300, 12, 0.25)
    check_against_reference(r, None, [3, 12], np.linspace(-2, 2, 5), degree=degree)


@pytest.mark.parametrize("kind", ["otm", "call", "put"])
def test_host_matches_restatement_rate_and_softmax_weights(kind):
    rng = np.random.default_rng(7)
    r = gbm_returns(rng, 257, 10, 0.3, rate=0.05)
    d = rng.random(257)
    w = sa.Softmax(d, eta=0.3).weights
    check_against_reference(r, w, [1, 4, 10], [-1.5, -0.2, 0.0, 0.7, 2.0], kind=kind, rate=0.05)


def test_host_matches_restatement_T1_and_zero_weights():
    rng = np.random.default_rng(3)
    r = gbm_returns(rng, 64, 5, 0.2)
    w = rng.random(64)
    w[::3] = 0.0
    r[::3, 1] = np.nan                     # a zero-weight path may hold anything
    check_against_reference(r, w, [1, 5], [-1.0, 0.0, 1.0])


def test_k1_is_the_discounted_payoff():
    r = np.array([[0.01, -0.02, 0.015, 0.005]], dtype=np.float32)
    rate = 0.03
    sm = check_against_reference(r, None, [4], [0.5], rate=rate)
    x0 = 100.0
    ST = x0 * math.exp(float(np.sum(r[0].astype(np.float64))))
    K = sm.strikes[0, 0]
    assert sm.prices[0, 0] == pytest.approx(math.exp(-rate * 4 / 252) * max(ST - K, 0.0), rel=1e-12)


def test_constant_paths():
    r = np.full((50, 6), 0.001, dtype=np.float32)
    sm = check_against_reference(r, None, [3, 6], [0.0], kind="call", rate=0.02)
    assert np.all(np.isfinite(sm.prices))


def test_put_call_parity():
    rng = np.random.default_rng(11)
    r = gbm_returns(rng, 2000, 30, 0.25, rate=0.04)
    x = prices_of(r)
    Ms = np.linspace(-2, 2, 9)
    c = sa.compute_smile(x, [10, 30], Ms, r=0.04, kind="call", cuda=False)
    p = sa.compute_smile(x, [10, 30], Ms, r=0.04, kind="put", cuda=False)
    ok = np.isfinite(c.ivs) & np.isfinite(p.ivs)
    assert ok.sum() >= 14
    np.testing.assert_allclose(c.ivs[ok], p.ivs[ok], rtol=0, atol=1e-7)


@pytest.mark.parametrize("T", [20, 60])
def test_gbm_recovers_sigma(T):
    rng = np.random.default_rng(100 + T)
    r = gbm_returns(rng, 16384, T, 0.2)
    Ms = np.linspace(-1.5, 1.5, 7)
    sm = sa.compute_smile(prices_of(r), [T], Ms, cuda=False)
    assert np.all(np.abs(sm.ivs - 0.2) < 0.01), sm.ivs


def test_weights_select_the_paths():
    rng = np.random.default_rng(5)
    r = np.concatenate([gbm_returns(rng, 4096, 20, 0.1), gbm_returns(rng, 4096, 20, 0.3)])
    w = np.concatenate([np.zeros(4096), np.ones(4096)])
    sm = sa.compute_smile(prices_of(r), [20], [-1.0, 0.0, 1.0], ave=sa.DiscreteProba(w), cuda=False)
    assert np.all(np.abs(sm.ivs - 0.3) < 0.015), sm.ivs
    uni = sa.compute_smile(prices_of(r), [20], [0.0], cuda=False)
    assert abs(uni.ivs[0, 0] - 0.3) > 0.05


def test_hedge_reduces_the_spread():
    hedged, unhedged = [], []
    for seed in range(8):
        rng = np.random.default_rng(1000 + seed)
        r = gbm_returns(rng, 4096, 20, 0.2)
        x = prices_of(r)
        sm = sa.compute_smile(x, [20], [0.0], kind="call", cuda=False)
        hedged.append(sm.prices[0, 0])
        unhedged.append(np.maximum(x[:, 20] - sm.strikes[0, 0], 0.0).mean())
    assert np.std(unhedged) >= 3 * np.std(hedged), (np.std(unhedged), np.std(hedged))


def test_nonfinite_inputs_give_nan_and_status():
    rng = np.random.default_rng(2)
    r = gbm_returns(rng, 3 * 40, 8, 0.2).reshape(3, 40, 8)
    r[1, 5, 3] = np.nan
    w = np.ones((3, 40))
    w[2, 7] = np.inf
    x = sa.PriceData(dlnx=r, x_init=100.0).x
    sm = sa.compute_smile(x, [4, 8], [0.0, 1.0], ave=sa.DiscreteProba(w), cuda=False)
    assert list(sm.status) == [0, pricing.STATUS_NONFINITE, pricing.STATUS_WEIGHTS]
    assert np.all(np.isfinite(sm.prices[0])) and np.all(np.isnan(sm.prices[1:])) and np.all(np.isnan(sm.ivs[1:]))
    z = sa.compute_smile(x[0], [4], [0.0], ave=sa.DiscreteProba(np.zeros(40)), cuda=False)
    assert z.status == pricing.STATUS_WEIGHTS and np.isnan(z.prices).all()


def test_price_data_round_trips():
    rng = np.random.default_rng(0)
    d = rng.standard_normal((3, 4, 10)) * 0.01
    pd = sa.PriceData(dlnx=d, x_init=50.0)
    assert pd.x.shape == (3, 4, 11) and np.all(pd.x[..., 0] == 50.0)
    np.testing.assert_allclose(pd.dlnx, d, atol=1e-14)
    np.testing.assert_allclose(sa.PriceData(lnx=pd.lnx, x_init=50.0).x, pd.x, rtol=1e-14)
    np.testing.assert_allclose(sa.PriceData(lnx=pd.lnx).x, pd.x, rtol=1e-14)
    np.testing.assert_allclose(sa.PriceData(x=pd.x).dx, np.diff(pd.x, axis=-1))
    np.testing.assert_allclose(sa.PriceData(x=pd.x, x_init=1.0).x, pd.x / 50.0, rtol=1e-14)
    with pytest.raises(ValueError):
        sa.PriceData(dlnx=d, x=pd.x)


def test_readme_snippet_shapes_with_1d_softmax():
    """README: ave = Softmax(distances[-1, :], eta=0.9); x = PriceData(dlnx=close_paths[-1, :, 0, 20:], x_init=100).x."""
    from shadowing import PriceData, Softmax, compute_smile
    rng = np.random.default_rng(4)
    B, k, W, h = 3, 512, 20, 20
    distances = np.sort(rng.random((B, k)), axis=1)
    close_paths = (rng.standard_normal((B, k, 1, W + h)) * 0.01).astype(np.float32)
    ave = Softmax(distances[-1, :], eta=0.9)
    assert ave.weights.shape == (k,) and ave.weights.sum() == pytest.approx(1.0)
    assert np.allclose(Softmax(distances, eta=0.9).weights[-1], ave.weights)      # 2-D input: unchanged behaviour
    x = PriceData(dlnx=close_paths[-1, :, 0, 20:], x_init=100.0).x
    Ts, Ms = [5, 10, 20], np.linspace(-2, 2, 9)
    smile = compute_smile(x, Ts, Ms, ave=ave)
    assert smile.ivs.shape == (3, 9) and smile.prices.shape == (3, 9) and smile.strikes.shape == (3, 9)
    assert np.isfinite(smile.prices).all()
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots()
    smile.plot(ax=ax, color="black", rescale=True, legend=True)
    smile.plot(ax=ax, rescale=False, legend=False)
    plt.close(fig)


def test_smile_from_paths_host_and_argument_checks():
    from shadowing_amd import synthetic as syn
    ds = syn.dataset(16, 400, 0)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20))
    q = syn.rolling_queries(2, 20, 1)
    d, paths, _ = obj.shadow(q, k=64, cuda=False)
    sm = obj.smile_from_paths(d, paths, [5, 20], [-1.0, 0.0, 1.0], eta=0.1)
    w = sa.Softmax(d, 0.1).weights
    ref_sm = sa.compute_smile(sa.PriceData(dlnx=paths[:, :, 0, 20:], x_init=100.0).x, [5, 20], [-1.0, 0.0, 1.0],
                              ave=sa.DiscreteProba(w), cuda=False)
    np.testing.assert_allclose(sm.prices, ref_sm.prices, rtol=1e-9)
    sm2 = obj.smile(q, 64, [5, 20], [-1.0, 0.0, 1.0], eta=0.1, cuda=False)
    np.testing.assert_array_equal(sm2.prices, sm.prices)
    with pytest.raises(ValueError):
        sa.compute_smile(prices_of(np.zeros((4, 5), np.float32)), [6], [0.0], cuda=False)
    with pytest.raises(ValueError):
        sa.compute_smile(prices_of(np.zeros((4, 5), np.float32)), [5], [0.0], degree=6, cuda=False)
    imp = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.ImputationContext(portion=(5, 10, 5)))
    with pytest.raises(NotImplementedError):
        imp.smile_from_paths(d, paths, [5], [0.0])


# ---- known answers that neither implementation produced
A, MS = ref.A, ref.MS
@pytest.mark.parametrize("rate", [0.0, 0.05, -0.02])
@pytest.mark.parametrize("kind", ["otm", "call", "put"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_binomial_tree_is_crr(P, kind, rate):
    """T <= P + 1: the fit is exact at every step, so the price is the discounted CRR price whatever the weights."""
    x0 = 100.0
    for T in range(1, P + 2):
        for reps, zero_half in [(3, False), (2, True), (16384 >> T, T % 2 == 0)]:
            r, w, K, sig, crr = ref.binomial_case(P, T, reps, rate, kind, 1000 * P + 10 * T + reps, zero_half)
            h = pricing.hedged_mc_host(r[None], w[None], [T], MS, x0, rate, P, pricing.KINDS[kind])
            assert h["status"][0] == 0
            np.testing.assert_allclose(h["sigma"][0], [sig], rtol=1e-14)
            np.testing.assert_allclose(h["strike"][0, 0], K, rtol=1e-14)
            np.testing.assert_allclose(h["price"][0, 0], crr, rtol=0, atol=1e-12 * x0)
            if reps <= 3 or (P == 5 and T == 6):               # the restatement: small trees, and the one at k = 16384
                rf = ref.hmc_date(r, w, x0, rate, [T], MS, P, kind)
                assert rf["status"] == 0
                np.testing.assert_allclose(rf["sigma"], [sig], rtol=1e-14)
                np.testing.assert_allclose(rf["strike"][0], K, rtol=1e-14)
                np.testing.assert_allclose(rf["price"][0], crr, rtol=0, atol=1e-12 * x0)


def test_binomial_tree_beyond_p_plus_1_is_not_exact():
    """The exactness above is a property of T <= P + 1 and not of the tree: one step more and the fit misses CRR."""
    r, w, K, _, crr = ref.binomial_case(3, 5, 4, 0.05, "otm", 7)
    h = pricing.hedged_mc_host(r[None], w[None], [5], MS, 100.0, 0.05, 3, 0)
    assert np.max(np.abs(h["price"][0, 0] - crr)) > 1e-4


@pytest.mark.parametrize("rate", [0.0, 0.04])
@pytest.mark.parametrize("P", [1, 3, 5])
def test_deterministic_paths_price_the_discounted_payoff(P, rate):
    """k copies of one path, or one path with all the weight: u = 0 at every step (the basis is {1}) and beta_0 is
    dropped, so the price is e^{-rho T} payoff(S_T)."""
    x0, Ts = 100.0, [1, 4, 9]
    g = np.random.default_rng(P)
    path = (0.01 * g.standard_normal(9)).astype(np.float32)
    copies = np.tile(path, (64, 1))
    other = (0.01 * g.standard_normal((64, 9))).astype(np.float32)
    other[17] = path
    w1 = np.zeros(64)
    w1[17] = 0.3
    for r, w in [(copies, None), (copies, g.uniform(0.1, 1.0, 64)), (other, w1)]:
        for kind in ["otm", "call", "put"]:
            h = pricing.hedged_mc_host(r[None], None if w is None else w[None], Ts, MS, x0, rate, P, pricing.KINDS[kind])
            rf = ref.hmc_date(r, w, x0, rate, Ts, MS, P, kind)
            assert h["status"][0] == 0 and rf["status"] == 0
            for q, T in enumerate(Ts):
                ST = x0 * math.exp(float(np.sum(path[:T].astype(np.float64))))
                K = h["strike"][0, q]
                call = np.array([kind == "call" or (kind == "otm" and M >= 0) for M in MS])
                want = math.exp(-rate * T / 252.0) * np.where(call, np.maximum(ST - K, 0.0), np.maximum(K - ST, 0.0))
                np.testing.assert_allclose(h["price"][0, q], want, rtol=1e-13, atol=1e-13 * x0)
                np.testing.assert_allclose(rf["price"][q], want, rtol=1e-13, atol=1e-13 * x0)


@pytest.mark.parametrize("rate", [0.0, 0.03, -0.02])
def test_all_zero_returns(rate):
    """sigma = 0, every strike is the forward, and the IV is NaN wherever the price is below BS(1e-4)."""
    x0, Ts = 100.0, [1, 5]
    r = np.zeros((32, 5), dtype=np.float32)
    for kind in ["call", "put"]:
        h = pricing.hedged_mc_host(r[None], None, Ts, MS, x0, rate, 3, pricing.KINDS[kind])
        rf = ref.hmc_date(r, None, x0, rate, Ts, MS, 3, kind)
        assert h["status"][0] == 0 and rf["status"] == 0
        assert np.all(h["sigma"][0] == 0.0) and np.all(rf["sigma"] == 0.0)
        for q, T in enumerate(Ts):
            tau = T / 252.0
            F = x0 * math.exp(rate * tau)
            np.testing.assert_allclose(h["strike"][0, q], F, rtol=1e-15)
            want = math.exp(-rate * tau) * (max(x0 - F, 0.0) if kind == "call" else max(F - x0, 0.0))
            np.testing.assert_allclose(h["price"][0, q], want, rtol=1e-13, atol=1e-13 * x0)
            np.testing.assert_allclose(rf["price"][q], want, rtol=1e-13, atol=1e-13 * x0)
            lo = ref.bs(x0, F, tau, rate, 1e-4, kind == "call")
            if want < lo:
                assert np.isnan(h["iv"][0, q]).all() and np.isnan(rf["iv"][q]).all()
            else:                              # (a put when rate > 0: the paths lag the forward)
                iv = ref.implied_vol(want, x0, F, tau, rate, kind == "call")
                assert np.isfinite(iv)
                np.testing.assert_allclose(h["iv"][0, q], iv, rtol=0, atol=1e-8)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_put_call_parity_of_prices(P):
    """C - P = x0 - K e^{-rate tau} for any paths and weights: S_T - K is fitted exactly at every step."""
    rng = np.random.default_rng(50 + P)
    r = gbm_returns(rng, 500, 20, 0.3, rate=0.03)
    w = rng.random(500)
    Ts, Ms, x0 = [1, 7, 20], np.linspace(-2, 2, 9), 100.0
    c = pricing.hedged_mc_host(r[None], w[None], Ts, Ms, x0, 0.03, P, pricing.KINDS["call"])
    p = pricing.hedged_mc_host(r[None], w[None], Ts, Ms, x0, 0.03, P, pricing.KINDS["put"])
    tau = (np.asarray(Ts) / 252.0)[:, None]
    np.testing.assert_allclose(c["price"][0] - p["price"][0], x0 - c["strike"][0] * np.exp(-0.03 * tau), rtol=0,
                               atol=1e-10 * x0)
    rc = ref.hmc_date(r, w, x0, 0.03, Ts, Ms[[0, 4, 8]], P, "call")
    rp = ref.hmc_date(r, w, x0, 0.03, Ts, Ms[[0, 4, 8]], P, "put")
    np.testing.assert_allclose(rc["price"] - rp["price"], x0 - rc["strike"] * np.exp(-0.03 * tau), rtol=0, atol=1e-10 * x0)


# ---- the ill-conditioned regime: a common drift and little spread between the paths
@pytest.mark.parametrize("P", [1, 3, 5])
@pytest.mark.parametrize("c", [0.0, 0.001, -0.001, 0.003, 0.01])
def test_drift_sweep_flags_or_agrees(c, P):
    Ts, Ms = [5, 20], [-1.0, 0.0, 1.0]
    flagged = []
    for e in ref.SWEEP_E:
        r, w = ref.drift_returns(c, e)
        h = pricing.hedged_mc_host(r[None], w[None], Ts, Ms, 100.0, 0.0, P, 0)
        rf = ref.hmc_date(r, w, 100.0, 0.0, Ts, Ms, P, "otm")
        nan = ref.check_sweep_case({k: v[0] for k, v in h.items()}, rf, Ts, Ms)
        flagged.append(bool(nan.any()))
    if c == 0.0:
        assert not any(flagged)                                           # no drift: the hedge is never riskless
    if abs(c) >= 0.003:
        assert flagged[-1] and flagged[-2]                                 # |c| >= 300 e


@pytest.mark.parametrize("P,seed", [(5, 2), (4, 0), (3, 1)])
def test_student_t_flags_or_agrees(P, seed):
    """Heavy tails at T = 75: dates whose fit a few outlying paths make nearly singular are flagged (any kept pivot below
    TAU_SING); the others agree with the restatement to 1e-9."""
    Ts, Ms = [10, 40, 75], [-1.0, 0.0, 1.0]
    r, w = ref.student_t_dates(seed)
    h = pricing.hedged_mc_host(r, w, Ts, Ms, 100.0, 0.01, P, 0)
    flagged = 0
    for b in range(r.shape[0]):
        rf = ref.hmc_date(r[b], w[b], 100.0, 0.01, Ts, Ms, P, "otm")
        flagged += bool(ref.check_sweep_case({k: v[b] for k, v in h.items()}, rf, Ts, Ms).any())
    assert 1 <= flagged < r.shape[0]                                  # some flagged, some priced
