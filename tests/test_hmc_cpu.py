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
