"""The numpy twin of psh_calibrate_weights (shadowing_amd/calibration.py) against closed forms, planted multipliers and the
behaviours README "Calibrating to market quotes" states; no GPU."""
import itertools
import math

import numpy as np
import pytest

import shadowing_amd as sa
from shadowing_amd import calibration as cal, synthetic as syn

import _calibration as C

X0 = C.X0


def test_binomial_tree_gets_the_risk_neutral_probability():
    """The 2^T paths of a full binomial tree, unit prior, the forward at T = 1 the only instrument, eps = 0: the up-paths get
    (e^rho - d') / (u' - d') in all, u', d' the exponentials of the float32 returns, shared equally.  The forward's residual
    is grad x_init = (w_up (u' - d') + d' - e^rho) x_init, so |w_up - w*| <= grad / (u' - d') plus the rounding of 16 terms."""
    T = 4
    u, d = np.float32(math.log(1.02)), np.float32(math.log(0.99))
    r = np.array(list(itertools.product([u, d], repeat=T)), dtype=np.float32)[None]
    for rate in (0.0, 0.05):
        out = cal.calibrate_host(r, None, [1], np.full((1, 1, 1), X0), np.full((1, 1, 1), np.nan), X0, rate, 0, True, 0.0, 1e-10)
        up, dn = math.exp(float(u)), math.exp(float(d))
        w_star = (math.exp(rate / 252.0) - dn) / (up - dn)
        w = out["weights"][0]
        assert out["status"][0] == 0 and out["lam"][0, 0] == 0.0
        print(f"rate {rate}: up-paths carry {w[:8].sum()!r}, closed form {w_star!r}, gradient {out['info'][0, 3]:.2e}")
        assert abs(w[:8].sum() - w_star) <= (out["info"][0, 3] + 64 * C.U) / (up - dn)
        assert np.abs(w[:8] - w[:8].mean()).max() <= 8 * C.U and np.abs(w[8:] - w[8:].mean()).max() <= 8 * C.U
        assert abs(w.sum() - 1.0) <= 16 * C.U


@pytest.mark.parametrize("k", (63, 65, 1025, 16384))
def test_planted_multiplier_is_found(k):
    r, strike, target, lam_star, mart = C.planted(k)
    out = cal.calibrate_host(r, None, C.PLANT_TS, strike, target, X0, 0.0, 0, mart, 0.0, 1e-11)
    lam = out["lam"][0]
    bound, smin, g1, g2 = C.stationary_bound(r, strike, target, lam, lam_star)
    err = float(np.linalg.norm(lam - lam_star))
    print(f"k = {k}: status {out['status'][0]}, {out['info'][0, 2]:.0f} steps, |lam - lam*| = {err:.3e} of {bound:.3e}; "
          f"sigma_min {smin:.2e}, gradients {g1:.2e} and {g2:.2e}")
    assert lam.shape == (8,) and err <= bound
    # the twin alone against long double: a small share of the device's consistency bound
    ex = C.exact(r[0], None, C.PLANT_TS, strike[0], target[0], lam)
    q = ex["q"].astype(np.float64)
    share = float((np.abs(out["weights"][0] - ex["q"]).astype(np.float64) / (C.weight_bound(ex, lam, k, 8) * q)).max())
    print(f"    the twin's weights use {share:.4f} of the consistency bound")
    assert share <= 0.05
    assert (np.abs(ex["grad"]).astype(np.float64) <= C.gradient_bound(ex, k, 1e-11)).all() or out["status"][0] & cal.STATUS_NOT_CONVERGED


@pytest.mark.parametrize("k", (2, 3))
def test_planted_weights_where_the_hessian_is_singular(k):
    r, strike, target, lam_star, mart = C.planted(k)
    out = cal.calibrate_host(r, None, C.PLANT_TS, strike, target, X0, 0.0, 0, mart, 0.0, 1e-11)
    bound, q_star = C.pinsker_bound(r, strike, target, out["lam"][0], lam_star, mart)
    err = float(np.abs(out["weights"][0] - q_star).sum())
    print(f"k = {k}: status {out['status'][0]}, |q - q*|_1 = {err:.3e} of {bound + 8 * k * C.U:.3e}")
    assert err <= bound + 8 * k * C.U and out["info"][0, 3] <= 1e-11


def _one_call(k=257, target=1e4):
    return C.returns(k, 12, 5), [12], np.full((1, 1, 1), 100.0), np.full((1, 1, 1), target)


def test_unattainable_quotes():
    r, Ts, K, high = _one_call()
    hard = cal.calibrate_host(r, None, Ts, K, high, X0, 0.0, 0, False, 0.0)
    assert hard["status"][0] & cal.STATUS_NOT_CONVERGED
    assert all(np.isfinite(hard[n]).all() for n in ("weights", "lam", "model", "info"))
    soft = cal.calibrate_host(r, None, Ts, K, high, X0, 0.0, 0, False, 1e-3)
    assert soft["status"][0] == 0
    resid = soft["model"][0, 0] - 1e4
    assert abs(resid + 1e-3 * soft["lam"][0, 0] * X0) <= 1e-8 * X0 + 1e-9 * abs(resid)


def test_redundant_quotes_are_dropped_and_converge():
    r, Ts, _, _ = _one_call()
    S = cal.terminal_prices(r[0], Ts, X0)[:, 0]
    price = float(np.maximum(S - 101.0, 0.0).mean()) + 0.05
    out = cal.calibrate_host(r, None, Ts, np.full((1, 1, 2), 101.0), np.full((1, 1, 2), price), X0, 0.0, 1, True, 0.0)
    assert out["status"][0] == cal.STATUS_DROPPED and out["lam"][0, 1] == 0.0 and out["info"][0, 3] <= 1e-8
    assert np.abs(out["model"][0, :2] - price).max() <= 1e-8 * X0


def test_an_unquoted_instrument_is_the_call_without_it():
    r = C.returns(513, 12, 11)
    Ts, Ms = [5, 12], [-0.5, 0.0, 0.5]
    strike = C.strikes_at(Ts, Ms)[None]
    tilt = np.exp(0.3 * np.random.default_rng(2).standard_normal(513))
    inst = cal.instruments(X0, 0.0, Ts, strike[0], strike[0], 0, False)
    target = ((tilt / tilt.sum()) @ cal.payoffs(cal.terminal_prices(r[0], Ts, X0), inst)).reshape(1, 2, 3)
    holed = target.copy()
    holed[0, :, 1] = np.nan
    a = cal.calibrate_host(r, None, Ts, strike, holed, X0, 0.0, 0, True, 1e-6)
    b = cal.calibrate_host(r, None, Ts, strike[:, :, [0, 2]], target[:, :, [0, 2]], X0, 0.0, 0, True, 1e-6)
    keep = [0, 2, 3, 5, 6, 7]
    assert a["status"][0] == b["status"][0] == 0 and (a["lam"][0, [1, 4]] == 0.0).all()
    # the same problem, the same iteration: only the order of numpy's sums can differ
    assert np.allclose(a["lam"][0, keep], b["lam"][0], rtol=1e-9, atol=1e-12)
    ex = C.exact(r[0], None, Ts, strike[0], holed[0], a["lam"][0], eps=1e-6)
    assert (np.abs(ex["grad"]).astype(np.float64) <= C.gradient_bound(ex, 513, 1e-8)).all()
    assert np.allclose(a["weights"], b["weights"], rtol=1e-9, atol=0.0)
    assert np.isfinite(a["model"]).all()                                 # the model prices the unquoted strike too


def test_status_nan_rules_zero_weights_and_scaling():
    r = C.returns(65, 12, 3, B=4)
    Ts, strike = [3, 12], np.broadcast_to(C.strikes_at([3, 12], [-0.5, 0.5]), (4, 2, 2)).copy()
    base0 = cal.calibrate_host(r, None, Ts, strike, np.full((4, 2, 2), np.nan), X0, 0.0, 0, True, 1e-6)
    target = base0["model"][:, :4].reshape(4, 2, 2) * 1.02
    prior = np.abs(np.random.default_rng(1).standard_normal((4, 65))) + 0.1
    prior[:, ::5] = 0.0
    rn = r.copy()
    rn[:, ::5, 1] = np.nan                                               # zero-weight paths with NaN returns: not looked at
    base = cal.calibrate_host(rn, prior, Ts, strike, target, X0, 0.0, 0, True, 1e-6)
    clean = cal.calibrate_host(r, prior, Ts, strike, target, X0, 0.0, 0, True, 1e-6)
    assert not base["status"].any() and (base["weights"][:, ::5] == 0.0).all()
    for name in base:
        assert np.array_equal(base[name], clean[name]), name
    assert np.abs(base["weights"].sum(axis=1) - 1.0).max() <= 200 * C.U
    scaled = cal.calibrate_host(rn, prior * 2.0 ** 9, Ts, strike, target, X0, 0.0, 0, True, 1e-6)
    for name in base:
        assert np.array_equal(base[name], scaled[name]), name
    # date by date: a date's bits do not depend on the others
    alone = cal.calibrate_host(rn[2:3], prior[2:3], Ts, strike[2:3], target[2:3], X0, 0.0, 0, True, 1e-6)
    for name in base:
        assert np.array_equal(base[name][2:3], alone[name]), name
    r2, p2, K2, c2 = rn.copy(), prior.copy(), strike.copy(), target.copy()
    r2[0, 1, 2], p2[1, 3], K2[2, 1, 1], c2[3, 0, 0] = np.inf, -1.0, 0.0, np.inf
    bad = cal.calibrate_host(r2, p2, Ts, K2, c2, X0, 0.0, 0, True, 1e-6)
    assert bad["status"].tolist() == [1, 2, 4, 4]
    assert all(np.isnan(bad[n]).all() for n in ("weights", "lam", "model", "info"))
    p2 = prior.copy()
    p2[0] = 0.0
    assert cal.calibrate_host(rn, p2, Ts, strike, target, X0)["status"].tolist() == [2, 0, 0, 0]
    # nothing quoted, no forwards: the normalised prior, at once
    none = cal.calibrate_host(rn, prior, Ts, strike, np.full((4, 2, 2), np.nan), X0, 0.0, 0, False, 1e-6)
    assert not none["status"].any() and (none["info"][:, 2] == 0).all() and (none["lam"] == 0).all()
    assert np.allclose(none["weights"], prior / prior.sum(axis=1, keepdims=True), rtol=200 * C.U, atol=0.0)
    for kw in ({"eps": -1.0}, {"eps": math.nan}, {"tol": 0.0}, {"max_iter": -1}):
        with pytest.raises(ValueError):
            cal.calibrate_host(r, None, Ts, strike, target, X0, **kw)
    with pytest.raises(ValueError):
        cal.calibrate_host(r, None, [13], strike[:, :1], target[:, :1], X0)


def test_market_quotes_from_a_smile_round_trip():
    """A report=True smile under Softmax weights; a uniform prior calibrated to its price_mc reprices it within
    tol x_init + eps |lambda| x_init."""
    g = np.random.default_rng(4)
    r = C.returns(512, 20, 9, B=2)
    px = X0 * np.exp(np.concatenate([np.zeros((2, 512, 1)), np.cumsum(r.astype(np.float64), axis=2)], axis=2))
    d = np.abs(g.standard_normal((2, 512))) * 0.1
    sm = sa.compute_smile(px, [5, 20], [-1.0, 0.0, 1.0], ave=sa.Softmax(d, 0.3), report=True)
    quotes = sa.MarketQuotes.from_smile(sm)
    assert quotes.kind == "otm" and np.array_equal(quotes.prices, sm.price_mc) and list(quotes.Ts) == [5, 20]
    res = sa.calibrate_weights(px, quotes, eps=1e-6, tol=1e-8)
    assert isinstance(res, sa.Calibration) and not res.status.any() and res.weights.shape == (2, 512)
    slack = 1e-8 * X0 + 1e-6 * np.abs(res.lam) * X0
    assert (np.abs(res.residual) <= slack * (1 + 1e-9)).all() and (res.iterations > 0).all() and (res.kl > 0).all()
    assert np.allclose(res.model[:, :6], sm.price_mc.reshape(2, 6), rtol=0.0, atol=float(slack.max()))
    # a Calibration is accepted wherever an `ave` is (the strikes of that smile follow its own sigma_T)
    again = sa.compute_smile(px, [5, 20], [-1.0, 0.0, 1.0], ave=res, report=True)
    hand = sa.pricing.smile_from_log_returns(np.diff(np.log(px), axis=-1).astype(np.float32), res.weights, [5, 20], [-1.0, 0.0, 1.0])
    assert np.array_equal(again.prices, hand.prices) and np.isfinite(again.prices).all()
    one = sa.calibrate_weights(px[0], sa.MarketQuotes([5, 20], sm.strikes[0], prices=sm.price_mc[0]))
    assert one.weights.shape == (512,) and one.status == 0 and np.array_equal(one.weights, res.weights[0])
    # implied vols become prices through bs_price; a NaN vol is not quoted
    ivs = np.full((2, 3), 0.2)
    ivs[1, 2] = np.nan
    K, t = quotes.strikes[0], sa.MarketQuotes([5, 20], quotes.strikes[0], ivs=ivs).arrays(1, X0, 0.0)[1][0]
    assert t[0, 0] == sa.pricing.bs_price(X0, K[0, 0], 5 / 252.0, 0.0, 0.2, False) and np.isnan(t[1, 2])
    assert t[1, 1] == sa.pricing.bs_price(X0, K[1, 1], 20 / 252.0, 0.0, 0.2, True)
    with pytest.raises(ValueError):
        sa.MarketQuotes([5, 20], K)
    with pytest.raises(ValueError):
        sa.MarketQuotes.from_smile(sa.compute_smile(px, [5], [0.0]))


def test_path_shadowing_calibrate_on_the_host_route():
    """PathShadowing.calibrate without a device is shadow() + the twin, and smile(calibrate_to=) prices under its weights."""
    ds = syn.dataset(64, 256, 0)
    q = syn.rolling_queries(3, 20, 1)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20))
    plain = obj.smile(q, 64, [5, 20], [-1.0, 0.0, 1.0], eta=0.3, report=True)
    assert plain.calibration is None
    quotes = sa.MarketQuotes([5, 20], plain.strikes, prices=plain.price_mc * 1.01)
    res = obj.calibrate(q, 64, quotes, eta=0.3, n_context_splits=3)
    d, paths, _ = obj.shadow(q, 64)
    hand = obj.calibrate_from_paths(d, paths, quotes, eta=0.3)
    for name in cal.CALIBRATION_FIELDS:
        assert np.array_equal(getattr(res, name), getattr(hand, name)), name
    assert res.weights.shape == (3, 64) and not (res.status & 7).any()
    sm = obj.smile(q, 64, [5, 20], [-1.0, 0.0, 1.0], eta=0.3, report=True, calibrate_to=quotes.rows(slice(0, 3)))
    assert np.array_equal(sm.calibration.weights, res.weights)
    future = obj.context.select_out_context(paths)[:, :, 0, :]
    ref = sa.pricing.smile_from_log_returns(future, res.weights, [5, 20], [-1.0, 0.0, 1.0], 100.0, 0.0, report=True)
    for name in ("prices", "ivs", "strikes", "price_mc", "delta"):
        assert np.array_equal(getattr(sm, name), getattr(ref, name), equal_nan=True), name
