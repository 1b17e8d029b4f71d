"""The hedge report on the host (shadowing_amd.pricing; no GPU): the twin against the independent restatement of
tests/_hmc_report_reference.py, the four identities of the definition, full binomial trees against Cox-Ross-Rubinstein
(pnl, risk, delta), a flagged maturity, the status bits, report=False, and hedge_pnl's checks."""
import math

import numpy as np
import pytest

import shadowing_amd as sa
from shadowing_amd import pricing
import _hmc_reference as ref
import _hmc_report_reference as rep

RTOL = ATOL = 1e-9                                            # the project's agreement rule (tests/test_gpu_hmc.py)
RESULTS = ("mean", "mc", "risk", "risk_unhedged", "se", "se_unhedged", "n_eff")


def close(a, b):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)


def fit_and_replay(r, w, Ts, Ms, rate, degree, kind, r2=None, w2=None):
    """The twin's fit with its policy on (r, w) and its replay on (r2, w2) (default: in-sample), one date."""
    fit = pricing.hedged_mc_host(r[None], None if w is None else w[None], Ts, Ms, 100.0, rate, degree, pricing.KINDS[kind],
                                 policy=True)
    r2, w2 = (r, w) if r2 is None else (r2, w2)
    out = pricing.replay_host(r2[None], None if w2 is None else w2[None], Ts, Ms, fit["policy"], fit["strike"],
                              fit["price"], 100.0, rate, degree, pricing.KINDS[kind], return_pnl=True)
    return fit, out


@pytest.mark.parametrize("degree,kind,rate", [(1, "otm", 0.0), (3, "call", 0.05), (5, "put", 0.02)])
def test_twin_matches_restatement(degree, kind, rate):
    (r,), (w,) = rep.mrw_like_returns(degree, 1, 150, 12)
    (r2,), (w2,) = rep.mrw_like_returns(degree + 10, 1, 90, 12)
    Ts, Ms = [1, 5, 12], [-1.5, 0.0, 0.8, 1.2]
    fit, ins = fit_and_replay(r, w, Ts, Ms, rate, degree, kind)
    assert fit["status"][0] == 0 and np.isfinite(fit["price"]).all()
    # the restatement's own fit (another standardisation, another Cholesky): the same prices, deltas and in-sample report
    pol, price, strike = rep.fit_policy(r, w, 100.0, rate, Ts, Ms, degree, kind)
    close(fit["price"][0], price)
    close(fit["policy"][0][:, :, 0, degree + 3], pol[:, :, 0, degree + 3])             # delta
    sums, pnl, st = rep.replay(r, w, 100.0, rate, Ts, Ms, degree, kind, pol, strike, price)
    assert st == 0
    close(ins["pnl"][0], pnl)
    want, got = rep.results(sums, price), pricing.report_from_sums(ins["sums"][0], fit["price"][0])
    for name in RESULTS:
        close(got[name], want[name])
    # the twin's replay of its own policy bits on other paths against the restatement's replay of the same bits
    _, oos = fit_and_replay(r, w, Ts, Ms, rate, degree, kind, r2, w2)
    sums2, pnl2, _ = rep.replay(r2, w2, 100.0, rate, Ts, Ms, degree, kind, fit["policy"][0], fit["strike"][0], fit["price"][0])
    close(oos["sums"][0], sums2)
    close(oos["pnl"][0], pnl2)
    assert np.isnan(oos["pnl"][0][:, :, w2 == 0]).all() and np.isfinite(oos["pnl"][0][:, :, w2 != 0]).all()


@pytest.mark.parametrize("degree,rate", [(2, 0.0), (3, 0.05), (5, 0.03)])
def test_identities(degree, rate):
    (r,), (w,) = rep.mrw_like_returns(7 * degree, 1, 400, 12)
    (r2,), (w2,) = rep.mrw_like_returns(7 * degree + 1, 1, 130, 12)
    Ts, Ms = [2, 12], [-1.0, 0.0, 0.5]
    fit, ins = fit_and_replay(r, w, Ts, Ms, rate, degree, "call")
    a1 = ins["sums"][0][..., 0]
    assert np.abs(a1).max() <= 1e-11 * 100.0                                           # in-sample: mean = V_0
    for r_, w_ in ((r, w), (r2, w2)):
        callf, c = fit_and_replay(r, w, Ts, Ms, rate, degree, "call", r_, w_)
        putf, p = fit_and_replay(r, w, Ts, Ms, rate, degree, "put", r_, w_)
        wn = w_ / w_.sum()
        res = pricing.report_from_sums(c["sums"][0], callf["price"][0])
        gain = res["mc"] - res["mean"]                                                  # mc - mean = sum w gain
        pay = np.maximum(100.0 * np.exp(np.cumsum(r_.astype(np.float64), axis=1))[:, [1, 11]].T[:, None, :]
                         - callf["strike"][0][:, :, None], 0.0) * np.exp(-rate / 252 * np.array([2, 12]))[:, None, None]
        live = w_ != 0
        close(gain, ((pay - c["pnl"][0])[:, :, live] * wn[live]).sum(-1))
        # put-call: pnl_call - pnl_put = x_init - K exp(-rho T), path by path, in and out of sample
        want = 100.0 - callf["strike"][0] * np.exp(-rate / 252 * np.array([2, 12]))[:, None]
        close((c["pnl"][0] - p["pnl"][0])[:, :, live], np.broadcast_to(want[:, :, None], c["pnl"][0].shape)[:, :, live])
        np.testing.assert_array_equal(callf["strike"], putf["strike"])


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("rate", [0.0, 0.05, -0.02])
def test_binomial_tree_pnl_is_crr(P, rate):
    T = min(P + 1, 4)
    r, w, K, sig, crr = ref.binomial_case(P, T, 4, rate, "otm", 10 * P + T, zero_half=True)
    sm = sa.compute_smile(sa.PriceData(dlnx=r, x_init=100.0).x, [T], ref.MS, r=rate, ave=sa.DiscreteProba(w), degree=P,
                          cuda=False, report=True)
    close(sm.strikes[0], K)
    close(sm.prices[0], crr)
    assert (sm.risk <= 1e-9).all() and (sm.price_se <= 1e-9).all()
    delta = [rep.crr_delta(100.0, K[j], ref.A, rate, T, ref.MS[j] >= 0) for j in range(len(ref.MS))]
    close(sm.delta[0], delta)
    h = sa.hedge_pnl(sm.policy, sa.PriceData(dlnx=r, x_init=100.0).x, ave=sa.DiscreteProba(w), return_paths=True, cuda=False)
    assert np.isnan(h.pnl[0][:, w == 0]).all()
    close(h.pnl[0][:, w != 0], np.broadcast_to(crr[:, None], h.pnl[0].shape)[:, w != 0])
    close(h.mean[0], crr)
    assert (sm.risk_unhedged[0, 1:4] > 0.1).all()             # (the far strikes never pay on a short tree)
    assert np.isclose(sm.n_eff, 1.0 / ((w / w.sum()) ** 2).sum()).all()


def test_flagged_maturity_reports_nan_for_that_maturity_only():
    r, w = ref.drift_returns(0.01, 1e-4)               # (T = 1 has no step n > 0: never "riskless")
    x = sa.PriceData(dlnx=r, x_init=100.0).x
    sm = sa.compute_smile(x, [1, 20], [-1.0, 0.0, 1.0], ave=sa.DiscreteProba(w), degree=3, cuda=False, report=True)
    assert sm.status == pricing.STATUS_ILL_CONDITIONED
    assert np.isnan(sm.prices[1]).all() and np.isfinite(sm.prices[0]).all()
    for name in pricing.REPORT_FIELDS:
        v = getattr(sm, name)
        if name == "iv_se":                                   # (NaN wherever the iv is NaN)
            assert np.isnan(v[1]).all()
            continue
        assert np.isnan(v[1]).all() and np.isfinite(v[0]).all(), name
    h = sa.hedge_pnl(sm.policy, x, ave=sa.DiscreteProba(w), return_paths=True, cuda=False)
    assert np.isnan(h.sums[1]).all() and np.isnan(h.pnl[1]).all() and np.isnan(h.mean[1]).all()
    assert np.isfinite(h.sums[0]).all() and np.isfinite(h.pnl[0][:, w != 0]).all() and h.status == 0


def test_status_bits():
    r, w = rep.mrw_like_returns(3, 4, 60, 12)
    w[:] = np.where(w == 0, 0.0, 1.0)
    Ts, Ms = [3, 8], [0.0, 1.0]
    fit = pricing.hedged_mc_host(r, w, Ts, Ms, 100.0, 0.0, 2, 0, policy=True)
    r2, w2 = r.copy(), w.copy()
    w2[0, 5], r2[0, 5, :] = 0.0, np.nan                       # zero weight: ignored
    w2[1, 3], r2[1, 3, 2] = 1.0, np.nan
    w2[1, 4], r2[1, 4, 9] = 1.0, np.inf                       # beyond max Ts = 8: ignored (the NaN above is not)
    w2[2, 0] = np.nan
    w2[3, :] = 0.0
    out = pricing.replay_host(r2, w2, Ts, Ms, fit["policy"], fit["strike"], fit["price"], 100.0, 0.0, 2, 0, return_pnl=True)
    assert list(out["status"]) == [0, pricing.STATUS_NONFINITE, pricing.STATUS_WEIGHTS, pricing.STATUS_WEIGHTS]
    assert np.isfinite(out["sums"][0]).all() and np.isnan(out["pnl"][0][:, :, 5]).all()
    assert np.isnan(out["sums"][1:]).all() and np.isnan(out["pnl"][1:]).all()
    for b in range(4):
        s, p, st = rep.replay(r2[b], w2[b], 100.0, 0.0, Ts, Ms, 2, "otm", fit["policy"][b], fit["strike"][b], fit["price"][b])
        assert st == out["status"][b]
        np.testing.assert_allclose(out["sums"][b], s, rtol=RTOL, atol=ATOL)
    # a fit on bad inputs: NaN prices, a policy of zeros, and a NaN report
    bad = pricing.smile_from_log_returns(r2, w2, Ts, Ms, degree=2, report=True)
    assert list(bad.status) == list(out["status"])
    assert np.isnan(bad.delta[1:]).all() and np.isnan(bad.risk[1:]).all() and (bad.policy.coef[1:] == 0).all()


def test_report_false_changes_nothing():
    (r,), (w,) = rep.mrw_like_returns(1, 1, 200, 12)
    x = sa.PriceData(dlnx=r, x_init=100.0).x
    plain = sa.compute_smile(x, [4, 12], [-1.0, 0.0, 1.0], r=0.01, ave=sa.DiscreteProba(w), cuda=False)
    full = sa.compute_smile(x, [4, 12], [-1.0, 0.0, 1.0], r=0.01, ave=sa.DiscreteProba(w), cuda=False, report=True)
    for name in pricing.REPORT_FIELDS + ("policy",):
        assert getattr(plain, name) is None and getattr(full, name) is not None, name
    for name in ("prices", "ivs", "strikes", "sigma", "status"):
        np.testing.assert_array_equal(getattr(plain, name), getattr(full, name))
    assert full.delta.shape == full.prices.shape == (2, 3) and full.policy.coef.shape == (1, 2, 3, 12, 10)
    # iv_se = price_se / vega
    tau = np.array([4, 12])[:, None] / 252.0
    d1 = (np.log(100.0 / full.strikes) + (0.01 + 0.5 * full.ivs ** 2) * tau) / (full.ivs * np.sqrt(tau))
    vega = 100.0 * np.exp(-0.5 * d1 ** 2) / math.sqrt(2 * math.pi) * np.sqrt(tau)
    np.testing.assert_allclose(full.iv_se, full.price_se / vega, rtol=1e-12)
    assert (full.price_se < full.price_se_unhedged).all()


def test_hedge_pnl_checks_its_paths():
    (r,), _ = rep.mrw_like_returns(2, 1, 100, 12)
    sm = sa.compute_smile(sa.PriceData(dlnx=r, x_init=100.0).x, [6], [0.0], cuda=False, report=True)
    with pytest.raises(ValueError, match="x_init"):
        sa.hedge_pnl(sm.policy, sa.PriceData(dlnx=r, x_init=50.0).x)
    with pytest.raises(ValueError):
        sa.hedge_pnl(sm.policy, sa.PriceData(dlnx=r[:, :5], x_init=100.0).x)                 # shorter than the maturity
    with pytest.raises(ValueError):
        sa.hedge_pnl(sm.policy, sa.PriceData(dlnx=np.stack([r, r]), x_init=100.0).x)         # two dates, one policy
    h = sa.hedge_pnl(sm.policy, sa.PriceData(dlnx=r[:40], x_init=100.0).x)
    assert h.mean.shape == (1, 1) and h.pnl is None and h.status == 0
    import shadowing
    assert shadowing.hedge_pnl is sa.hedge_pnl and shadowing.HedgePolicy is sa.HedgePolicy


def test_errorbars_plot_and_the_out_of_sample_recipe():
    r, w = rep.mrw_like_returns(9, 2, 400, 12)
    paths = sa.PriceData(dlnx=r, x_init=100.0).x                                            # (B, k, N + 1)
    Ts, Ms = [4, 12], [-1.0, 0.0, 1.0]
    fit = sa.compute_smile(paths[:, 0::2], Ts, Ms, cuda=False, report=True)
    oos = sa.hedge_pnl(fit.policy, paths[:, 1::2], return_paths=True, cuda=False)
    assert oos.pnl.shape == (2, 2, 3, 200) and np.isfinite(oos.pnl).all() and (oos.risk > 0).all()
    close(oos.n_eff, 200.0)
    var = sa.weighted_quantiles(np.moveaxis(oos.pnl, -1, 1), None, [0.01, 0.05], cuda=False)
    assert var.q.shape == (2, 2, 2, 3)
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots()
    fit.plot(ax=ax, errorbars=True)
    assert len(ax.containers) == 2                                                           # one error-bar line per maturity
    with pytest.raises(ValueError, match="report=True"):
        sa.compute_smile(paths[:, 0::2], Ts, Ms, cuda=False).plot(ax=ax, errorbars=True)
    plt.close(fig)
