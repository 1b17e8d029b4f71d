"""PathShadowing.calibrate and smile(calibrate_to=) on the MI355X: the flows against the same kernels composed by hand, the
two ways of forming the prior against each other, and smile() without the new keyword against the bits of the commit before
it."""
from pathlib import Path

import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, calibration as cal, pricing, synthetic as syn

import _calibration as C

pytestmark = pytest.mark.gpu

K, ETA = 64, 0.3
TS, MS = [5, 20], [-1.0, 0.0, 1.0]


@pytest.fixture(scope="module")
def flow(hip_device):
    """A small ensemble (the scan is not what is tested), its queries, shadow(cuda=True)'s distances and
    the out-context of its paths uploaded again, and quotes 1 % above the model's own Monte Carlo prices."""
    ds = syn.dataset(64, 256, 0)
    q = syn.rolling_queries(5, 20, 1)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20))
    d, paths, _ = obj.shadow(q, K, cuda=True)
    assert obj.last_path == "hip"
    future = obj.context.select_out_context(torch.from_numpy(paths).to(hip_device))[:, :, 0, :]
    base = obj.smile(q, K, TS, MS, eta=ETA, cuda=True, report=True)
    quotes = sa.MarketQuotes(TS, base.strikes, prices=base.price_mc * 1.01)
    return obj, q, d, future, quotes


def by_hand(future, prior, quotes, dev):
    strike, target = quotes.arrays(future.shape[0], 100.0, 0.0)
    return _native.calibrate_weights(future, prior, TS, torch.from_numpy(strike).to(dev), torch.from_numpy(target).to(dev), 100.0, 0.0,
                                     0, True, 1e-6, 1e-8, 100)


def test_calibrate_is_the_hand_composition(hip_device, flow):
    obj, q, d, future, quotes = flow
    got = obj.calibrate(q, K, quotes, eta=ETA, cuda=True, device_weights=True)
    assert obj.last_weights == "device" and obj.last_path == "hip"
    assert isinstance(got.weights, torch.Tensor) and got.weights.is_cuda and tuple(got.weights.shape) == (5, K)
    hand = by_hand(future, sa.softmax_weights(d, [ETA], cuda=True)[0, 0], quotes, hip_device)
    assert torch.equal(got.weights, hand["weights"])
    for name, mine in (("lam", got.lam), ("model", got.model), ("status", got.status)):
        assert np.array_equal(mine, hand[name].cpu().numpy()), name
    info = hand["info"].cpu().numpy()
    assert np.array_equal(got.kl, info[:, 0]) and np.array_equal(got.n_eff, info[:, 1]) and np.array_equal(got.grad, info[:, 3])
    assert not got.status.any() and (got.iterations > 0).all() and (got.kl > 0).all()
    assert (np.abs(got.residual + 1e-6 * got.lam * 100.0) <= 1e-8 * 100.0 * (1 + 1e-6)).all()
    # in splits, with quotes that follow their dates
    split = obj.calibrate(q, K, quotes, eta=ETA, cuda=True, device_weights=True, n_context_splits=5)
    assert torch.equal(split.weights, got.weights) and np.array_equal(split.lam, got.lam)


def test_the_two_priors_agree_within_the_widened_rule(hip_device, flow):
    """device_weights=True against False: priors that differ by (2 k + 16) 2^-53 relative each move e_i and Z by as much, so the
    weights at ONE lambda differ by 2 (2 k + 16) 2^-53 more than the consistency bound; the two runs stop at two lambdas, each
    within its optimality bound, which the stationary-point argument turns into weights: both are held to the definition at
    their own lambda with the widened bound, and to each other through the residuals they report."""
    obj, q, d, future, quotes = flow
    dev = obj.calibrate(q, K, quotes, eta=ETA, cuda=True, device_weights=True)
    host = obj.calibrate(q, K, quotes, eta=ETA, cuda=True)
    assert obj.last_weights == "host" and np.array_equal(dev.status, host.status)
    r = future.cpu().numpy()
    prior = np.asarray(sa.Softmax(d.astype(np.float64), ETA).weights, dtype=np.float64).reshape(5, K)
    strike, target = quotes.arrays(5, 100.0, 0.0)
    for name, res in (("device prior", dev), ("host prior", host)):
        w = res.weights.cpu().numpy()
        worst = 0.0
        for b in range(5):
            ex = C.exact(r[b], prior[b], TS, strike[b], target[b], res.lam[b], eps=1e-6)
            bound = C.weight_bound(ex, res.lam[b], K, 8) + 2 * (2 * K + 16) * C.U
            worst = max(worst, float((np.abs(w[b] - ex["q"]).astype(np.float64) / (bound * ex["q"].astype(np.float64))).max()))
            assert (np.abs(ex["grad"]).astype(np.float64) <= C.gradient_bound(ex, K, 1e-8) + 2 * (2 * K + 16) * C.U).all()
        print(f"{name}: the weights use {worst:.4f} of the widened bound")
        assert worst <= 1.0
    assert np.abs(dev.model - host.model).max() <= 2e-8 * 100.0 + 1e-6 * np.abs(dev.lam - host.lam).max() * 100.0


def test_smile_calibrated_to_quotes(hip_device, flow):
    obj, q, d, future, quotes = flow
    sm = obj.smile(q, K, [10], [-0.5, 0.5], eta=ETA, cuda=True, device_weights=True, report=True, calibrate_to=quotes)
    assert obj.last_weights == "device" and sm.calibration is not None and sm.calibration.weights.is_cuda
    hand = by_hand(future, sa.softmax_weights(d, [ETA], cuda=True)[0, 0], quotes, hip_device)
    assert torch.equal(sm.calibration.weights, hand["weights"])
    ref = pricing.smile_from_log_returns(future, hand["weights"], [10], [-0.5, 0.5], 100.0, 0.0, degree=3, kind="otm", cuda=True,
                                         report=True)
    for name in ("prices", "ivs", "strikes", "sigma", "status", "price_mc", "delta", "risk"):
        assert np.array_equal(getattr(sm, name), getattr(ref, name), equal_nan=True), name
    # the calibrated weights feed the other consumers as they are
    qs = _native.weighted_quantiles(future[:, :, :2].contiguous(), sm.calibration.weights, [0.05, 0.5])
    assert not qs[3].cpu().numpy().any()


# smile() of the fixture's object at (K, TS, MS, eta = 0.3, cuda=True), recorded by running the commit before calibrate_to
# existed on an MI355X
GOLDEN = Path(__file__).resolve().parent / "golden" / "smile_before_calibrate_to.npz"


def test_smile_without_the_keyword_is_unchanged(hip_device, flow):
    obj, q, d, future, quotes = flow
    sm = obj.smile(q, K, TS, MS, eta=ETA, cuda=True)
    assert sm.calibration is None
    hand = pricing.smile_from_log_returns(future, torch.from_numpy(np.asarray(sa.Softmax(d.astype(np.float64), ETA).weights,
                                                                               dtype=np.float64).reshape(5, K)).to(hip_device),
                                          TS, MS, 100.0, 0.0, degree=3, kind="otm", cuda=True)
    for name in ("prices", "ivs", "strikes", "sigma", "status"):
        assert np.array_equal(getattr(sm, name), getattr(hand, name), equal_nan=True), name
    golden = np.load(GOLDEN)
    for name in ("prices", "ivs", "strikes", "sigma"):
        assert np.array_equal(getattr(sm, name), golden[name], equal_nan=True), name
