"""psh_hedged_mc on the MI355X against the numpy twin (shadowing_amd.pricing) and the independent restatement
(tests/_hmc_reference.py): every degree and kind, k from 1 to PSH_MAX_K, batches of dates, the strided out-context view
of gathered paths, bitwise repeatability, argument errors, non-finite inputs, and PathShadowing.smile(cuda=True)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, pricing
import _hmc_reference as ref

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_device")]
DT = 1.0 / 252.0
# prices: rtol 1e-9, and an absolute floor of 1e-11 of the spot for the deep out-of-the-money ones, which are differences
# of O(1) terms of the regression and zero up to its rounding
PRICE_ATOL = 1e-9


def returns(seed, B, k, L, sigma=0.2, rate=0.0):
    g = np.random.default_rng(seed)
    sig = sigma * (0.5 + g.random((B, k, 1)))                          # a spread of vols: a real smile
    return (sig * math.sqrt(DT) * g.standard_normal((B, k, L)) + (rate - 0.5 * sig ** 2) * DT).astype(np.float32)


def softmax_weights(seed, B, k):
    d = np.random.default_rng(seed + 99).random((B, k))
    return sa.Softmax(d, eta=0.3).weights


def both(r, w, Ts, Ms, rate=0.0, degree=3, kind="otm", x0=100.0):
    dev = pricing.smile_from_log_returns(torch.from_numpy(r).cuda(), None if w is None else torch.from_numpy(w).cuda(),
                                         Ts, Ms, x0, rate, degree=degree, kind=kind, cuda=True)
    host = pricing.smile_from_log_returns(r, w, Ts, Ms, x0, rate, degree=degree, kind=kind, cuda=False)
    return dev, host


def iv_tolerance(sm):
    """1e-8, plus the implied-vol move that the price tolerance allows where the option has almost no vega (a deep
    in-the-money option one sample from expiry): the inversion, not the kernel, is ill-conditioned there."""
    tau = (np.asarray(sm.Ts, dtype=np.float64) / 252.0)[:, None]
    sig = np.where(np.isfinite(sm.ivs), sm.ivs, 1.0)
    d1 = (np.log(sm.x_init / sm.strikes) + (sm.r + 0.5 * sig ** 2) * tau) / (sig * np.sqrt(tau))
    vega = sm.x_init * np.exp(-0.5 * d1 ** 2) / math.sqrt(2 * math.pi) * np.sqrt(tau)
    return 1e-8 + (1e-9 * np.abs(sm.prices) + PRICE_ATOL) / np.maximum(vega, 1e-300)


def assert_iv_close(dev_ivs, host):
    both_nan = np.isnan(dev_ivs) & np.isnan(host.ivs)
    ok = both_nan | (np.abs(dev_ivs - host.ivs) <= iv_tolerance(host))
    assert ok.all(), np.argwhere(~ok)


def assert_close(dev, host):
    np.testing.assert_array_equal(dev.status, host.status)
    np.testing.assert_allclose(dev.strikes, host.strikes, rtol=1e-12)
    np.testing.assert_allclose(dev.sigma, host.sigma, rtol=1e-12)
    np.testing.assert_allclose(dev.prices, host.prices, rtol=1e-9, atol=PRICE_ATOL)
    assert_iv_close(dev.ivs, host)


CASES = [  # B, k, L, Ts, degree, kind, weighted, rate
    (2, 1, 20, [5, 20], 3, "otm", False, 0.0),
    (3, 17, 20, [1, 5, 20], 1, "call", True, 0.03),
    (4, 1000, 252, [7, 25, 75], 2, "put", True, 0.0),
    (2, 8192, 20, [5, 10, 20], 3, "otm", True, 0.0),
    (1, 8192, 252, [7, 25, 75], 3, "otm", True, 0.02),
    (1, 16384, 20, [20], 4, "call", False, 0.0),
    (64, 256, 20, [5, 10, 20], 5, "otm", True, 0.0),
    (16, 1000, 252, [75], 5, "put", False, 0.05),
]


@pytest.mark.parametrize("B,k,L,Ts,degree,kind,weighted,rate", CASES)
def test_kernel_matches_host(B, k, L, Ts, degree, kind, weighted, rate):
    r = returns(B * 1000 + k, B, k, L, rate=rate)
    w = softmax_weights(k, B, k) if weighted else None
    dev, host = both(r, w, Ts, np.linspace(-2, 2, 9), rate, degree, kind)
    assert_close(dev, host)
    assert np.isfinite(dev.prices).all()


@pytest.mark.parametrize("k,degree,kind", [(1, 2, "otm"), (17, 1, "put"), (300, 3, "call"), (300, 5, "put")])
def test_kernel_matches_restatement(k, degree, kind):
    r = returns(k, 2, k, 20, rate=0.01)
    w = softmax_weights(k, 2, k)
    Ts, Ms = [1, 7, 20], [-1.5, 0.0, 0.8]
    dev, _ = both(r, w, Ts, Ms, 0.01, degree, kind)
    for b in range(2):
        rf = ref.hmc_date(r[b], w[b], 100.0, 0.01, Ts, Ms, degree, kind)
        np.testing.assert_allclose(dev.prices[b], rf["price"], rtol=1e-9, atol=PRICE_ATOL)
        host_b = pricing.Smile(rf["price"][None], rf["iv"][None], rf["strike"][None], rf["sigma"][None], np.asarray(Ts),
                               np.asarray(Ms), kind, np.zeros(1), 100.0, 0.01)
        assert_iv_close(dev.ivs[b][None], host_b)


def test_strided_view_of_gathered_paths_and_repeatability():
    g = np.random.default_rng(3)
    R, Cc, T, W, h, k, B = 40, 2, 600, 20, 40, 512, 3
    ds = torch.from_numpy((g.standard_normal((R, Cc, T)) * 0.012).astype(np.float32)).cuda()
    idx = torch.from_numpy(np.stack([g.integers(0, R, (B, k)), g.integers(0, T - W - h, (B, k))], -1).astype(np.int32)).cuda()
    paths = _native.gather_paths(ds, idx, W + h)                         # (B, k, C, W + h)
    view = paths[:, :, 1, W:]                                             # channel 1, the out-context: strided, no copy
    assert not view.is_contiguous()
    w = torch.from_numpy(softmax_weights(5, B, k)).cuda()
    Ts, Ms = [5, 20, 40], np.linspace(-2, 2, 9)
    a = _native.hedged_mc(view, w, Ts, Ms, 100.0, 0.01, 3, _native.PSH_HMC_OTM)
    b = _native.hedged_mc(view, w, Ts, Ms, 100.0, 0.01, 3, _native.PSH_HMC_OTM)
    for name in a:
        assert torch.equal(a[name], b[name]), name                        # bitwise
    host = pricing.smile_from_log_returns(view.contiguous().cpu().numpy(), w.cpu().numpy(), Ts, Ms, 100.0, 0.01, cuda=False)
    np.testing.assert_allclose(a["price"].cpu().numpy(), host.prices, rtol=1e-9, atol=PRICE_ATOL)
    assert_iv_close(a["iv"].cpu().numpy(), host)


def test_nonfinite_inputs_on_device():
    r = returns(8, 4, 100, 20)
    r[1, 3, 2] = np.nan
    r[3, 7, 19] = np.inf                                                  # beyond max Ts = 10: ignored
    w = np.ones((4, 100))
    w[2, 0] = np.nan
    w[0, 5] = 0.0
    r[0, 5, :] = np.nan                                                   # zero weight: ignored
    dev, host = both(r, w, [5, 10], [0.0, 1.0])
    assert list(dev.status) == [0, _native.PSH_HMC_STATUS_NONFINITE, _native.PSH_HMC_STATUS_WEIGHTS, 0]
    assert np.isnan(dev.prices[1:3]).all() and np.isnan(dev.sigma[1:3]).all()
    assert np.isfinite(dev.prices[[0, 3]]).all()
    assert_close(dev, host)


def test_invalid_arguments_return_error_codes():
    L = _native.load()
    x = torch.zeros((2, 8, 10), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, 1, 1), dtype=torch.float64, device="cuda")
    Ts, Ms = (C.c_int * 1)(5), (C.c_double * 1)(0.0)
    s = _native._stream_ptr(x.device)

    def call(k=8, ln=10, stride=10, ts=Ts, nT=1, degree=3, kind=0, x0=100.0, ptr=None):
        return L.psh_hedged_mc(x.device.index, s, x.data_ptr() if ptr is None else ptr, stride, 2, k, ln, None, x0, 0.0,
                               ts, nT, Ms, 1, degree, kind, out.data_ptr(), out.data_ptr(), out.data_ptr(), None, None)
    assert call() == _native.PSH_OK
    torch.cuda.synchronize()
    assert call(ptr=0) == -1
    assert call(stride=5) == -1
    assert call(ts=(C.c_int * 1)(11)) == -1
    assert call(ts=(C.c_int * 1)(0)) == -1
    assert call(degree=0) == -1
    assert call(kind=3) == -1
    assert call(x0=-1.0) == -1
    assert call(k=0) == -1
    assert call(degree=6) == -2
    assert call(k=_native.PSH_MAX_K + 1) == -2
    with pytest.raises(_native.NativeLibraryError):
        _native.hedged_mc(x, None, [5], [0.0], degree=6)


def test_compute_smile_device_equals_host():
    r = returns(21, 2, 2048, 30)
    x = sa.PriceData(dlnx=r, x_init=100.0).x
    ave = sa.DiscreteProba(softmax_weights(2, 2, 2048))
    hs = sa.compute_smile(x, [10, 30], np.linspace(-2, 2, 9), ave=ave)
    ds = sa.compute_smile(torch.from_numpy(x).cuda(), [10, 30], np.linspace(-2, 2, 9), ave=ave)     # cuda=None: the device
    np.testing.assert_allclose(ds.prices, hs.prices, rtol=1e-9, atol=PRICE_ATOL)
    assert_iv_close(ds.ivs, hs)


def test_path_shadowing_smile_on_device_equals_host():
    from shadowing_amd import synthetic as syn
    ds = syn.dataset(256, 1024, 0)
    q = syn.rolling_queries(3, 20, 1)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20), cache=True)
    Ts, Ms = [5, 10, 20], np.linspace(-2, 2, 9)
    dev = obj.smile(q, 256, Ts, Ms, eta=0.1, r=0.01, cuda=True)
    assert obj.last_path == "hip"
    d, paths, _ = obj.shadow(q, k=256, cuda=True)
    host = obj.smile_from_paths(d, paths, Ts, Ms, eta=0.1, r=0.01)
    np.testing.assert_array_equal(dev.status, host.status)
    np.testing.assert_allclose(dev.prices, host.prices, rtol=1e-9, atol=PRICE_ATOL)
    assert_iv_close(dev.ivs, host)
    uni = obj.smile(q, 256, Ts, Ms, proba_name="uniform", cuda=True)
    uh = obj.smile_from_paths(d, paths, Ts, Ms, proba_name="uniform")
    np.testing.assert_allclose(uni.prices, uh.prices, rtol=1e-9, atol=PRICE_ATOL)
