"""psh_hedged_mc_policy and psh_hedge_replay on the MI355X: the fit with its policy kept against psh_hedged_mc (bit for
bit), policy and report against the numpy twin (shadowing_amd.pricing), the replay of a device policy on other paths
against replay_host of the same bits, full binomial trees against Cox-Ross-Rubinstein, put-call path by path, bad inputs,
repeatability, argument errors, and PathShadowing.smile(report=True, cuda=True).  Shapes: every k around the wave, block
and path-tile edges, T = 1, 2 and L, strike groups of 1, 3, 3 + 1 and 3 + 3 + 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, pricing
import _hmc_reference as ref
import _hmc_report_reference as rep

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_device")]
RTOL = ATOL = 1e-9                                            # the project's agreement rule (tests/test_gpu_hmc.py)
TILE = 512                                                    # PSH_HEDGE_TILE
FIT_OUTPUTS = ("price", "iv", "strike", "sigma", "status")
RESULTS = ("mean", "mc", "risk", "risk_unhedged", "se", "se_unhedged", "n_eff")


def close(a, b):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(out):
    return {name: t.cpu().numpy() for name, t in out.items()}


def moneyness(nM):
    return list(np.linspace(-1.5, 1.5, nM)) if nM > 1 else [0.3]


def device_fit(r, w, Ts, Ms, rate, degree, kind):
    return _native.hedged_mc(dev(r), dev(w), Ts, Ms, 100.0, rate, degree, pricing.KINDS[kind], policy=True)


def device_replay(fit, r, w, Ts, Ms, rate, degree, kind, pnl=True):
    return host(_native.hedge_replay(dev(r), dev(w), Ts, Ms, fit["policy"], fit["strike"], fit["price"], 100.0, rate, degree,
                                     pricing.KINDS[kind], return_pnl=pnl))


@pytest.mark.parametrize("degree", [1, 3, 5])
@pytest.mark.parametrize("weighted", [False, True])
def test_fit_outputs_are_those_of_psh_hedged_mc_bit_for_bit(degree, weighted):
    B, k, L, Ts, Ms = 3, 300, 12, [1, 5, 12], moneyness(4)
    r, w = rep.mrw_like_returns(degree, B, k, L)
    w = dev(w) if weighted else None
    wide = torch.zeros((B, k, L + 5), dtype=torch.float32, device="cuda")
    wide[:, :, 2:2 + L] = dev(r)
    for x in (dev(r), wide[:, :, 2:2 + L]):                   # contiguous, and a strided view (row_stride > L)
        plain = _native.hedged_mc(x, w, Ts, Ms, 100.0, 0.03, degree, _native.PSH_HMC_OTM)
        kept = _native.hedged_mc(x, w, Ts, Ms, 100.0, 0.03, degree, _native.PSH_HMC_OTM, policy=True)
        for name in FIT_OUTPUTS:
            assert torch.equal(plain[name].view(torch.int64 if plain[name].dtype == torch.float64 else torch.int32),
                               kept[name].view(torch.int64 if kept[name].dtype == torch.float64 else torch.int32)), name
        assert np.isfinite(host(kept)["price"]).all()
        pol = kept["policy"].cpu().numpy()
        assert pol.shape == (B, 3, 4, 12, 2 * degree + 4)
        for q, T in enumerate(Ts):                            # rows n >= T are 0, row 0 is the basis {1} at x_init
            assert (pol[:, q, :, T:, :] == 0).all() and (pol[:, q, :, :T, 0] != 0).all()
            assert (pol[:, q, :, 0, 0] == 100.0).all() and (pol[:, q, :, 0, 1] == 0.0).all()
            np.testing.assert_array_equal(pol[:, q, :, 0, 2], host(kept)["price"][:, q])      # gamma_0[0] = V_0


CASES = [  # k, Ts, nM, degree, kind, rate, weighted
    (1, [1, 2, 12], 1, 1, "otm", 0.0, False),
    (63, [1, 2, 12], 3, 3, "call", 0.05, True),
    (65, [2, 12], 4, 1, "put", 0.0, True),
    (257, [1, 12], 7, 5, "otm", 0.05, True),
    (TILE + 1, [1, 2, 12], 4, 3, "otm", 0.0, False),
    (TILE + 1, [12], 7, 5, "put", 0.05, True),
    (257, [2], 1, 3, "call", 0.0, True),
]


@pytest.mark.parametrize("k,Ts,nM,degree,kind,rate,weighted", CASES)
def test_device_policy_and_report_match_the_twin(k, Ts, nM, degree, kind, rate, weighted):
    r, w = rep.mrw_like_returns(k + degree, 2, k, 12)
    w = w if weighted else None
    Ms = moneyness(nM)
    tw = pricing.hedged_mc_host(r, w, Ts, Ms, 100.0, rate, degree, pricing.KINDS[kind], policy=True)
    tr = pricing.replay_host(r, w, Ts, Ms, tw["policy"], tw["strike"], tw["price"], 100.0, rate, degree, pricing.KINDS[kind],
                             return_pnl=True)
    fit = device_fit(r, w, Ts, Ms, rate, degree, kind)
    out = device_replay(fit, r, w, Ts, Ms, rate, degree, kind)
    fit = host(fit)
    np.testing.assert_array_equal(fit["status"], tw["status"])
    assert (tw["status"] == 0).all()
    for name in ("price", "strike", "sigma"):
        close(fit[name], tw[name])
    assert fit["policy"].shape == tw["policy"].shape
    close(fit["policy"][:, :, :, 0, degree + 3], tw["policy"][:, :, :, 0, degree + 3])       # delta
    close(fit["policy"][..., :2], tw["policy"][..., :2])                                     # mu, isd
    np.testing.assert_array_equal(out["status"], tr["status"])
    close(out["sums"], tr["sums"])
    close(out["pnl"], tr["pnl"])
    got, want = pricing.report_from_sums(out["sums"], fit["price"]), pricing.report_from_sums(tr["sums"], tw["price"])
    for name in RESULTS:
        close(got[name], want[name])
    assert np.abs(out["sums"][..., 0]).max() <= 1e-9                                         # in-sample a1 = 0
    # the public path: the same numbers through report=True
    sm = pricing.smile_from_log_returns(dev(r), dev(w), Ts, Ms, 100.0, rate, degree=degree, kind=kind, cuda=True, report=True)
    hs = pricing.smile_from_log_returns(r, w, Ts, Ms, 100.0, rate, degree=degree, kind=kind, cuda=False, report=True)
    for name in pricing.REPORT_FIELDS:
        if name != "iv_se":
            close(getattr(sm, name), getattr(hs, name))
    assert isinstance(sm.policy.coef, torch.Tensor) and sm.policy.coef.is_cuda


@pytest.mark.parametrize("degree,kind,rate", [(3, "otm", 0.05), (5, "call", 0.0)])
def test_replay_on_other_paths_matches_replay_host(degree, kind, rate):
    B, k, k2, L, Ts, Ms = 2, 300, 2 * TILE + 76, 12, [1, 5, 12], moneyness(4)        # three tiles, a ragged last one
    r, w = rep.mrw_like_returns(40 + degree, B, k, L)
    r2, w2 = rep.mrw_like_returns(50 + degree, B, k2, L)
    r2[:, w2[0] == 0, 3] = np.nan                              # zero-weight paths with NaN returns: not read
    w2[1] = w2[0]
    assert (w2 == 0).any() and np.isnan(r2).any()
    fit = device_fit(r, w, Ts, Ms, rate, degree, kind)
    f = host(fit)
    want = pricing.replay_host(r2, w2, Ts, Ms, f["policy"], f["strike"], f["price"], 100.0, rate, degree, pricing.KINDS[kind],
                               return_pnl=True)
    with_pnl = device_replay(fit, r2, w2, Ts, Ms, rate, degree, kind, pnl=True)
    without = device_replay(fit, r2, w2, Ts, Ms, rate, degree, kind, pnl=False)
    assert "pnl" not in without
    np.testing.assert_array_equal(with_pnl["sums"].view(np.int64), without["sums"].view(np.int64))
    assert (with_pnl["status"] == 0).all() and np.isfinite(with_pnl["sums"]).all()
    close(with_pnl["sums"], want["sums"])
    close(with_pnl["pnl"], want["pnl"])
    assert np.isnan(with_pnl["pnl"][:, :, :, w2[0] == 0]).all() and np.isfinite(with_pnl["pnl"][:, :, :, w2[0] != 0]).all()
    # uniform weights (NULL) on the same paths, cleaned
    r3 = np.nan_to_num(r2)
    uni = device_replay(fit, r3, None, Ts, Ms, rate, degree, kind)
    close(uni["sums"], pricing.replay_host(r3, None, Ts, Ms, f["policy"], f["strike"], f["price"], 100.0, rate, degree,
                                           pricing.KINDS[kind])["sums"])
    close(uni["sums"][..., 8], 1.0 / k2)


@pytest.mark.parametrize("P,rate", [(1, 0.0), (3, 0.05), (5, 0.0), (5, 0.05)])
def test_binomial_tree_on_device(P, rate):
    T = min(P + 1, 4)
    r, w, K, sig, crr = ref.binomial_case(P, T, 4, rate, "otm", 10 * P + T, zero_half=True)
    x = torch.from_numpy(sa.PriceData(dlnx=r, x_init=100.0).x).cuda()
    sm = sa.compute_smile(x, [T], ref.MS, r=rate, ave=sa.DiscreteProba(w), degree=P, report=True)       # cuda=None: device
    assert sm.status == 0
    close(sm.prices[0], crr)
    assert (sm.risk <= 1e-9).all() and (sm.price_se <= 1e-9).all()
    close(sm.delta[0], [rep.crr_delta(100.0, K[j], ref.A, rate, T, ref.MS[j] >= 0) for j in range(len(ref.MS))])
    h = sa.hedge_pnl(sm.policy, x, ave=sa.DiscreteProba(w), return_paths=True)
    assert np.isnan(h.pnl[0][:, w == 0]).all()
    close(h.pnl[0][:, w != 0], np.broadcast_to(crr[:, None], h.pnl[0].shape)[:, w != 0])
    assert (h.risk <= 1e-9).all()


def test_put_call_identity_per_path_out_of_sample():
    B, k, k2, L, Ts, Ms, rate = 2, 300, TILE + 40, 12, [2, 12], moneyness(4), 0.05
    r, w = rep.mrw_like_returns(60, B, k, L)
    r2, w2 = rep.mrw_like_returns(61, B, k2, L)
    call = device_fit(r, w, Ts, Ms, rate, 3, "call")
    put = device_fit(r, w, Ts, Ms, rate, 3, "put")
    assert torch.equal(call["strike"], put["strike"])
    pc = device_replay(call, r2, w2, Ts, Ms, rate, 3, "call")["pnl"]
    pp = device_replay(put, r2, w2, Ts, Ms, rate, 3, "put")["pnl"]
    want = 100.0 - call["strike"].cpu().numpy() * np.exp(-rate / 252.0 * np.array(Ts))[None, :, None]
    for b in range(B):
        live = w2[b] != 0
        close((pc[b] - pp[b])[:, :, live], np.broadcast_to(want[b][:, :, None], pc[b].shape)[:, :, live])


def test_bad_replay_inputs_and_a_flagged_maturity():
    B, k, L, Ts, Ms = 3, 200, 12, [3, 8], [0.0, 1.0]
    r, w = rep.mrw_like_returns(70, B, k, L)
    fit = device_fit(r, w, Ts, Ms, 0.0, 2, "otm")
    r2, w2 = rep.mrw_like_returns(71, B, TILE + 8, L)
    w2[1, TILE + 3], r2[1, TILE + 3, 2] = 1.0, np.nan          # a weighted path of the second tile
    w2[0, 5], r2[0, 5, 9] = 1.0, np.inf                        # beyond max Ts = 8: ignored
    w2[2, 7] = np.nan
    out = device_replay(fit, r2, w2, Ts, Ms, 0.0, 2, "otm")
    assert list(out["status"]) == [0, _native.PSH_HMC_STATUS_NONFINITE, _native.PSH_HMC_STATUS_WEIGHTS]
    assert np.isfinite(out["sums"][0]).all() and np.isfinite(out["pnl"][0][:, :, w2[0] != 0]).all()
    assert np.isnan(out["sums"][1:]).all() and np.isnan(out["pnl"][1:]).all()
    f = host(fit)
    want = pricing.replay_host(r2, w2, Ts, Ms, f["policy"], f["strike"], f["price"], 100.0, 0.0, 2, 0)
    np.testing.assert_array_equal(out["status"], want["status"])
    close(out["sums"], want["sums"])
    # a maturity the fit flags: NaN there, in the fit's own report and in a replay; finite elsewhere
    rd, wd = ref.drift_returns(0.01, 1e-4)
    x = torch.from_numpy(sa.PriceData(dlnx=rd, x_init=100.0).x).cuda()
    sm = sa.compute_smile(x, [1, 20], [-1.0, 0.0, 1.0], ave=sa.DiscreteProba(wd), degree=3, report=True)
    assert sm.status == _native.PSH_HMC_STATUS_ILL_CONDITIONED
    for name in ("prices", "delta", "price_mc", "risk", "risk_unhedged", "price_se", "price_se_unhedged", "n_eff"):
        v = getattr(sm, name)
        assert np.isnan(v[1]).all() and np.isfinite(v[0]).all(), name
    h = sa.hedge_pnl(sm.policy, x, ave=sa.DiscreteProba(wd), return_paths=True)
    assert np.isnan(h.sums[1]).all() and np.isnan(h.pnl[1]).all() and h.status == 0
    assert np.isfinite(h.sums[0]).all() and np.isfinite(h.pnl[0][:, wd != 0]).all()


def test_two_calls_give_identical_bits():
    B, k, L, Ts, Ms = 2, 2 * TILE + 5, 12, [1, 5, 12], moneyness(7)
    r, w = rep.mrw_like_returns(80, B, k, L)
    a, b = device_fit(r, w, Ts, Ms, 0.02, 5, "otm"), device_fit(r, w, Ts, Ms, 0.02, 5, "otm")
    for name in a:
        assert torch.equal(a[name], b[name]) or (name in ("price", "iv") and torch.equal(a[name].view(torch.int64), b[name].view(torch.int64))), name
    ra, rb = device_replay(a, r, w, Ts, Ms, 0.02, 5, "otm"), device_replay(a, r, w, Ts, Ms, 0.02, 5, "otm")
    for name in ra:
        np.testing.assert_array_equal(ra[name].view(np.int64 if ra[name].dtype == np.float64 else np.int32),
                                      rb[name].view(np.int64 if rb[name].dtype == np.float64 else np.int32))


def test_invalid_arguments_return_error_codes():
    L = _native.load()
    x = torch.zeros((2, 8, 10), dtype=torch.float32, device="cuda")
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    Ts, Ms = (C.c_int * 1)(5), (C.c_double * 1)(0.0)
    s = _native._stream_ptr(x.device)
    n = C.c_size_t(0)
    assert L.psh_hmc_policy_doubles(2, 1, 1, 5, 3, C.byref(n)) == 0 and n.value == 2 * 5 * 10
    assert L.psh_hmc_policy_doubles(2, 1, 1, 5, 3, None) == -1 and L.psh_hmc_policy_doubles(2, 1, 1, 5, 6, C.byref(n)) == -2
    assert L.psh_hedge_replay_workspace_bytes(2, 8, 1, 1, C.byref(n)) == 0 and n.value == 2 * 11 * 8
    assert L.psh_hedge_replay_workspace_bytes(2, 8, 1, 1, None) == -1

    def fit(degree=3, pol=buf.data_ptr()):
        return L.psh_hedged_mc_policy(x.device.index, s, x.data_ptr(), 10, 2, 8, 10, None, 100.0, 0.0, Ts, 1, Ms, 1, degree, 0,
                                      buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, None, pol)

    def replay(degree=3, pol=buf.data_ptr(), sums=buf[1024:].data_ptr(), ws=buf[2048:].data_ptr(), nbytes=n.value, k=8, stride=10):
        return L.psh_hedge_replay(x.device.index, s, x.data_ptr(), stride, 2, k, 10, None, 100.0, 0.0, Ts, 1, Ms, 1, degree, 0,
                                  pol, buf.data_ptr(), buf.data_ptr(), sums, None, None, ws, nbytes)
    assert fit() == _native.PSH_OK and replay() == _native.PSH_OK
    torch.cuda.synchronize()
    assert fit(pol=None) == -1 and fit(degree=0) == -1 and fit(degree=6) == -2
    assert replay(pol=None) == -1 and replay(sums=None) == -1 and replay(ws=None) == -1 and replay(stride=5) == -1
    assert replay(degree=0) == -1 and replay(degree=6) == -2 and replay(nbytes=n.value - 8) == -3


def test_path_shadowing_smile_report_on_device_equals_host():
    from shadowing_amd import synthetic as syn
    ds = syn.dataset(64, 256, 0)
    q = syn.rolling_queries(3, 20, 1)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20), cache=True)
    Ts, Ms = [5, 20], np.linspace(-1.5, 1.5, 5)
    d = obj.smile(q, 128, Ts, Ms, eta=0.1, r=0.01, cuda=True, report=True)
    assert obj.last_path == "hip"
    h = obj.smile(q, 128, Ts, Ms, eta=0.1, r=0.01, cuda=False, report=True)
    np.testing.assert_array_equal(d.status, h.status)
    close(d.prices, h.prices)
    for name in pricing.REPORT_FIELDS:
        if name != "iv_se":
            close(getattr(d, name), getattr(h, name))
    tau = (np.asarray(Ts) / 252.0)[None, :, None]                                         # iv_se: its definition
    np.testing.assert_allclose(d.iv_se, d.price_se / pricing.bs_vega(100.0, d.strikes, tau, 0.01, d.ivs), rtol=1e-12)
    np.testing.assert_array_equal(np.isnan(d.iv_se), np.isnan(d.ivs))
    assert d.delta.shape == (3, 2, 5) and d.policy.coef.is_cuda and tuple(d.policy.coef.shape) == (3, 2, 5, 20, 10)
    plain = obj.smile(q, 128, Ts, Ms, eta=0.1, r=0.01, cuda=True)
    assert plain.delta is None and plain.policy is None
    np.testing.assert_array_equal(plain.prices, d.prices)
