"""psh_calibrate_weights on the MI355X against the definition of README "Calibrating to market quotes" and its numpy twin.

The comparison rule (tests/_calibration.py states the bounds):
  1. Consistency.  q recomputed in long double from the DEVICE's lambda by the definition; the device's weights within
       (2 k + 16) 2^-53 + 4 max_i A_i   relative,   A_i = sum_j |lambda_j| (4 S_ij / x_init + (J + 5) |h_ij|) 2^-53.
     tests/test_calibration_cpu.py holds the twin alone to a small share of it.
  2. Optimality.  The long-double gradient at the device's lambda is at most tol + 2 (k + 2) 2^-53 sum_i q_i |h_ij|, unless the
     status says not converged.
  3. Device against twin on the planted inputs: both within 2 (|grad(lam)| + |grad(lam*)|) / sigma_min(H(lam*)) of lambda*,
     and the weights within 2 max_i |h_i|_2 times the sum of the two sides' bounds, relative.
Zero weights, NaN patterns and status words are exact; two calls give equal bits; a date's bits are the same alone and among
300."""
import functools
import math

import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, calibration as cal

import _calibration as C

pytestmark = pytest.mark.gpu

L = 12
KS = (1, 2, 63, 64, 65, 1023, 1025, 16384)
# J: (nT, Ts, nM, martingale)
CONFIGS = {1: ((L,), 1, False), 2: ((1,), 1, True), 31: ((L,), 30, True), 32: ((1, 3, 7, L), 7, True)}
EPS = (0.0, 1e-6, 1e-3)
SHARES = {"weights": 0.0, "gradient": 0.0}


@functools.lru_cache(maxsize=None)
def case(k, J, B=3):
    """(r (B, k, L), prior (B, k) or None, Ts, strike, target (B, nT, nM), martingale, eps) with quotes that a tilt of the prior
    prices: attainable where k allows.  Odd k take a Softmax prior with a few zero weights, whose paths hold NaN returns."""
    Ts, nM, mart = CONFIGS[J]
    seed = 1000 * J + k
    g = np.random.default_rng(seed)
    r = C.returns(k, L, seed, B)
    prior = None
    if k % 2:
        d = (np.abs(g.standard_normal((B, k))) * 0.1).astype(np.float32)
        prior = sa.softmax_weights(d, [0.1], cuda=False)[0, 0].copy()
        if k > 2:
            prior[:, ::7] = 0.0
            r[:, ::7, 0] = np.nan
    Ms = np.linspace(-1.5, 1.5, nM) if nM > 1 else np.array([0.0])
    strike = np.broadcast_to(C.strikes_at(Ts, Ms), (B, len(Ts), nM)).copy()
    target = np.empty_like(strike)
    for b in range(B):
        p = np.ones(k) if prior is None else prior[b]
        live = p > 0
        tilt = p[live] * np.exp(0.3 * g.standard_normal(int(live.sum())))
        inst = cal.instruments(C.X0, 0.0, Ts, strike[b], strike[b], 0, False)
        target[b] = ((tilt / tilt.sum()) @ cal.payoffs(cal.terminal_prices(r[b][live], Ts, C.X0), inst)).reshape(len(Ts), nM)
    if nM > 3:
        target[:, 0, 1] = np.nan                                   # one instrument is not quoted
    return r, prior, list(Ts), strike, target, mart, EPS[(KS.index(k) + J) % 3]


def on_device(dev, r, prior, Ts, strike, target, mart, eps, tol=1e-8, max_iter=100, strided=False):
    x = torch.from_numpy(r).to(dev)
    if strided:
        wide = torch.full((r.shape[0], r.shape[1], r.shape[2] + 5), float("nan"), dtype=torch.float32, device=dev)
        wide[:, :, 3:3 + r.shape[2]] = x
        x = wide[:, :, 3:3 + r.shape[2]]
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    out = _native.calibrate_weights(x, up(prior), Ts, up(strike), up(target), C.X0, 0.0, 0, mart, eps, tol, max_iter)
    return {name: t.cpu().numpy() for name, t in out.items()}


def check_against_definition(got, r, prior, Ts, strike, target, mart, eps, tol=1e-8, dates=None):
    """Parts 1 and 2 of the rule for every date; the largest shares."""
    k = r.shape[1]
    ws = gs = 0.0
    for b in (range(r.shape[0]) if dates is None else dates):
        lam, st = got["lam"][b], int(got["status"][b])
        assert st & 7 == 0, st
        J = lam.shape[0]
        ex = C.exact(r[b], None if prior is None else prior[b], Ts, strike[b], target[b], lam, martingale=mart, eps=eps)
        q = ex["q"].astype(np.float64)
        w = got["weights"][b]
        assert (w[~ex["live"]] == 0.0).all() and not np.signbit(w).any()      # (a live path's exp may underflow to 0 as well)
        assert (lam[~ex["act"]] == 0.0).all()
        share = np.abs(w - ex["q"]).astype(np.float64)[ex["live"]] / (C.weight_bound(ex, lam, k, J) * q[ex["live"]] + 2.0 ** -1070)
        ws = max(ws, float(share.max()))
        assert abs(float(w.sum()) - 1.0) <= (2 * k + 16) * C.U
        if not st & cal.STATUS_NOT_CONVERGED:
            gshare = np.abs(ex["grad"]).astype(np.float64) / C.gradient_bound(ex, k, tol)
            gs = max(gs, float(gshare.max()))
            # model_j = sum q_i g_ij: the weights' bound and a k-term sum on sum q |g|, and S_T's 3 ulps through S - K
            ql, g = ex["ql"].astype(np.float64), np.abs(ex["g"]).astype(np.float64)
            slack = (C.weight_bound(ex, lam, k, J) + (k + 4) * C.U) * (ql @ g) + 4 * C.U * (ql @ ex["S"][:, ex["qidx"]])
            assert (np.abs(got["model"][b] - (ex["ql"] @ ex["g"]).astype(np.float64)) <= slack).all()
            assert abs(got["info"][b, 1] - 1.0 / float((q * q).sum())) <= 1e-9 * got["info"][b, 1]
    return ws, gs


@pytest.mark.parametrize("J", sorted(CONFIGS))
@pytest.mark.parametrize("k", KS)
def test_device_against_the_definition(hip_device, k, J):
    r, prior, Ts, strike, target, mart, eps = case(k, J)
    got = on_device(hip_device, r, prior, Ts, strike, target, mart, eps, strided=(k + J) % 2 == 1)
    ws, gs = check_against_definition(got, r, prior, Ts, strike, target, mart, eps)
    SHARES["weights"], SHARES["gradient"] = max(SHARES["weights"], ws), max(SHARES["gradient"], gs)
    print(f"k = {k}, J = {J}, eps = {eps}: status {got['status']}, steps {got['info'][:, 2]}, weights use {ws:.4f} of the bound, "
          f"the gradient {gs:.4f}; largest so far {SHARES['weights']:.4f}, {SHARES['gradient']:.4f}")
    assert ws <= 1.0 and gs <= 1.0, (ws, gs)
    twin = cal.calibrate_host(r, prior, Ts, strike, target, C.X0, 0.0, 0, mart, eps)
    print(f"    twin: status {twin['status']}, steps {twin['info'][:, 2]}")
    assert np.array_equal(got["status"], twin["status"])
    again = on_device(hip_device, r, prior, Ts, strike, target, mart, eps, strided=(k + J) % 2 == 0)
    for name in got:                                                    # two calls, either row stride: equal bits
        assert np.array_equal(got[name], again[name], equal_nan=True), name


@pytest.mark.parametrize("k", (63, 65, 1025, 16384))
def test_device_and_twin_at_a_planted_multiplier(hip_device, k):
    r, strike, target, lam_star, mart = C.planted(k)
    got = on_device(hip_device, r, None, list(C.PLANT_TS), strike, target, mart, 0.0, tol=1e-11)
    twin = cal.calibrate_host(r, None, C.PLANT_TS, strike, target, C.X0, 0.0, 0, mart, 0.0, 1e-11)
    bounds = []
    for side, res in (("device", got), ("twin", twin)):
        b, smin, g1, g2 = C.stationary_bound(r, strike, target, res["lam"][0], lam_star)
        err = float(np.linalg.norm(res["lam"][0] - lam_star))
        print(f"k = {k}, {side}: status {res['status'][0]}, steps {res['info'][0, 2]}, |lam - lam*| = {err:.3e} of {b:.3e} "
              f"(sigma_min {smin:.2e}, gradients {g1:.2e}, {g2:.2e})")
        assert err <= b, (side, err, b)
        bounds.append(b)
    ex = C.exact(r[0], None, C.PLANT_TS, strike[0], target[0], lam_star)
    hmax = float(np.sqrt((ex["h"].astype(np.float64) ** 2).sum(axis=1)).max())
    rel = np.abs(got["weights"][0] - twin["weights"][0]) / twin["weights"][0]
    bound = 2.0 * hmax * (bounds[0] + bounds[1]) + 2 * (2 * k + 16) * C.U
    print(f"    weights: device against twin {float(rel.max()):.3e} of {bound:.3e}")
    assert float(rel.max()) <= bound


def test_a_date_alone_and_among_300(hip_device):
    """More dates than compute units: every date within the rule, and date 137's bits the same alone."""
    r, prior, Ts, strike, target, mart, _ = case(65, 32, B=300)
    got = on_device(hip_device, r, prior, Ts, strike, target, mart, 1e-6)
    ws, gs = check_against_definition(got, r, prior, Ts, strike, target, mart, 1e-6, dates=(0, 137, 299))
    print(f"B = 300: weights use {ws:.4f} of the bound, the gradient {gs:.4f}; statuses {np.unique(got['status'])}")
    assert ws <= 1.0 and gs <= 1.0
    cut = lambda a: None if a is None else a[137:138]   # noqa: E731
    alone = on_device(hip_device, cut(r), cut(prior), Ts, cut(strike), cut(target), mart, 1e-6)
    for name in got:
        assert np.array_equal(got[name][137:138], alone[name], equal_nan=True), name


def test_flags_nan_patterns_and_scaling(hip_device):
    r, prior, Ts, strike, target, mart, _ = case(65, 32, B=3)
    base = on_device(hip_device, r, prior, Ts, strike, target, mart, 1e-6)
    scaled = on_device(hip_device, r, prior * 2.0 ** -7, Ts, strike, target, mart, 1e-6)
    for name in base:                                                   # a power of two on the prior: no bit moves
        assert np.array_equal(base[name], scaled[name], equal_nan=True), name
    # a NaN return on a live path of date 0, a negative weight on date 1, a zero strike on date 2
    r2, p2, K2 = r.copy(), prior.copy(), strike.copy()
    r2[0, 1, 2], p2[1, 3], K2[2, 1, 1] = np.inf, -1.0, 0.0
    bad = on_device(hip_device, r2, p2, Ts, K2, target, mart, 1e-6)
    twin = cal.calibrate_host(r2, p2, Ts, K2, target, C.X0, 0.0, 0, mart, 1e-6)
    assert bad["status"].tolist() == [1, 2, 4] == twin["status"].tolist()
    for name in ("weights", "lam", "model", "info"):
        assert np.isnan(bad[name]).all() and np.isnan(twin[name]).all(), name
    # a NaN return past the longest maturity, or on a path of weight 0, is not looked at
    r3 = np.concatenate([r, np.full((3, r.shape[1], 2), np.nan, dtype=np.float32)], axis=2)
    same = on_device(hip_device, r3, prior, Ts, strike, target, mart, 1e-6)
    for name in base:
        assert np.array_equal(base[name], same[name], equal_nan=True), name
    # nothing quoted, no forwards: the normalised prior
    none = on_device(hip_device, r, prior, Ts, strike, np.full_like(target, np.nan), False, 1e-6)
    twin = cal.calibrate_host(r, prior, Ts, strike, np.full_like(target, np.nan), C.X0, 0.0, 0, False, 1e-6)
    assert not none["status"].any() and (none["lam"] == 0.0).all() and (none["info"][:, 2] == 0.0).all()
    assert np.allclose(none["weights"], prior / prior.sum(axis=1, keepdims=True), rtol=(2 * 65 + 16) * C.U, atol=0.0)
    assert np.allclose(none["weights"], twin["weights"], rtol=(2 * 65 + 16) * C.U, atol=0.0)


def test_unattainable_and_redundant_quotes(hip_device):
    r = C.returns(257, L, 5)
    Ts, K = [L], np.full((1, 1, 1), 100.0)
    high = np.full((1, 1, 1), 1e4)                                      # above the largest payoff
    hard = on_device(hip_device, r, None, Ts, K, high, False, 0.0)
    assert hard["status"][0] & cal.STATUS_NOT_CONVERGED and np.isfinite(hard["weights"]).all() and np.isfinite(hard["lam"]).all()
    soft = on_device(hip_device, r, None, Ts, K, high, False, 1e-3)
    assert soft["status"][0] == 0
    resid = soft["model"][0, 0] - 1e4
    assert abs(resid + 1e-3 * soft["lam"][0, 0] * C.X0) <= 1e-8 * C.X0 + 1e-9 * abs(resid)
    # the same call quoted twice: identical columns, the second unknown is dropped and the first converges
    S = cal.terminal_prices(r[0], Ts, C.X0)[:, 0]
    price = float(np.maximum(S - 101.0, 0.0).mean()) + 0.05
    Kc, x = np.full((1, 1, 2), 101.0), torch.from_numpy(r).to(hip_device)
    dup = np.array([[[price, price]]])
    out = _native.calibrate_weights(x, None, Ts, torch.from_numpy(Kc).to(hip_device), torch.from_numpy(dup).to(hip_device), C.X0, 0.0,
                                    _native.PSH_HMC_CALL, True, 0.0, 1e-8, 100)
    assert int(out["status"][0]) == cal.STATUS_DROPPED and float(out["lam"][0, 1]) == 0.0
    assert float(out["info"][0, 3]) <= 1e-8


def test_argument_errors_and_routing(hip_device):
    r, prior, Ts, strike, target, mart, _ = case(65, 2)
    x = torch.from_numpy(r).to(hip_device)
    K, c = torch.from_numpy(strike).to(hip_device), torch.from_numpy(target).to(hip_device)
    for kw in ({"eps": -1.0}, {"eps": math.nan}, {"tol": 0.0}, {"max_iter": -1}):
        with pytest.raises(ValueError):
            _native.calibrate_weights(x, None, Ts, K, c, **kw)
    with pytest.raises(ValueError):
        _native.calibrate_weights(x, None, [L + 1], K, c)
    with pytest.raises(_native.NativeLibraryError):                   # 33 instruments
        _native.calibrate_weights(x, None, Ts, K.expand(3, 1, 33).contiguous(), c.expand(3, 1, 33).contiguous(), martingale=False)
    lib, size = _native.load(), __import__("ctypes").c_size_t(0)
    assert lib.psh_calibrate_workspace_bytes(3, 65, 1, size) == 0 and size.value >= 3 * 65 * 8
    ws = torch.empty(8, dtype=torch.int64, device=hip_device)         # too small a workspace: PSH_ERR_WORKSPACE
    out = {n: torch.empty(3 * 65, dtype=torch.float64, device=hip_device) for n in "wlmi"}
    st = torch.empty(3, dtype=torch.int32, device=hip_device)
    Tarr = (__import__("ctypes").c_int * 1)(1)
    assert lib.psh_calibrate_weights(0, None, x.data_ptr(), L, 3, 65, L, None, 100.0, 0.0, Tarr, 1, K.data_ptr(), c.data_ptr(), 1, 0, 1,
                                     1e-6, 1e-8, 100, out["w"].data_ptr(), out["l"].data_ptr(), out["m"].data_ptr(),
                                     out["i"].data_ptr(), st.data_ptr(), ws.data_ptr(), 64) == -3
    # the public entry: prices in, a HIP tensor of weights out; cuda=None follows the tensor
    px = C.X0 * np.exp(np.concatenate([np.zeros((3, 65, 1)), np.cumsum(r.astype(np.float64), axis=2)], axis=2))
    quotes = sa.MarketQuotes(Ts, strike, prices=target)
    ave = sa.Softmax(np.zeros((3, 65)), 1.0)                              # any `ave`: what counts is its weights
    ave.weights = prior                                                   # (the paths of weight 0 hold NaN returns)
    dev = sa.calibrate_weights(torch.from_numpy(np.nan_to_num(px, nan=C.X0)).to(hip_device), quotes, ave=ave)
    host = sa.calibrate_weights(np.nan_to_num(px, nan=C.X0), quotes, ave=ave)
    assert isinstance(dev.weights, torch.Tensor) and dev.weights.is_cuda and isinstance(host.weights, np.ndarray)
    for res in (dev, host):
        quoted = ~np.isnan(res.residual)
        assert not res.status.any() and res.weights.shape == (3, 65)
        assert (np.abs(res.residual + 1e-6 * res.lam * C.X0)[quoted] <= 1e-8 * C.X0 * (1 + 1e-6)).all()
    with pytest.raises(_native.NativeLibraryError):
        sa.calibrate_weights(np.ones((1, 16385, 3)), sa.MarketQuotes([1], np.full((1, 1), 1.0), prices=np.full((1, 1), 0.1)), cuda=True)
