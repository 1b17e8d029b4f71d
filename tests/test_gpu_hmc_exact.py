"""psh_hedged_mc on the MI355X against answers that neither host implementation produced (binomial trees priced by CRR,
deterministic paths, all-zero returns, put-call parity), against the independent restatement (tests/_hmc_reference.py)
at production shapes, and on the ill-conditioned regimes of drifting and of heavy-tailed paths, where the kernel, the
numpy twin and the restatement must flag the same maturities or agree."""
import math

import numpy as np
import pytest
import torch

from shadowing_amd import _native, pricing
import _hmc_reference as ref

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_device")]
ILL = _native.PSH_HMC_STATUS_ILL_CONDITIONED
A, MS, SWEEP_E = ref.A, ref.MS, ref.SWEEP_E
binomial_case, check_sweep_case = ref.binomial_case, ref.check_sweep_case
KIND = {"otm": _native.PSH_HMC_OTM, "call": _native.PSH_HMC_CALL, "put": _native.PSH_HMC_PUT}


def kernel(r, w, Ts, Ms, x0=100.0, rate=0.0, degree=3, kind="otm"):
    """(B, k, L) float32 returns, (B, k) weights or None -> dict of numpy arrays."""
    x = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)).cuda()
    wt = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).cuda()
    out = _native.hedged_mc(x, wt, Ts, Ms, x0, rate, degree, KIND[kind])
    return {name: t.cpu().numpy() for name, t in out.items()}


def date(res, b):
    return {name: v[b] for name, v in res.items()}


def test_status_bits_are_distinct():
    assert ILL == pricing.STATUS_ILL_CONDITIONED == 4
    assert len({_native.PSH_HMC_STATUS_NONFINITE, _native.PSH_HMC_STATUS_WEIGHTS, ILL}) == 3


@pytest.mark.parametrize("rate", [0.0, 0.05, -0.02])
@pytest.mark.parametrize("kind", ["otm", "call", "put"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_binomial_tree_is_crr_on_device(P, kind, rate):
    """Every T <= P + 1 of one tree of depth P + 1 (a T-prefix of a full tree is a full tree): the discounted CRR price,
    sigma = a sqrt(252), the closed-form strikes.  k = 3 * 2^(P+1) and PSH_MAX_K; random weights, half of them zero."""
    x0, D = 100.0, P + 1
    Ts = list(np.random.default_rng(P).permutation(np.arange(1, D + 1)))
    for reps, zero_half in [(3, False), (_native.PSH_MAX_K >> D, False), (_native.PSH_MAX_K >> D, True)]:
        r, w, _, sig, _ = binomial_case(P, D, reps, rate, kind, 100 * P + reps, zero_half)
        res = date(kernel(r[None], w[None], Ts, MS, x0, rate, P, kind), 0)
        assert res["status"] == 0
        np.testing.assert_allclose(res["sigma"], sig, rtol=1e-14)
        for q, T in enumerate(Ts):
            tau = T / 252.0
            K = x0 * math.exp(rate * tau) * np.exp(np.asarray(MS) * A * math.sqrt(T))      # sigma_T sqrt(tau) = a sqrt(T)
            call = [kind == "call" or (kind == "otm" and M >= 0) for M in MS]
            crr = [ref.crr_price(x0, K[j], A, rate, T, call[j]) for j in range(len(MS))]
            np.testing.assert_allclose(res["strike"][q], K, rtol=1e-14)
            np.testing.assert_allclose(res["price"][q], crr, rtol=0, atol=1e-12 * x0)


@pytest.mark.parametrize("P", [1, 3, 5])
def test_deterministic_paths_on_device(P):
    """k copies of one path (uniform and random weights), and one path with all the weight among random paths at w = 0:
    the price is e^{-rho T} payoff(S_T) (u = 0 at every step, beta_0 dropped)."""
    x0, Ts, rate = 100.0, [1, 4, 9], 0.04
    g = np.random.default_rng(P)
    path = (0.01 * g.standard_normal(9)).astype(np.float32)
    copies = np.tile(path, (300, 1))
    other = (0.01 * g.standard_normal((300, 9))).astype(np.float32)
    other[211] = path
    w1 = np.zeros(300)
    w1[211] = 2.5
    r = np.stack([copies, copies, other])
    w = np.stack([np.ones(300), g.uniform(0.1, 1.0, 300), w1])
    for kind in ["otm", "call", "put"]:
        res = kernel(r, w, Ts, MS, x0, rate, P, kind)
        assert (res["status"] == 0).all()
        call = np.array([kind == "call" or (kind == "otm" and M >= 0) for M in MS])
        for q, T in enumerate(Ts):
            ST = x0 * math.exp(float(np.sum(path[:T].astype(np.float64))))
            K = res["strike"][:, q]
            want = math.exp(-rate * T / 252.0) * np.where(call, np.maximum(ST - K, 0.0), np.maximum(K - ST, 0.0))
            np.testing.assert_allclose(res["price"][:, q], want, rtol=1e-13, atol=1e-13 * x0)


@pytest.mark.parametrize("rate", [0.0, 0.03])
def test_all_zero_returns_on_device(rate):
    x0, Ts = 100.0, [1, 5]
    r = np.zeros((1, 32, 5), dtype=np.float32)
    for kind in ["call", "put"]:
        res = date(kernel(r, None, Ts, MS, x0, rate, 3, kind), 0)
        assert res["status"] == 0 and (res["sigma"] == 0.0).all()
        for q, T in enumerate(Ts):
            tau = T / 252.0
            F = x0 * math.exp(rate * tau)
            np.testing.assert_allclose(res["strike"][q], F, rtol=1e-15)
            want = math.exp(-rate * tau) * (max(x0 - F, 0.0) if kind == "call" else max(F - x0, 0.0))
            np.testing.assert_allclose(res["price"][q], want, rtol=1e-13, atol=1e-13 * x0)
            if want < ref.bs(x0, F, tau, rate, 1e-4, kind == "call"):
                assert np.isnan(res["iv"][q]).all()
            else:
                np.testing.assert_allclose(res["iv"][q], ref.implied_vol(want, x0, F, tau, rate, kind == "call"), atol=1e-8)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_put_call_parity_on_device(P):
    """C - P = x0 - K e^{-rate tau} for any paths and weights (S_T - K is fitted exactly), on a batch of dates."""
    g = np.random.default_rng(70 + P)
    B, k, L = 3, 2048, 30
    sig = 0.25 * (0.5 + g.random((B, k, 1)))
    r = (sig * math.sqrt(1 / 252) * g.standard_normal((B, k, L)) + 0.0001).astype(np.float32)
    w = g.random((B, k))
    Ts, Ms, x0, rate = [1, 10, 30], np.linspace(-2, 2, 9), 100.0, 0.03
    c = kernel(r, w, Ts, Ms, x0, rate, P, "call")
    p = kernel(r, w, Ts, Ms, x0, rate, P, "put")
    assert (c["status"] == 0).all() and (p["status"] == 0).all()
    np.testing.assert_array_equal(c["strike"], p["strike"])
    tau = (np.asarray(Ts) / 252.0)[None, :, None]
    np.testing.assert_allclose(c["price"] - p["price"], x0 - c["strike"] * np.exp(-rate * tau), rtol=0, atol=1e-10 * x0)


SHAPES = [  # id, B, k, L, Ts, Ms, degree, kind, returns
    ("k8192", 1, 8192, 20, [3], [0.3], 3, "otm", "gbm"),
    ("k16384", 1, 16384, 20, [2], [-0.7, 0.9], 4, "call", "gbm"),
    ("L252_T75", 1, 300, 252, [75, 7], [-1.5, -0.2, 0.4, 1.8], 4, "put", "gbm"),
    ("deg4_otm_nM64", 1, 64, 20, [5], list(np.linspace(-2.5, 2.5, 64)), 4, "otm", "gbm"),
    ("nT64_unsorted", 1, 40, 30, "nT64", [0.0], 4, "call", "gbm"),
    ("student_t", 2, 1000, 40, [10, 40], [-1.0, 0.0, 1.0], 3, "otm", "student_t"),
]


@pytest.mark.parametrize("name,B,k,L,Ts,Ms,degree,kind,kind_r", SHAPES, ids=[s[0] for s in SHAPES])
def test_kernel_matches_restatement_at_production_shapes(name, B, k, L, Ts, Ms, degree, kind, kind_r):
    g = np.random.default_rng(k + L)
    if Ts == "nT64":
        Ts = [int(t) for t in g.integers(1, L + 1, _native.PSH_HMC_MAX_T)]
        Ts[5] = Ts[40] = L
    if kind_r == "gbm":
        sig = 0.2 * (0.5 + g.random((B, k, 1)))
        r = (sig * math.sqrt(1 / 252) * g.standard_normal((B, k, L)) - 0.5 * sig ** 2 / 252).astype(np.float32)
    else:
        r = ref.student_t_dates(5, B, k, L)[0]
    d = g.random((B, k))
    w = np.exp(-(d - d.min(axis=1, keepdims=True)) / 0.3)
    res = kernel(r, w, Ts, Ms, 100.0, 0.01, degree, kind)
    assert (res["status"] == 0).all()
    assert np.isfinite(res["price"]).all()
    for b in range(B):
        rf = ref.hmc_date(r[b], w[b], 100.0, 0.01, Ts, Ms, degree, kind)
        assert rf["status"] == 0
        np.testing.assert_allclose(res["strike"][b], rf["strike"], rtol=1e-12)
        np.testing.assert_allclose(res["sigma"][b], rf["sigma"], rtol=1e-12)
        np.testing.assert_allclose(res["price"][b], rf["price"], rtol=1e-9, atol=1e-9)
        ref.assert_iv_close(res["iv"][b], rf["iv"], rf["price"], rf["strike"], Ts, 100.0, 0.01)


def test_grid_of_40k_blocks():
    """B x nT x ceil(nM / 3) = 4000 x 10 x 1 blocks: k = 1 per date, so every date's answer is the discounted payoff of
    its one path, which numpy computes for all of them; the restatement checks a few dates."""
    B, L, x0, rate = 4000, 10, 100.0, 0.02
    g = np.random.default_rng(9)
    r = (0.02 * g.standard_normal((B, 1, L))).astype(np.float32)
    Ts = [int(t) for t in g.permutation(np.arange(1, L + 1))]
    Ms = [-0.8, 0.1, 1.2]
    res = kernel(r, None, Ts, Ms, x0, rate, 2, "otm")
    assert (res["status"] == 0).all()
    cum = np.cumsum(r[:, 0].astype(np.float64), axis=1)
    for q, T in enumerate(Ts):
        tau = T / 252.0
        sig = np.sqrt((252.0 / T) * np.sum(r[:, 0, :T].astype(np.float64) ** 2, axis=1))
        np.testing.assert_allclose(res["sigma"][:, q], sig, rtol=1e-13)
        K = x0 * math.exp(rate * tau) * np.exp(np.asarray(Ms)[None] * sig[:, None] * math.sqrt(tau))
        np.testing.assert_allclose(res["strike"][:, q], K, rtol=1e-13)
        ST = x0 * np.exp(cum[:, T - 1])[:, None]
        call = np.asarray(Ms)[None] >= 0
        want = math.exp(-rate * tau) * np.where(call, np.maximum(ST - K, 0.0), np.maximum(K - ST, 0.0))
        np.testing.assert_allclose(res["price"][:, q], want, rtol=1e-12, atol=1e-12 * x0)
    for b in [0, 1, 1999, B - 1]:
        rf = ref.hmc_date(r[b], None, x0, rate, Ts, Ms, 2, "otm")
        np.testing.assert_allclose(res["price"][b], rf["price"], rtol=1e-12, atol=1e-12 * x0)


@pytest.mark.parametrize("P", [1, 3, 5])
def test_drift_sweep_on_device(P):
    """Drift c and spread e between the paths: the kernel, the twin and the restatement flag the same maturities (NaN
    prices / IVs, strikes and sigma kept, status bit ILL) or agree to 1e-9 with bounded prices."""
    Ts, Ms = [5, 20], [-1.0, 0.0, 1.0]
    cases = [(c, e) for c in [0.0, 0.001, -0.001, 0.003, 0.01] for e in SWEEP_E]
    r = np.stack([ref.drift_returns(c, e)[0] for c, e in cases])
    w = np.stack([ref.drift_returns(c, e)[1] for c, e in cases])
    dev = kernel(r, w, Ts, Ms, 100.0, 0.0, P, "otm")
    host = pricing.hedged_mc_host(r, w, Ts, Ms, 100.0, 0.0, P, 0)
    n_flagged = 0
    for b in range(len(cases)):
        rf = ref.hmc_date(r[b], w[b], 100.0, 0.0, Ts, Ms, P, "otm")
        nan = check_sweep_case(date(dev, b), rf, Ts, Ms)
        check_sweep_case(date(dev, b), date(host, b), Ts, Ms)
        n_flagged += bool(nan.any())
    assert n_flagged >= 8


@pytest.mark.parametrize("P,seed", [(5, 2), (4, 0)])
def test_student_t_flags_or_agrees_on_device(P, seed):
    """Heavy tails at T = 75, where a few outlying paths make some dates' fits nearly singular: the kernel, the twin and
    the restatement flag the same maturities or agree to 1e-9."""
    Ts, Ms = [10, 40, 75], list(np.linspace(-1.5, 1.5, 7))
    r, w = ref.student_t_dates(seed)
    dev = kernel(r, w, Ts, Ms, 100.0, 0.01, P, "otm")
    host = pricing.hedged_mc_host(r, w, Ts, Ms, 100.0, 0.01, P, 0)
    flagged = 0
    for b in range(r.shape[0]):
        rf = ref.hmc_date(r[b], w[b], 100.0, 0.01, Ts, Ms, P, "otm")
        flagged += bool(check_sweep_case(date(dev, b), rf, Ts, Ms).any())
        check_sweep_case(date(dev, b), date(host, b), Ts, Ms)
    assert 1 <= flagged < r.shape[0]


def test_ill_conditioned_maturity_is_flagged_whatever_block_finishes_first():
    """Many strike groups and maturities per date, and dates that flag among dates that do not: the status word of a
    date collects the bit from whichever block sets it, and only flagged maturities are NaN."""
    Ts = [20, 5, 2, 20, 12]
    Ms = list(np.linspace(-2, 2, 40))
    good, _ = ref.drift_returns(0.0, 1e-2, k=500, L=20, seed=1)
    bad, _ = ref.drift_returns(0.01, 1e-5, k=500, L=20, seed=2)
    late = good.copy()
    late[:, 10:] = bad[:, 10:]                  # well-conditioned until step 10: only the maturities beyond it flag
    r = np.stack([good, bad, late, good])
    dev = kernel(r, None, Ts, Ms, 100.0, 0.0, 3, "otm")
    assert list(dev["status"]) == [0, ILL, ILL, 0]
    flagged = np.isnan(dev["price"]).all(axis=2)
    assert list(flagged[2]) == [True, False, False, True, True]
    assert flagged[1].all() and not flagged[[0, 3]].any()
    assert np.isnan(dev["iv"][flagged]).all() and np.isfinite(dev["strike"]).all() and np.isfinite(dev["sigma"]).all()
    host = pricing.hedged_mc_host(r, None, Ts, Ms, 100.0, 0.0, 3, 0)
    np.testing.assert_array_equal(host["status"], dev["status"])
    np.testing.assert_array_equal(np.isnan(host["price"]), np.isnan(dev["price"]))
