"""The skewed multifractal random walk's numpy twin (shadowing_amd/mrw.py, smrw_*): the FFT convolution against the double
loop, K0 = 0 against the MRW, the counter property of the draws and of the pre-history, the moments and the leverage the
model promises (against its closed form), the skew it puts into a smile, and the argument errors.  No GPU."""
import math

import numpy as np
import pytest

import shadowing_amd as sa
from shadowing_amd import mrw, pdv

LEVERAGE_SETS = [(0.0, 0.1, 0.6), (0.1, 0.1, 0.6), (0.2, 0.05, 0.75)]         # (lam, K0, alpha)


def _noise(R, n, m, seed):
    """(R, m + n): eps of times -m .. n - 1 of paths 0 .. R - 1, from the counters the model names."""
    key = (seed & 0xFFFFFFFF, seed >> 32)
    g = np.arange(R, dtype=np.uint64)[:, None]
    out = np.empty((R, m + n))
    for t in range(-m, n):
        if t >= 0:
            z = pdv.normal_pairs((np.uint64(t // 2), np.uint64(2), g, np.uint64(0)), key)
            out[:, m + t] = z[t % 2][:, 0]
        else:
            i = (-1 - t) // 2                                    # eps[-1 - 2i] = z0, eps[-2 - 2i] = z1 of counter (i, 3, g)
            z = pdv.normal_pairs((np.uint64(i), np.uint64(3), g, np.uint64(0)), key)
            out[:, m + t] = z[(-1 - t) % 2][:, 0]
    return out


def _direct(e, K, n, m, lo=1):
    """A[t] = sum_{j=lo..m} K(j) eps[t - j] by the double loop; e holds times -m .. n - 1."""
    A = np.zeros((e.shape[0], n))
    for t in range(n):
        for j in range(lo, m + 1):
            A[:, t] += K[j - 1] * e[:, m + t - j]
    return A


@pytest.mark.parametrize("n,m", [(300, 212), (64, 64), (33, 1), (1000, 1048)])
def test_convolution_equals_the_double_loop(n, m):
    R, K0, alpha, seed = 3, 0.1, 0.6, 31 + n
    if (n, m) == (1000, 1048):
        assert n + m == mrw._embedding_size(n)                   # the largest memory the circulant holds
    _, lv = mrw.smrw_log_returns(R, n, K0, alpha, lam=0.0, memory=m, seed=seed, return_logvol=True)
    A = -lv                                                      # lam = 0: omega = 0
    D = _direct(_noise(R, n, m, seed), mrw.smrw_kernel(m, K0, alpha), n, m)
    err = np.abs(A - D).max() / np.abs(D).max()
    print(f"n={n} m={m}: max|A - direct| / max|A| = {err:.3e}")
    assert err <= 1e-12


def test_k0_zero_gives_the_bits_of_the_mrw():
    for n, R in ((200, 5), (33, 4)):
        a, om = mrw.mrw_log_returns(R, n, seed=9, return_omega=True)
        b, lv = mrw.smrw_log_returns(R, n, 0.0, 0.6, seed=9, return_logvol=True)
        assert b.dtype == np.float32 and b.shape == (R, 1, n) and lv.shape == (R, n) and lv.dtype == np.float64
        assert np.array_equal(a, b) and np.array_equal(om, lv)
    assert not np.array_equal(mrw.smrw_log_returns(5, 200, 0.1, 0.6, seed=9), mrw.mrw_log_returns(5, 200, seed=9))


@pytest.mark.parametrize("n", [200, 33])
def test_a_path_does_not_depend_on_how_many_are_made(n):
    eight, lv8 = mrw.smrw_log_returns(8, n, 0.1, 0.6, seed=5, return_logvol=True)
    four, lv4 = mrw.smrw_log_returns(4, n, 0.1, 0.6, seed=5, return_logvol=True)
    odd = mrw.smrw_log_returns(5, n, 0.1, 0.6, seed=5)
    assert np.array_equal(eight[:4], four) and np.array_equal(lv8[:4], lv4)
    assert np.array_equal(eight[:5], odd)
    assert not np.array_equal(eight[0], eight[1])
    assert not np.array_equal(eight, mrw.smrw_log_returns(8, n, 0.1, 0.6, seed=6))
    # ... nor on where the batch of paths starts (the twin's chunks)
    r, _ = mrw._smrw_host(3, n, mrw.smrw_kernel(n, 0.1, 0.6), 0.2, float(n), mrw.DEFAULT_SIGMA, 5, first_path=3)
    assert np.array_equal(r.astype(np.float32), eight[3:6, 0])


def test_the_pre_history_does_not_depend_on_the_memory():
    R, n, m, m2, K0, alpha, seed = 3, 100, 90, 37, 0.1, 0.6, 17
    _, lv = mrw.smrw_log_returns(R, n, K0, alpha, lam=0.0, memory=m, seed=seed, return_logvol=True)
    _, lv2 = mrw.smrw_log_returns(R, n, K0, alpha, lam=0.0, memory=m2, seed=seed, return_logvol=True)
    tail = _direct(_noise(R, n, m, seed), mrw.smrw_kernel(m, K0, alpha), n, m, lo=m2 + 1)    # lags m2 + 1 .. m
    assert np.abs(tail).max() > 0.0
    assert np.abs((-lv) - (-lv2) - tail).max() <= 1e-12 * np.abs(lv).max()


@pytest.mark.parametrize("lam,K0,alpha", LEVERAGE_SETS)
def test_moments_and_leverage_of_the_twin(lam, K0, alpha):
    """R = 8192 independent paths; every bound is 6 standard errors."""
    R, n, sigma = 8192, 512, 1.0
    K = mrw.smrw_kernel(n, K0, alpha)
    r, _ = mrw._smrw_host(R, n, K, lam, float(n), sigma, 11)
    c0, v = lam * lam * math.log(n), float(np.sum(K ** 2))
    # r^2 / sigma^2 = eps^2 exp(2 lv - 2 c0 - 2 v): mean 1, second moment 3 exp(4 (c0 + v))
    bound = 6.0 * math.sqrt((3.0 * math.exp(4.0 * (c0 + v)) - 1.0) / R)
    for t in (0, 100, 511):
        got = float(np.mean(r[:, t] ** 2)) / sigma ** 2
        print(f"lam={lam} K0={K0} alpha={alpha} t={t}: mean r^2 / sigma^2 = {got:.4f} bound = {bound:.4f}")
        assert abs(got - 1.0) <= bound
    for tau in (1, 2, 5, 20):
        x = (r[:, :n - tau] * r[:, tau:] ** 2).mean(axis=1)      # per-path means: R independent terms
        se = float(x.std(ddof=1)) / math.sqrt(R)
        th = mrw.smrw_leverage(tau, n, K0, alpha, lam=lam, sigma=sigma)
        print(f"   tau={tau}: estimate {x.mean():+.5f} se {se:.5f} closed form {th:+.5f} z {(x.mean() - th) / se:+.2f}")
        assert th < 0.0 and float(x.mean()) < 0.0
        assert abs(float(x.mean()) - th) <= 6.0 * se


def test_leverage_closed_form_spelt_out():
    """smrw_leverage against the sums written as loops, and its scaling in sigma."""
    n, m, K0, alpha, lam, tau = 64, 40, 0.07, 0.7, 0.15, 3
    K = lambda j: K0 / j ** alpha if 1 <= j <= m else 0.0        # noqa: E731
    S = sum((K(j) + 2 * K(j + tau)) ** 2 for j in range(1, m + 1)) + 4 * sum(K(j) ** 2 for j in range(1, tau)) + 4 * K(tau) ** 2
    v = sum(K(j) ** 2 for j in range(1, m + 1))
    c0, ct = lam * lam * math.log(n), lam * lam * math.log(n / (tau + 1.0))
    want = -2 * K(tau) * math.exp(S / 2 + 2 * ct - c0 / 2 - 3 * v)
    assert mrw.smrw_leverage(tau, n, K0, alpha, lam=lam, memory=m, sigma=1.0) == pytest.approx(want, rel=1e-13)
    assert mrw.smrw_leverage(tau, n, K0, alpha, lam=lam, memory=m, sigma=2.0) == pytest.approx(8.0 * want, rel=1e-13)
    assert mrw.smrw_leverage(tau, n, 0.0, alpha) == 0.0
    assert np.array_equal(mrw.smrw_kernel(3, 0.5, 1.0), np.array([0.5, 0.25, 0.5 / 3.0]))
    for bad in (0, m + 1, 1.5):
        with pytest.raises(ValueError):
            mrw.smrw_leverage(bad, n, K0, alpha, memory=m)


def test_the_smile_is_skewed_and_the_skew_grows_with_k0():
    """An ordering on common noise (one seed): no tolerance."""
    Ts, Ms = np.array([5, 10, 20]), np.linspace(-2.0, 2.0, 9)
    skews = []
    for K0 in (0.0, 0.05, 0.1):
        dl = sa.smrw_log_returns(8192, 64, K0, 0.6, lam=0.2, memory=64, seed=5)
        x = sa.PriceData(dlnx=dl[:, 0, :20], x_init=100.0).x
        sm = sa.compute_smile(x, Ts, Ms, 0.0, ave=None, cuda=False)
        assert np.all(np.asarray(sm.status) == 0)
        skews.append(np.asarray(sm.ivs)[..., 2] - np.asarray(sm.ivs)[..., 6])      # iv(M = -1) - iv(M = +1)
        print(f"K0={K0}: skew {np.round(skews[-1], 4)}")
    assert Ms[2] == -1.0 and Ms[6] == 1.0
    assert np.all(skews[2] > skews[1]) and np.all(skews[1] > skews[0])


def test_generator_gives_log_prices_from_zero():
    from shadowing import SMRWGenerator
    assert SMRWGenerator is sa.SMRWGenerator is mrw.SMRWGenerator
    assert sa.smrw_log_returns is mrw.smrw_log_returns and sa.smrw_leverage is mrw.smrw_leverage
    assert sa.smrw_kernel is mrw.smrw_kernel
    gen = SMRWGenerator(T=257, K0=0.1, alpha=0.6, H=0.5, lam=0.2, cache_path="/nonexistent/_cache")
    lnx = gen.load(R=6, seed=3)
    assert lnx.shape == (6, 1, 257) and lnx.dtype == np.float64 and np.all(lnx[:, :, 0] == 0.0)
    np.testing.assert_allclose(np.diff(lnx, axis=-1), mrw.smrw_log_returns(6, 256, 0.1, 0.6, seed=3), rtol=1e-6, atol=1e-12)
    assert np.array_equal(SMRWGenerator(T=257, K0=0.0, alpha=0.6).load(R=6, seed=3), mrw.MRWGenerator(T=257).load(R=6, seed=3))
    np.random.seed(4)
    a = gen.load(R=2)
    np.random.seed(4)
    assert np.array_equal(a, gen.load(R=2))
    with pytest.raises(ValueError):
        SMRWGenerator(T=257, K0=0.1, alpha=0.6, H=0.3)
    with pytest.raises(ValueError):
        SMRWGenerator(T=257, K0=0.1, alpha=0.6, memory=257)       # M - n = 256
    with pytest.raises(ValueError):
        gen.load(R=0)


@pytest.mark.parametrize("kw", [dict(memory=0), dict(memory=17), dict(memory=2.5), dict(memory=-1), dict(K0=math.nan),
                                dict(K0=math.inf), dict(alpha=math.nan), dict(alpha=-math.inf), dict(n=1), dict(n=0),
                                dict(n=2.5), dict(lam=-0.1), dict(lam=math.nan), dict(L=0.5), dict(L=math.inf),
                                dict(L=math.nan), dict(sigma=math.nan), dict(sigma=-1.0), dict(R=0), dict(seed=-1),
                                dict(seed=2 ** 64)])
def test_argument_errors_raise(kw):
    args = dict(R=2, n=16, K0=0.1, alpha=0.6, lam=0.2, L=None, memory=None, sigma=0.01, seed=1)      # M = 32: memory <= 16
    args.update(kw)
    with pytest.raises(ValueError):
        mrw.smrw_log_returns(**args)


def test_the_largest_memory_is_accepted_and_fractional_noise_is_not():
    assert mrw.smrw_log_returns(2, 16, 0.1, 0.6, memory=16, seed=1).shape == (2, 1, 16)
    assert mrw.smrw_log_returns(2, 12, 0.1, 0.6, memory=20, seed=1).shape == (2, 1, 12)
    with pytest.raises(TypeError):
        mrw.smrw_log_returns(2, 16, 0.1, 0.6, H=0.3)             # the function has no H; the generator refuses H != 0.5
