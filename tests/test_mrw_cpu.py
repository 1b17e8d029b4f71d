"""The multifractal random walk generator's numpy twin (shadowing_amd/mrw.py): the circulant spectra, the synthesis against
a dense DFT, the counter property of the draws, the moments the model promises, MRWGenerator's contract and the argument
errors.  No GPU."""
import math

import numpy as np
import pytest

from shadowing_amd import mrw, pdv

MRW_CASES = [(4096, 4096), (4096, 1024), (1000, 1000), (64, 16), (1024, 4096), (2, 2), (3, 3), (4096, 1)]


def _check_spectrum(s, M, c_half):
    """sum_k (s[k] / M) cos(2 pi j k / M) gives back c[j] for every j <= M / 2, and nothing is clipped."""
    assert s.shape == (M,)
    print(f"M={M} min s={s.min():.6e} max s={s.max():.6e}")
    assert s.min() >= -1e-9 * s.max()
    back = np.fft.ifft(s).real                       # s is even: the inverse transform is the cosine sum / M
    assert np.abs(back[:M // 2 + 1] - c_half).max() <= 1e-12 * max(c_half[0], 1e-300)
    # ... and spelt out as the cosine sum itself at a few lags
    k = np.arange(M)
    for j in (0, 1, M // 4 + 1, M // 2):
        direct = np.sum(s / M * np.cos(2 * np.pi * ((j * k) % M) / M))
        assert abs(direct - c_half[j]) <= 1e-12 * max(c_half[0], 1e-300)


@pytest.mark.parametrize("n,L", MRW_CASES)
def test_mrw_spectrum_reproduces_the_covariance(n, L):
    s, M = mrw.mrw_spectrum(n, L, 0.2)
    assert M >= 2 * n and M & (M - 1) == 0 and (M // 2 < 2 * n or M == 4)
    _check_spectrum(s, M, 0.04 * np.maximum(np.log(L / (np.arange(M // 2 + 1) + 1.0)), 0.0))


@pytest.mark.parametrize("H", [0.1, 0.3, 0.7, 0.9])
@pytest.mark.parametrize("n", [4096, 1000, 64])
def test_fgn_spectrum_reproduces_the_covariance(n, H):
    s, M = mrw.fgn_spectrum(n, H)
    j = np.arange(M // 2 + 1, dtype=np.float64)
    _check_spectrum(s, M, 0.5 * ((j + 1) ** (2 * H) - 2 * j ** (2 * H) + np.abs(j - 1) ** (2 * H)))


def test_a_spectrum_that_is_not_nonnegative_is_an_error():
    c = np.array([1.0, 0.99, 0.0])                    # not convex: s = (2.98, 1, -0.98, 1)
    with pytest.raises(ValueError, match="non-negative"):
        mrw._spectrum(c, 4, "a test sequence")


@pytest.mark.parametrize("H", [0.5, 0.3])
def test_synthesis_equals_the_dense_dft_product(H):
    """M = 64: omega (and eps) of the twin against the M x M DFT matrix applied to a * Z on the same draws."""
    n, L, lam, seed = 32, 32, 0.2, 77
    s, M = mrw.mrw_spectrum(n, L, lam)
    assert M == 64
    key = (seed & 0xFFFFFFFF, seed >> 32)
    k = np.arange(M)
    F = np.exp(-2j * np.pi * np.outer(k, k) / M)

    def dense(spec, stream, q):
        z0, z1 = pdv.normal_pairs((k.astype(np.uint64), np.uint64(stream), np.uint64(q), np.uint64(0)), key)
        return F @ (np.sqrt(spec / M) * (z0 + 1j * z1))

    r, omega = mrw._host(5, n, H, lam, float(L), 0.01, seed)
    for q in range(3):
        Y = dense(s, 0, q)
        np.testing.assert_allclose(omega[2 * q], Y.real[:n], rtol=0, atol=1e-12)
        if 2 * q + 1 < 5:
            np.testing.assert_allclose(omega[2 * q + 1], Y.imag[:n], rtol=0, atol=1e-12)
        if H != 0.5:
            E = dense(mrw.fgn_spectrum(n, H)[0], 1, q)
            np.testing.assert_allclose(r[2 * q], (0.01 * E.real[:n]) * np.exp(omega[2 * q] - 0.04 * math.log(L)), rtol=0,
                                       atol=1e-12)


@pytest.mark.parametrize("H", [0.5, 0.7])
@pytest.mark.parametrize("n", [200, 33])
def test_a_path_does_not_depend_on_how_many_are_made(n, H):
    eight, om8 = mrw.mrw_log_returns(8, n, H=H, seed=5, return_omega=True)
    four, om4 = mrw.mrw_log_returns(4, n, H=H, seed=5, return_omega=True)
    odd = mrw.mrw_log_returns(5, n, H=H, seed=5)
    assert eight.shape == (8, 1, n) and eight.dtype == np.float32 and om8.shape == (8, n) and om8.dtype == np.float64
    assert np.array_equal(eight[:4], four) and np.array_equal(om8[:4], om4)
    assert np.array_equal(eight[:5], odd)
    assert not np.array_equal(eight[0], eight[1])
    assert not np.array_equal(eight, mrw.mrw_log_returns(8, n, H=H, seed=6))
    # ... nor on where the batch of paths starts (the twin's chunks)
    r, _ = mrw._host(3, n, H, 0.2, float(n), mrw.DEFAULT_SIGMA, 5, first_path=3)
    assert np.array_equal(r.astype(np.float32), eight[3:6, 0])


def test_moments_of_the_twin():
    """R = 4096 independent paths; every bound is 6 standard errors of the mean of R independent terms."""
    R, n, lam, sigma = 4096, 1024, 0.2, mrw.DEFAULT_SIGMA
    dlnx, omega = mrw.mrw_log_returns(R, n, lam=lam, sigma=sigma, seed=2024, return_omega=True)
    c = mrw.mrw_covariance(np.arange(n), float(n), lam)
    assert c[0] == pytest.approx(lam * lam * math.log(n))
    for j in (0, 1, 10, 100, 1000):
        # omega[0] omega[j] with (omega[0], omega[j]) centred Gaussian: Var = c0^2 + c[j]^2 (Isserlis)
        bound = 6.0 * math.sqrt((c[0] ** 2 + c[j] ** 2) / R)
        got = float(np.mean(omega[:, 0] * omega[:, j]))
        print(f"j={j} mean={got:.5f} c[j]={c[j]:.5f} bound={bound:.5f}")
        assert abs(got - c[j]) <= bound
    # r^2 / sigma^2 = eps^2 exp(2 omega - 2 c0): mean 1, second moment E[eps^4] E[exp(4 omega - 4 c0)] = 3 exp(4 c0),
    # so its relative variance is 3 exp(4 c0) - 1
    r = mrw._host(R, n, 0.5, lam, float(n), sigma, 2024)[0]
    bound = 6.0 * math.sqrt((3.0 * math.exp(4.0 * c[0]) - 1.0) / R)
    for t in (0, 1, 511, n - 1):
        got = float(np.mean(r[:, t] ** 2)) / sigma ** 2
        print(f"t={t} mean r^2 / sigma^2={got:.4f} bound={bound:.4f}")
        assert abs(got - 1.0) <= bound
    assert np.array_equal(r.astype(np.float32), dlnx[:, 0])
    # eps and omega are independent: E[r] = 0, Var r = sigma^2
    assert abs(float(np.mean(r[:, 7]))) <= 6.0 * sigma / math.sqrt(R)


def test_fgn_increments_have_the_stated_covariance():
    """lam = 0 leaves r = sigma * eps: the lag-1 covariance of fGn is 2^(2H - 1) - 1."""
    R, n, H = 4096, 64, 0.3
    r = mrw._host(R, n, H, 0.0, float(n), 1.0, 11)[0]
    rho = 2.0 ** (2 * H - 1) - 1.0
    for j, cj in ((0, 1.0), (1, rho)):
        bound = 6.0 * math.sqrt((1.0 + cj ** 2) / R)
        assert abs(float(np.mean(r[:, 5] * r[:, 5 + j])) - cj) <= bound


def test_generator_gives_log_prices_from_zero():
    import shadowing_amd as sa
    from shadowing import MRWGenerator
    assert MRWGenerator is sa.MRWGenerator is mrw.MRWGenerator
    gen = MRWGenerator(T=257, H=0.5, lam=0.2, cache_path="/nonexistent/_cache")
    lnx = gen.load(R=6, seed=3)
    assert lnx.shape == (6, 1, 257) and lnx.dtype == np.float64
    assert np.all(lnx[:, :, 0] == 0.0)
    r = mrw._host(6, 256, 0.5, 0.2, 256.0, mrw.DEFAULT_SIGMA, 3)[0]
    np.testing.assert_allclose(np.diff(lnx, axis=-1)[:, 0], r, rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.diff(lnx, axis=-1), mrw.mrw_log_returns(6, 256, seed=3), rtol=1e-6, atol=1e-12)
    # seed=None: a seed from numpy's global stream, as PDVModelDiscrete.gen
    np.random.seed(4)
    a = gen.load(R=2)
    np.random.seed(4)
    assert np.array_equal(a, gen.load(R=2))
    assert not np.array_equal(a, gen.load(R=2))


@pytest.mark.parametrize("kw", [dict(n=1), dict(n=0), dict(n=2.5), dict(lam=-0.1), dict(lam=math.nan), dict(H=0.0),
                                dict(H=1.0), dict(H=-0.2), dict(H=math.inf), dict(L=0.5), dict(L=math.inf),
                                dict(L=math.nan), dict(sigma=math.nan), dict(sigma=-1.0), dict(R=0), dict(seed=-1),
                                dict(seed=2 ** 64)])
def test_argument_errors_raise(kw):
    args = dict(R=2, n=16, H=0.5, lam=0.2, L=None, sigma=0.01, seed=1)
    args.update(kw)
    with pytest.raises(ValueError):
        mrw.mrw_log_returns(**args)


def test_generator_argument_errors_raise():
    with pytest.raises(ValueError):
        mrw.MRWGenerator(T=2)                         # one return
    with pytest.raises(ValueError):
        mrw.MRWGenerator(T=100, H=1.5)
    with pytest.raises(ValueError):
        mrw.MRWGenerator(T=100).load(R=0)
    with pytest.raises(ValueError):
        mrw.mrw_spectrum(1)
    with pytest.raises(ValueError):
        mrw.fgn_spectrum(16, 1.0)
