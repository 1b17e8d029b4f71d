"""psh_smrw_generate on the MI355X: against the numpy twin on the same seed, K0 = 0 against psh_mrw_generate, bitwise
repeatability and the counter property, the row stride, the native envelope, the leverage of the device's own output
against the closed form, and end to end: the generated ensemble scanned where it lies (bit for bit against the oracle)
and priced into a skewed smile."""
import math

import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, mrw

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_device")]
PRICE_ATOL = 1e-9                                    # tests/test_gpu_hmc.py
ALL = ("dlnx", "lnx", "logvol")


def _generate(R, n, m, K0, alpha, lam, sigma, seed, outputs, **kw):
    dev = torch.device("cuda", torch.cuda.current_device())
    a_om, _ = mrw._device_tables(n, 0.5, lam, float(n), dev)
    K = mrw.smrw_kernel(m, K0, alpha)
    k_hat = torch.from_numpy(mrw._k_hat(K, mrw._embedding_size(n))).to(dev)
    return _native.smrw_generate(R, n, m, sigma, a_om, k_hat, float(mrw.mrw_covariance(0, float(n), lam)),
                                 float(np.sum(K ** 2)), seed=seed, outputs=outputs, **kw)


# M = 8192 (n = 4096 and a non-power-of-two n), n + m = M twice, m = 1, n = 2 (M = 4, both memories), odd R throughout
@pytest.mark.parametrize("n,m,R", [(4096, 4096, 7), (3000, 1500, 3), (3000, 5192, 3), (1000, 1000, 9), (1000, 1048, 5),
                                   (1000, 1, 5), (1025, 333, 3), (64, 64, 33), (33, 7, 3), (5, 3, 2), (2, 1, 3), (2, 2, 3)])
def test_device_matches_twin(n, m, R):
    K0, alpha, lam, sigma, seed = 0.1, 0.6, 0.2, mrw.DEFAULT_SIGMA, 4321 + n
    out = _generate(R, n, m, K0, alpha, lam, sigma, seed, ALL)
    r, lv = mrw._smrw_host(R, n, mrw.smrw_kernel(m, K0, alpha), lam, float(n), sigma, seed)
    lnx = np.concatenate([np.zeros((R, 1)), np.cumsum(r, axis=-1)], axis=-1)
    assert out["dlnx"].shape == (R, 1, n) and out["dlnx"].dtype == torch.float32
    assert out["lnx"].shape == (R, n + 1) and out["logvol"].shape == (R, n)
    d_lv, d_lnx, d_r = out["logvol"].cpu().numpy(), out["lnx"].cpu().numpy(), out["dlnx"].cpu().numpy()[:, 0]
    e_lv = np.abs(d_lv - lv).max() / np.abs(lv).max()
    e_lnx = np.abs(d_lnx - lnx).max() / np.abs(lnx).max()
    print(f"n={n} m={m} R={R}: logvol {e_lv:.3e} lnx {e_lnx:.3e} (of max|twin|)")
    assert np.abs(d_lv - lv).max() <= 1e-9 * np.abs(lv).max()
    assert np.abs(d_lnx - lnx).max() <= 1e-9 * np.abs(lnx).max()
    assert np.all(d_lnx[:, 0] == 0.0)
    np.testing.assert_allclose(d_r, r.astype(np.float32), rtol=2.0 ** -23, atol=1e-9 * sigma)


@pytest.mark.parametrize("n,R", [(4096, 5), (1000, 6), (2, 3)])
def test_k0_zero_through_the_kernel_is_the_mrw(n, R):
    """An all-zero k_hat goes through psh_smrw_generate's own kernel (there is no short cut to the MRW's)."""
    lam, sigma, seed = 0.2, mrw.DEFAULT_SIGMA, 77
    dev = torch.device("cuda", torch.cuda.current_device())
    a_om, _ = mrw._device_tables(n, 0.5, lam, float(n), dev)
    c0 = float(mrw.mrw_covariance(0, float(n), lam))
    k_hat = torch.zeros(mrw._embedding_size(n), dtype=torch.complex128, device=dev)
    s = _native.smrw_generate(R, n, min(n, 7), sigma, a_om, k_hat, c0, 0.0, seed=seed, outputs=ALL)
    p = _native.mrw_generate(R, n, sigma, a_om, None, c0, seed=seed, outputs=("dlnx", "lnx", "omega"))
    om, lnx = p["omega"].cpu().numpy(), p["lnx"].cpu().numpy()
    print(f"n={n}: bit-equal logvol {torch.equal(s['logvol'], p['omega'])} lnx {torch.equal(s['lnx'], p['lnx'])} "
          f"dlnx {torch.equal(s['dlnx'], p['dlnx'])}")
    assert np.abs(s["logvol"].cpu().numpy() - om).max() <= 1e-9 * np.abs(om).max()
    assert np.abs(s["lnx"].cpu().numpy() - lnx).max() <= 1e-9 * np.abs(lnx).max()
    np.testing.assert_allclose(s["dlnx"].cpu().numpy(), p["dlnx"].cpu().numpy(), rtol=2.0 ** -23, atol=1e-9 * sigma)


@pytest.mark.parametrize("n,m", [(1000, 1000), (4096, 2000)])
def test_two_calls_give_identical_bits_and_paths_do_not_depend_on_R(n, m):
    a = _generate(8, n, m, 0.1, 0.6, 0.2, 0.01, 5, ALL)
    b = _generate(8, n, m, 0.1, 0.6, 0.2, 0.01, 5, ALL)
    four = _generate(4, n, m, 0.1, 0.6, 0.2, 0.01, 5, ALL)
    five = _generate(5, n, m, 0.1, 0.6, 0.2, 0.01, 5, ALL)
    for key in ALL:
        assert torch.equal(a[key], b[key])
        assert torch.equal(a[key][:4], four[key])
        assert torch.equal(a[key][:5], five[key])               # path 4 of an odd R: its partner is made, not stored
    assert not torch.equal(a["dlnx"][0], a["dlnx"][1])
    assert not torch.equal(a["dlnx"], _generate(8, n, m, 0.1, 0.6, 0.2, 0.01, 6, ("dlnx",))["dlnx"])
    assert not torch.equal(a["dlnx"], _generate(8, n, m - 1, 0.1, 0.6, 0.2, 0.01, 5, ("dlnx",))["dlnx"])


def test_row_stride_leaves_the_bytes_between_rows_untouched():
    R, n, pad = 5, 1000, 24
    buf = torch.full((R, n + pad), 7.25, dtype=torch.float32, device="cuda")
    out = _generate(R, n, n, 0.1, 0.6, 0.2, 0.01, 5, ("dlnx",), dlnx_out=buf)
    assert out["dlnx"] is buf
    plain = _generate(R, n, n, 0.1, 0.6, 0.2, 0.01, 5, ("dlnx",))["dlnx"]
    assert torch.equal(buf[:, :n], plain[:, 0])
    assert torch.all(buf[:, n:] == 7.25)
    with pytest.raises(ValueError):
        _generate(R, n, n, 0.1, 0.6, 0.2, 0.01, 5, ("dlnx",), dlnx_out=buf[:, :n - 1])


def test_public_functions_on_the_device():
    dl, lv = sa.smrw_log_returns(6, 500, 0.1, 0.6, memory=300, seed=8, cuda=True, return_logvol=True)
    assert dl.is_cuda and dl.dtype == torch.float32 and dl.shape == (6, 1, 500) and lv.shape == (6, 500)
    hl, hlv = sa.smrw_log_returns(6, 500, 0.1, 0.6, memory=300, seed=8, return_logvol=True)
    np.testing.assert_allclose(dl.cpu().numpy(), hl, rtol=2.0 ** -23, atol=1e-9 * mrw.DEFAULT_SIGMA)
    assert np.abs(lv.cpu().numpy() - hlv).max() <= 1e-9 * np.abs(hlv).max()
    gen = sa.SMRWGenerator(T=4097, K0=0.1, alpha=0.6, lam=0.2, cache_path=None)
    dev, host = gen.load(R=3, seed=12, cuda=True), gen.load(R=3, seed=12)
    assert isinstance(dev, np.ndarray) and dev.shape == (3, 1, 4097) and dev.dtype == np.float64
    assert np.abs(dev - host).max() <= 1e-9 * np.abs(host).max()
    np.random.seed(3)
    a = sa.smrw_log_returns(2, 100, 0.1, 0.6, cuda=True)
    np.random.seed(3)
    assert torch.equal(a, sa.smrw_log_returns(2, 100, 0.1, 0.6, cuda=True))


def test_the_native_envelope_and_the_error_codes():
    with pytest.raises(ValueError, match="4096"):
        sa.smrw_log_returns(2, 4097, 0.1, 0.6, seed=1, cuda=True)
    with pytest.raises(ValueError, match="4096"):
        sa.SMRWGenerator(T=4099, K0=0.1, alpha=0.6).load(R=2, seed=1, cuda=True)
    # the C ABI itself: PSH_ERR_UNSUPPORTED (-2) for n > 4096, PSH_ERR_ARG (-1) before anything touches the device
    L = _native.load()
    tab = torch.zeros(2 * 16384, dtype=torch.float64, device="cuda")
    t = tab.data_ptr()
    call = lambda R, n, m, sigma, a, k, c0, v, out=None, stride=0: L.psh_smrw_generate(   # noqa: E731
        0, None, R, n, m, sigma, a, k, c0, v, 1, out, stride, None, None)
    assert call(2, 4097, 4097, 0.01, t, t, 0.3, 0.1) == -2
    assert call(2, 64, 64, 0.01, t, t, 0.3, 0.1) == 0
    assert call(2, 1, 1, 0.01, t, t, 0.3, 0.1) == -1
    assert call(0, 64, 64, 0.01, t, t, 0.3, 0.1) == -1
    assert call(2, 64, 64, 0.01, None, t, 0.3, 0.1) == -1
    assert call(2, 64, 64, 0.01, t, None, 0.3, 0.1) == -1
    assert call(2, 64, 0, 0.01, t, t, 0.3, 0.1) == -1
    assert call(2, 64, 65, 0.01, t, t, 0.3, 0.1) == -1          # M = 128: n + m > M
    assert call(2, 60, 68, 0.01, t, t, 0.3, 0.1) == 0           # n + m = M
    assert call(2, 60, 69, 0.01, t, t, 0.3, 0.1) == -1
    assert call(2, 64, 64, float("nan"), t, t, 0.3, 0.1) == -1
    assert call(2, 64, 64, 0.01, t, t, float("inf"), 0.1) == -1
    assert call(2, 64, 64, 0.01, t, t, 0.3, float("nan")) == -1
    assert call(2, 64, 64, 0.01, t, t, 0.3, float("inf")) == -1
    assert call(2, 64, 64, 0.01, t, t, 0.3, 0.1, t, 63) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("lam,K0,alpha", [(0.0, 0.1, 0.6), (0.1, 0.1, 0.6), (0.2, 0.05, 0.75)])
def test_leverage_of_the_device_output_matches_the_closed_form(lam, K0, alpha):
    """What a wrong shift or a wrapped convolution cannot pass: E[r_t r_{t+tau}^2] of the kernel's own returns (dlnx: one
    float32 rounding, 6e-8 relative, against standard errors of a per cent) within 6 standard errors of smrw_leverage."""
    R, n, sigma = 8192, 512, 1.0
    out = _generate(R, n, n, K0, alpha, lam, sigma, 11, ("dlnx",))
    r = out["dlnx"].cpu().numpy()[:, 0].astype(np.float64)
    K = mrw.smrw_kernel(n, K0, alpha)
    c0, v = lam * lam * math.log(n), float(np.sum(K ** 2))
    bound = 6.0 * math.sqrt((3.0 * math.exp(4.0 * (c0 + v)) - 1.0) / R)
    for t in (0, 100, 511):
        got = float(np.mean(r[:, t] ** 2)) / sigma ** 2
        print(f"lam={lam} K0={K0} alpha={alpha} t={t}: mean r^2 / sigma^2 = {got:.4f} bound = {bound:.4f}")
        assert abs(got - 1.0) <= bound
    for tau in (1, 2, 5, 20):
        x = (r[:, :n - tau] * r[:, tau:] ** 2).mean(axis=1)
        se = float(x.std(ddof=1)) / math.sqrt(R)
        th = mrw.smrw_leverage(tau, n, K0, alpha, lam=lam, sigma=sigma)
        print(f"   tau={tau}: estimate {x.mean():+.5f} se {se:.5f} closed form {th:+.5f} z {(x.mean() - th) / se:+.2f}")
        assert th < 0.0 and float(x.mean()) < 0.0
        assert abs(float(x.mean()) - th) <= 6.0 * se


def test_identity_scan_of_the_generated_ensemble_equals_the_oracle(oracle_mod):
    ds = sa.smrw_log_returns(2048, 4096, 0.1, 0.6, seed=21, cuda=True)
    assert ds.is_cuda and ds.shape == (2048, 1, 4096)
    query = mrw.smrw_log_returns(1, 64, 0.1, 0.6, seed=22)[0, 0, :20]
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(20))
    d, paths, idx = obj.shadow(query, k=256, cuda=True)
    assert obj.last_path == "hip"
    host = ds.cpu().numpy()
    od, opaths, oidx = oracle_mod.shadow(host, query, 256, 20)
    assert np.array_equal(np.asarray(d).view(np.uint32), od.view(np.uint32))
    assert np.array_equal(idx, oidx) and np.array_equal(paths, opaths)
    assert np.isfinite(host).all() and 0.5 < host.std() / mrw.DEFAULT_SIGMA < 1.5


def test_the_smile_of_the_device_ensemble_is_skewed():
    """The ordering of tests/test_smrw_cpu.py on ensembles made and priced on the device: the ensemble against the host
    twin's, the prices against the host pricing of the same ensemble, at the tolerances of tests/test_gpu_mrw.py."""
    Ts, Ms = np.array([5, 10, 20]), np.linspace(-2.0, 2.0, 9)
    skews = []
    for K0 in (0.0, 0.05, 0.1):
        dl = sa.smrw_log_returns(8192, 64, K0, 0.6, lam=0.2, memory=64, seed=5, cuda=True)
        hl = sa.smrw_log_returns(8192, 64, K0, 0.6, lam=0.2, memory=64, seed=5)
        np.testing.assert_allclose(dl.cpu().numpy(), hl, rtol=2.0 ** -23, atol=1e-9 * mrw.DEFAULT_SIGMA)
        x = sa.PriceData(dlnx=dl.cpu().numpy()[:, 0, :20], x_init=100.0).x
        dev = sa.compute_smile(torch.from_numpy(x).cuda(), Ts, Ms, 0.0, ave=None)
        host = sa.compute_smile(x, Ts, Ms, 0.0, ave=None, cuda=False)
        assert np.all(np.asarray(dev.status) == 0) and np.all(np.asarray(host.status) == 0)
        np.testing.assert_allclose(dev.strikes, host.strikes, rtol=1e-12)
        print(f"K0={K0}: max |price dev - host| = {np.abs(dev.prices - host.prices).max():.3e}")
        np.testing.assert_allclose(dev.prices, host.prices, rtol=1e-9, atol=PRICE_ATOL)
        skews.append(np.asarray(dev.ivs)[..., 2] - np.asarray(dev.ivs)[..., 6])    # iv(M = -1) - iv(M = +1)
        print(f"K0={K0}: skew {np.round(skews[-1], 4)}")
    assert np.all(skews[2] > skews[1]) and np.all(skews[1] > skews[0])
