"""psh_mrw_generate on the MI355X: against the numpy twin on the same seed, bitwise repeatability and the counter
property, the row stride, the generated ensemble scanned where it lies (bit for bit against the oracle), the tutorial's
average smile on windows of one generated path, and the native envelope."""
import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, mrw, pdv, pricing

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_device")]
PRICE_ATOL = 1e-9                                    # tests/test_gpu_hmc.py


def _generate(R, n, H, lam, L, sigma, seed, outputs, **kw):
    dev = torch.device("cuda", torch.cuda.current_device())
    a_om, a_eps = mrw._device_tables(n, H, lam, float(L), dev)
    return _native.mrw_generate(R, n, sigma, a_om, a_eps, float(mrw.mrw_covariance(0, float(L), lam)), seed=seed,
                                outputs=outputs, **kw)


@pytest.mark.parametrize("H", [0.5, 0.3])
@pytest.mark.parametrize("n,L,R", [(4096, 4096, 7), (4096, 1024, 4), (1000, 1000, 9), (1000, 250, 5), (64, 64, 33),
                                   (64, 16, 3), (2, 2, 3), (5, 5, 2), (2048, 2048, 3), (1025, 1025, 3)])
def test_device_matches_twin(n, L, R, H):
    lam, sigma, seed = 0.2, mrw.DEFAULT_SIGMA, 1234 + n
    out = _generate(R, n, H, lam, L, sigma, seed, ("dlnx", "lnx", "omega"))
    r, omega = mrw._host(R, n, H, lam, float(L), sigma, seed)
    lnx = np.concatenate([np.zeros((R, 1)), np.cumsum(r, axis=-1)], axis=-1)
    assert out["dlnx"].shape == (R, 1, n) and out["dlnx"].dtype == torch.float32
    assert out["lnx"].shape == (R, n + 1) and out["omega"].shape == (R, n)
    d_om, d_lnx, d_r = out["omega"].cpu().numpy(), out["lnx"].cpu().numpy(), out["dlnx"].cpu().numpy()[:, 0]
    e_om = np.abs(d_om - omega).max() / max(np.abs(omega).max(), 1e-300)
    e_lnx = np.abs(d_lnx - lnx).max() / np.abs(lnx).max()
    print(f"n={n} L={L} R={R} H={H}: omega {e_om:.3e} lnx {e_lnx:.3e} (of max|twin|)")
    # an absolute bound: an FFT's error is absolute and samples cross zero
    assert np.abs(d_om - omega).max() <= 1e-9 * np.abs(omega).max()
    assert np.abs(d_lnx - lnx).max() <= 1e-9 * np.abs(lnx).max()
    assert np.all(d_lnx[:, 0] == 0.0)
    np.testing.assert_allclose(d_r, r.astype(np.float32), rtol=2.0 ** -23, atol=1e-9 * sigma)


@pytest.mark.parametrize("H", [0.5, 0.3])
def test_two_calls_give_identical_bits_and_paths_do_not_depend_on_R(H):
    a = _generate(8, 1000, H, 0.2, 1000, 0.01, 5, ("dlnx", "lnx", "omega"))
    b = _generate(8, 1000, H, 0.2, 1000, 0.01, 5, ("dlnx", "lnx", "omega"))
    four = _generate(4, 1000, H, 0.2, 1000, 0.01, 5, ("dlnx", "lnx", "omega"))
    five = _generate(5, 1000, H, 0.2, 1000, 0.01, 5, ("dlnx", "lnx", "omega"))
    for key in ("dlnx", "lnx", "omega"):
        assert torch.equal(a[key], b[key])
        assert torch.equal(a[key][:4], four[key])
        assert torch.equal(a[key][:5], five[key])
    assert not torch.equal(a["dlnx"][0], a["dlnx"][1])
    assert not torch.equal(a["dlnx"], _generate(8, 1000, H, 0.2, 1000, 0.01, 6, ("dlnx",))["dlnx"])


def test_row_stride_leaves_the_bytes_between_rows_untouched():
    R, n, pad = 5, 1000, 24
    buf = torch.full((R, n + pad), 7.25, dtype=torch.float32, device="cuda")
    out = _generate(R, n, 0.5, 0.2, n, 0.01, 5, ("dlnx",), dlnx_out=buf)
    assert out["dlnx"] is buf
    plain = _generate(R, n, 0.5, 0.2, n, 0.01, 5, ("dlnx",))["dlnx"]
    assert torch.equal(buf[:, :n], plain[:, 0])
    assert torch.all(buf[:, n:] == 7.25)
    with pytest.raises(ValueError):
        _generate(R, n, 0.5, 0.2, n, 0.01, 5, ("dlnx",), dlnx_out=buf[:, :n - 1])


def test_public_functions_on_the_device():
    dl, om = sa.mrw_log_returns(6, 500, H=0.3, seed=8, cuda=True, return_omega=True)
    assert dl.is_cuda and dl.dtype == torch.float32 and dl.shape == (6, 1, 500) and om.shape == (6, 500)
    hl, hom = sa.mrw_log_returns(6, 500, H=0.3, seed=8, return_omega=True)
    np.testing.assert_allclose(dl.cpu().numpy(), hl, rtol=2.0 ** -23, atol=1e-9 * mrw.DEFAULT_SIGMA)
    assert np.abs(om.cpu().numpy() - hom).max() <= 1e-9 * np.abs(hom).max()
    gen = sa.MRWGenerator(T=4097, H=0.5, lam=0.2, cache_path=None)
    dev, host = gen.load(R=3, seed=12, cuda=True), gen.load(R=3, seed=12)
    assert isinstance(dev, np.ndarray) and dev.shape == (3, 1, 4097) and dev.dtype == np.float64
    assert np.abs(dev - host).max() <= 1e-9 * np.abs(host).max()
    np.random.seed(3)
    a = sa.mrw_log_returns(2, 100, cuda=True)
    np.random.seed(3)
    assert torch.equal(a, sa.mrw_log_returns(2, 100, cuda=True))


def test_identity_scan_of_the_generated_ensemble_equals_the_oracle(oracle_mod):
    ds = sa.mrw_log_returns(2048, 4096, seed=21, cuda=True)
    assert ds.is_cuda and ds.shape == (2048, 1, 4096)
    query = mrw.mrw_log_returns(1, 64, seed=22)[0, 0, :20]
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(20))
    d, paths, idx = obj.shadow(query, k=256, cuda=True)
    assert obj.last_path == "hip"
    host = ds.cpu().numpy()
    od, opaths, oidx = oracle_mod.shadow(host, query, 256, 20)
    assert np.array_equal(np.asarray(d).view(np.uint32), od.view(np.uint32))
    assert np.array_equal(idx, oidx) and np.array_equal(paths, opaths)
    assert np.isfinite(host).all() and 0.5 < host.std() / mrw.DEFAULT_SIGMA < 1.5


def test_foveal_scan_of_the_generated_ensemble_equals_the_oracle(oracle_mod):
    """The tutorial's setting: Foveal(1.15, 0.9, 126), horizon 252, on the ensemble of its first cell."""
    ds = sa.mrw_log_returns(2048, 4096, seed=21, cuda=True)
    x = mrw.mrw_log_returns(2, 126, seed=23)[:, 0, :]
    fov = sa.Foveal(alpha=1.15, beta=0.9, max_context=126)
    obj = sa.PathShadowing(fov, sa.RelativeMSE(), ds, sa.PredictionContext(horizon=252))
    d, _, idx = obj.shadow(x, k=256, cuda=True)
    assert obj.last_path == "hip"
    hx = fov(torch.tensor(x)[:, None, :])[:, 0, :].numpy()
    od, oidx = oracle_mod.scan_topk_embedded(ds.cpu().numpy(), fov.kernel[:, 0, :].numpy(), hx, 256, h=252)
    assert np.array_equal(np.asarray(d).view(np.uint32), od.view(np.uint32)), "distances differ from the oracle"
    assert np.array_equal(idx, oidx), "indices differ from the oracle"


def test_average_smile_on_windows_of_a_generated_path():
    """tutorial.ipynb, "Average Smile": windows of one MRW log-price path priced with ave=None, device against host."""
    lnx = sa.MRWGenerator(T=4097, H=0.5, lam=0.2).load(R=2, seed=40, cuda=True)
    snippets = pdv.windows(lnx[0, 0, :], w=252, s=1)
    x = sa.PriceData(lnx=snippets, x_init=100.0).x
    Ts, Ms = np.array([7, 25, 75]), np.linspace(-2.0, 2.0, 9)
    host = sa.compute_smile(x, Ts, Ms, 0.0, ave=None, cuda=False)
    dev = sa.compute_smile(torch.from_numpy(x).cuda(), Ts, Ms, 0.0, ave=None)
    np.testing.assert_array_equal(dev.status, host.status)
    good = np.isfinite(host.prices).all(axis=-1)             # maturities not flagged ill-conditioned
    assert good.any()
    if not (np.asarray(host.status) & pricing.STATUS_ILL_CONDITIONED).any():
        assert good.all()
    assert np.isfinite(dev.ivs[good]).all() and np.isfinite(host.ivs[good]).all()
    np.testing.assert_allclose(dev.prices, host.prices, rtol=1e-9, atol=PRICE_ATOL)
    np.testing.assert_allclose(dev.strikes, host.strikes, rtol=1e-12)
    both_nan = np.isnan(dev.ivs) & np.isnan(host.ivs)
    tau = (Ts.astype(np.float64) / 252.0)[:, None]
    sig = np.where(np.isfinite(host.ivs), host.ivs, 1.0)
    d1 = (np.log(host.x_init / host.strikes) + 0.5 * sig ** 2 * tau) / (sig * np.sqrt(tau))
    vega = host.x_init * np.exp(-0.5 * d1 ** 2) / np.sqrt(2 * np.pi) * np.sqrt(tau)
    tol = 1e-8 + (1e-9 * np.abs(host.prices) + PRICE_ATOL) / np.maximum(vega, 1e-300)
    assert (both_nan | (np.abs(dev.ivs - host.ivs) <= tol)).all()


def test_longer_paths_than_the_native_envelope_raise():
    with pytest.raises(ValueError, match="4096"):
        sa.mrw_log_returns(2, 4097, seed=1, cuda=True)
    with pytest.raises(ValueError, match="4096"):
        sa.MRWGenerator(T=4099).load(R=2, seed=1, cuda=True)
    # the C ABI itself: PSH_ERR_UNSUPPORTED (-2) for n > 4096, PSH_ERR_ARG (-1) before anything touches the device
    L = _native.load()
    tab = torch.zeros(16384, dtype=torch.float64, device="cuda")
    assert L.psh_mrw_generate(0, None, 2, 4097, 0.01, tab.data_ptr(), None, 0.3, 1, None, 0, None, None) == -2
    assert L.psh_mrw_generate(0, None, 2, 1, 0.01, tab.data_ptr(), None, 0.3, 1, None, 0, None, None) == -1
    assert L.psh_mrw_generate(0, None, 0, 64, 0.01, tab.data_ptr(), None, 0.3, 1, None, 0, None, None) == -1
    assert L.psh_mrw_generate(0, None, 2, 64, 0.01, None, None, 0.3, 1, None, 0, None, None) == -1
    assert L.psh_mrw_generate(0, None, 2, 64, float("nan"), tab.data_ptr(), None, 0.3, 1, None, 0, None, None) == -1
    assert L.psh_mrw_generate(0, None, 2, 64, 0.01, tab.data_ptr(), None, 0.3, 1, tab.data_ptr(), 63, None, None) == -1
