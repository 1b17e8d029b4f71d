"""psh_pdv_generate on the MI355X: against the reference's outputs on their own draws (tests/golden/pdv_*.npz), against the
numpy twin on the same seed and on the device's own draws, bitwise repeatability and batching, the normalised draws, the
generator's distributions, and PDV paths priced by compute_smile on the device."""
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, pdv, pricing

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_device")]
GOLDEN = Path(__file__).resolve().parent / "golden"
DT = 1 / 252
DISC = ["disc_b3_gauss_T75", "disc_b4_gauss_T1", "disc_b3_t3_T1", "disc_b4_t3_T75", "disc_clip", "disc_floor", "disc_nan"]
LAMS = dict(lams1=[60.0, 4.0], lams2=[40.0, 1.5], thetas=[0.6, 0.3])


def load(name):
    with np.load(GOLDEN / f"pdv_{name}.npz") as z:
        return {k: z[k] for k in z.files}


def assert_same(dev, host, rtol=1e-10):
    """NaN in exactly the same places, the rest to rtol (only the order of the per-path sums differs)."""
    dev = dev.cpu().numpy() if isinstance(dev, torch.Tensor) else dev
    np.testing.assert_array_equal(np.isnan(dev), np.isnan(host))
    ok = ~np.isnan(host)
    np.testing.assert_allclose(dev[ok], host[ok], rtol=rtol, atol=0)


def model(betas=(0.04, -0.12, 0.6, 0.5), nu=None):
    return pdv.PDVModelDiscrete(**LAMS, betas=list(betas), nu=nu)


@pytest.mark.parametrize("name", DISC)
def test_device_matches_reference_on_its_draws(name):
    g = load(name)
    nu = float(g["nu"])
    m = pdv.PDVModelDiscrete(g["lams1"], g["lams2"], g["thetas"], g["betas"], nu=nu if nu > 0 else None)
    sigma, St = m.gen(float(g["T"]), DT, float(g["S0"]), int(g["S"]), g["R10"], g["R20"], cuda=True,
                      draws=torch.from_numpy(g["raw"]).cuda())
    assert sigma.is_cuda and St.is_cuda and St.dtype == torch.float64
    assert_same(sigma, g["sigma"])
    assert_same(St, g["St"])


@pytest.mark.parametrize("betas,nu", [((0.04, -0.12, 0.6), None), ((0.04, -0.12, 0.6, 0.5), None),
                                      ((0.04, -0.12, 0.6), 3.0), ((0.04, -0.12, 0.6, 0.5), 5.0)])
def test_seeded_device_matches_host_twin(betas, nu):
    m = model(betas, nu)
    B, S, n = 3, 700, 130
    R10 = np.array([[0.0, 0.01], [0.05, -0.02], [-0.03, 0.0]])
    R20 = np.array([[0.04, 0.03], [0.02, 0.05], [0.09, 0.01]])
    dec = lambda lam: np.exp(-np.asarray(lam)[None, :] / 252)[0]   # noqa: E731
    dev = _native.pdv_generate(B, S, n, m.lams1, m.lams2, dec(m.lams1), dec(m.lams2), m.thetas, m.betas, 100.0, np.sqrt(DT),
                               m._draw_nu(), R10, R20, seed=1234, outputs=("sigma", "St", "dlnx", "raw"))
    host = m._host(B, S, n, 100.0, DT, R10, R20, 1234, None, want_dlnx=True)
    raw = dev["raw"].cpu().numpy()
    np.testing.assert_allclose(raw, pdv.philox_draws(1234, B * S, n, m._draw_nu()), rtol=1e-12, atol=1e-13)
    assert_same(dev["sigma"], host["sigma"])
    assert_same(dev["St"], host["St"])
    np.testing.assert_allclose(dev["dlnx"].cpu().numpy(), host["dlnx"], rtol=1e-6, atol=1e-9)
    # ... and the host twin on the device's own draws
    again = m._host(B, S, n, 100.0, DT, R10, R20, None, raw)
    assert_same(dev["sigma"], again["sigma"])
    assert_same(dev["St"], again["St"])


def test_two_calls_give_identical_bits():
    m = model(nu=3.0)
    a = m.gen(1.0, DT, 100.0, 3000, [0.0, 0.01], [0.04, 0.03], seed=9, cuda=True)
    b = m.gen(1.0, DT, 100.0, 3000, [0.0, 0.01], [0.04, 0.03], seed=9, cuda=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_dates_batch_like_paths():
    """(B = 2, S = 1024) with equal factors is (B = 1, S = 2048): path g = b * S + p of one generator."""
    m = model()
    x = 100.0 * np.exp(np.cumsum(0.01 * np.random.default_rng(1).standard_normal(100)))
    two = pdv.pdv_future_paths(np.stack([x, x]), m, 100, 100.0, 1024, 75 / 252, DT, seed=77, cuda=True)
    R10, R20 = pdv.compute_factor(x[None], m, 100, DT)
    _, one = m.gen(75 / 252, DT, 100.0, 2048, R10, R20, seed=77, cuda=True)
    assert two.shape == (2, 1024, 75)
    assert torch.equal(two.reshape(2048, 75), one)


@pytest.mark.parametrize("nu", [0.0, 3.0])
def test_normalised_draws_have_zero_mean_and_step_std(nu):
    m = model(nu=nu or None)
    dec = np.exp(-np.asarray(m.lams1)[None, :] / 252)[0]
    out = _native.pdv_generate(2, 500, 252, m.lams1, m.lams2, dec, dec, m.thetas, m.betas, 100.0, np.sqrt(DT), nu,
                               np.zeros((2, 2)), np.full((2, 2), 0.04), seed=3, outputs=("dw",))
    dw = out["dw"].cpu().numpy()
    assert np.abs(dw.mean(axis=1)).max() < 1e-12
    assert np.abs(dw.std(axis=1) / np.sqrt(DT) - 1).max() < 1e-12


def _ks(x, cdf):
    x = np.sort(x)
    n = x.size
    F = cdf(x)
    i = np.arange(1, n + 1)
    return max((i / n - F).max(), (F - (i - 1) / n).max())


@pytest.mark.parametrize("nu", [0.0, 3.0])
def test_raw_draw_distribution(nu):
    m = model(nu=nu or None)
    dec = np.exp(-np.asarray(m.lams1)[None, :] / 252)[0]
    out = _native.pdv_generate(1, 1000, 1000, m.lams1, m.lams2, dec, dec, m.thetas, m.betas, 100.0, np.sqrt(DT), nu,
                               np.zeros((1, 2)), np.full((1, 2), 0.04), seed=2024, outputs=("raw",))
    z = out["raw"].cpu().numpy().ravel()
    if nu == 0.0:
        cdf = lambda v: torch.special.ndtr(torch.from_numpy(v)).numpy()       # noqa: E731
    else:                                                                       # t(3): closed form
        cdf = lambda v: 0.5 + (np.arctan(v / math.sqrt(3)) + (v / math.sqrt(3)) / (1 + v * v / 3)) / math.pi   # noqa: E731
    assert _ks(z, cdf) < 1.63 / math.sqrt(z.size)


def test_future_paths_priced_on_the_device_match_the_host_pipeline():
    m = model()
    g = np.random.default_rng(5)
    x_past = 100.0 * np.exp(np.cumsum(0.012 * g.standard_normal((16, 100)), axis=1))
    Ts, Ms = [7, 25, 60], np.linspace(-2, 2, 9)
    St_dev = pdv.pdv_future_paths(x_past, m, 100, 100.0, 2048, 75 / 252, DT, seed=31, cuda=True)
    assert St_dev.is_cuda and St_dev.shape == (16, 2048, 75)
    dev = sa.compute_smile(St_dev, Ts, Ms)                                      # psh_hedged_mc on the HIP tensor
    St_host = pdv.pdv_future_paths(x_past, m, 100, 100.0, 2048, 75 / 252, DT, seed=31, cuda=False)
    host = sa.compute_smile(St_host, Ts, Ms, cuda=False)
    np.testing.assert_array_equal(dev.status, host.status)
    assert (host.status == 0).all()
    # strikes and sigma: 1e-10, not the 1e-12 of tests/test_gpu_hmc.py -- the paths agree to ~1e-15, and their float32
    # log-returns can round to neighbouring values, each such return moving sigma_T by ~1e-12
    np.testing.assert_allclose(dev.strikes, host.strikes, rtol=1e-10)
    np.testing.assert_allclose(dev.sigma, host.sigma, rtol=1e-10)
    np.testing.assert_allclose(dev.prices, host.prices, rtol=1e-9, atol=1e-9)
    tau = (np.asarray(Ts, dtype=np.float64) / 252.0)[:, None]
    sig = np.where(np.isfinite(host.ivs), host.ivs, 1.0)
    d1 = (np.log(host.x_init / host.strikes) + 0.5 * sig ** 2 * tau) / (sig * np.sqrt(tau))
    vega = host.x_init * np.exp(-0.5 * d1 ** 2) / math.sqrt(2 * math.pi) * np.sqrt(tau)
    tol = 1e-8 + (1e-9 * np.abs(host.prices) + 1e-9) / np.maximum(vega, 1e-300)
    ok = (np.isnan(dev.ivs) & np.isnan(host.ivs)) | (np.abs(dev.ivs - host.ivs) <= tol)
    assert ok.all(), np.argwhere(~ok)


def test_argument_errors_raise():
    m = model()
    with pytest.raises(ValueError):
        m.gen(1.0, DT, 100.0, 4, [0, 0], [0.04, 0.04], cuda=True, draws=torch.zeros((4, 3), dtype=torch.float64).cuda())
    with pytest.raises(ValueError):
        _native.pdv_generate(1, 4, 10, m.lams1, m.lams2, m.lams1, m.lams2, m.thetas, m.betas, 100.0, 0.06, -1.0,
                             np.zeros((1, 2)), np.zeros((1, 2)))
