"""Generating from scattering spectra without a GPU: the torch twin's sums against the numpy twin's, the loss at and off the
target, a generation on the CPU against a skewed-MRW target (the loss falls fiftyfold, the leverage signature Im phi3[1, 3]
is the target's), its start, its determinism, the argument checks and the library surface."""
import functools

import numpy as np
import pytest
import torch

import shadowing
import shadowing_amd as sa
from shadowing_amd import _build, _native, scattering

N, J, ROWS = 256, 5, 64


@functools.lru_cache(maxsize=None)
def _target():
    """The spectra of a 2048 x 256 skewed-MRW twin ensemble at J = 5: measured once, shared."""
    ens = sa.smrw_log_returns(2048, N, K0=0.1, alpha=0.6, lam=0.2, sigma=1.0, seed=1, cuda=False)
    return sa.scattering_spectra(ens, J=J, cuda=False)


@functools.lru_cache(maxsize=None)
def _generated(seed):
    """(rows, info) of one generation of 64 rows on the CPU, 60 evaluations: made once per seed, read-only."""
    return sa.scattering_generate(_target(), ROWS, batch=ROWS, max_eval=60, tol=0, seed=seed, cuda=False, return_info=True)


def _rows(R, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, n)) * np.exp(rng.standard_normal((R, n)))).astype(np.float32)


@pytest.mark.parametrize("n,Jc,R,G", [(8, 1, 3, 3), (64, 4, 9, 4), (256, 6, 11, 5)])
def test_torch_twin_sums_equal_the_numpy_twins(n, Jc, R, G):
    x = _rows(R, n, 11 + n)
    x[R - 1, 3] = np.nan                                       # a row left out: zeros, not counted
    ref, ref_rows = scattering._host_sums(x, sa.scattering_bank(n, Jc), G)
    sums, rows = sa.scattering_sums(torch.from_numpy(x), J=Jc, groups=G)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (G, scattering.n_outputs(Jc)) and rows.dtype == torch.int64
    assert np.array_equal(rows.numpy(), ref_rows) and int(rows.sum()) == R - 1
    err = np.abs(sums.numpy() - ref).max() / np.abs(ref).max()
    print(f"n={n} J={Jc}: max |torch twin - numpy twin| / max|numpy twin| = {err:.2e}")
    assert err <= 1e-12
    same, _ = sa.scattering_sums(torch.from_numpy(x)[:, None, :], J=Jc, groups=G)          # the (R, 1, n) layout
    assert torch.equal(same, sums)


def test_torch_twin_is_differentiable_and_leaves_out_rows_get_no_gradient():
    x = torch.from_numpy(_rows(4, 32, 5)).double()
    x[2, 7] = float("inf")
    x.requires_grad_(True)
    sums, rows = sa.scattering_sums(x, J=3, groups=2)
    sums.sum().backward()
    assert rows.tolist() == [2, 1] and torch.isfinite(x.grad).all()
    assert torch.all(x.grad[2] == 0.0) and all(float(x.grad[r].abs().max()) > 0 for r in (0, 1, 3))
    zero = torch.zeros((1, 32), dtype=torch.float64, requires_grad=True)                   # |W| = 0: sgn, never a NaN
    sa.scattering_sums(zero, J=3)[0].sum().backward()
    assert torch.all(zero.grad == 0.0)


def test_loss_is_zero_at_the_target_and_the_hand_computed_value_off_it():
    t = _target()
    nout = scattering.n_outputs(J)
    sums, rows = torch.from_numpy(t.group_sums), torch.from_numpy(t.group_rows)
    # (m and T are the same sums added in another order: a relative 1e-15 apart at the most, and the loss is its square)
    assert float(sa.scattering_loss(sums, rows, t)) <= 1e-28
    T = t.group_sums.sum(axis=0) / t.rows_used
    sigma2 = T[J:2 * J]
    assert np.array_equal(sigma2, t.phi2)
    # one row whose values are the target's means, moved by 0.3 sigma_1 in S1[1], -0.2 sigma2_2 in S2[2], 0.1 sigma_1 sigma_3 in
    # Im C3[1, 3] and 0.05 sigma_2 sigma_3 in Re C4[2, 3, 4]: loss = (0.09 + 0.04 + 0.01 + 0.0025) / NOUT
    P3, P4 = J * (J + 1) // 2, J * (J + 1) * (J + 2) // 6
    v = T.copy()
    v[0] += 0.3 * np.sqrt(sigma2[0])
    v[J + 1] -= 0.2 * sigma2[1]
    v[2 * J + P3 + scattering.pair_index(1, 3)] += 0.1 * np.sqrt(sigma2[0] * sigma2[2])
    v[2 * J + 2 * P3 + scattering.triple_index(2, 3, 4)] += 0.05 * np.sqrt(sigma2[1] * sigma2[2])
    got = float(sa.scattering_loss(torch.from_numpy(v[None] * 3.0), torch.tensor([3]), t))   # three such rows in one group
    np.testing.assert_allclose(got, 0.1425 / nout, rtol=1e-12)
    # quadratic in the sums: its gradient at the target is zero
    s = sums.clone().requires_grad_(True)
    sa.scattering_loss(s, rows, t).backward()
    assert float(s.grad.abs().max()) <= 1e-14
    with pytest.raises(ValueError, match="J = 5"):
        sa.scattering_loss(torch.zeros((1, scattering.n_outputs(4)), dtype=torch.float64), torch.tensor([1]), t)


def test_generation_on_the_cpu_reaches_the_targets_spectra():
    t = _target()
    x, info = _generated(0)
    assert isinstance(x, torch.Tensor) and x.dtype == torch.float32 and tuple(x.shape) == (ROWS, 1, N) and not x.is_cuda
    first, last, evals = info["initial_loss"][0], info["final_loss"][0], info["evaluations"][0]
    print(f"loss {first:.3e} -> {last:.3e} in {evals} evaluations: ratio {last / first:.2e}")
    assert evals == 60 and len(info["initial_loss"]) == 1
    assert last <= 0.02 * first
    got = sa.scattering_spectra(x.numpy(), J=J, cuda=False)
    # the loss reported is the loss of the rows returned
    sums, rows = torch.from_numpy(got.group_sums), torch.from_numpy(got.group_rows)
    np.testing.assert_allclose(float(sa.scattering_loss(sums, rows, t)), last, rtol=1e-6)
    dev = abs(got.phi3[0, 2].imag - t.phi3[0, 2].imag)
    print(f"Im phi3[1,3]: generated {got.phi3[0, 2].imag:.4f}, target {t.phi3[0, 2].imag:.4f} +- {t.phi3_se[0, 2]:.4f}: "
          f"{dev / t.phi3_se[0, 2]:.2f} of the standard error")
    assert t.phi3[0, 2].imag < -0.02 and dev <= t.phi3_se[0, 2]


def test_the_same_seed_gives_the_same_bits_and_another_seed_other_rows():
    x, info = _generated(0)
    again, info2 = sa.scattering_generate(_target(), ROWS, batch=ROWS, max_eval=60, tol=0, seed=0, cuda=False,
                                          return_info=True)
    assert torch.equal(x.view(torch.int32), again.view(torch.int32)) and info == info2
    other = sa.scattering_generate(_target(), 8, batch=8, max_eval=2, tol=0, seed=1, cuda=False)
    assert not torch.equal(other, sa.scattering_generate(_target(), 8, batch=8, max_eval=2, tol=0, seed=2, cuda=False))


def test_the_start_is_white_noise_of_the_targets_power_and_batches_are_their_own_problems():
    t = _target()
    bank = sa.scattering_bank(N, J)
    var = scattering.start_variance(t)
    np.testing.assert_allclose(var, t.phi2.sum() / ((bank * bank).sum() / N), rtol=1e-14)
    assert 0.9 < var < 1.1                                      # a unit-variance target
    # one evaluation: the rows returned are the start itself
    x, info = sa.scattering_generate(t, 600, batch=256, max_eval=1, tol=0, seed=3, cuda=False, return_info=True)
    assert tuple(x.shape) == (600, 1, N) and info["evaluations"] == [1, 1, 1]
    np.testing.assert_allclose(float(x.double().var()), var, rtol=0.02)
    white = sa.scattering_spectra(x.numpy(), J=J, cuda=False)
    np.testing.assert_allclose(white.phi2.sum(), t.phi2.sum(), rtol=0.02)
    # batch b is seeded with (seed, b): the second batch of 256 does not depend on how many rows are asked for
    short = sa.scattering_generate(t, 300, batch=256, max_eval=1, tol=0, seed=3, cuda=False)
    assert torch.equal(short[:256], x[:256]) and torch.equal(short[256:], x[256:300])
    # a loose tolerance stops at once
    _, info = sa.scattering_generate(t, 8, batch=8, max_eval=50, tol=1.0, seed=3, cuda=False, return_info=True)
    assert info["evaluations"] == [1]


def test_argument_errors():
    t = _target()
    with pytest.raises(ValueError, match="power of two"):
        sa.scattering_generate(np.zeros((4, 100), dtype=np.float32), 4, cuda=False)
    with pytest.raises(ValueError, match="power of two"):
        sa.scattering_sums(torch.zeros((4, 100)))
    for R in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="R must be"):
            sa.scattering_generate(t, R, cuda=False)
    with pytest.raises(ValueError, match="batch must be"):
        sa.scattering_generate(t, 4, batch=0, cuda=False)
    with pytest.raises(ValueError, match="no rows"):
        sa.scattering_generate(np.full((4, 64), np.nan, dtype=np.float32), 4, cuda=False)
    with pytest.raises(TypeError, match="torch tensor"):
        sa.scattering_sums(np.zeros((4, 64), dtype=np.float32))
    with pytest.raises(ValueError, match="groups must be"):
        sa.scattering_sums(torch.zeros((4, 64)), groups=5)
    with pytest.raises(ValueError, match="J must be"):
        sa.scattering_sums(torch.zeros((4, 64)), J=5)
    if not torch.cuda.is_available():
        with pytest.raises(_native.NativeLibraryError, match="no host fallback"):
            sa.scattering_generate(t, 4, cuda=True)


def test_the_library_surface():
    assert "psh_scattering_vjp" in _native.EXPORTS and "psh_scattering_vjp_workspace_bytes" in _native.EXPORTS
    assert _build.CSRC / "psh_scattering_grad.hip" in _build.SOURCES
    assert _build.CSRC / "psh_scat_lds.h" in _build.DEPS        # the inverse transform the two scattering kernels share
    for name in ("scattering_sums", "scattering_loss", "scattering_generate"):
        assert getattr(shadowing, name) is getattr(sa, name) and name in sa.__all__
    assert callable(_native.scattering_vjp)
