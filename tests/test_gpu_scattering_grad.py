"""psh_scattering_vjp on the MI355X: against autograd through the torch float64 twin (an independent derivation: torch.fft on
the time-domain definition) at the project's bound for an in-LDS double transform, with a random cotangent and with every
unit cotangent by itself; bitwise repeatability and independence of a row's gradient from everything but the row and its
group's cotangent; strides; rows with NaN / inf and rows of zeros; the autograd path of scattering_sums; the error codes; and
a generation on the device."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, scattering

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_device")]

BOUND = 1e-9                                         # tests/test_gpu_scattering.py's bound for these transforms in double
# (n, J, R, G): both LDS-size instantiations (n <= 1024, n <= 4096); log2(n) = 0, 1, 2 mod 3 (the inverse's first pass takes
# 0, 1 or 2 stages); the top J of each size; G not dividing R
CASES = [(8, 1, 3, 3), (16, 2, 5, 2), (64, 4, 9, 4), (256, 6, 33, 5), (1024, 3, 4, 1), (2048, 9, 3, 3), (4096, 9, 7, 3),
         (4096, 10, 2, 1)]


def _rows(R, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, n)) * np.exp(rng.standard_normal((R, n)))).astype(np.float32)


def _twin_grad(x, J, G, cot):
    """(R, n) float64 numpy: d sum(cot * sums) / dx by autograd through the CPU twin (x float32 numpy, cot (G, NOUT))."""
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    sums, _ = sa.scattering_sums(xt, J=J, groups=G)
    (sums * torch.as_tensor(cot)).sum().backward()
    return xt.grad.numpy()


@functools.lru_cache(maxsize=None)
def _case(n, J, R, G):
    """(x, cot, twin gradient): computed once per case, read-only."""
    x = _rows(R, n, 2000 + n + J)
    cot = np.random.default_rng(n + J).standard_normal((G, scattering.n_outputs(J)))
    grad = _twin_grad(x, J, G, cot)
    for a in (x, cot, grad):
        a.setflags(write=False)
    return x, cot, grad


def _device(x, J, G, cot, out=None):
    t = x if isinstance(x, torch.Tensor) else torch.tensor(x).cuda()
    c = cot if isinstance(cot, torch.Tensor) else torch.tensor(cot).cuda()
    return _native.scattering_vjp(t, J, G, scattering._device_bank(t.shape[-1], J, t.device), c, out=out)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _check_rows(dev, twin, what):
    """Per row: |device - twin| <= 1e-9 max_t |twin|."""
    top = np.abs(twin).max(axis=1)
    err = np.abs(dev - twin).max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.max(np.where(top > 0, err / (BOUND * top), np.where(err > 0, np.inf, 0.0))))
    print(f"{what}: max over rows of max_t |dev - twin| / (1e-9 max_t |twin|) = {ratio:.3e}  (relative {ratio * BOUND:.2e})")
    assert np.isfinite(dev).all() and ratio <= 1.0
    return ratio


@pytest.mark.parametrize("n,J,R,G", CASES)
def test_device_gradient_matches_autograd_through_the_twin(n, J, R, G):
    x, cot, twin = _case(n, J, R, G)
    grad, status = _device(x, J, G, cot)
    assert grad.dtype == torch.float64 and tuple(grad.shape) == (R, n) and int(status.item()) == 0
    assert np.abs(twin).max(axis=1).min() > 0
    _check_rows(grad.cpu().numpy(), twin, f"n={n} J={J} R={R} G={G}")


@functools.lru_cache(maxsize=None)
def _twin_jacobian(n, J, R):
    """(x, jac (NOUT, R, n)): the gradient of each output of each row by itself, by autograd through the twin (one group
    per row, so sums[r] is row r's own values)."""
    x = _rows(R, n, 77 + n)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    sums, _ = sa.scattering_sums(xt, J=J, groups=R)
    jac = np.stack([torch.autograd.grad(sums[:, o].sum(), xt, retain_graph=True)[0].numpy()
                    for o in range(sums.shape[1])])
    return x, jac


@pytest.mark.parametrize("n,J", [(16, 2), (32, 3)])
def test_every_unit_cotangent_by_itself(n, J):
    """A wrong p3 / p4 index or a wrong conjugate shows here and hides under a random cotangent."""
    R = 2
    x, jac = _twin_jacobian(n, J, R)
    nout = scattering.n_outputs(J)
    assert nout == {2: 18, 3: 38}[J] and jac.shape == (nout, R, n)
    P3, P4 = J * (J + 1) // 2, J * (J + 1) * (J + 2) // 6
    zero = {2 * J + 2 * P3 + P4 + scattering.triple_index(j1, j1, j2) for j2 in range(1, J + 1) for j1 in range(1, j2 + 1)}
    xd = torch.tensor(x).cuda()
    worst = 0.0
    for o in range(nout):
        cot = torch.zeros((1, nout), dtype=torch.float64, device="cuda")
        cot[0, o] = 1.0
        grad = _device(xd, J, 1, cot)[0].cpu().numpy()
        if o in zero:                                            # Im C4[j, j, j2] is identically 0: its cotangent is ignored
            assert np.all(grad == 0.0) and np.all(jac[o] == 0.0), o
        else:
            assert np.abs(jac[o]).max(axis=1).min() > 0, o
            worst = max(worst, _check_rows(grad, jac[o], f"n={n} J={J} output {o}"))
    print(f"n={n} J={J}: worst ratio over the {nout} unit cotangents {worst:.3e}")


def test_two_calls_give_identical_bits_and_a_row_alone_gets_the_bits_it_gets_in_a_larger_call():
    n, J = 64, 4
    x = torch.from_numpy(_rows(47, n, 4)).cuda()
    cot = torch.from_numpy(np.random.default_rng(5).standard_normal((2, scattering.n_outputs(J)))).cuda()
    a, b = _device(x, J, 2, cot), _device(x, J, 2, cot)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and int(a[1].item()) == 0
    assert scattering.group_bounds(47, 2).tolist() == [0, 23, 47]
    for r in (0, 22, 23, 46):                                    # both edges of both groups
        alone = _device(x[r:r + 1], J, 1, cot[(0 if r < 23 else 1):(1 if r < 23 else 2)].contiguous())
        assert torch.equal(_bits(alone[0][0]), _bits(a[0][r])), r
    # the same with more rows than workgroups' worth of anything: a row's bits do not depend on R or G
    many = _device(x[5:40], J, 35, cot[:1].expand(35, -1).contiguous())
    assert torch.equal(_bits(many[0][:18]), _bits(a[0][5:23]))


def test_more_rows_than_workgroups_and_a_row_after_one_left_out():
    """Past 1024 rows a workgroup takes several rows in turn: row 1027 follows row 3, which holds a NaN and is left out."""
    n, J, R, G = 16, 2, 1030, 7
    x = _rows(R, n, 12)
    x[3, 5] = np.nan
    cot = np.random.default_rng(13).standard_normal((G, scattering.n_outputs(J)))
    grad, status = _device(x, J, G, cot)
    assert int(status.item()) == _native.PSH_SCATTERING_STATUS_ROWS_EXCLUDED and torch.all(grad[3] == 0.0)
    twin = _twin_grad(x, J, G, cot)
    keep = np.arange(R) != 3
    _check_rows(grad.cpu().numpy()[keep], twin[keep], f"n={n} J={J} R={R} G={G}")
    bounds = scattering.group_bounds(R, G)
    for r in (1023, 1024, 1027, 1029):
        g = int(np.searchsorted(bounds, r, side="right")) - 1
        alone = _device(np.ascontiguousarray(x[r:r + 1]), J, 1, np.ascontiguousarray(cot[g:g + 1]))
        assert torch.equal(_bits(alone[0][0]), _bits(grad[r])), r


def test_row_stride_and_gradient_stride_are_handled_in_place():
    J, G, n = 6, 2, 256
    wide = torch.from_numpy(_rows(6, 300, 5)).cuda()
    view = wide[:, :n]
    assert view.stride(0) == 300 and not view.is_contiguous()
    cot = torch.from_numpy(np.random.default_rng(6).standard_normal((G, scattering.n_outputs(J)))).cuda()
    ref = _device(view.contiguous(), J, G, cot)[0]
    assert torch.equal(_bits(_device(view, J, G, cot)[0]), _bits(ref))
    assert torch.equal(_bits(_device(view.contiguous().reshape(6, 1, n), J, G, cot)[0]), _bits(ref))
    out = torch.full((6, 300), 7.0, dtype=torch.float64, device="cuda")
    got, _ = _device(view, J, G, cot, out=out)
    assert got.data_ptr() == out.data_ptr() and got.stride(0) == 300
    assert torch.equal(_bits(out[:, :n]), _bits(ref)) and torch.all(out[:, n:] == 7.0)     # the padding is left untouched


def test_rows_with_nan_or_inf_get_zeros_and_rows_of_zeros_get_zeros():
    n, J = 64, 4
    x = _rows(5, n, 7)
    cot = np.random.default_rng(8).standard_normal((2, scattering.n_outputs(J)))
    clean, status = _device(x, J, 2, cot)
    assert int(status.item()) == 0
    bad = x.copy()
    bad[1, n - 1] = np.nan
    bad[3, 0] = np.inf
    grad, status = _device(bad, J, 2, cot)
    assert int(status.item()) & _native.PSH_SCATTERING_STATUS_ROWS_EXCLUDED
    assert torch.all(grad[1] == 0.0) and torch.all(grad[3] == 0.0) and torch.isfinite(grad).all()
    assert torch.equal(_bits(grad[[0, 2, 4]]), _bits(clean[[0, 2, 4]]))                    # their neighbours are unchanged
    twin = _twin_grad(bad, J, 2, cot)
    assert np.all(twin[[1, 3]] == 0.0)
    _check_rows(grad.cpu().numpy()[[0, 2, 4]], twin[[0, 2, 4]], "beside non-finite rows")
    zeroed = x.copy()
    zeroed[2] = 0.0                                              # W_j = 0 everywhere: the phase is taken as 0
    grad, status = _device(zeroed, J, 2, cot)
    assert int(status.item()) == 0 and torch.all(grad[2] == 0.0) and torch.isfinite(grad).all()
    assert torch.equal(_bits(grad[[0, 1, 3, 4]]), _bits(clean[[0, 1, 3, 4]]))
    assert np.all(_twin_grad(zeroed, J, 2, cot)[2] == 0.0)


@functools.lru_cache(maxsize=None)
def _target():
    """The spectra of tests/test_scattering_grad_cpu.py's target: a 2048 x 256 skewed-MRW twin ensemble at J = 5."""
    ens = sa.smrw_log_returns(2048, 256, K0=0.1, alpha=0.6, lam=0.2, sigma=1.0, seed=1, cuda=False)
    return sa.scattering_spectra(ens, J=5, cuda=False)


def test_scattering_sums_backpropagates_through_the_kernels():
    t = _target()
    n, J, G = 256, 5, 3
    x = torch.from_numpy(_rows(7, n, 9)).cuda().reshape(7, 1, n).requires_grad_(True)
    sums, rows = sa.scattering_sums(x, J=J, groups=G)
    assert sums.is_cuda and sums.dtype == torch.float64 and sums.requires_grad and not rows.requires_grad
    ref = _native.scattering_spectra(x.detach(), J, G, scattering._device_bank(n, J, x.device))
    assert torch.equal(_bits(sums.detach()), _bits(ref[0])) and rows.tolist() == [2, 2, 3]
    sa.scattering_loss(sums, rows, t).backward()
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    leaf = sums.detach().clone().requires_grad_(True)
    sa.scattering_loss(leaf, rows, t).backward()                 # the cotangent the loss hands to the sums
    direct, _ = _device(x.detach(), J, G, leaf.grad)
    assert torch.equal(x.grad[:, 0, :], direct.to(torch.float32)) and float(x.grad.abs().max()) > 0
    # and it is the twin's gradient
    xt = x.detach().cpu().double().requires_grad_(True)
    s2, r2 = sa.scattering_sums(xt, J=J, groups=G)
    sa.scattering_loss(s2, r2, t).backward()
    _check_rows(direct.cpu().numpy(), xt.grad[:, 0, :].numpy(), "loss gradient")


def test_argument_errors_return_codes_without_touching_the_device():
    x = torch.zeros((4, 8192), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="4096"):
        sa.scattering_sums(x)                                    # the transforms of a longer row leave LDS
    with pytest.raises(ValueError, match="4096"):
        sa.scattering_generate(sa.scattering_spectra(_rows(2, 8192, 1), cuda=False), 4, cuda=True)
    L = _native.load()
    psi = torch.zeros((11, 4096), dtype=torch.float64, device="cuda")
    cot = torch.zeros(4 * 570, dtype=torch.float64, device="cuda")
    out = torch.full((4, 4096), 3.0, dtype=torch.float64, device="cuda")
    nbytes = C.c_size_t(0)
    assert L.psh_scattering_vjp_workspace_bytes(4, 4096, 10, 4, C.byref(nbytes)) == 0 and nbytes.value > 0
    assert L.psh_scattering_vjp_workspace_bytes(4, 8192, 9, 4, C.byref(nbytes)) == -2
    assert L.psh_scattering_vjp_workspace_bytes(4, 4095, 9, 4, C.byref(nbytes)) == -1
    assert L.psh_scattering_vjp_workspace_bytes(4, 4096, 11, 4, C.byref(nbytes)) == -1
    assert L.psh_scattering_vjp_workspace_bytes(4, 4096, 9, 5, C.byref(nbytes)) == -1
    assert L.psh_scattering_vjp_workspace_bytes(4, 4096, 9, 4, None) == -1
    assert L.psh_scattering_vjp_workspace_bytes(4, 4096, 10, 4, C.byref(nbytes)) == 0
    ws = torch.zeros((nbytes.value + 7) // 8, dtype=torch.int64, device="cuda")
    call = lambda n, J, stride=8192, gstride=4096, nb=nbytes.value, R=4, G=4, c=cot.data_ptr(): L.psh_scattering_vjp(   # noqa: E731
        0, None, x.data_ptr(), R, stride, n, J, psi.data_ptr(), G, c, out.data_ptr(), gstride, None, ws.data_ptr(), nb)
    assert call(8192, 9, gstride=8192) == -2                     # PSH_ERR_UNSUPPORTED
    assert call(4096, 11) == -1 and call(256, 7) == -1           # J > log2(n) - 2: PSH_ERR_ARG
    assert call(4095, 9) == -1 and call(4096, 9, stride=4095) == -1 and call(4096, 9, gstride=4095) == -1
    assert call(4096, 9, R=0) == -1 and call(4096, 9, G=5) == -1 and call(4096, 9, c=None) == -1
    assert call(4096, 10, nb=nbytes.value - 1) == -3             # PSH_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.all(out == 3.0)
    assert call(4096, 10) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 0.0)                                 # rows of zeros: every gradient is zero


def test_generation_on_the_device_reaches_the_targets_spectra(monkeypatch):
    t = _target()
    x, info = sa.scattering_generate(t, 64, batch=64, max_eval=60, tol=0, seed=0, cuda=True, return_info=True)
    assert isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (64, 1, 256)
    first, last, evals = info["initial_loss"][0], info["final_loss"][0], info["evaluations"][0]
    print(f"loss {first:.3e} -> {last:.3e} in {evals} evaluations: ratio {last / first:.2e}")
    assert evals == 60 and last <= 0.02 * first
    monkeypatch.setattr(scattering, "_host_sums", None)          # the result is read in place: no twin
    got = sa.scattering_spectra(x, J=5)
    monkeypatch.undo()
    dev = abs(got.phi3[0, 2].imag - t.phi3[0, 2].imag)
    print(f"Im phi3[1,3]: generated {got.phi3[0, 2].imag:.4f}, target {t.phi3[0, 2].imag:.4f} +- {t.phi3_se[0, 2]:.4f}: "
          f"{dev / t.phi3_se[0, 2]:.2f} of the standard error")
    assert got.rows_used == 64 and dev <= t.phi3_se[0, 2]
