"""psh_scattering_spectra on the MI355X: against the numpy twin (time-domain sums against the kernel's Fourier-domain forms)
at the project's bound for an in-LDS double transform, bitwise repeatability, a group's sums depending on its rows alone, the
row stride and the (R, 1, n) view, rows with NaN / inf, an ensemble made on the device measured where it lies, and the
public surface."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, scattering

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_device")]

BOUND = 1e-9                                         # tests/test_gpu_mrw.py's bound for this transform in double
# (n, J, R, G): the smallest transform; the top J of each size; G not dividing R; both LDS-size instantiations (n <= 1024,
# n <= 4096); log2(n) = 0, 1, 2 mod 3 (the inverse's first pass takes 0, 1 or 2 stages)
CASES = [(8, 1, 3, 3), (16, 2, 5, 2), (64, 4, 9, 4), (256, 6, 33, 5), (1024, 3, 4, 1), (2048, 9, 3, 3), (4096, 9, 7, 3),
         (4096, 10, 2, 1)]


def _rows(R, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, n)) * np.exp(rng.standard_normal((R, n)))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _twin(n, J, R, G):
    """(x, sums, rows) of the twin: computed once per case, read-only."""
    x = _rows(R, n, 1000 + n + J)
    sums, rows = scattering._host_sums(x, sa.scattering_bank(n, J), G)
    for a in (x, sums, rows):
        a.setflags(write=False)
    return x, sums, rows


def _families(v, J):
    """S1, S2 (real), C3, C4 (complex) of (G, NOUT) sums."""
    P3, P4 = J * (J + 1) // 2, J * (J + 1) * (J + 2) // 6
    o4 = 2 * J + 2 * P3
    return (v[:, :J], v[:, J:2 * J], v[:, 2 * J:2 * J + P3] + 1j * v[:, 2 * J + P3:o4], v[:, o4:o4 + P4] + 1j * v[:, o4 + P4:])


def _check_against_twin(dev, twin, J, what):
    """For every group and family: |device - twin| <= 1e-9 max |twin of that family in that group|."""
    assert dev.shape == twin.shape == (twin.shape[0], scattering.n_outputs(J))
    worst = 0.0
    for name, d, t in zip(("S1", "S2", "C3", "C4"), _families(dev, J), _families(twin, J)):
        top = np.abs(t).max(axis=1, keepdims=True)
        err = np.abs(d - t)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = float(np.nanmax(np.where(top > 0, err / (BOUND * top), np.where(err > 0, np.inf, 0.0))))
        print(f"{what} {name}: max |dev - twin| / (1e-9 max|twin|) = {ratio:.3e}  (|dev - twin| / max|twin| = {ratio * BOUND:.2e})")
        worst = max(worst, ratio)
    assert worst <= 1.0
    return worst


def _device(x, J, G):
    t = x if isinstance(x, torch.Tensor) else torch.tensor(x).cuda()
    return _native.scattering_spectra(t, J, G, scattering._device_bank(t.shape[-1], J, t.device))


def _bits(t):
    return t.view(torch.int64)


@pytest.mark.parametrize("n,J,R,G", CASES)
def test_device_matches_twin(n, J, R, G):
    x, sums, rows = _twin(n, J, R, G)
    d_sums, d_rows, status = _device(x, J, G)
    assert d_sums.dtype == torch.float64 and d_rows.dtype == torch.int64 and int(status.item()) == 0
    _check_against_twin(d_sums.cpu().numpy(), sums, J, f"n={n} J={J} R={R} G={G}")
    assert np.array_equal(d_rows.cpu().numpy(), rows) and int(rows.sum()) == R
    P3, P4 = J * (J + 1) // 2, J * (J + 1) * (J + 2) // 6
    im4 = d_sums.cpu().numpy()[:, 2 * J + 2 * P3 + P4:]
    assert all(im4[:, scattering.triple_index(j1, j1, j2)].tolist() == [0.0] * G
               for j2 in range(1, J + 1) for j1 in range(1, j2 + 1))          # C4 is real at j1 = j1'


def test_two_calls_give_identical_bits_and_a_groups_sums_depend_on_its_rows_alone():
    n, J = 256, 6
    x = torch.from_numpy(_rows(9, n, 3)).cuda()
    a, b = _device(x, J, 2), _device(x, J, 2)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and a[1].tolist() == [4, 5]
    head = _device(x[:4], J, 1)                              # rows [0, 4): the first group of the call above
    assert torch.equal(_bits(head[0][0]), _bits(a[0][0])) and head[1].tolist() == [4]
    tail = _device(x[4:], J, 1)
    assert torch.equal(_bits(tail[0][0]), _bits(a[0][1])) and tail[1].tolist() == [5]
    # more rows than units: 40 rows in one group are 14 units of 3 rows; the same rows as the second of two groups
    big = torch.from_numpy(_rows(47, 64, 4)).cuda()
    whole = _device(big[7:], 4, 1)
    assert scattering.group_bounds(47, 2).tolist() == [0, 23, 47]
    both = _device(big, 4, 2)
    alone = _device(big[23:], 4, 1)
    assert torch.equal(_bits(alone[0][0]), _bits(both[0][1])) and whole[1].tolist() == [40]
    _check_against_twin(whole[0].cpu().numpy(), scattering._host_sums(big[7:].cpu().numpy(), sa.scattering_bank(64, 4), 1)[0],
                        4, "40 rows in one group")


def test_row_stride_and_the_ensemble_view_are_read_in_place():
    J, G = 6, 2
    wide = torch.from_numpy(_rows(6, 300, 5)).cuda()
    view = wide[:, :256]
    flat = view.contiguous()
    assert view.stride(0) == 300 and not view.is_contiguous()
    ref = _device(flat, J, G)
    for other in (_device(view, J, G), _device(flat.reshape(6, 1, 256), J, G)):
        assert torch.equal(_bits(other[0]), _bits(ref[0])) and torch.equal(other[1], ref[1]) and int(other[2].item()) == 0
    got = sa.scattering_spectra(wide[:, None, :256], J=J, groups=G)
    assert np.array_equal(got.group_sums, ref[0].cpu().numpy()) and got.rows_used == 6


def test_rows_with_nan_or_inf_are_left_out():
    n, J = 64, 4
    x = _rows(5, n, 7)
    bad = x.copy()
    bad[1, n - 1] = np.nan
    bad[3, 0] = np.inf
    d_sums, d_rows, status = _device(bad, J, 1)
    assert int(status.item()) & _native.PSH_SCATTERING_STATUS_ROWS_EXCLUDED and d_rows.tolist() == [3]
    assert np.isfinite(d_sums.cpu().numpy()).all()
    # ... with the bits of a call without those rows: one row per unit either way, the units added in order
    kept = _device(np.ascontiguousarray(x[[0, 2, 4]]), J, 1)
    assert torch.equal(_bits(d_sums), _bits(kept[0])) and int(kept[2].item()) == 0
    # the same in a layout of groups: the other rows keep their bits when zeros stand where the bad rows stood
    zeroed = x.copy()
    zeroed[[1, 3]] = 0.0
    two, ref = _device(bad, J, 2), _device(zeroed, J, 2)
    assert torch.equal(_bits(two[0]), _bits(ref[0])) and two[1].tolist() == [1, 2] and ref[1].tolist() == [2, 3]
    sums, rows = scattering._host_sums(bad, sa.scattering_bank(n, J), 2)
    assert rows.tolist() == [1, 2]
    _check_against_twin(two[0].cpu().numpy(), sums, J, "non-finite rows")
    # a group with no row left: sums 0, rows_used 0, standard errors NaN
    bad[0, 5] = -np.inf
    d_sums, d_rows, status = _device(bad, J, 2)
    assert d_rows.tolist() == [0, 2] and torch.all(d_sums[0] == 0.0) and int(status.item()) == 1
    s = sa.scattering_spectra(torch.from_numpy(bad).cuda(), J=J, groups=2)
    assert s.rows_used == 2 and s.rows_excluded == 3 and np.all(np.isnan(s.phi1_se)) and np.all(np.isfinite(s.phi1))


def test_an_ensemble_made_on_the_device_is_measured_where_it_lies(monkeypatch):
    ens = sa.smrw_log_returns(512, 256, K0=0.1, alpha=0.6, lam=0.2, seed=1, cuda=True)
    assert isinstance(ens, torch.Tensor) and ens.is_cuda and ens.shape == (512, 1, 256)
    copied = []
    to_host = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copied.append(self.numel()), to_host(self, *a, **k))[1])
    monkeypatch.setattr(scattering, "_host_sums", None)      # cuda=None on a HIP float32 tensor is the device
    s = sa.scattering_spectra(ens, J=5)
    monkeypatch.undo()
    assert copied and max(copied) <= 64 * scattering.n_outputs(5), copied    # only the (G, NOUT) sums and the rows cross
    print(f"device smrw phi3[1,3] = {s.phi3[0, 2]:.4f} +- {s.phi3_se[0, 2]:.4f}")
    assert s.phi3[0, 2].imag < -0.015 and s.rows_used == 512 and s.group_rows.size == 64
    twin = sa.scattering_spectra(ens.cpu().numpy(), J=5, cuda=False)
    _check_against_twin(s.group_sums, twin.group_sums, 5, "smrw ensemble")
    np.testing.assert_allclose(s.phi3[0, 2], twin.phi3[0, 2], rtol=1e-8)


def test_the_public_surface_and_the_error_codes():
    x = torch.zeros((4, 8192), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="4096"):
        sa.scattering_spectra(x)                                              # the transforms of a longer row leave LDS
    with pytest.raises(ValueError, match="J must be"):
        sa.scattering_spectra(x[:, :256], J=7)
    with pytest.raises(ValueError, match=r"x\[\.\.\., :4096\]"):
        sa.scattering_spectra(x[:, :5000])
    up = sa.scattering_spectra(_rows(3, 64, 9), J=3, cuda=True)               # cuda=True uploads a numpy ensemble
    dev = sa.scattering_spectra(torch.from_numpy(_rows(3, 64, 9)).cuda(), J=3)
    assert np.array_equal(up.group_sums, dev.group_sums)
    own = sa.scattering_spectra(torch.from_numpy(_rows(3, 64, 9)).cuda(), J=3, bank=sa.scattering_bank(64, 3))
    assert np.array_equal(own.group_sums, dev.group_sums)
    half = sa.scattering_spectra(torch.from_numpy(_rows(3, 64, 9)).cuda().double(), J=3)   # not float32: the twin
    np.testing.assert_allclose(half.group_sums, dev.group_sums, rtol=0, atol=1e-9 * np.abs(dev.group_sums).max())
    # the C ABI on real buffers
    L = _native.load()
    psi = torch.zeros((11, 4096), dtype=torch.float64, device="cuda")
    out = torch.zeros(4 * 570, dtype=torch.float64, device="cuda")
    rows = torch.zeros(4, dtype=torch.int64, device="cuda")
    nbytes = C.c_size_t(0)
    assert L.psh_scattering_spectra_workspace_bytes(4, 10, 4, C.byref(nbytes)) == 0 and nbytes.value == 4 * (570 * 8 + 8)
    ws = torch.zeros(nbytes.value // 8, dtype=torch.int64, device="cuda")
    call = lambda n, J, stride=8192, nb=nbytes.value: L.psh_scattering_spectra(   # noqa: E731
        0, None, x.data_ptr(), 4, stride, n, J, psi.data_ptr(), 4, out.data_ptr(), rows.data_ptr(), None, ws.data_ptr(), nb)
    assert call(4096, 10) == 0
    assert call(8192, 9) == -2                                   # PSH_ERR_UNSUPPORTED
    assert call(4096, 11) == -1 and call(256, 7) == -1           # J > log2(n) - 2: PSH_ERR_ARG
    assert call(4095, 9) == -1 and call(4096, 9, stride=4095) == -1
    assert call(4096, 10, nb=nbytes.value - 1) == -3
    torch.cuda.synchronize()
    assert rows.tolist() == [1, 1, 1, 1] and torch.all(out == 0.0)           # rows of zeros: every sum is zero
