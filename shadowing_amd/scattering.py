"""The wavelet scattering spectra of an ensemble, measured where it lies (Morel et al., arXiv 2204.10177, stated in this
project's own terms: parity with scatspectra is not pinned).

For R rows of n returns, n a power of two, and J scales, with F the DFT of size n (convolutions are circular over a row) and
psi_hat[j] the real Fourier multiplier of an analytic wavelet, per row
    W_j = IDFT(F[x] psi_hat[j]),   U_j = |W_j|,   V_{j1,j2} = IDFT(F[U_j1] psi_hat[j2]),  j1 <= j2,
    S1[j] = mean_t U_j               S2[j] = mean_t U_j^2
    C3[j1,j2] = mean_t W_j2 conj(V_{j1,j2}),  j1 <= j2               C4[j1,j1',j2] = mean_t V_{j1,j2} conj(V_{j1',j2}),  j1 <= j1' <= j2
every sample converted to double first, a row that holds a NaN or an inf left out whole.  Averaged over the rows and with
sigma2[j] = mean S2[j]:
    phi1[j] = mean S1[j] / sqrt(sigma2[j])              sparsity of the wavelet coefficients (sqrt(pi) / 2 for a Gaussian)
    phi2[j] = sigma2[j]                                 the wavelet power spectrum
    phi3[j1,j2] = mean C3 / sqrt(sigma2[j1] sigma2[j2]) phase-envelope cross-spectrum: skewness, time asymmetry (leverage)
    phi4[j1,j1',j2] = mean C4 / sqrt(sigma2[j1] sigma2[j1'])   envelope cross-spectrum: kurtosis, volatility clustering
The rows are cut into G groups (stylized.group_bounds) and the scatter of the group values gives each its standard error.
The stock wavelets (scattering_bank): with k_j = n / 2^(j+1), psi_hat[j][k] = cos(pi/2 log2(k / k_j)) for |log2(k / k_j)| < 1,
else 0, so psi_j^2 + psi_(j+1)^2 = 1 between two centres and bin 0 (a row's mean) is in no band.

On a HIP float32 tensor the sums are psh_scattering_spectra's (the method heads shadowing_amd/csrc/psh_scattering.hip, which
uses the Fourier-domain forms of C3 and C4): the ensemble is read in place, every transform stays in LDS and only the
(G, NOUT) sums come to the host.  `cuda=False` is the numpy float64 twin: np.fft on the time-domain sums above, on
float32-rounded inputs.

Generating from them (scattering_generate): `scattering_sums` is the same measurement made differentiable in the rows -- on a
HIP float32 tensor a torch.autograd.Function over psh_scattering_spectra and psh_scattering_vjp (the gradient kernel heads
shadowing_amd/csrc/psh_scattering_grad.hip), on a CPU tensor a torch float64 twin (torch.fft on the time-domain definition,
differentiated by autograd: an independent derivation) -- `scattering_loss` the squared distance of a batch's mean values to
a target's in the normalisations of phi1 .. phi4 frozen at the target, and `scattering_generate` gradient descent from white
noise on that loss, batch by batch.  It is this project's counterpart of scatspectra's `generate`; parity is not pinned.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .stylized import DEFAULT_GROUPS, _is_torch, group_bounds

MAX_N_DEVICE = 4096                                  # PSH_SCAT_MAX_N: the transforms of a longer row leave LDS
DEFAULT_MAX_J = 9
_TWIN_BYTES = 1 << 26                                # the twin walks the rows in chunks of about this many bytes of V


@dataclass(frozen=True)
class ScatteringSpectra:
    """The normalised scattering spectra of an ensemble, their standard errors from the scatter of the row groups (each
    group normalised with the ensemble's sigma2, weighted by its rows; NaN with fewer than two non-empty groups), and what
    they were made from.  Scale j is index j - 1."""
    n: int
    J: int
    phi1: np.ndarray                                 # (J,)
    phi2: np.ndarray                                 # (J,)
    phi3: np.ndarray                                 # (J, J) complex [j1, j2], NaN where j1 > j2
    phi4: np.ndarray                                 # (J, J, J) complex [j1, j1', j2], NaN outside j1 <= j1' <= j2
    phi1_se: np.ndarray
    phi2_se: np.ndarray
    phi3_se: np.ndarray                              # (J, J) float64: of the modulus of the deviation
    phi4_se: np.ndarray
    rows_used: int
    rows_excluded: int
    group_sums: np.ndarray = field(repr=False)       # (G, NOUT) float64: the sums as measured (they add across ranks)
    group_rows: np.ndarray = field(repr=False)       # (G,) int64


def n_outputs(J: int) -> int:
    """NOUT = 2 J + 2 P3 + 2 P4: [S1 (J), S2 (J), Re C3 (P3), Im C3 (P3), Re C4 (P4), Im C4 (P4)]."""
    return 2 * J + J * (J + 1) + J * (J + 1) * (J + 2) // 3


def pair_index(j1: int, j2: int) -> int:
    """p3 of C3[j1, j2], 1 <= j1 <= j2."""
    return j2 * (j2 - 1) // 2 + (j1 - 1)


def triple_index(j1: int, j1p: int, j2: int) -> int:
    """p4 of C4[j1, j1', j2], 1 <= j1 <= j1' <= j2."""
    return (j2 - 1) * j2 * (j2 + 1) // 6 + j1p * (j1p - 1) // 2 + (j1 - 1)


def _check_n_J(n: int, J) -> int:
    if n < 8:
        raise ValueError(f"rows must hold at least 8 samples, got n = {n}")
    if n & (n - 1):
        raise ValueError(f"rows must hold a power of two of samples, got n = {n}: slice the ensemble, e.g. "
                         f"x[..., :{1 << (n.bit_length() - 1)}] (a view, read in place)")
    top = n.bit_length() - 3                         # log2(n) - 2
    if J is None:
        return min(top, DEFAULT_MAX_J)
    if isinstance(J, bool) or int(J) != J or not 1 <= J <= top:
        raise ValueError(f"J must be an integer with 1 <= J <= log2(n) - 2 = {top}, got {J!r}")
    return int(J)


def scattering_bank(n: int, J: int) -> np.ndarray:
    """(J, n / 2) float64: psi_hat[j][k] = cos(pi/2 log2(k / k_j)), k_j = n / 2^(j+1), inside n / 2^(j+2) < k < n / 2^j and 0
    outside; row j - 1 is scale j."""
    n = int(n)
    J = _check_n_J(n, J)
    k = np.arange(n // 2)
    bank = np.zeros((J, n // 2))
    for j in range(1, J + 1):
        band = (k > (n >> (j + 2))) & (k < (n >> j))
        bank[j - 1, band] = np.cos(0.5 * np.pi * np.log2(k[band] / float(n >> (j + 1))))
    return bank


_device_banks: dict = {}


def _device_bank(n: int, J: int, dev):
    """The stock bank on `dev`, computed on the host once per (n, J, device)."""
    import torch
    key = (n, J, str(dev))
    if key not in _device_banks:
        _device_banks[key] = torch.from_numpy(scattering_bank(n, J)).to(dev)
    return _device_banks[key]


def _row_values(x: np.ndarray, bank: np.ndarray) -> np.ndarray:
    """(r, NOUT) float64: S1, S2, C3, C4 of each row of x (r, n) float64 by the time-domain sums of the definition."""
    r, n = x.shape
    J = bank.shape[0]
    P3, P4 = J * (J + 1) // 2, J * (J + 1) * (J + 2) // 6
    psi = np.zeros((J, n))
    psi[:, :n // 2] = bank
    W = np.fft.ifft(np.fft.fft(x, axis=-1)[:, None, :] * psi, axis=-1)         # (r, J, n)
    U = np.abs(W)
    FU = np.fft.fft(U, axis=-1)
    out = np.zeros((r, 2 * J + 2 * P3 + 2 * P4))
    out[:, :J] = U.mean(axis=-1)
    out[:, J:2 * J] = (U * U).mean(axis=-1)
    c3 = out[:, 2 * J:2 * J + 2 * P3]
    c4 = out[:, 2 * J + 2 * P3:]
    for j2 in range(1, J + 1):
        V = np.fft.ifft(FU[:, :j2, :] * psi[j2 - 1], axis=-1)                  # (r, j1 = 1 .. j2, n)
        a3 = (W[:, j2 - 1, None, :] * np.conj(V)).mean(axis=-1)                # (r, j1)
        a4 = np.einsum("rat,rbt->rab", V, np.conj(V)) / n                      # (r, j1, j1')
        for j1 in range(1, j2 + 1):
            p3 = pair_index(j1, j2)
            c3[:, p3], c3[:, P3 + p3] = a3[:, j1 - 1].real, a3[:, j1 - 1].imag
            for j1p in range(j1, j2 + 1):
                p4 = triple_index(j1, j1p, j2)
                c4[:, p4] = a4[:, j1 - 1, j1p - 1].real
                c4[:, P4 + p4] = a4[:, j1 - 1, j1p - 1].imag if j1p > j1 else 0.0
    return out


def _host_sums(X: np.ndarray, bank: np.ndarray, G: int):
    """The numpy twin of psh_scattering_spectra on (R, n) float32: (sums (G, NOUT) float64, rows_used (G,) int64)."""
    R, n = X.shape
    J = bank.shape[0]
    ok = np.isfinite(X).all(axis=1)
    vals = np.zeros((R, n_outputs(J)))                                         # an excluded row adds zeros
    live = np.flatnonzero(ok)
    step = max(1, _TWIN_BYTES // (16 * n * max(J * (J + 1) // 2, 1)))
    for i in range(0, live.size, step):
        rows = live[i:i + step]
        vals[rows] = _row_values(X[rows].astype(np.float64), bank)
    starts = group_bounds(R, G)[:-1]
    return np.add.reduceat(vals, starts, axis=0), np.add.reduceat(ok.astype(np.int64), starts)


def _unpack(v: np.ndarray, J: int):
    """(..., NOUT) -> S1 (..., J), S2 (..., J), C3 (..., J, J) complex, C4 (..., J, J, J) complex, NaN off the index sets."""
    P3, P4 = J * (J + 1) // 2, J * (J + 1) * (J + 2) // 6
    lead = v.shape[:-1]
    c3 = np.full(lead + (J, J), np.nan + 1j * np.nan)
    c4 = np.full(lead + (J, J, J), np.nan + 1j * np.nan)
    o3, o4 = 2 * J, 2 * J + 2 * P3
    for j2 in range(1, J + 1):
        for j1 in range(1, j2 + 1):
            p3 = pair_index(j1, j2)
            c3[..., j1 - 1, j2 - 1] = v[..., o3 + p3] + 1j * v[..., o3 + P3 + p3]
            for j1p in range(j1, j2 + 1):
                p4 = triple_index(j1, j1p, j2)
                c4[..., j1 - 1, j1p - 1, j2 - 1] = v[..., o4 + p4] + 1j * v[..., o4 + P4 + p4]
    return v[..., :J], v[..., J:2 * J], c3, c4


def _summarise(sums: np.ndarray, rows: np.ndarray, R: int, n: int, J: int) -> ScatteringSpectra:
    used = int(rows.sum())
    live = rows > 0

    def normalise(v, sigma2):
        s1, s2, c3, c4 = _unpack(v, J)
        root = np.sqrt(sigma2)
        return (s1 / root, s2, c3 / (root[:, None] * root[None, :]),
                c4 / (root[:, None, None] * root[None, :, None]))

    with np.errstate(invalid="ignore", divide="ignore"):
        mean = sums.sum(axis=0) / used                                          # 0 / 0 = NaN with no row left
        sigma2 = mean[J:2 * J]
        phi = normalise(mean, sigma2)
        if int(live.sum()) >= 2:
            grp = normalise(sums[live] / rows[live, None], sigma2)
            wgt = rows[live] / float(used)
            se = tuple(np.sqrt(np.tensordot(wgt, np.abs(gv - pv) ** 2, axes=1) / (int(live.sum()) - 1))
                       for gv, pv in zip(grp, phi))
        else:
            se = tuple(np.full(pv.shape, np.nan) for pv in phi)
    return ScatteringSpectra(n=n, J=J, phi1=phi[0], phi2=phi[1], phi3=phi[2], phi4=phi[3], phi1_se=se[0], phi2_se=se[1],
                             phi3_se=se[2], phi4_se=se[3], rows_used=used, rows_excluded=R - used, group_sums=sums,
                             group_rows=rows)


def scattering_spectra(x, J: int | None = None, groups: int | None = None, cuda: bool | None = None,
                       bank=None) -> ScatteringSpectra:
    """The scattering spectra of an ensemble x, (n,), (R, n) or (R, 1, n), numpy or torch, n a power of two >= 8 (a longer
    or odd-length ensemble is sliced by the caller: x[..., :4096] is a view and is read in place), at J scales (default
    min(log2(n) - 2, 9)), with standard errors from `groups` row groups (default min(R, 64)).  bank: (J, n / 2) Fourier
    multipliers of the caller's own analytic wavelets, zero outside n / 2^(j+2) < k < n / 2^j (default: scattering_bank).
    cuda=None: psh_scattering_spectra when x is a HIP float32 tensor (read in place; n <= 4096), the numpy twin otherwise;
    cuda=True: the device (x is rounded to float32 and uploaded if it is not there; no host fallback); cuda=False: the
    twin."""
    on_device = _is_torch(x) and x.is_cuda
    if not _is_torch(x):
        x = np.asarray(x)
    if x.ndim == 1:
        x = x[None, :]
    elif x.ndim == 3 and x.shape[1] == 1:
        x = x[:, 0, :]
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"x must be (n,), (R, n) or (R, 1, n) and not empty, got shape {tuple(x.shape)}")
    R, n = int(x.shape[0]), int(x.shape[1])
    J = _check_n_J(n, J)
    G = min(R, DEFAULT_GROUPS) if groups is None else groups
    if isinstance(G, bool) or int(G) != G or not 1 <= G <= R:
        raise ValueError(f"groups must be an integer with 1 <= groups <= R = {R}, got {groups!r}")
    G = int(G)
    if bank is not None:
        host_bank = bank.detach().cpu().numpy() if _is_torch(bank) else np.asarray(bank)
        if host_bank.shape != (J, n // 2) or not np.isrealobj(host_bank):
            raise ValueError(f"bank must be real and ({J}, {n // 2}), got shape {tuple(host_bank.shape)}")
        host_bank = np.ascontiguousarray(host_bank, dtype=np.float64)
    if cuda is None:
        cuda = bool(on_device and str(x.dtype) == "torch.float32")
    if cuda:
        import torch
        from . import _native
        if not on_device:
            if not torch.cuda.is_available():
                raise _native.NativeLibraryError("cuda=True needs a HIP device, and there is no host fallback under it")
            x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32) if not _is_torch(x) else x).to("cuda")
        if x.dtype != torch.float32:
            x = x.to(torch.float32)
        if n > MAX_N_DEVICE:
            raise ValueError(f"cuda=True takes rows of n <= {MAX_N_DEVICE} samples (got {n}): the transforms of a longer row "
                             f"leave LDS; slice the ensemble, e.g. x[..., :{MAX_N_DEVICE}], or use cuda=False")
        psi = _device_bank(n, J, x.device) if bank is None else torch.from_numpy(host_bank).to(x.device)
        sums, rows, _ = _native.scattering_spectra(x, J, G, psi)
        return _summarise(sums.cpu().numpy(), rows.cpu().numpy(), R, n, J)
    X = x.detach().cpu().numpy() if _is_torch(x) else x
    sums, rows = _host_sums(np.ascontiguousarray(X, dtype=np.float32), scattering_bank(n, J) if bank is None else host_bank, G)
    return _summarise(sums, rows, R, n, J)


def _torch_row_values(x, psi):
    """(r, NOUT) float64 torch: _row_values in torch ops (x (r, n) float64, psi (J, n) float64 padded with zeros), so that
    autograd differentiates the time-domain definition.  torch's abs has the gradient sgn: 0 where W_j(t) = 0."""
    import torch
    n = x.shape[-1]
    J = psi.shape[0]
    W = torch.fft.ifft(torch.fft.fft(x, dim=-1)[:, None, :] * psi, dim=-1)     # (r, J, n)
    U = W.abs()
    FU = torch.fft.fft(U, dim=-1)
    c3, c4 = [], []
    for j2 in range(1, J + 1):
        V = torch.fft.ifft(FU[:, :j2, :] * psi[j2 - 1], dim=-1)                # (r, j1 = 1 .. j2, n)
        c3.append((W[:, j2 - 1, None, :] * V.conj()).mean(dim=-1))             # (r, j1): p3 runs on with j2, then j1
        a4 = torch.einsum("rat,rbt->rab", V, V.conj()) / n                     # (r, j1, j1')
        c4.extend(a4[:, :j1p, j1p - 1] for j1p in range(1, j2 + 1))            # p4 runs on with j2, j1', then j1
    c3, c4 = torch.cat(c3, dim=1), torch.cat(c4, dim=1)
    real4 = torch.tensor([0.0 if j1 == j1p else 1.0 for j2 in range(1, J + 1) for j1p in range(1, j2 + 1)
                          for j1 in range(1, j1p + 1)], dtype=x.dtype, device=x.device)       # Im C4[j1, j1, j2] = 0
    return torch.cat([U.mean(dim=-1), (U * U).mean(dim=-1), c3.real, c3.imag, c4.real, c4.imag * real4], dim=1)


def _torch_sums(x, bank, G: int):
    """The torch float64 twin of psh_scattering_spectra on (R, n), differentiable in x: (sums (G, NOUT), rows (G,) int64)."""
    import torch
    R, n = x.shape
    x = x.to(torch.float64)
    x = x + (x.to(torch.float32).to(torch.float64) - x).detach()               # the kernels read float32 (the gradient stays float64)
    psi = torch.zeros((bank.shape[0], n), dtype=torch.float64, device=x.device)
    psi[:, :n // 2] = torch.as_tensor(bank, dtype=torch.float64, device=x.device)
    ok = torch.isfinite(x).all(dim=1)
    vals = _torch_row_values(torch.where(ok[:, None], x, torch.zeros((), dtype=x.dtype, device=x.device)), psi) * ok[:, None]
    bounds = group_bounds(R, G)
    group = torch.as_tensor(np.repeat(np.arange(G), np.diff(bounds)), device=x.device)
    sums = torch.zeros((G, vals.shape[1]), dtype=torch.float64, device=x.device).index_add(0, group, vals)
    rows = torch.zeros((G,), dtype=torch.int64, device=x.device).index_add(0, group, ok.to(torch.int64))
    return sums, rows


_DeviceSums = None


def _device_sums_function():
    """The torch.autograd.Function over psh_scattering_spectra and psh_scattering_vjp (made on first use: torch is imported
    lazily here)."""
    global _DeviceSums
    if _DeviceSums is None:
        import torch
        from . import _native

        class DeviceSums(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, J, G, psi):
                sums, rows, _ = _native.scattering_spectra(x, J, G, psi)
                ctx.save_for_backward(x, psi)
                ctx.J, ctx.G = J, G
                ctx.mark_non_differentiable(rows)
                return sums, rows

            @staticmethod
            def backward(ctx, cot, _rows):
                x, psi = ctx.saved_tensors
                grad, _ = _native.scattering_vjp(x, ctx.J, ctx.G, psi, cot.to(torch.float64).contiguous())
                return grad.to(torch.float32), None, None, None

        _DeviceSums = DeviceSums
    return _DeviceSums


def scattering_sums(x, J: int | None = None, groups: int | None = None, bank=None):
    """(sums (G, NOUT) float64, rows (G,) int64) of a torch ensemble x, (R, n) or (R, 1, n): the group sums
    scattering_spectra summarises (ScatteringSpectra.group_sums, .group_rows), as torch tensors where x lies and
    differentiable in x.  On a HIP tensor: psh_scattering_spectra forward, psh_scattering_vjp backward (x is rounded to
    float32 if it is not float32; the gradient is float32; n <= 4096; no host fallback).  On a CPU tensor: the torch float64
    twin on float32-rounded rows.  J, groups and bank as scattering_spectra."""
    import torch
    if not _is_torch(x):
        raise TypeError(f"x must be a torch tensor, got {type(x).__name__}")
    if x.ndim == 3 and x.shape[1] == 1:
        x = x[:, 0, :]
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"x must be (R, n) or (R, 1, n) and not empty, got shape {tuple(x.shape)}")
    R, n = int(x.shape[0]), int(x.shape[1])
    J = _check_n_J(n, J)
    G = min(R, DEFAULT_GROUPS) if groups is None else groups
    if isinstance(G, bool) or int(G) != G or not 1 <= G <= R:
        raise ValueError(f"groups must be an integer with 1 <= groups <= R = {R}, got {groups!r}")
    G = int(G)
    if bank is None:
        host_bank = None
    else:
        host_bank = bank.detach().cpu().numpy() if _is_torch(bank) else np.asarray(bank)
        if host_bank.shape != (J, n // 2) or not np.isrealobj(host_bank):
            raise ValueError(f"bank must be real and ({J}, {n // 2}), got shape {tuple(host_bank.shape)}")
        host_bank = np.ascontiguousarray(host_bank, dtype=np.float64)
    if x.is_cuda:
        if n > MAX_N_DEVICE:
            raise ValueError(f"cuda=True takes rows of n <= {MAX_N_DEVICE} samples (got {n}): the transforms of a longer row "
                             f"leave LDS; slice the ensemble, e.g. x[..., :{MAX_N_DEVICE}], or use cuda=False")
        if x.dtype != torch.float32:
            x = x.to(torch.float32)
        psi = _device_bank(n, J, x.device) if host_bank is None else torch.from_numpy(host_bank).to(x.device)
        return _device_sums_function().apply(x, J, G, psi)
    return _torch_sums(x, scattering_bank(n, J) if host_bank is None else host_bank, G)


def _normalisers(J: int, sigma2: np.ndarray) -> np.ndarray:
    """(NOUT,) the factors s_o that turn S1, S2, C3, C4 into phi1 .. phi4 at a fixed sigma2 (phi2 relative to sigma2)."""
    root = np.sqrt(sigma2)
    P3, P4 = J * (J + 1) // 2, J * (J + 1) * (J + 2) // 6
    s3, s4 = np.empty(P3), np.empty(P4)
    for j2 in range(1, J + 1):
        for j1 in range(1, j2 + 1):
            s3[pair_index(j1, j2)] = 1.0 / (root[j1 - 1] * root[j2 - 1])
            for j1p in range(j1, j2 + 1):
                s4[triple_index(j1, j1p, j2)] = 1.0 / (root[j1 - 1] * root[j1p - 1])
    return np.concatenate([1.0 / root, 1.0 / sigma2, s3, s3, s4, s4])


def _loss_terms(target: ScatteringSpectra):
    """(T (NOUT,), s (NOUT,)) float64 numpy: the target's per-row means and the normalisers frozen at its sigma2."""
    if not isinstance(target, ScatteringSpectra):
        raise TypeError(f"target must be a ScatteringSpectra, got {type(target).__name__}")
    if target.rows_used < 1:
        raise ValueError("the target has no rows: every row it was measured on held a NaN or an inf")
    T = target.group_sums.sum(axis=0) / float(target.rows_used)
    sigma2 = T[target.J:2 * target.J]
    if not (np.all(np.isfinite(sigma2)) and np.all(sigma2 > 0)):
        raise ValueError("the target has no power at some scale (sigma2 = 0 or not finite): nothing to normalise with")
    return T, _normalisers(target.J, sigma2)


def _loss(sums, rows, T, s):
    m = sums.sum(dim=0) / rows.sum()
    return ((s * (m - T)) ** 2).mean()


def scattering_loss(sums, rows, target: ScatteringSpectra):
    """The squared distance of a batch to a target, a 0-dim float64 torch tensor, differentiable in sums:
        loss = (1 / NOUT) sum_o (s_o (m_o - T_o))^2,   m = sums.sum(0) / rows.sum(),   T = the target's per-row means,
    with s_o the normalisations of phi1 .. phi4 frozen at the target's sigma2 = T[S2]: 1 / sqrt(sigma2[j]) for S1,
    1 / sigma2[j] for S2, 1 / sqrt(sigma2[j1] sigma2[j2]) for both parts of C3 and 1 / sqrt(sigma2[j1] sigma2[j1']) for both
    parts of C4.  sums, rows: scattering_sums' (the target's J).  The loss is quadratic in the sums."""
    import torch
    T, s = _loss_terms(target)
    if tuple(sums.shape[1:]) != (T.size,):
        raise ValueError(f"sums must be (G, {T.size}) for the target's J = {target.J}, got shape {tuple(sums.shape)}")
    return _loss(sums, rows, torch.as_tensor(T, device=sums.device), torch.as_tensor(s, device=sums.device))


def start_variance(target: ScatteringSpectra) -> float:
    """The variance of the white noise a generation starts from: sum_j phi2[j] / sum_{j,k} (psi_hat[j][k]^2 / n), the level
    at which white noise has the target's total wavelet power (E S2[j] = variance sum_k psi_hat[j][k]^2 / n)."""
    bank = scattering_bank(target.n, target.J)
    return float(np.sum(target.phi2) / (np.sum(bank * bank) / target.n))


class _Stop(Exception):
    pass


def scattering_generate(target, R: int, batch: int = 256, max_eval: int = 200, tol: float = 1e-3, seed: int = 0,
                        cuda: bool | None = None, return_info: bool = False):
    """(R, 1, n) float32 log-returns that carry the scattering spectra of `target`: a ScatteringSpectra (n and J are its own;
    the stock wavelets), or data that scattering_spectra measures first.  A torch tensor, on the HIP device under cuda=True
    (cuda=None: when one is present; rows of n <= 4096, no host fallback), the layout PathShadowing takes as `dataset`.

    Each batch of `batch` rows is its own problem.  Start: torch.randn from a CPU generator seeded with (seed, batch index),
    scaled to start_variance(target).  Descent: torch.optim.LBFGS (strong_wolfe, history 20) on a float64 master copy that
    is rounded to float32 at every evaluation, because the kernels read float32, on scattering_loss of the batch with
    one group per row.  Stop: sqrt(loss) <= tol, or max_eval evaluations; the rows returned are the float32 rows of the
    evaluation with the smallest loss.  return_info=True returns (rows, info) with info["initial_loss"], ["final_loss"]
    and ["evaluations"], one entry per batch."""
    import torch
    if not isinstance(target, ScatteringSpectra):
        target = scattering_spectra(target, cuda=cuda)
    for name, v in (("R", R), ("batch", batch), ("max_eval", max_eval)):
        if isinstance(v, bool) or int(v) != v or v < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    R, batch, max_eval, n = int(R), int(batch), int(max_eval), int(target.n)
    J = _check_n_J(n, target.J)
    T_host, s_host = _loss_terms(target)
    if cuda is None:
        cuda = torch.cuda.is_available()
    if cuda:
        from . import _native
        if not torch.cuda.is_available():
            raise _native.NativeLibraryError("cuda=True needs a HIP device, and there is no host fallback under it")
        if n > MAX_N_DEVICE:
            raise ValueError(f"cuda=True takes rows of n <= {MAX_N_DEVICE} samples (got {n}): the transforms of a longer row "
                             f"leave LDS; slice the ensemble, e.g. x[..., :{MAX_N_DEVICE}], or use cuda=False")
    dev = torch.device("cuda" if cuda else "cpu")
    T, s = torch.as_tensor(T_host, device=dev), torch.as_tensor(s_host, device=dev)
    std = float(np.sqrt(start_variance(target)))
    out = torch.empty((R, 1, n), dtype=torch.float32, device=dev)
    info = {"initial_loss": [], "final_loss": [], "evaluations": []}
    for b, r0 in enumerate(range(0, R, batch)):
        rows = min(batch, R - r0)
        gen = torch.Generator().manual_seed(int(np.random.SeedSequence([int(seed), b]).generate_state(2, np.uint32)
                                                .view(np.uint64)[0] >> 1))
        master = (torch.randn((rows, n), generator=gen, dtype=torch.float64) * std).to(dev).requires_grad_(True)
        opt = torch.optim.LBFGS([master], lr=1.0, max_iter=max_eval, max_eval=max_eval, history_size=20,
                                tolerance_grad=0.0, tolerance_change=0.0, line_search_fn="strong_wolfe")
        state = {"evals": 0, "first": None, "best": float("inf"), "rows": None}

        def closure():
            opt.zero_grad()
            x32 = master.to(torch.float32)
            sums, used = scattering_sums(x32 if cuda else x32.to(torch.float64), J, groups=rows)
            loss = _loss(sums, used, T, s)
            loss.backward()
            value = float(loss.detach())
            state["evals"] += 1
            if state["first"] is None:
                state["first"] = value
            if value < state["best"]:
                state["best"], state["rows"] = value, x32.detach().clone()
            if not np.isfinite(value) or np.sqrt(value) <= tol or state["evals"] >= max_eval:
                raise _Stop
            return loss

        try:
            while state["evals"] < max_eval:
                before = state["evals"]
                opt.step(closure)
                if state["evals"] == before:
                    break
        except _Stop:
            pass
        out[r0:r0 + rows, 0, :] = state["rows"]
        info["initial_loss"].append(state["first"])
        info["final_loss"].append(state["best"])
        info["evaluations"].append(state["evals"])
    return (out, info) if return_info else out


__all__ = ["ScatteringSpectra", "scattering_spectra", "scattering_bank", "scattering_sums", "scattering_loss",
           "scattering_generate"]
