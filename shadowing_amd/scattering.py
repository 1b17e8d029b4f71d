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


__all__ = ["ScatteringSpectra", "scattering_spectra", "scattering_bank"]
