"""The shadowing ensemble made here: log-normal multifractal random walks (Bacry, Delour, Muzy 2001, "Multifractal random
walk", Phys. Rev. E 64), the generated dataset of the tutorial's first cell.  The reference takes `MRWGenerator` from
scatspectra; this module is the project's own statement of the model, with that class's name and call
(`MRWGenerator(T, H, lam, cache_path=).load(R=)`), and parity with scatspectra is not pinned, as for pricing.PriceData.

The model at unit step, n returns per path (the method, in full, heads shadowing_amd/csrc/psh_mrw.hip):
    r[t] = sigma * eps[t] * exp(omega[t] - c[0]),   lnx[0] = 0, lnx[t+1] = lnx[t] + r[t],
    omega Gaussian, Cov(omega[s], omega[t]) = c[|s-t|], c[j] = lam^2 max(ln(L / (j + 1)), 0), L the integral scale (default n),
    eps unit-variance fractional Gaussian noise of Hurst exponent H (white noise for H = 0.5), independent of omega,
so E[r^2] = sigma^2.  Both Gaussian sequences are made exactly by circulant embedding of size M, the smallest power of
two >= 2n, one complex transform giving two paths, on counter-based Philox draws: a path's samples depend only on
(seed, path, n, parameters).  `cuda=False` is the numpy float64 twin (np.fft.fft on the same draws); `cuda=True` runs
psh_mrw_generate, which keeps the transform in LDS and therefore takes n <= 4096.

The skewed MRW (Pochart, Bouchaud 2002; smrw_log_returns, SMRWGenerator, smrw_leverage) adds the leverage effect: the
log-volatility becomes omega[t] - sum_{j=1..m} K0 / j^alpha eps[t-j] at white noise, which makes E[r_t r_{t+tau}^2]
negative and the smile skewed.  Its statement heads shadowing_amd/csrc/psh_smrw.hip; `cuda=True` runs psh_smrw_generate.
smrw_sq_moment is E[r_t^2 r_{t+tau}^2] in closed form; stylized.fit_smrw fits both closed forms to a measured ensemble.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from .pdv import _LO32, _SH32, _check_seed, normal_pairs

MAX_N_DEVICE = 4096                                  # PSH_MRW_MAX_N: M = 8192 complex doubles fill the LDS of one CU
DEFAULT_SIGMA = 0.2 / math.sqrt(252.0)               # the daily volatility synthetic.py uses
STREAM_OMEGA, STREAM_FGN, STREAM_WHITE = 0, 1, 2     # the second counter word of the draws (psh_mrw.hip)
STREAM_PAST = 3                                      # ... of the skewed MRW's pre-history (psh_smrw.hip)


def _embedding_size(n: int) -> int:
    M = 4
    while M < 2 * n:
        M *= 2
    return M


def _check_n(n) -> int:
    if isinstance(n, bool) or int(n) != n or n < 2:
        raise ValueError(f"a path needs n >= 2 returns (an integer), got {n!r}")
    return int(n)


def _spectrum(c_half: np.ndarray, M: int, what: str) -> np.ndarray:
    """Eigenvalues s[k] = sum_j chat[j] cos(2 pi j k / M) of the circulant matrix of the even extension of c[0 .. M/2]."""
    chat = np.concatenate([c_half, c_half[-2:0:-1]])
    assert chat.size == M
    s = np.fft.fft(chat).real
    if s.min() < -1e-9 * s.max():
        raise ValueError(f"the circulant embedding of {what} is not non-negative definite (min eigenvalue {s.min():.3e}, "
                         f"max {s.max():.3e}): these parameters are outside what the generator accepts")
    return s


def mrw_covariance(j, L: float, lam: float) -> np.ndarray:
    """c[j] = lam^2 max(ln(L / (j + 1)), 0): the covariance of omega at lag j."""
    return lam * lam * np.maximum(np.log(L / (np.asarray(j, dtype=np.float64) + 1.0)), 0.0)


def fgn_covariance(j, H: float) -> np.ndarray:
    """(|j+1|^2H - 2 |j|^2H + |j-1|^2H) / 2: the covariance of unit fractional Gaussian noise at lag j."""
    j = np.asarray(j, dtype=np.float64)
    return 0.5 * (np.abs(j + 1.0) ** (2 * H) - 2.0 * np.abs(j) ** (2 * H) + np.abs(j - 1.0) ** (2 * H))


def _check_params(n, H, lam, L, sigma):
    n = _check_n(n)
    L = float(n if L is None else L)
    H, lam, sigma = float(H), float(lam), float(sigma)
    if not (math.isfinite(H) and 0.0 < H < 1.0):
        raise ValueError(f"H must lie in (0, 1), got {H}")
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"lam must be finite and >= 0, got {lam}")
    if not (math.isfinite(L) and L >= 1.0):
        raise ValueError(f"the integral scale L must be finite and >= 1, got {L}")
    if not (math.isfinite(sigma) and sigma >= 0.0):
        raise ValueError(f"sigma must be finite and >= 0, got {sigma}")
    return n, H, lam, L, sigma


@functools.lru_cache(maxsize=32)
def _mrw_spectrum(n: int, L: float, lam: float):
    M = _embedding_size(n)
    s = _spectrum(mrw_covariance(np.arange(M // 2 + 1), L, lam), M, f"omega (n={n}, L={L}, lam={lam})")
    s.setflags(write=False)
    return s, M


@functools.lru_cache(maxsize=32)
def _fgn_spectrum(n: int, H: float):
    M = _embedding_size(n)
    s = _spectrum(fgn_covariance(np.arange(M // 2 + 1), H), M, f"fractional Gaussian noise (n={n}, H={H})")
    s.setflags(write=False)
    return s, M


def mrw_spectrum(n: int, L: float | None = None, lam: float = 0.2):
    """(s, M): the M eigenvalues of the circulant embedding of omega's covariance for paths of n returns.  Raises
    ValueError when min s < -1e-9 max s (the embedding would not be exact)."""
    n, _, lam, L, _ = _check_params(n, 0.5, lam, L, 0.0)
    return _mrw_spectrum(n, L, lam)


def fgn_spectrum(n: int, H: float):
    """(s, M): the same for unit fractional Gaussian noise of Hurst exponent H."""
    n, H, _, _, _ = _check_params(n, H, 0.0, None, 0.0)
    return _fgn_spectrum(n, H)


def _table(s: np.ndarray, M: int) -> np.ndarray:
    """a[k] = sqrt(max(s[k], 0) / M): what the kernel and the twin multiply the draws by."""
    return np.sqrt(np.maximum(s, 0.0) / M)


def _gaussian_pairs(key, pairs: np.ndarray, a: np.ndarray, stream: int, n: int) -> np.ndarray:
    """(len(pairs), M) complex Y = FFT_M(a * Z), cut to its first n samples: Z[k] the Box-Muller pair of counter
    (k, stream, pair lo, pair hi)."""
    q = pairs.astype(np.uint64)[:, None]
    k = np.arange(a.size, dtype=np.uint64)[None, :]
    z0, z1 = normal_pairs((k, np.uint64(stream), q & _LO32, q >> _SH32), key)
    return np.fft.fft(a[None, :] * (z0 + 1j * z1), axis=-1)[:, :n]


def _interleave(Y: np.ndarray) -> np.ndarray:
    """(P, n) complex -> (2P, n) real: path 2q is Re Y[q], path 2q + 1 is Im Y[q]."""
    out = np.empty((2 * Y.shape[0], Y.shape[1]))
    out[0::2], out[1::2] = Y.real, Y.imag
    return out


def _white_noise(key, g: np.ndarray, stream: int, n: int) -> np.ndarray:
    """(len(g), n) independent unit Gaussians: samples 2i and 2i + 1 of path g are the Box-Muller pair of counter
    (i, stream, g lo, g hi)."""
    gg = g.astype(np.uint64)[:, None]
    i = np.arange((n + 1) // 2, dtype=np.uint64)[None, :]
    eps = np.empty((g.size, 2 * i.shape[1]))
    eps[:, 0::2], eps[:, 1::2] = normal_pairs((i, np.uint64(stream), gg & _LO32, gg >> _SH32), key)
    return eps[:, :n]


def _host(R: int, n: int, H: float, lam: float, L: float, sigma: float, seed: int, first_path: int = 0):
    """The numpy twin of psh_mrw_generate: (r, omega), both (R, n) float64, of paths first_path .. first_path + R - 1."""
    key = (seed & 0xFFFFFFFF, seed >> 32)
    s, M = _mrw_spectrum(n, L, lam)
    a_om = _table(s, M)
    a_eps = None if H == 0.5 else _table(*_fgn_spectrum(n, H))
    c0 = float(mrw_covariance(0, L, lam))
    r = np.empty((R, n))
    omega = np.empty((R, n))
    q_first, q_last = first_path // 2, (first_path + R - 1) // 2
    rows = max(1, (1 << 19) // M)                                        # pairs per chunk: bounded temporaries
    for q0 in range(q_first, q_last + 1, rows):
        pairs = np.arange(q0, min(q0 + rows, q_last + 1))
        g = np.arange(2 * pairs[0], 2 * pairs[-1] + 2)                   # the paths of these pairs
        om = _interleave(_gaussian_pairs(key, pairs, a_om, STREAM_OMEGA, n))
        if a_eps is None:
            eps = _white_noise(key, g, STREAM_WHITE, n)
        else:
            eps = _interleave(_gaussian_pairs(key, pairs, a_eps, STREAM_FGN, n))
        keep = (g >= first_path) & (g < first_path + R)
        omega[g[keep] - first_path] = om[keep]
        r[g[keep] - first_path] = ((sigma * eps) * np.exp(om - c0))[keep]
    return r, omega


def _device_tables(n: int, H: float, lam: float, L: float, dev):
    import torch
    a_om = torch.from_numpy(_table(*_mrw_spectrum(n, L, lam))).to(dev)
    a_eps = None if H == 0.5 else torch.from_numpy(_table(*_fgn_spectrum(n, H))).to(dev)
    return a_om, a_eps


def _device(R: int, n: int, H: float, lam: float, L: float, sigma: float, seed: int, outputs):
    """psh_mrw_generate on the current HIP device: the requested outputs as device tensors."""
    import torch
    from . import _native
    if n > MAX_N_DEVICE:
        raise ValueError(f"cuda=True makes paths of n <= {MAX_N_DEVICE} returns (got {n}): the transform of a longer path "
                         "leaves LDS, and there is no host fallback under cuda=True")
    dev = torch.device("cuda", torch.cuda.current_device())
    a_om, a_eps = _device_tables(n, H, lam, L, dev)
    return _native.mrw_generate(R, n, sigma, a_om, a_eps, float(mrw_covariance(0, L, lam)), seed=seed, outputs=outputs)


def _seed_or_draw(seed) -> int:
    if seed is None:
        return int.from_bytes(np.random.bytes(8), "little")             # numpy's global stream picks the key
    return _check_seed(seed)


def mrw_log_returns(R: int, n: int, H: float = 0.5, lam: float = 0.2, L: float | None = None,
                    sigma: float = DEFAULT_SIGMA, seed: int | None = None, cuda: bool = False, return_omega: bool = False):
    """(R, 1, n) float32 log-returns of R multifractal random walks: the layout PathShadowing takes as `dataset`.  A numpy
    array (cuda=False, the float64 twin rounded once) or a HIP tensor written by psh_mrw_generate (cuda=True, n <= 4096;
    no host copy, no host fallback).  seed=None takes a seed from numpy's global stream.  return_omega=True returns
    (returns, omega) with omega (R, n) float64, the log-volatility."""
    n, H, lam, L, sigma = _check_params(n, H, lam, L, sigma)
    if isinstance(R, bool) or int(R) != R or R < 1:
        raise ValueError(f"R must be a positive integer, got {R!r}")
    R, seed = int(R), _seed_or_draw(seed)
    if cuda:
        out = _device(R, n, H, lam, L, sigma, seed, ("dlnx", "omega") if return_omega else ("dlnx",))
        return (out["dlnx"], out["omega"]) if return_omega else out["dlnx"]
    r, omega = _host(R, n, H, lam, L, sigma, seed)
    dlnx = r.astype(np.float32)[:, None, :]
    return (dlnx, omega) if return_omega else dlnx


class MRWGenerator:
    """Log-prices of multifractal random walks: `MRWGenerator(T=4097, H=0.5, lam=0.2).load(R=B)` is (B, 1, T) float64,
    each path starting at 0, so the tutorial's two lines run as written.  T counts log-prices: a path has n = T - 1
    returns.  `cache_path` is accepted for the tutorial's call and ignored: paths are regenerated from the seed, which
    takes less time than reading them back."""

    def __init__(self, T: int, H: float = 0.5, lam: float = 0.2, L: float | None = None, sigma: float = DEFAULT_SIGMA,
                 cache_path=None):
        if isinstance(T, bool) or int(T) != T:
            raise ValueError(f"T must be an integer, got {T!r}")
        self.T = int(T)
        self.n, self.H, self.lam, self.L, self.sigma = _check_params(self.T - 1, H, lam, L, sigma)
        self.cache_path = cache_path

    def load(self, R: int, seed: int | None = None, cuda: bool = False) -> np.ndarray:
        """(R, 1, T) float64 numpy log-prices.  cuda=True generates them on the HIP device (T <= 4097) and copies them
        to the host; seed=None takes a seed from numpy's global stream."""
        if isinstance(R, bool) or int(R) != R or R < 1:
            raise ValueError(f"R must be a positive integer, got {R!r}")
        R, seed = int(R), _seed_or_draw(seed)
        if cuda:
            lnx = _device(R, self.n, self.H, self.lam, self.L, self.sigma, seed, ("lnx",))["lnx"].cpu().numpy()
        else:
            r, _ = _host(R, self.n, self.H, self.lam, self.L, self.sigma, seed)
            lnx = np.concatenate([np.zeros((R, 1)), np.cumsum(r, axis=-1)], axis=-1)
        return lnx[:, None, :]


# ---- the skewed MRW (Pochart, Bouchaud 2002): lv = omega - A, A a causal power-law kernel on past noise.  The model,
# ---- in full, heads shadowing_amd/csrc/psh_smrw.hip and README "Skewed MRW".

def smrw_kernel(m: int, K0: float, alpha: float) -> np.ndarray:
    """(m,) float64: K(j) = K0 / j^alpha, j = 1 .. m, the leverage kernel."""
    if isinstance(m, bool) or int(m) != m or m < 1:
        raise ValueError(f"the memory must be an integer >= 1, got {m!r}")
    K0, alpha = float(K0), float(alpha)
    if not (math.isfinite(K0) and math.isfinite(alpha)):
        raise ValueError(f"K0 and alpha must be finite, got {K0}, {alpha}")
    return K0 / np.arange(1, int(m) + 1, dtype=np.float64) ** alpha


def _check_smrw(n, K0, alpha, H, lam, L, memory, sigma):
    n, H, lam, L, sigma = _check_params(n, H, lam, L, sigma)
    if H != 0.5:
        raise ValueError(f"the skewed MRW takes white noise (H = 0.5), got H = {H}: with fractional noise eps[t] would "
                         "not be independent of the leverage term")
    M = _embedding_size(n)
    m = n if memory is None else memory
    if isinstance(m, bool) or int(m) != m or not 1 <= m <= M - n:
        raise ValueError(f"the memory must be an integer with 1 <= memory <= M - n = {M - n} (the convolution is linear "
                         f"inside the circulant of size M = {M}), got {m!r}")
    K = smrw_kernel(int(m), K0, alpha)
    return n, lam, L, int(m), sigma, K


def _k_hat(K: np.ndarray, M: int) -> np.ndarray:
    """(M,) complex128, the table psh_smrw_generate takes: conj(FFT_M(K))[k] exp(-2 pi i k m / M) / M with K(j) at index
    j (psh.h), so that A = FFT_M(k_hat[k] X[(-k) mod M]) for X the transform of the noise."""
    m = K.size
    pad = np.zeros(M)
    pad[1:m + 1] = K
    phase = np.exp(-2j * np.pi * ((np.arange(M) * m) % M) / M)
    return np.conj(np.fft.fft(pad)) * phase / M


def smrw_leverage(tau: int, n: int, K0: float, alpha: float, lam: float = 0.2, L: float | None = None,
                  memory: int | None = None, sigma: float = DEFAULT_SIGMA) -> float:
    """E[r_t r_{t+tau}^2] of the skewed MRW in closed form, 1 <= tau <= memory:
        -2 K(tau) sigma^3 exp(S(tau) / 2 + 2 c[tau] - c0 / 2 - 3 v),
        S(tau) = sum_{j>=1} (K(j) + 2 K(j + tau))^2 + 4 sum_{j<tau} K(j)^2 + 4 K(tau)^2
    (every exponent is Gaussian; eps[t] enters with coefficient -2 K(tau) and E[e exp(a e)] = a exp(a^2 / 2)).  What a
    measured leverage curve is fitted against to choose K0 and alpha."""
    n, lam, L, m, sigma, K = _check_smrw(n, K0, alpha, 0.5, lam, L, memory, sigma)
    if isinstance(tau, bool) or int(tau) != tau or not 1 <= tau <= m:
        raise ValueError(f"tau must be an integer with 1 <= tau <= memory = {m}, got {tau!r}")
    tau = int(tau)
    shifted = np.zeros(m)
    shifted[:m - tau] = K[tau:]                                          # K(j + tau), 0 past the memory
    S = float(np.sum((K + 2.0 * shifted) ** 2) + 4.0 * np.sum(K[:tau - 1] ** 2) + 4.0 * K[tau - 1] ** 2)
    c0, ct, v = float(mrw_covariance(0, L, lam)), float(mrw_covariance(tau, L, lam)), float(np.sum(K ** 2))
    return -2.0 * float(K[tau - 1]) * sigma ** 3 * math.exp(0.5 * S + 2.0 * ct - 0.5 * c0 - 3.0 * v)


def smrw_sq_moment(tau: int, n: int, K0: float, alpha: float, lam: float = 0.2, L: float | None = None,
                   memory: int | None = None, sigma: float = DEFAULT_SIGMA) -> float:
    """E[r_t^2 r_{t+tau}^2] of the skewed MRW in closed form, 1 <= tau (K(j) = 0 past the memory):
        sigma^4 (1 + 4 K(tau)^2) exp(4 c[tau] + 2 K(tau)^2 + 2 sum_{j>=1} (K(j) + K(j + tau))^2 + 2 sum_{j<tau} K(j)^2 - 4 v)
    (the exponent 2 lv[t] + 2 lv[t+tau] is Gaussian; eps[t] enters it with coefficient -2 K(tau) and
    E[e^2 exp(a e)] = (1 + a^2) exp(a^2 / 2); eps[t+tau] is independent of it).  sigma^4 exp(4 c[tau]) at K0 = 0: the
    volatility clustering of the MRW.  With smrw_leverage, what fit_smrw fits a measured ensemble against."""
    n, lam, L, m, sigma, K = _check_smrw(n, K0, alpha, 0.5, lam, L, memory, sigma)
    if isinstance(tau, bool) or int(tau) != tau or tau < 1:
        raise ValueError(f"tau must be an integer >= 1, got {tau!r}")
    tau = int(tau)
    shifted = np.zeros(m)
    if tau < m:
        shifted[:m - tau] = K[tau:]                                      # K(j + tau), 0 past the memory
    Kt = float(K[tau - 1]) if tau <= m else 0.0
    ct, v = float(mrw_covariance(tau, L, lam)), float(np.sum(K ** 2))
    expo = 4.0 * ct + 2.0 * Kt ** 2 + 2.0 * float(np.sum((K + shifted) ** 2)) + 2.0 * float(np.sum(K[:min(tau - 1, m)] ** 2)) - 4.0 * v
    return sigma ** 4 * (1.0 + 4.0 * Kt ** 2) * math.exp(expo)


def _smrw_host(R: int, n: int, K: np.ndarray, lam: float, L: float, sigma: float, seed: int, first_path: int = 0):
    """The numpy twin of psh_smrw_generate: (r, lv), both (R, n) float64, of paths first_path .. first_path + R - 1."""
    key = (seed & 0xFFFFFFFF, seed >> 32)
    s, M = _mrw_spectrum(n, L, lam)
    a_om = _table(s, M)
    m = K.size
    pad = np.zeros(M)
    pad[1:m + 1] = K
    Khat = np.fft.fft(pad)
    c0, v = float(mrw_covariance(0, L, lam)), float(np.sum(K ** 2))
    r = np.empty((R, n))
    lv = np.empty((R, n))
    q_first, q_last = first_path // 2, (first_path + R - 1) // 2
    rows = max(1, (1 << 19) // M)                                        # pairs per chunk: bounded temporaries
    for q0 in range(q_first, q_last + 1, rows):
        pairs = np.arange(q0, min(q0 + rows, q_last + 1))
        g = np.arange(2 * pairs[0], 2 * pairs[-1] + 2)                   # the paths of these pairs
        om = _interleave(_gaussian_pairs(key, pairs, a_om, STREAM_OMEGA, n))
        z = np.zeros((g.size, M))                                        # eps of times -m .. n - 1 at 0 .. n + m - 1
        eps = _white_noise(key, g, STREAM_WHITE, n)
        z[:, :m] = _white_noise(key, g, STREAM_PAST, m)[:, ::-1]            # sample j of that stream is eps[-1 - j]
        z[:, m:m + n] = eps
        X = np.fft.fft(z[0::2] + 1j * z[1::2], axis=-1)                  # K is real: one transform serves both paths
        A = _interleave(np.fft.ifft(X * Khat[None, :], axis=-1)[:, m:m + n])
        keep = (g >= first_path) & (g < first_path + R)
        lv[g[keep] - first_path] = (om - A)[keep]
        r[g[keep] - first_path] = ((sigma * eps) * np.exp((om - A) - c0 - v))[keep]
    return r, lv


def _smrw_device(R: int, n: int, K: np.ndarray, lam: float, L: float, sigma: float, seed: int, outputs):
    """psh_smrw_generate on the current HIP device: the requested outputs as device tensors."""
    import torch
    from . import _native
    if n > MAX_N_DEVICE:
        raise ValueError(f"cuda=True makes paths of n <= {MAX_N_DEVICE} returns (got {n}): the transform of a longer path "
                         "leaves LDS, and there is no host fallback under cuda=True")
    dev = torch.device("cuda", torch.cuda.current_device())
    a_om, _ = _device_tables(n, 0.5, lam, L, dev)
    k_hat = torch.from_numpy(_k_hat(K, _embedding_size(n))).to(dev)
    return _native.smrw_generate(R, n, K.size, sigma, a_om, k_hat, float(mrw_covariance(0, L, lam)), float(np.sum(K ** 2)),
                                 seed=seed, outputs=outputs)


def smrw_log_returns(R: int, n: int, K0: float, alpha: float, lam: float = 0.2, L: float | None = None,
                     memory: int | None = None, sigma: float = DEFAULT_SIGMA, seed: int | None = None, cuda: bool = False,
                     return_logvol: bool = False):
    """(R, 1, n) float32 log-returns of R skewed multifractal random walks, r = sigma eps exp(lv - c0 - v) with
    lv[t] = omega[t] - sum_{j=1..memory} K0 / j^alpha eps[t - j]: K0 > 0 is the leverage effect (a negative return
    raises later volatility), K0 = 0 gives the bits of mrw_log_returns on the same seed.  memory defaults to n and is at
    most M - n.  Conventions as mrw_log_returns: a numpy array (cuda=False, the float64 twin rounded once) or a HIP tensor
    written by psh_smrw_generate (cuda=True, n <= 4096; no host fallback).  return_logvol=True returns (returns, lv) with
    lv (R, n) float64."""
    n, lam, L, m, sigma, K = _check_smrw(n, K0, alpha, 0.5, lam, L, memory, sigma)
    if isinstance(R, bool) or int(R) != R or R < 1:
        raise ValueError(f"R must be a positive integer, got {R!r}")
    R, seed = int(R), _seed_or_draw(seed)
    if cuda:
        out = _smrw_device(R, n, K, lam, L, sigma, seed, ("dlnx", "logvol") if return_logvol else ("dlnx",))
        return (out["dlnx"], out["logvol"]) if return_logvol else out["dlnx"]
    r, lv = _smrw_host(R, n, K, lam, L, sigma, seed)
    dlnx = r.astype(np.float32)[:, None, :]
    return (dlnx, lv) if return_logvol else dlnx


class SMRWGenerator:
    """Log-prices of skewed multifractal random walks: `SMRWGenerator(T=4097, K0=0.1, alpha=0.6).load(R=B)` is (B, 1, T)
    float64, each path starting at 0, as MRWGenerator.  H is accepted for that class's call and must be 0.5."""

    def __init__(self, T: int, K0: float, alpha: float, H: float = 0.5, lam: float = 0.2, L: float | None = None,
                 memory: int | None = None, sigma: float = DEFAULT_SIGMA, cache_path=None):
        if isinstance(T, bool) or int(T) != T:
            raise ValueError(f"T must be an integer, got {T!r}")
        self.T, self.K0, self.alpha, self.H = int(T), float(K0), float(alpha), float(H)
        self.n, self.lam, self.L, self.memory, self.sigma, self._K = _check_smrw(self.T - 1, K0, alpha, H, lam, L, memory,
                                                                                 sigma)
        self.cache_path = cache_path

    def load(self, R: int, seed: int | None = None, cuda: bool = False) -> np.ndarray:
        """(R, 1, T) float64 numpy log-prices.  cuda=True generates them on the HIP device (T <= 4097) and copies them
        to the host; seed=None takes a seed from numpy's global stream."""
        if isinstance(R, bool) or int(R) != R or R < 1:
            raise ValueError(f"R must be a positive integer, got {R!r}")
        R, seed = int(R), _seed_or_draw(seed)
        if cuda:
            lnx = _smrw_device(R, self.n, self._K, self.lam, self.L, self.sigma, seed, ("lnx",))["lnx"].cpu().numpy()
        else:
            r, _ = _smrw_host(R, self.n, self._K, self.lam, self.L, self.sigma, seed)
            lnx = np.concatenate([np.zeros((R, 1)), np.cumsum(r, axis=-1)], axis=-1)
        return lnx[:, None, :]


__all__ = ["MRWGenerator", "mrw_log_returns", "mrw_spectrum", "fgn_spectrum", "mrw_covariance", "fgn_covariance",
           "SMRWGenerator", "smrw_log_returns", "smrw_kernel", "smrw_leverage", "smrw_sq_moment", "MAX_N_DEVICE", "DEFAULT_SIGMA"]
