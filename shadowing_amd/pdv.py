"""The path-dependent volatility (PDV) model of Guyon & Lekeufack (2024), "Volatility is (mostly) path-dependent",
Quantitative Finance 23(9): the baseline that Path Shadowing Monte Carlo's volatility predictions and smiles are compared
against.  The reference ships it as shadowing/PDV/PDV.py; this module is the project's own statement of it, with the
same public names and signatures (`shadowing.PDV.PDV` re-exports it), and it does not need scatspectra.

Deliberate deviations from the reference:
  * `windows(x, w, s, offset)` is defined here (the reference takes it from scatspectra): windows of length w, stride s,
    the first starting at `offset`, along the last axis.  Parity with scatspectra is not pinned, as for pricing.PriceData.
  * The predictor's regression is `np.linalg.lstsq` (the least-squares problem sklearn's
    LinearRegression(fit_intercept=False) solves); `.linreg.coef_` is kept.
  * `calibrate_log_returns` imports scipy lazily.  Student-t draws for `nu=` come from numpy's `standard_t`, which is
    what scipy's `t(df=nu).rvs()` calls, so that path needs no scipy.
  * `compute_factor` also accepts 3 betas.  The reference unpacks three values from the two factor columns of a 3-beta
    embedding and raises ValueError.

New here:
  * `PDVModelDiscrete.gen(..., seed=, cuda=, draws=)`: a counter-based Philox4x32-10 generator whose draws depend only
    on (seed, path, step), in numpy (`cuda=False`) and in the psh_pdv_generate kernel (`cuda=True`, which returns HIP
    tensors); `draws=` takes the raw draws instead.  The method heads shadowing_amd/csrc/psh_pdv.hip.
  * `pdv_future_paths(x_past (B, w), ...)`: (B, S, n_steps) price paths, each date from its own initial factors.
Without seed, draws and cuda, `gen` consumes numpy's global stream with the reference's calls: under np.random.seed(s)
it gives the reference's output bit for bit.
"""
from __future__ import annotations

import math
from typing import Dict, List, Literal, Tuple

import numpy as np

TWO_PI = 6.283185307179586          # the double the kernel multiplies by (== 2 * math.pi)
MAX_ATTEMPTS = 64                   # Bailey's polar method: attempts per Student-t draw (psh_pdv.hip)


def kernel_pl(taus: np.ndarray, delta: float, alpha: float) -> np.ndarray:
    """Power-law kernel (tau + delta)^-alpha; the lag delta keeps it finite at tau = 0."""
    return (taus + delta) ** (-alpha)


def kernel_exp(taus: np.ndarray, lam: float) -> np.ndarray:
    """Exponential kernel lam exp(-lam tau)."""
    return lam * np.exp(-lam * taus)


def get_RV(x: np.ndarray, from_dln: bool = False) -> np.ndarray:
    """Annualised realized volatility along the last axis of prices x (of log-returns x with from_dln=True)."""
    if from_dln:
        squares, years = (x ** 2).sum(-1), x.shape[-1] / 252
    else:
        squares, years = (np.diff(np.log(x)) ** 2).sum(-1), (x.shape[-1] - 1) / 252
    return (squares / years) ** 0.5


# the kernels' parameters fitted by Guyon & Lekeufack (2024): k1 on returns, k2 on squared returns
DEFAULT1 = {"power-law": {"delta": 0.044, "alpha": 2.82}, "exp": {"lam0": 64.5, "lam1": 3.83, "theta": 0.67}}
DEFAULT2 = {"power-law": {"delta": 0.025, "alpha": 1.86}, "exp": {"lam0": 37.6, "lam1": 1.2, "theta": 0.2}}


def windows(x, w: int, s: int, offset: int = 0) -> np.ndarray:
    """Windows of length w, stride s, the first starting at `offset`, along the last axis of x: (..., n, w) with n the
    number of whole windows.  Our own definition; the reference takes `windows` from scatspectra (parity unpinned)."""
    if w < 1 or s < 1 or offset < 0:
        raise ValueError(f"windows needs w >= 1, s >= 1, offset >= 0 (got {w}, {s}, {offset})")
    x = np.asarray(x)
    n = max((x.shape[-1] - offset - w) // s + 1, 0)
    return x[..., offset + s * np.arange(n)[:, None] + np.arange(w)[None, :]]


class LeastSquares:
    """y ~ X coef_ without an intercept, by np.linalg.lstsq: the fit of sklearn's LinearRegression(fit_intercept=False),
    with its `coef_`, `intercept_`, `fit` and `predict`."""

    def __init__(self):
        self.coef_ = None
        self.intercept_ = 0.0

    def fit(self, X: np.ndarray, y: np.ndarray) -> "LeastSquares":
        self.coef_ = np.linalg.lstsq(np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), rcond=None)[0]
        return self

    def predict(self, X: np.ndarray) -> np.ndarray:
        if self.coef_ is None:
            raise RuntimeError("LeastSquares.predict before fit")
        return np.asarray(X) @ self.coef_ + self.intercept_


class AutoregressiveLinearPredictor:
    """Future realized volatility over T days regressed on kernels of the past w returns and squared returns (Guyon,
    Lekeufack 2024): features [1, R1, sqrt(R2)] (+ ((|R1| + R1) / 2)^2 with extra_term)."""

    def __init__(self, T: int, w: int, s: int, dt: float, ktype: Literal["exp", "power-law"], k1_dict: Dict | None = None,
                 k2_dict: Dict | None = None, extra_term: bool = False):
        self.T, self.w, self.s, self.dt = T, w, s, dt
        k1_dict = DEFAULT1[ktype] if k1_dict is None else k1_dict
        k2_dict = DEFAULT2[ktype] if k2_dict is None else k2_dict
        make = self.init_pl_kernel if ktype == "power-law" else self.init_exp_kernel_2_factors
        self.k1 = make(w=w, dt=dt, **k1_dict)
        self.k2 = make(w=w, dt=dt, **k2_dict)
        self.linreg = LeastSquares()
        self.extra_term = extra_term

    @staticmethod
    def init_exp_kernel_2_factors(w: int, dt: float, lam0: float, lam1: float, theta: float) -> np.ndarray:
        """(1 - theta) k_lam0 + theta k_lam1 over the lags (w-1 .. 0) dt, each exponential normalised to sum 1 / dt."""
        taus = np.arange(w)[::-1] * dt
        fast, slow = kernel_exp(taus, lam=lam0), kernel_exp(taus, lam=lam1)
        fast = fast / fast.sum() / dt
        slow = slow / slow.sum() / dt
        return (1 - theta) * fast + theta * slow

    @staticmethod
    def init_pl_kernel(w: int, dt: float, delta: float, alpha: float) -> np.ndarray:
        """The power-law kernel over the lags (w-1 .. 0) dt, normalised to sum 252."""
        k = kernel_pl(np.arange(w)[::-1] * dt, delta=delta, alpha=alpha)
        return k * 252 / k.sum()

    def separate(self, x: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Windows of w + 1 + T prices of x (stride s): their first w + 1 prices give the past log-returns, their last T + 1
        the future realized volatility (one shared price, disjoint increments).  Returns (idx_x, idx_y, x_train, y_train)."""
        assert x.ndim == 1
        spec = {"w": self.w + 1 + self.T, "s": self.s, "offset": 0}
        idx = windows(np.arange(x.size), **spec)
        xw = windows(x, **spec)
        return (idx[:, :-self.T - 1], idx[:, -self.T - 1:], np.diff(np.log(xw[:, :self.w + 1])), get_RV(xw[:, self.w:]))

    @staticmethod
    def embedding(dlnx: np.ndarray, k1: np.ndarray, k2: np.ndarray, extra_term: bool = False) -> np.ndarray:
        """(B, 3) features [1, R1, R2] of past log-returns dlnx (B, w): R1 = sum k1 dlnx, R2 = sqrt(sum k2 dlnx^2); with
        extra_term a fourth, ((|R1| + R1) / 2)^2."""
        assert dlnx.shape[-1] == k1.size == k2.size
        r1 = (dlnx * k1).sum(-1)
        r2 = ((dlnx ** 2) * k2).sum(-1) ** 0.5
        cols = [np.ones_like(r1), r1, r2]
        if extra_term:
            cols.append((0.5 * np.abs(r1) + 0.5 * r1) ** 2)
        return np.stack(cols, axis=-1)

    def train(self, x: np.ndarray) -> None:
        """Fit on the price series x (sampled every dt)."""
        _, _, dlnx, y = self.separate(x)
        self.linreg.fit(self.embedding(dlnx, self.k1, self.k2, self.extra_term), y)

    def predict(self, x: np.ndarray) -> np.ndarray:
        """Predicted volatility for past log-returns x (B, w)."""
        return self.linreg.predict(self.embedding(x, self.k1, self.k2, self.extra_term))


class _StudentT:
    """The Student-t of `nu=` / `snp=` as the reference draws it: scipy's t(df, loc, scale).rvs() is
    standard_t(df) * scale + loc on numpy's global stream."""

    def __init__(self, df: float, loc: float = 0.0, scale: float = 1.0):
        self.df, self.loc, self.scale = float(df), float(loc), float(scale)

    def rvs(self, size) -> np.ndarray:
        return np.random.standard_t(self.df, size=size) * self.scale + self.loc


class _PDVBase:
    def __init__(self, lams1: List[float], lams2: List[float], thetas: List[float], betas: List[float], snp=None,
                 nu: float | None = None):
        """lams1, lams2: decay rates of the factors on returns and on squared returns; thetas: how each pair of
        factors is mixed; betas: b0 + b1 r1 + b2 sqrt(r2) [+ b3 ((|r1| + r1) / 2)^2]; snp: a PriceData whose log-returns
        a Student-t is fitted to (scipy), or nu: the Student-t's degrees of freedom (Gaussian draws without either)."""
        self.lams1, self.lams2 = np.array(lams1), np.array(lams2)
        self.thetas, self.betas = np.array(thetas), np.array(betas)
        self.snp, self.nu = snp, nu
        self.fit_params = None
        self.dlnx_dist = None
        if snp is not None:
            self.calibrate_log_returns(snp)
        if nu is not None:
            self.define_dlnx_dist(nu)

    def define_dlnx_dist(self, nu: float):
        self.dlnx_dist = _StudentT(nu)

    def calibrate_log_returns(self, snp):
        try:
            from scipy.stats import t as student_t
        except ImportError as e:
            raise ImportError("PDV models fit snp's log-returns with scipy.stats.t, and scipy is not installed "
                              "(nu= needs no scipy)") from e
        self.fit_params = student_t.fit(snp.dlnx.ravel().copy())
        self.dlnx_dist = _StudentT(*self.fit_params)

    def _raw_draws(self, size) -> np.ndarray:
        """Draws from numpy's global stream, with the reference's calls."""
        if self.snp is not None or self.nu is not None:
            return self.dlnx_dist.rvs(size=size)
        return np.random.randn(*size)

    def _draw_nu(self) -> float:
        """Degrees of freedom of the counter-based generator's draws (0: Gaussian).  The affine normalisation of the
        draws cancels a fitted loc and scale."""
        if (self.snp is not None or self.nu is not None) and self.dlnx_dist is not None:
            return float(self.dlnx_dist.df)
        return 0.0

    def sigma(self, R1: np.ndarray, R2: np.ndarray) -> np.ndarray:
        """Volatility from the factors, clipped to [0, 1.5] (a NaN stays NaN)."""
        r1 = self.mixing(self.thetas[0], R1)
        r2 = self.mixing(self.thetas[1], R2)
        sig = self.betas[0] + self.betas[1] * r1 + self.betas[2] * r2 ** 0.5
        if len(self.betas) > 3:
            sig += self.betas[3] * (0.5 * np.abs(r1) + 0.5 * r1) ** 2
        return np.clip(sig, 0.0, 1.5)


class PDVModel(_PDVBase):
    """Path-dependent volatility model of Guyon & Lekeufack (2024), continuous form (Euler steps, one path)."""

    def gen_dw(self, s: float, size: Tuple) -> np.ndarray:
        dw = self._raw_draws(size)
        dw -= dw.mean()
        dw /= dw.std()
        dw *= s
        return dw

    def mixing(self, theta: float, X: np.ndarray) -> np.ndarray:
        return (1 - theta) * X[0] + theta * X[1]

    def actualize_factors(self, R1: np.ndarray, R2: np.ndarray, dt: float, dwt: np.ndarray):
        """One Euler step of the factors: dR1 = lams1 (sigma dw - R1 dt), dR2 = lams2 (sigma^2 - R2) dt."""
        sig = self.sigma(R1, R2)
        return R1 + (sig * dwt - R1 * dt) * self.lams1, R2 + (sig ** 2 - R2) * dt * self.lams2

    def gen(self, T: int, dt: float, S0: float, R10: np.ndarray, R20: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(sigma, S) of one path of int(T / dt) steps from the factors R10, R20 (host only)."""
        n = int(T / dt)
        S = np.ones(n) * S0
        sigma = np.zeros(n)
        dW = self.gen_dw(s=np.sqrt(dt), size=(n - 1,))
        R1, R2 = np.array(R10), np.array(R20)
        sigma[0] = self.sigma(R1, R2)
        for t in range(1, n):
            sigma[t] = self.sigma(R1, R2)
            S[t] = S[t - 1] * (1 + sigma[t] * dW[t - 1])
            R1, R2 = self.actualize_factors(R1, R2, dt, dW[t - 1])
        return sigma, S


class PDVModelDiscrete(_PDVBase):
    """The discrete form of the PDV model (daily steps, S paths at once): the factors decay by exp(-lam / 252) a day and
    take in the return rt = max(sigma dw, -0.999999) and its square.  The method, as the kernel runs it, heads
    shadowing_amd/csrc/psh_pdv.hip."""

    def gen_dw(self, s: float, size: Tuple) -> np.ndarray:
        return _normalise(self._raw_draws(size), s)

    def mixing(self, theta: float, X: np.ndarray) -> np.ndarray:
        return (1 - theta) * X[:, 0] + theta * X[:, 1]

    def actualize_factors(self, R1: np.ndarray, R2: np.ndarray, dwt: np.ndarray):
        """One day of the factors: R <- exp(-lams / 252) R + lams rt (R1) or lams rt^2 (R2); dwt is the day's return."""
        R1n = np.exp(-self.lams1[None, :] / 252) * R1 + self.lams1[None, :] * dwt[:, None]
        R2n = np.exp(-self.lams2[None, :] / 252) * R2 + self.lams2[None, :] * dwt[:, None] ** 2
        return R1n, R2n

    def gen(self, T: int, dt: float, S0: float, S: int, R10: np.ndarray, R20: np.ndarray, *, seed: int | None = None,
            cuda: bool = False, draws=None):
        """(sigma, St), both (S, int(T / dt)): S paths from the factors R10, R20 (2 values each).
        draws: raw draws (S, n_steps) to use (they are normalised per path); seed: the counter-based generator's key;
        neither: numpy's global stream (cuda=False) or a seed drawn from it (cuda=True).  cuda=True returns HIP tensors."""
        n = _n_steps(T, dt)
        R10, R20 = _factor_rows(R10, 1), _factor_rows(R20, 1)
        if cuda:
            out = self._device(1, S, n, S0, dt, R10, R20, seed, draws, ("sigma", "St"))
            return out["sigma"], out["St"]
        out = self._host(1, S, n, S0, dt, R10, R20, seed, draws)
        return out["sigma"], out["St"]

    # ---- the two implementations of the discrete model behind gen and pdv_future_paths
    def _host(self, B: int, S: int, n: int, S0: float, dt: float, R10: np.ndarray, R20: np.ndarray, seed, draws,
              want_dlnx: bool = False) -> dict:
        """The numpy twin of psh_pdv_generate: (B*S, n) sigma, St (and float32 dlnx)."""
        if draws is not None:
            raw = _as_draws(draws, B * S, n)
        elif seed is not None:
            raw = philox_draws(_check_seed(seed), B * S, n, self._draw_nu())
        else:
            raw = self._raw_draws((B * S, n))
        dW = _normalise(raw, np.sqrt(dt))
        R1 = np.repeat(R10, S, axis=0)
        R2 = np.repeat(R20, S, axis=0)
        St = np.ones((B * S, n)) * S0
        sigma = np.zeros((B * S, n))
        dlnx = np.empty((B * S, n - 1), dtype=np.float32) if want_dlnx else None
        sigma[:, 0] = self.sigma(R1, R2)
        for t in range(1, n):
            sigma[:, t] = self.sigma(R1, R2)
            rt = np.maximum(sigma[:, t] * dW[:, t], -0.999999)
            St[:, t] = St[:, t - 1] * (1 + rt)
            if dlnx is not None:
                dlnx[:, t - 1] = np.log1p(rt)
            R1, R2 = self.actualize_factors(R1, R2, rt)
        return {"sigma": sigma, "St": St, "dlnx": dlnx}

    def _device(self, B: int, S: int, n: int, S0: float, dt: float, R10: np.ndarray, R20: np.ndarray, seed, draws,
                outputs) -> dict:
        """psh_pdv_generate on the current HIP device: the requested outputs as device tensors."""
        import torch
        from . import _native
        dev = torch.device("cuda", torch.cuda.current_device())
        dr = None
        if draws is not None:
            dr = draws if isinstance(draws, torch.Tensor) else torch.from_numpy(_as_draws(draws, B * S, n))
            if tuple(dr.shape) != (B * S, n):
                raise ValueError(f"draws must be ({B * S}, {n}), got {tuple(dr.shape)}")
            dr = dr.to(dev, torch.float64).contiguous()
            seed = 0
        elif seed is None:
            seed = int.from_bytes(np.random.bytes(8), "little")       # numpy's global stream picks the key
        return _native.pdv_generate(B, S, n, self.lams1, self.lams2, np.exp(-self.lams1[None, :] / 252)[0],
                                    np.exp(-self.lams2[None, :] / 252)[0], self.thetas, self.betas, S0, np.sqrt(dt),
                                    self._draw_nu(), R10, R20, draws=dr, seed=_check_seed(seed), outputs=outputs,
                                    device=dev)


def _n_steps(T: float, dt: float) -> int:
    if np.abs(dt - 1 / 252) > 1e-6:
        raise ValueError("dt should be 1.0 in the discrete model")
    return int(T / dt)


def _factor_rows(R, B: int) -> np.ndarray:
    R = np.asarray(R, dtype=np.float64)
    if R.size != 2 * B:
        raise ValueError(f"initial factors must hold 2 values per date, got shape {R.shape}")
    return R.reshape(B, 2)


def _check_seed(seed) -> int:
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    return seed


def _as_draws(draws, rows: int, n: int) -> np.ndarray:
    if hasattr(draws, "detach"):
        draws = draws.detach().cpu().numpy()
    raw = np.array(draws, dtype=np.float64)                       # (a copy: it is normalised in place)
    if raw.shape != (rows, n):
        raise ValueError(f"draws must be ({rows}, {n}), got {raw.shape}")
    return raw


def _normalise(dw: np.ndarray, s: float) -> np.ndarray:
    """Per path (last axis): zero mean, population std s, as the reference does it (in place)."""
    dw -= dw.mean(-1, keepdims=True)
    dw /= dw.std(-1, keepdims=True)
    dw *= s
    return dw


# ---- the counter-based generator (psh_philox.h and psh_pdv.hip state it; this is its numpy twin, shared with mrw.py)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_LO32, _SH32, _SH11 = np.uint64(0xFFFFFFFF), np.uint64(32), np.uint64(11)


def philox4x32_10(counter, key):
    """Random123's Philox4x32-10: counter = 4 arrays (broadcast) of 32-bit values, key = 2 ints.  Returns the 4 output
    words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _SH32) ^ c1 ^ np.uint64(k0), p1 & _LO32, (p0 >> _SH32) ^ c3 ^ np.uint64(k1), p0 & _LO32
    return c0, c1, c2, c3


def _words(counter, key):
    x0, x1, x2, x3 = philox4x32_10(counter, key)
    return ((x1 << _SH32) | x0) >> _SH11, ((x3 << _SH32) | x2) >> _SH11


def normal_pairs(counter, key):
    """One Box-Muller pair (z0, z1) per counter (4 broadcast arrays of 32-bit values), as psh_philox.h states it:
    u1 = (a + 1) 2^-53, u2 = b 2^-53 from the call's two 53-bit words, rad = sqrt(-2 ln u1), z0 = rad cos(2 pi u2),
    z1 = rad sin(2 pi u2)."""
    a, b = _words(counter, key)
    u1 = (a + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = b.astype(np.float64) * 2.0 ** -53
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = TWO_PI * u2
    return rad * np.cos(ang), rad * np.sin(ang)


def philox_draws(seed: int, n_paths: int, n_steps: int, nu: float = 0.0, first_path: int = 0) -> np.ndarray:
    """(n_paths, n_steps) raw draws of paths first_path.. of the counter-based generator: Gaussian (nu = 0) or
    Student-t(nu), exactly as psh_pdv.hip states them."""
    key = (seed & 0xFFFFFFFF, seed >> 32)
    out = np.empty((n_paths, n_steps))
    rows = max(1, (1 << 21) // max(n_steps, 1))                    # bounded temporaries
    for p0 in range(0, n_paths, rows):
        g = np.arange(first_path + p0, first_path + min(p0 + rows, n_paths), dtype=np.uint64)[:, None]
        glo, ghi = g & _LO32, g >> _SH32
        if nu == 0.0:
            m = np.arange((n_steps + 1) // 2, dtype=np.uint64)[None, :]
            z = np.empty((g.shape[0], 2 * m.shape[1]))
            z[:, 0::2], z[:, 1::2] = normal_pairs((m, np.uint64(0), glo, ghi), key)
            out[p0:p0 + g.shape[0]] = z[:, :n_steps]
            continue
        nexp = -2.0 / nu
        z = np.zeros((g.shape[0], n_steps))
        todo = np.ones(z.shape, dtype=bool)
        for j in range(MAX_ATTEMPTS):
            pi, ti = np.nonzero(todo)
            if pi.size == 0:
                break
            a, b = _words((ti.astype(np.uint64), np.uint64(j), glo[pi, 0], ghi[pi, 0]), key)
            U = a.astype(np.float64) * 2.0 ** -52 - 1.0
            V = b.astype(np.float64) * 2.0 ** -52 - 1.0
            W = U * U + V * V
            ok = (W < 1.0) & (W > 0.0)
            z[pi[ok], ti[ok]] = U[ok] * np.sqrt(nu * (W[ok] ** nexp - 1.0) / W[ok])
            todo[pi[ok], ti[ok]] = False
        out[p0:p0 + g.shape[0]] = z
    return out


# ---- initial factors and future paths
def _factors(x_past: np.ndarray, pdv_model, w: int, dt: float) -> Tuple[np.ndarray, np.ndarray]:
    """(R10, R20), each (B, 2): the factors at the end of each row of past prices x_past (B, w)."""
    dlnx = np.diff(np.log(x_past))
    taus = np.arange(w)[::-1][1:] * dt

    def normalised(lam):
        k = kernel_exp(taus, lam=lam)
        return k / k.sum() / dt

    extra = len(pdv_model.betas) > 3
    cols = [AutoregressiveLinearPredictor.embedding(dlnx, normalised(pdv_model.lams1[i]), normalised(pdv_model.lams2[i]),
                                                    extra_term=extra) for i in range(2)]
    R10 = np.stack([cols[0][:, 1], cols[1][:, 1]], axis=-1)
    R20 = np.stack([cols[0][:, 2], cols[1][:, 2]], axis=-1) ** 2.0
    return R10, R20


def compute_factor(x_past: np.ndarray, pdv_model, w: int, dt: float) -> Tuple[np.ndarray, np.ndarray]:
    """Initial factors R10, R20 (2 values each) at the end of the past prices x_past (1, w) (its first row).  Unlike the
    reference, 3 betas work too."""
    R10, R20 = _factors(np.atleast_2d(x_past), pdv_model, w, dt)
    return R10[0], R20[0]


def future_pdv_model(x_past: np.ndarray, pdv_model, w: int, S0: float, S: int, T: int, dt: float) -> np.ndarray:
    """S price paths (S, int(T / dt)) from the factors at the end of x_past's first row (a PDVModelDiscrete)."""
    R10, R20 = compute_factor(x_past, pdv_model, w, dt)
    _, x_gen = pdv_model.gen(T=T, dt=dt, S0=S0, S=S, R10=R10, R20=R20)
    return x_gen


def pdv_future_paths(x_past: np.ndarray, pdv_model: PDVModelDiscrete, w: int, S0: float, S: int, T: int, dt: float, *,
                     seed: int | None = None, cuda: bool = False):
    """(B, S, int(T / dt)) price paths: S for each of the B dates of x_past (B, w), each date from its own initial
    factors.  Path p of date b is path g = b * S + p of the counter-based generator, so with a seed the paths do not
    depend on how the dates are batched.  cuda=True: one psh_pdv_generate launch, a HIP tensor (compute_smile prices it
    without a host copy); seed=None draws from numpy's global stream (cuda=False) or picks the key from it."""
    if not isinstance(pdv_model, PDVModelDiscrete):
        raise TypeError("pdv_future_paths needs a PDVModelDiscrete")
    x_past = np.atleast_2d(np.asarray(x_past, dtype=np.float64))
    B = x_past.shape[0]
    R10, R20 = _factors(x_past, pdv_model, w, dt)
    n = _n_steps(T, dt)
    if cuda:
        return pdv_model._device(B, S, n, S0, dt, R10, R20, seed, None, ("St",))["St"].view(B, S, n)
    return pdv_model._host(B, S, n, S0, dt, R10, R20, seed, None)["St"].reshape(B, S, n)


__all__ = ["kernel_pl", "kernel_exp", "get_RV", "DEFAULT1", "DEFAULT2", "windows", "AutoregressiveLinearPredictor",
           "PDVModel", "PDVModelDiscrete", "compute_factor", "future_pdv_model", "pdv_future_paths", "philox4x32_10",
           "normal_pairs", "philox_draws"]
