"""What the calibration tests share: the definition of README "Calibrating to market quotes" evaluated in long double
(weights, gradient and Hessian at a given lambda), the bounds of its comparison rule, and the inputs with a planted
multiplier."""
import functools
import math

import numpy as np

from shadowing_amd import calibration as cal

LD = np.longdouble
U = 2.0 ** -53
X0 = 100.0


def returns(k, L, seed, B=1):
    """Student-t log-returns, 4 degrees of freedom, scale 0.2 / sqrt(252), float32 (B, k, L)."""
    g = np.random.default_rng(seed)
    return (g.standard_t(4, size=(B, k, L)) * (0.2 / math.sqrt(252.0))).astype(np.float32)


def strikes_at(Ts, Ms, rate=0.0, sigma=0.2):
    """(nT, nM) strikes F exp(M sigma sqrt(T / 252))."""
    return np.stack([X0 * math.exp(rate / 252.0 * T) * np.exp(np.asarray(Ms) * sigma * math.sqrt(T / 252.0)) for T in Ts])


def exact(r, prior, Ts, strike, target, lam, rate=0.0, kind=0, martingale=True, eps=0.0):
    """The definition at `lam` for one date in long double: dict of q (k,), h and g (k_live, J), live, act, mu, grad (J,), H (J, J),
    S (k_live, nT).  S_T is the double the definition states (a sequential double sum, exp, times x_init); everything after it
    is long double."""
    k = r.shape[0]
    p = np.ones(k) if prior is None else np.asarray(prior, dtype=np.float64)
    live = p > 0.0
    inst = cal.instruments(X0, rate, Ts, strike, target, kind, martingale)
    c, act = inst[2].astype(LD), inst[5]
    S = cal.terminal_prices(r[live], Ts, X0)
    g = cal.payoffs(S, inst, dtype=LD)
    h = (g - c[None, :]) / LD(X0)
    lam = np.where(act, np.asarray(lam, dtype=np.float64), 0.0).astype(LD)
    a = h[:, act] @ lam[act]
    e = p[live].astype(LD) * np.exp(a - a.max())
    ql = e / e.sum()
    mu = np.where(act, ql @ h, LD(0.0))
    H = (ql[:, None] * h).T @ h - np.outer(mu, mu) + LD(eps) * np.eye(len(c), dtype=LD)
    q = np.zeros(k, dtype=LD)
    q[live] = ql
    return {"q": q, "ql": ql, "h": h, "g": g, "live": live, "act": act, "mu": mu, "grad": np.where(act, mu + LD(eps) * lam, LD(0.0)),
            "H": H, "S": S, "a": a, "qidx": inst[0]}


def weight_bound(ex, lam, k, J):
    """The relative bound on |q_device - q_exact|: the argument a_i = sum_j lambda_j h_ij of the device carries at most
        A_i = sum_j |lambda_j| (4 S_ij / x_init + (J + 5) |h_ij|) 2^-53
    (S_T within 3 ulps of the definition's double -- exp, its argument's last place, the product -- through the payoff, the
    discount, the subtraction and the division; then J products and J sums of terms |lambda_j h_ij|), which enters e_i and Z
    through a_i and amax: 4 max_i A_i relative; two 1-ulp exps a side, a sum of at most k non-negative terms, one division:
    (2 k + 16) 2^-53."""
    lam = np.abs(np.where(ex["act"], np.asarray(lam, dtype=np.float64), 0.0))
    Sj = ex["S"][:, ex["qidx"]] / X0
    A = ((4.0 * Sj + (J + 5) * np.abs(ex["h"].astype(np.float64))) @ lam) * U
    return (2 * k + 16) * U + 4.0 * float(A.max(initial=0.0))


def gradient_bound(ex, k, tol):
    """Optimality: tol plus the rounding of a k-term sum, 2 (k + 2) 2^-53 sum_i q_i |h_ij|, per instrument."""
    return tol + 2 * (k + 2) * U * (ex["ql"] @ np.abs(ex["h"])).astype(np.float64)


PLANT_TS, PLANT_MS = (10, 30), (-0.5, 0.0, 0.5)


@functools.lru_cache(maxsize=None)
def planted(k, seed=7):
    """Inputs whose multiplier is known: (r (1, k, 30), strike (1, 2, 3), target (1, 2, 3), lam_star (8,), martingale).  With
    fewer than 8 paths there are no forwards (k paths cannot reprice them in general), lam_star is (6,) and martingale False.
    The six option
    multipliers are chosen; the two forward multipliers are then solved for in long double (a 2 x 2 Newton iteration on the
    same convex dual) so that the forwards reprice; the option targets are c = sum q* g, rounded to double -- which is why
    lambda* is only an approximate stationary point."""
    r = returns(k, 30, seed + k)
    strike = strikes_at(PLANT_TS, PLANT_MS)
    g0 = np.random.default_rng(seed)
    mart = k >= 8
    lam = np.concatenate([g0.uniform(-3.0, 3.0, 6), np.zeros(2 if mart else 0)]).astype(LD)
    inst = cal.instruments(X0, 0.0, PLANT_TS, strike, np.zeros((2, 3)), 0, mart)
    g = cal.payoffs(cal.terminal_prices(r[0], PLANT_TS, X0), inst, dtype=LD)
    hf = (g[:, 6:] - LD(X0)) / LD(X0)
    for _ in range(60 if mart else 0):
        a = (g / LD(X0)) @ lam
        q = np.exp(a - a.max())
        q = q / q.sum()
        mu = q @ hf
        H = (q[:, None] * hf).T @ hf - np.outer(mu, mu)
        step = np.linalg.solve(H.astype(np.float64), -mu.astype(np.float64)).astype(LD)
        lam[6:] = lam[6:] + step
        if float(np.abs(mu).max()) < 1e-19:
            break
    a = (g / LD(X0)) @ lam
    q = np.exp(a - a.max())
    q = q / q.sum()
    target = (q @ g[:, :6]).astype(np.float64).reshape(1, 2, 3)
    return r, strike[None], target, lam.astype(np.float64), mart


def stationary_bound(r, strike, target, lam, lam_star, martingale=True):
    """|lam - lam*|_2 <= 2 (|grad(lam)|_2 + |grad(lam*)|_2) / sigma_min(H(lam*)), both gradients in long double: (the bound,
    sigma_min, the two gradient norms)."""
    at = exact(r[0], None, PLANT_TS, strike[0], target[0], lam, martingale=martingale)
    star = exact(r[0], None, PLANT_TS, strike[0], target[0], lam_star, martingale=martingale)
    smin = float(np.linalg.svd(star["H"].astype(np.float64), compute_uv=False).min())
    g1, g2 = float(np.sqrt((at["grad"] ** 2).sum())), float(np.sqrt((star["grad"] ** 2).sum()))
    return 2.0 * (g1 + g2) / smin, smin, g1, g2


def pinsker_bound(r, strike, target, lam, lam_star, martingale):
    """Where H is singular lambda is not unique but q is.  q(lam) and q* = q(lam*) belong to one exponential family, so
    KL(q* | q) + KL(q | q*) = (lam - lam*) . (mu(lam) - mu(lam*)), and by Pinsker |q - q*|_1 <= sqrt(2 KL): returns
    (sqrt(2 |(lam - lam*) . (grad(lam) - grad(lam*))|), q*), both gradients in long double."""
    at = exact(r[0], None, PLANT_TS, strike[0], target[0], lam, martingale=martingale)
    star = exact(r[0], None, PLANT_TS, strike[0], target[0], lam_star, martingale=martingale)
    dot = float(np.abs(((np.asarray(lam, dtype=LD) - np.asarray(lam_star, dtype=LD)) * (at["grad"] - star["grad"])).sum()))
    return math.sqrt(2.0 * dot), star["q"].astype(np.float64)
