"""numpy twins of the long-window front end (shadowing_amd/csrc/psh_long.h): each reproduces the device's order of
operations and its roundings, not a sum in a better precision.  Every fused multiply-add is computed exactly (fractions)
and rounded once to float32."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import _wave_twin as tw

SEG = 1024
ROW, SFLOATS, NSTAGE = 40, 1280, 5
GAMMA = np.float32(2.0 ** -17)
INF32 = np.float32(np.inf)
F32 = np.float32


def ksteps(W: int) -> int:
    return (W + 31 + 15) // 16


def bucket(W: int) -> int:
    n = ksteps(W)
    return 6 if n <= 6 else 10 if n <= 10 else 14 if n <= 14 else 18


def copy_chunks(nks: int) -> int:
    return 20 if 2 * nks + 4 <= 20 else 36 if 2 * nks + 4 <= 36 else 52


def query_halves(nks: int) -> int:
    return 8 * copy_chunks(nks) * 8


def long_rows(nks: int) -> int:
    return 31 + (nks + 1) // 2


def mx_window(r, lane):
    """slot r of lane (m = lane & 31, hk = lane >> 5) -> the window's index in the segment"""
    return 32 * ((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) + (lane & 31)


def round_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the exact x, ties to even; overflow to inf.  (A zero comes out +0: what an fma gives when its
    product and its addend are not both -0.)"""
    if x == 0:
        return F32(0.0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()         # 2^(e-1) <= a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                        # 2^e <= a < 2^(e+1)
    q = Fraction(2) ** (max(e, -126) - 23)                            # the spacing of float32 there (denormals: 2^-149)
    n, rem = divmod(a, q)
    n = int(n)
    if rem * 2 > q or (rem * 2 == q and n & 1):
        n += 1
    v = Fraction(n) * q
    if v >= Fraction(2) ** 128:
        return F32(s * np.inf)
    return F32(s * float(v))                                          # exact: n < 2^25, q a power of two in float64's range


def fma32(a, b, c) -> np.float32:
    """fl32(a * b + c), one rounding; NaN / inf operands by IEEE rules"""
    a, b, c = F32(a), F32(b), F32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))  # the result is a NaN or an inf: no rounding at issue
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# ---------------------------------------------------------------------------------- staging
def stage_row(ds: np.ndarray, T: int, row: int, seg_start: int, nfloat: int) -> np.ndarray:
    """The 1280 words a wave stages (word 4 (lane + 64 q) + i): the row's floats from seg_start on, zero past the row's end,
    all bits set where the last group loads nothing (lane + 256 >= ceil(nfloat / 4))."""
    out = np.full(4 * 64 * NSTAGE, 0xffffffff, dtype=np.uint32)
    nq4 = (nfloat + 3) >> 2
    words = np.ascontiguousarray(ds, dtype=np.float32).view(np.uint32).ravel()
    for mm in range(64 * NSTAGE):
        if mm >= 256 and mm >= nq4:
            continue
        for i in range(4):
            t = seg_start + 4 * mm + i
            out[4 * mm + i] = words[row * T + t] if t < T else 0
    return out


# ---------------------------------------------------------------------------------- the C operand, the tile's minimum
def energy_operand(sp: np.ndarray, W: int, upper: bool) -> np.ndarray:
    """[64 lanes, 16 slots]: fl32(S[p + W] (1 +- gamma) - S[p]), p = mx_window(r, lane)"""
    f = F32(1.0) + GAMMA if upper else F32(1.0) - GAMMA
    out = np.empty((64, 16), dtype=np.float32)
    for lane in range(64):
        for r in range(16):
            p = mx_window(r, lane)
            out[lane, r] = fma32(sp[p + W], f, -sp[p])
    return out


def tile_min(tile: np.ndarray, nvalid: int) -> np.ndarray:
    """[64]: the chain of fminf over the slots whose window exists, from +inf, then the wave's butterfly"""
    mn = np.full(64, np.inf, dtype=np.float32)
    for r in range(16):
        p = mx_window(r, np.arange(64))
        mn = np.where((nvalid >= SEG) | (p < nvalid), tw.fmin_(mn, tile[:, r]), mn)
    return tw.wave_reduce(mn[None, :], tw.fmin_)[0]


def upper_bound(est, nx, W: int, sexp: int) -> np.ndarray:
    """long_upper_bound, every operation a float32 operation in the source's order"""
    est, nx = np.asarray(est, dtype=np.float32), np.asarray(nx, dtype=np.float32)
    with np.errstate(all="ignore"):
        b = F32(2 * W + 2) / F32(64.0) / F32(262144.0)
        f = F32(1.0) + F32(2.0) / F32(900.0) + F32(1.0e-5) + F32(6.0) * GAMMA
        ub = (est + nx * (F32(3.0) / F32(900.0)) + b) * f * (F32(1.0) + F32(1e-6))
        inv = np.ldexp(F32(1.0), -sexp)
        ub = (ub * inv * inv).astype(np.float32)
    return np.where(np.isnan(ub), INF32, ub).astype(np.float32)


# ---------------------------------------------------------------------------------- a query's tables
def query_tables(xs: np.ndarray, W: int, scale, nks: int) -> np.ndarray:
    """[nq, 8 copies, CP chunks, 8] float16: copy c, chunk v, half i holds f16(-2 (x[j] scale)), j = 8 (v - 3) + i - c; zero
    outside the window"""
    CP = copy_chunks(nks)
    xs = np.asarray(xs, dtype=np.float32)
    out = np.zeros((xs.shape[0], 8, CP, 8), dtype=np.float16)
    c, v, i = np.meshgrid(np.arange(8), np.arange(CP), np.arange(8), indexing="ij")
    j = 8 * (v - 3) + i - c
    inside = (j >= 0) & (j < W)
    with np.errstate(over="ignore", invalid="ignore"):
        for q in range(xs.shape[0]):
            val = (F32(-2.0) * (xs[q][np.where(inside, j, 0)] * F32(scale)).astype(np.float32)).astype(np.float32)
            out[q] = np.where(inside, val, F32(0.0)).astype(np.float16)
    return out


# ---------------------------------------------------------------------------------- the exact chain
def exact_window(y: np.ndarray, x: np.ndarray, W: int) -> np.float32:
    """v = fma(D, D, v), D = fl32(x[j] - y[j]), j = 0 .. W - 1 in order"""
    v = F32(0.0)
    with np.errstate(all="ignore"):
        for j in range(W):
            D = F32(F32(x[j]) - F32(y[j]))
            v = fma32(D, D, v)
    return v
