"""Exact inputs for psh_lagged_moments (shared by tests/test_stylized_cpu.py and tests/test_gpu_stylized.py; numpy only).

With samples that are small integers every product and every partial sum is an integer far below 2^53 (|summand| <= 256,
fewer than 10^5 pairs a sum), so the double sums of the device and of the numpy twin are exact whatever their summation
order, and both must EQUAL an int64 reference: no tolerance.

lag_plan() restates moments_lag_plan (psh_moments.hip): a lane owns U lags, the 8 waves are C lag chunks times S slices
of a tile's t range (waves beyond C * S do not work: C = 3 leaves two).

    m            U  C  S        m            U  C  S
    1 ..  64     1  1  8        257 .. 512   4  2  4
    65 .. 128    2  1  8        513 .. 768   4  3  2
    129 .. 256   4  1  8        769 .. 1024  4  4  2
"""
from __future__ import annotations

import numpy as np

from shadowing_amd import stylized

LT = 2048                            # PSH_MOM_TILE
WAVES = 8                            # PSH_MOM_THREADS / 64
CENSUS_M = (64, 65, 128, 129, 256, 257, 400, 512, 513, 600, 768, 769, 1023)
BOUNDARIES = ((64, 65), (128, 129), (256, 257), (512, 513), (768, 769))
PLANT_M = (40, 100, 200, 400, 600, 1024)             # one m of every (U, C)
PLANT_N = 2 * LT + 5


def lag_plan(m: int):
    """(U, C, S) of moments_lag_plan and moments_kernel."""
    U = 1 if m <= 64 else 2 if m <= 128 else 4
    C = 1 if m <= 64 * U else -(-m // (64 * U))
    return U, C, WAVES // C


def slice_len(m: int, V: int = LT) -> int:
    """The t range a slice takes of a tile of V samples (moments_kernel's q): ceil(Vr / S) rounded up to U."""
    U, _, S = lag_plan(m)
    Vr = -(-V // U) * U
    return -(-(-(-Vr // S)) // U) * U


def census_shapes():
    """(R, n, m, G): both row lengths of every census m -- LT + m + 3 (a second tile of m + 3 samples, a multiple of 4 only
    where m = 1 mod 4, pairs reaching the end of the halo) and m + 1 (one short tile, one pair at the largest lag) -- with 1 and 3 groups."""
    return [(3, n, m, G) for m in CENSUS_M for n in (LT + m + 3, m + 1) for G in (1, 3)]


def census_id(shape) -> str:
    R, n, m, G = shape
    U, C, S = lag_plan(m)
    return f"m{m}-U{U}C{C}S{S}-n{n}-G{G}"


def int_ensemble(R: int, n: int, seed: int) -> np.ndarray:
    """(R, n) float32 holding integers in [-4, 4]."""
    return np.random.default_rng([seed, R, n]).integers(-4, 5, size=(R, n)).astype(np.float32)


def int_sums(x: np.ndarray, m: int, G: int, drop=None) -> np.ndarray:
    """(G, 4, m + 1) int64: the four sums of psh_lagged_moments by numpy slices per lag, reduced per group.
    drop = (row, tau): a deliberately wrong reference that leaves out that row's LAST pair of lag tau."""
    xi = np.asarray(x).astype(np.int64)
    assert np.array_equal(xi, x) and np.abs(xi).max(initial=0) <= 4
    R, n = xi.shape
    sq = xi * xi
    starts = stylized.group_bounds(R, G)[:-1]
    out = np.empty((G, 4, m + 1), np.int64)
    for tau in range(m + 1):
        a, a2, b, b2 = xi[:, :n - tau], sq[:, :n - tau], xi[:, tau:], sq[:, tau:]
        for q, (u, w) in enumerate(((a, b), (a, b2), (a2, b), (a2, b2))):
            prod = u * w
            if drop is not None and drop[1] == tau:
                prod = prod.copy()
                prod[drop[0], n - 1 - tau] = 0
            out[:, q, tau] = np.add.reduceat(prod.sum(axis=1), starts)
    return out


def plant_positions(m: int, n: int = PLANT_N) -> list:
    """(t1, tau): pairs at the first and last sample, across the first tile's end at the smallest and the largest lag
    from both sides, inside the ragged last tile, and on both sides of every slice boundary of the first tile at lags 1
    and m."""
    assert n == 2 * LT + 5 and 4 <= m < LT
    p = [(0, m), (LT - 1, 1), (LT - 1, m), (LT - m, m), (n - 1 - m, m), (n - 2, 1), (2 * LT, 4)]
    q, S = slice_len(m), lag_plan(m)[2]
    for s in range(1, S):
        for t1 in (s * q - 1, s * q):
            p += [(t1, 1), (t1, m)]
    assert all(1 <= tau <= m and 0 <= t1 and t1 + tau < n for t1, tau in p)
    return p


def plants(m: int, n: int = PLANT_N):
    """One row per plant, zero except 2 at t1 and 3 at t1 + tau; a group per row.  Returns (x (R, n) float32,
    expected (R, 4, m + 1) int64): (6, 18, 12, 36) at lag tau, (13, 35, 35, 97) at lag 0, 0 elsewhere."""
    pos = plant_positions(m, n)
    x = np.zeros((len(pos), n), np.float32)
    want = np.zeros((len(pos), 4, m + 1), np.int64)
    for i, (t1, tau) in enumerate(pos):
        x[i, t1], x[i, t1 + tau] = 2.0, 3.0
        want[i, :, tau] = (6, 18, 12, 36)
        want[i, :, 0] = (13, 35, 35, 97)
    return x, want
