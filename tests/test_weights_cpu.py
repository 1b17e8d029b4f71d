"""The numpy twin of psh_softmax_weights (shadowing_amd/weights.py) against the definition it shares with the kernel: an
independent statement of it, the stand-in averaging.Softmax, the properties the definition promises, and a long double
evaluation on the same arguments -- which shows what part of the device bound two correct implementations use up.  No GPU."""
import math

import numpy as np
import pytest

import shadowing_amd as sa
from shadowing_amd import path_shadowing as ps
from shadowing_amd import weights as W

U = 2.0 ** -53


def device_bound(w_ref, kc):
    """|w_device - w_twin| <= (2 k' + 16) 2^-53 w_twin + 2^-1070: the arguments of exp are bit-identical, each exp is within
    1 ulp (4 * 2^-53 between the sides a term), each sum of k' non-negative terms carries (k' - 1) 2^-53, one division a
    side; the absolute term covers subnormal e_j under Z >= 1."""
    return (2 * kc + 16) * U * np.abs(w_ref) + 2.0 ** -1070


def rows(B, k, seed, scale=0.1):
    g = np.random.default_rng(seed)
    return (np.abs(g.standard_normal((B, k))) * scale).astype(np.float32)


def by_definition(d32, eta, kc):
    """One row, written as the definition reads: a sorted loop, Python floats, math.exp."""
    k = len(d32)
    d = [float(x) for x in d32]
    order = sorted(range(k), key=lambda j: ((2, 0.0) if math.isnan(d[j]) else (1, d[j]), j))
    kept = order[:kc]
    w = [0.0] * k
    if eta is None:
        for j in kept:
            w[j] = 1.0 / kc
        return np.array(w)
    s = 2.0 * (eta * eta)
    z = [-(d[j] * d[j]) / s for j in kept]
    zmax = math.nan if any(math.isnan(v) for v in z) else max(z)
    e = []
    for v in z:
        a = v - zmax
        e.append(a if math.isnan(a) else math.exp(a))
    Z = 0.0
    for v in e:
        Z += v
    for j, v in zip(kept, e):
        w[j] = v / Z if Z == Z else math.nan
    return np.array(w)


@pytest.mark.parametrize("k", [1, 2, 65, 777])
def test_twin_against_the_definition_as_a_loop(k):
    d = rows(2, k, k)
    d[1] = d[1][::-1].copy() if k > 1 else d[1]
    etas, ks = (0.003, 0.1, 30.0, None), sorted({1, max(1, k // 3), k})
    w = W.softmax_weights(d, etas, ks)
    assert w.shape == (4, len(ks), 2, k) and w.dtype == np.float64
    for a, eta in enumerate(etas):
        for c, kc in enumerate(ks):
            for b in range(2):
                ref = by_definition(d[b], eta, kc)
                assert np.array_equal(w[a, c, b] == 0.0, ref == 0.0)
                assert (np.abs(w[a, c, b] - ref) <= device_bound(ref, kc)).all(), (eta, kc, b)


@pytest.mark.parametrize("eta", [0.003, 0.07, 30.0])
def test_twin_is_bit_equal_to_the_stand_in_softmax_on_ascending_rows(eta):
    from shadowing_amd.averaging import HAVE_SCATSPECTRA, Softmax
    assert not HAVE_SCATSPECTRA
    d = np.sort(rows(3, 777, 1), axis=1)
    w = W.softmax_weights(d, [eta])[0, 0]
    assert np.array_equal(w.view(np.uint64), np.asarray(Softmax(d.astype(np.float64), eta).weights).view(np.uint64))
    assert np.array_equal(W.softmax_weights(d, [None])[0, 0], np.asarray(Softmax(d.astype(np.float64), None).weights))


def test_rows_sum_to_one_and_weights_past_the_cut_off_are_zero():
    k = 1000
    d = rows(3, k, 2)
    ks = (1, 2, 500, 999, 1000)
    w = W.softmax_weights(d, (0.003, 0.1, 30.0, None), ks)
    order = np.argsort(d, axis=1, kind="stable")
    for c, kc in enumerate(ks):
        assert (np.abs(w[:, c].sum(axis=-1) - 1.0) <= (kc + 2) * U).all(), kc
        past = np.take_along_axis(w[:, c], np.broadcast_to(order[:, kc:], (4, 3, k - kc)), axis=-1)
        assert (past == 0.0).all() and not np.signbit(past).any()
        kept = np.take_along_axis(w[:, c], np.broadcast_to(order[:, :kc], (4, 3, kc)), axis=-1)
        assert (kept[:3] >= 0.0).all() and (kept[3] == 1.0 / kc).all()


def test_a_tie_at_the_cut_off_goes_to_the_lower_index():
    d = np.array([[0.3, 0.1, 0.2, 0.1, 0.2, 0.2, -0.0, 0.0]], dtype=np.float32)
    w = W.softmax_weights(d, [0.1, None], [1, 3, 5])
    for a in range(2):
        assert np.array_equal(w[a, 0, 0] > 0, [0, 0, 0, 0, 0, 0, 1, 0])          # -0.0 == +0.0: index 6 before index 7
        assert np.array_equal(w[a, 1, 0] > 0, [0, 1, 0, 0, 0, 0, 1, 1])          # 0.1 at index 1 before 0.1 at index 3
        assert np.array_equal(w[a, 2, 0] > 0, [0, 1, 1, 1, 0, 0, 1, 1])          # 0.2 at index 2 before those at 4 and 5
    assert w[0, 2, 0, 1] == w[0, 2, 0, 3] and w[0, 2, 0, 6] == w[0, 2, 0, 7]


def test_unsorted_and_descending_rows_carry_the_sorted_rows_weights():
    k = 257
    asc = np.sort(rows(2, k, 3), axis=1)
    asc[:, 100:104] = asc[:, 100:101]                                            # ties
    g = np.random.default_rng(4)
    for perm in (np.arange(k)[::-1], g.permutation(k)):
        d = asc[:, perm]
        order = np.argsort(d, axis=1, kind="stable")
        for kc in (1, 102, k):
            w_sorted = W.softmax_weights(np.take_along_axis(d, order, axis=1), [0.05], [kc])[0, 0]
            w = W.softmax_weights(d, [0.05], [kc])[0, 0]
            assert np.array_equal(np.take_along_axis(w, order, axis=1).view(np.uint64), w_sorted.view(np.uint64))


def test_nan_and_inf_as_the_definition_says():
    inf, nan = np.inf, np.nan
    neg_nan = np.array([0xffc00000], dtype=np.uint32).view(np.float32)[0]
    d = np.array([[0.2, neg_nan, 0.1, inf, nan, 0.3]], dtype=np.float32)        # order: 2, 0, 5, 3 (inf), 1 (NaN), 4 (NaN)
    w = W.softmax_weights(d, [0.1, None], [3, 4, 5, 6])
    assert np.isfinite(w[0, 0]).all() and np.array_equal(w[0, 0, 0] > 0, [1, 0, 1, 0, 0, 1])      # NaN, inf past the cut: harmless
    assert np.array_equal(w[0, 1, 0] > 0, [1, 0, 1, 0, 0, 1]) and w[0, 1, 0, 3] == 0.0           # a kept inf weighs exactly 0
    assert abs(w[0, 1, 0].sum() - 1.0) <= 6 * U
    assert np.array_equal(np.isnan(w[0, 2, 0]), [1, 1, 1, 1, 0, 1]) and w[0, 2, 0, 4] == 0.0     # a kept NaN: every kept weight
    assert np.isnan(w[0, 3, 0]).all()
    assert np.array_equal(w[1, 2, 0], [0.2, 0.2, 0.2, 0.2, 0.0, 0.2])                            # uniform: whatever the distances
    allinf = np.array([[inf, inf, 0.5]], dtype=np.float32)
    w = W.softmax_weights(allinf[:, :2], [0.1])[0, 0]
    assert np.isnan(w).all()                                                                     # -inf - -inf
    w = W.softmax_weights(allinf, [0.1], [1, 3])[0, :, 0]
    assert np.array_equal(w[0], [0.0, 0.0, 1.0]) and np.array_equal(w[1], [0.0, 0.0, 1.0])


def test_a_sets_bits_do_not_depend_on_the_other_sets():
    d = rows(3, 300, 5)
    etas, ks = (0.003, 0.02, 0.1, None), (1, 7, 150, 300)
    grid = W.softmax_weights(d, etas, ks)
    for a, eta in enumerate(etas):
        for c, kc in enumerate(ks):
            alone = W.softmax_weights(d, [eta], [kc])[0, 0]
            assert np.array_equal(alone.view(np.uint64), grid[a, c].view(np.uint64))
    assert np.array_equal(grid.view(np.uint64), W.softmax_weights(d, etas, ks).view(np.uint64))
    assert np.array_equal(W.softmax_weights(d.astype(np.float64) * (1 + 1e-9), etas, ks), grid)  # rounded to float32 first


@pytest.mark.parametrize("k", [1, 2, 63, 1000, 16384])
def test_twin_against_long_double_on_the_same_arguments_uses_under_half_the_device_bound(k):
    """exp, sum and division in long double on the SAME double arguments a_j: the twin's own share of the bound the GPU test
    holds the kernel to.  (Recomputing z itself in long double is another question: at eta = 0.003 the argument reaches
    10^4 and its rounding is multiplied by that much.)"""
    assert np.finfo(np.longdouble).nmant >= 63
    d = np.sort(rows(1, k, 6), axis=1)
    worst = 0.0
    for eta in (0.003, 0.1, 30.0):
        for kc in sorted({1, (k + 1) // 2, k}):
            w = W.softmax_weights(d, [eta], [kc])[0, 0, 0, :kc]
            dk = d[0, :kc].astype(np.float64)
            z = -(dk * dk) / (2.0 * (eta * eta))
            a = z - z.max()
            e = np.exp(a.astype(np.longdouble))
            ref = e / e.sum()
            share = np.abs(w.astype(np.longdouble) - ref) / ((2 * kc + 16) * U * ref + 2.0 ** -1070)
            worst = max(worst, float(share.max()))
    assert worst <= 0.5, worst


def test_arguments_are_checked_as_the_c_entry_checks_them():
    d = rows(2, 8, 7)
    for bad in ([], [0.0], [-0.1], [math.nan]):
        with pytest.raises(ValueError):
            W.softmax_weights(d, bad)
    for bad in ([], [0], [9], [4, -1]):
        with pytest.raises(ValueError):
            W.softmax_weights(d, [0.1], bad)
    with pytest.raises(ValueError):
        W.softmax_weights(d, [0.1] * 9, [1, 2, 3, 4, 5, 6, 7, 8])                # 72 sets
    with pytest.raises(ValueError):
        W.softmax_weights(d[0], [0.1])
    assert W.softmax_weights(d, [0.1] * 8, [1, 2, 3, 4, 5, 6, 7, 8]).shape == (8, 8, 2, 8)
    assert W.softmax_weights(d, [math.inf])[0, 0, 0, 0] == 0.125                 # the C entry's spelling of None


def test_module_is_exported_and_cuda_true_has_no_fallback():
    import torch

    import shadowing
    from shadowing_amd import _native
    assert sa.softmax_weights is W.softmax_weights and "softmax_weights" in sa.__all__
    assert shadowing.softmax_weights is sa.softmax_weights
    assert "psh_softmax_weights" in _native.EXPORTS and callable(_native.softmax_weights)
    with pytest.raises(_native.NativeLibraryError):
        _native.softmax_weights(torch.zeros(1, 4), [0.1])
    if not torch.cuda.is_available():
        with pytest.raises(_native.NativeLibraryError):
            sa.softmax_weights(np.zeros((1, 4), dtype=np.float32), [0.1], cuda=True)
    with pytest.raises(_native.NativeLibraryError):
        sa.softmax_weights(np.zeros((1, 16385), dtype=np.float32), [0.1], cuda=True)           # k > PSH_MAX_K
    assert sa.softmax_weights(np.zeros((1, 16385), dtype=np.float32), [0.1], cuda=False)[0, 0, 0, 0] == 1.0 / 16385


class Sharper(sa.DiscreteProba):
    """Another formula: exp(-d / eta)."""

    def __init__(self, distances, eta):
        d = np.asarray(distances, dtype=np.float64)
        w = np.ones_like(d) if eta is None else np.exp(-(d - d.min(axis=1, keepdims=True)) / eta)
        super().__init__(w / w.sum(axis=1, keepdims=True))


class Mute:
    """No `weights` at all."""

    def __init__(self, distances, eta):
        pass


def test_the_probe_takes_the_stand_ins_and_rejects_other_weights(monkeypatch):
    monkeypatch.setattr(ps, "_WEIGHT_CLASSES", {})
    probe = ps._WEIGHT_PROBE
    for eta in (0.07, None):
        assert ps.weights_follow_twin(sa.Softmax(probe.astype(np.float64), eta), probe, eta)
        assert ps.weights_follow_twin(sa.Uniform(), probe, None)
        assert not ps.weights_follow_twin(Mute(probe, eta), probe, eta)
    assert not ps.weights_follow_twin(Sharper(probe, 0.07), probe, 0.07)
    assert ps._WEIGHT_CLASSES[(Sharper, False)] is False and ps._WEIGHT_CLASSES[(sa.Softmax, False)] is True

    obj = sa.PathShadowing(sa.Identity(4), sa.RelativeMSE(), np.zeros((2, 1, 16), dtype=np.float32), sa.PredictionContext(horizon=2))
    assert obj._device_eta("softmax", 0.2, moments=True) == 0.2 and obj._device_eta("softmax", None) is None
    assert obj._device_eta("uniform", 0.2, moments=True) is None
    assert obj.last_weights is None

    class Installed(sa.PathShadowing):
        @staticmethod
        def init_averaging_proba(proba_name, distances, eta):
            return (Sharper if proba_name == "softmax" else Mute)(distances, eta)

    other = Installed(sa.Identity(4), sa.RelativeMSE(), np.zeros((2, 1, 16), dtype=np.float32), sa.PredictionContext(horizon=2))
    for name in ("softmax", "uniform"):
        with pytest.raises(TypeError, match="device_weights"):
            other._device_eta(name, 0.2)


def test_device_weights_is_the_last_keyword_and_off_by_default():
    import inspect
    for name in ("predict", "predict_quantiles", "score", "smile"):
        params = list(inspect.signature(getattr(sa.PathShadowing, name)).parameters.values())
        assert params[-1].name == "device_weights" and params[-1].default is False, name
