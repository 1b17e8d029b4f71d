"""shadowing_amd.quantiles without a GPU: the numpy twin of psh_weighted_quantiles against numpy's own weighted quantile and
a brute-force evaluation of the definition, the properties README "Predictive quantiles" states, every status case, and the
PathShadowing methods against the twin applied to shadow()'s output."""
import math

import numpy as np
import pytest

import _quantiles as qu
import shadowing_amd as sa
from shadowing_amd import quantiles as qn, synthetic as syn

KS = (1, 2, 63, 64, 65, 1000, 2048, 2049, 4097, 16384)


@pytest.mark.parametrize("k", KS)
def test_q_is_numpys_inverted_cdf(k):
    B, m = 2, 2
    v = qu.values(B, k, m, seed=k)
    w = qu.softmax_weights(B, k, seed=k)
    for weights in (w, None):
        res = sa.weighted_quantiles(v, weights, qu.LEVELS, cuda=False)
        assert res.q.shape == (B, len(qu.LEVELS), m) and not res.status.any()
        for b in range(B):
            for i in range(m):
                kw = {} if weights is None else {"weights": weights[b]}
                ref = np.quantile(v[b, :, i].astype(np.float64), qu.LEVELS, method="inverted_cdf", **kw)
                assert np.array_equal(res.q[b, :, i], ref), (k, b, i, weights is None)


@pytest.mark.parametrize("k", (1, 2, 65, 1000))
def test_tail_means_against_fsum(k):
    v = qu.values(1, k, 2, seed=7 + k)
    w = qu.softmax_weights(1, k, seed=7 + k)
    q, lo, up, st, det = qu.twin(v, w, qu.LEVELS)
    for i in range(2):
        x = [float(a) for a in v[0, :, i]]
        order = sorted(range(k), key=lambda j: (x[j], j))
        C, acc = [], 0.0
        for j in order:
            acc += float(w[0, j])
            C.append(acc)
        W = C[-1]
        for a, p in enumerate(qu.LEVELS):
            t = float(p) * W
            s = next(n for n in range(k) if C[n] >= t)
            xq = x[order[s]]
            assert q[0, a, i] == xq
            Cp = C[s - 1] if s else 0.0
            lower = math.fsum([float(w[0, j]) * x[j] for j in order[:s]] + [(t - Cp) * xq]) / t
            upper = math.fsum([(C[s] - t) * xq] + [float(w[0, j]) * x[j] for j in order[s + 1:]]) / (W - t)
            assert abs(lo[0, a, i] - lower) <= det["bound_lower"][0, a, i]
            assert abs(up[0, a, i] - upper) <= det["bound_upper"][0, a, i]


@pytest.mark.parametrize("k", (2, 65, 2049))
def test_properties(k):
    B, m = 2, 3
    v = qu.values(B, k, m, seed=11 + k)
    w = 3.7 * qu.softmax_weights(B, k, seed=11 + k)                # unnormalised: nothing is renormalised
    lv = np.sort(qu.LEVELS32)
    r = sa.weighted_quantiles(v, w, lv, cuda=False)
    W = w.sum(axis=1)[:, None, None]
    mean = np.einsum("bk,bkm->bm", w, v.astype(np.float64))[:, None, :] / W
    p = lv[None, :, None]
    scale = np.abs(v).max()
    assert np.allclose(p * r.lower + (1 - p) * r.upper, mean, rtol=0, atol=1e-12 * scale * k)      # the weighted mean
    ulps = 2.0 ** -50 * scale                                      # (t x) / t is x to a rounding or two, not to the bit
    assert (r.lower <= r.q + ulps).all() and (r.q <= r.upper + ulps).all()
    for a in (r.q, r.lower, r.upper):                                                              # monotone in p
        assert (np.diff(a, axis=1) >= -1e-13 * scale).all()
    r4 = sa.weighted_quantiles(v, 4.0 * w, lv, cuda=False)                                         # weights x 4: no bit changes
    for name in ("q", "lower", "upper"):
        assert np.array_equal(getattr(r4, name).view(np.uint64), getattr(r, name).view(np.uint64)), name
    perm = np.random.default_rng(k).permutation(k)                                                 # a joint permutation
    rp = sa.weighted_quantiles(v[:, perm], w[:, perm], lv, cuda=False)
    det = qu.twin(v, w, lv)[4]
    assert not det["edge"].any()
    assert np.array_equal(rp.q, r.q)
    assert (np.abs(rp.lower - r.lower) <= det["bound_lower"]).all() and (np.abs(rp.upper - r.upper) <= det["bound_upper"]).all()


def test_unit_weights_take_the_order_statistic():
    for k in (1, 2, 63, 64, 65, 1000):
        v = qu.values(1, k, 1, seed=k)
        r = sa.weighted_quantiles(v, None, qu.LEVELS, cuda=False)
        xs = np.sort(v[0, :, 0].astype(np.float64))
        assert np.array_equal(r.q[0, :, 0], xs[np.ceil(qu.LEVELS * k).astype(int) - 1])


def test_status_cases():
    k = 65
    v = qu.values(3, k, 2, seed=5)
    w = qu.softmax_weights(3, k, seed=5)
    clean = sa.weighted_quantiles(v, w, qu.LEVELS, cuda=False)
    assert not clean.status.any() and np.isfinite(clean.q).all()
    # a NaN / inf at a zero-weight path: nothing changes but the weight that left
    v0, w0 = v.copy(), w.copy()
    w0[1, 7] = 0.0
    ref = sa.weighted_quantiles(v0, w0, qu.LEVELS, cuda=False)
    v0[1, 7, 0], v0[1, 7, 1] = np.nan, np.inf
    r = sa.weighted_quantiles(v0, w0, qu.LEVELS, cuda=False)
    assert not r.status.any() and np.isfinite(r.q).all()
    for name in ("q", "lower", "upper"):
        assert np.array_equal(getattr(r, name), getattr(ref, name))
    # a non-finite value at a positive weight: that column alone
    for bad in (np.nan, np.inf, -np.inf):
        v1 = v.copy()
        v1[2, 9, 1] = bad
        r = sa.weighted_quantiles(v1, w, qu.LEVELS, cuda=False)
        assert r.status.tolist() == [0, 0, qn.STATUS_NONFINITE]
        for a in (r.q, r.lower, r.upper):
            assert np.isnan(a[2, :, 1]).all() and np.isfinite(a[2, :, 0]).all() and np.isfinite(a[:2]).all()
    # bad weights: the whole query
    for bad in (np.nan, np.inf, -1e-3):
        w1 = w.copy()
        w1[0, 3] = bad
        r = sa.weighted_quantiles(v, w1, qu.LEVELS, cuda=False)
        assert r.status.tolist() == [qn.STATUS_WEIGHTS, 0, 0]
        for a in (r.q, r.lower, r.upper):
            assert np.isnan(a[0]).all() and np.isfinite(a[1:]).all()
    w1 = w.copy()
    w1[1] = 0.0                                                    # W = 0
    r = sa.weighted_quantiles(v, w1, qu.LEVELS, cuda=False)
    assert r.status.tolist() == [0, qn.STATUS_WEIGHTS, 0] and np.isnan(r.q[1]).all() and np.isfinite(r.q[[0, 2]]).all()
    # the zeros are one value
    vz = np.zeros((1, 4, 1), dtype=np.float32)
    vz[0, 1, 0] = -0.0
    r = sa.weighted_quantiles(vz, None, [0.5], cuda=False)
    assert r.q[0, 0, 0] == 0.0 and r.lower[0, 0, 0] == 0.0 and r.upper[0, 0, 0] == 0.0


def test_arguments():
    v = qu.values(1, 8, 1, seed=1)
    for lv in ([], [0.0], [1.0], [0.5, np.nan], [-0.1], np.linspace(0.01, 0.99, 33)):
        with pytest.raises(ValueError):
            sa.weighted_quantiles(v, None, lv, cuda=False)
    with pytest.raises(ValueError):
        sa.weighted_quantiles(v, np.ones((1, 7)), [0.5], cuda=False)
    with pytest.raises(ValueError):
        sa.weighted_quantiles(v[0, :, 0], None, [0.5], cuda=False)
    # trailing dimensions are kept, and any k is taken
    r = sa.weighted_quantiles(qu.values(2, 20000, 6, seed=2).reshape(2, 20000, 2, 3), None, [0.5, 0.9], cuda=False)
    assert r.q.shape == r.lower.shape == r.upper.shape == (2, 2, 2, 3) and r.status.shape == (2,)


@pytest.fixture(scope="module")
def shadowed():
    ds = syn.dataset(64, 256, 0)
    q = syn.rolling_queries(3, 20, 1)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20))
    d, paths, _ = obj.shadow(q, k=64)
    return obj, q, d, paths


@pytest.mark.parametrize("proba_name,eta", (("softmax", 0.2), ("uniform", None)))
def test_path_shadowing_methods_equal_the_twin_on_shadows_output(shadowed, proba_name, eta):
    obj, q, d, paths = shadowed
    stat = lambda x: sa.realized_variance(x[:, :, 0, :], [5, 10, 20])     # noqa: E731
    vals = stat(obj.context.select_out_context(paths))
    w = None if proba_name == "uniform" else np.asarray(sa.Softmax(d, eta).weights)
    ref = sa.weighted_quantiles(vals, w, qu.LEVELS, cuda=False)
    a = obj.quantiles_from_paths(d, paths, stat, qu.LEVELS, proba_name, eta)
    b = obj.predict_quantiles(q, 64, stat, qu.LEVELS, eta=eta, proba_name=proba_name, cuda=False)
    assert obj.last_quantile_reduction == "host"
    for got in (a, b):
        assert isinstance(got, sa.PredictiveQuantiles) and got.q.shape == (3, len(qu.LEVELS), 3)
        for name in ("levels", "q", "lower", "upper", "status"):
            assert np.array_equal(getattr(got, name), getattr(ref, name)), name


def test_an_averaging_class_without_weights_is_refused(shadowed, monkeypatch):
    obj, q, d, paths = shadowed

    class Opaque:
        def __init__(self, *a):
            pass

    monkeypatch.setattr(type(obj), "init_averaging_proba", staticmethod(lambda name, dist, eta: Opaque()))
    with pytest.raises(TypeError):
        obj.quantiles_from_paths(d, paths, lambda x: sa.realized_variance(x[:, :, 0, :], [5]), [0.5], "softmax", 0.2)


def test_exports():
    import shadowing
    for name in ("weighted_quantiles", "PredictiveQuantiles"):
        assert getattr(shadowing, name) is getattr(sa, name) and name in sa.__all__
    from shadowing_amd import _native
    assert "psh_weighted_quantiles" in _native.EXPORTS and callable(_native.weighted_quantiles)
    assert (_native.PSH_QUANTILE_MAX_LEVELS, _native.PSH_QUANTILE_STATUS_NONFINITE, _native.PSH_QUANTILE_STATUS_WEIGHTS) == \
        (qn.MAX_LEVELS, qn.STATUS_NONFINITE, qn.STATUS_WEIGHTS) == (32, 1, 2)
