"""psh_weighted_quantiles on the MI355X against the numpy twin under the comparison rule of tests/_quantiles.py: q equal with
== off the edges the twin reports, the tail means within 2 (k + 2) 2^-53 (sum w |x| + W |q|) / t (or / (W - t)).  Sizes: the
small k, each capacity boundary of the three instantiations (1024, 4096, 16384 entries) and the boundary + 1, one and 32
levels; then every kind of input that can upset a sort or a scan, every status case, and predict_quantiles() end to end."""
import functools

import numpy as np
import pytest
import torch

import _quantiles as qu
import shadowing_amd as sa
from shadowing_amd import _native, quantiles as qn, synthetic as syn

pytestmark = pytest.mark.gpu

KS = (1, 2, 63, 64, 65, 1024, 1025, 4096, 4097, 16384)
MS = (1, 3, 5)


def device_call(v, w, levels, dev):
    vt = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
    wt = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(dev)
    return tuple(t.cpu().numpy() for t in _native.weighted_quantiles(vt, wt, levels))


@functools.lru_cache(maxsize=None)
def generic(k, m):
    return qu.values(3, k, m, seed=100 + k), qu.softmax_weights(3, k, seed=100 + k)


@pytest.mark.parametrize("n,k", list(enumerate(KS)))
def test_generic_values_with_ties(hip_device, n, k):
    m = MS[n % 3]
    v, w = generic(k, m)
    levels = qu.LEVELS32 if n % 2 else qu.LEVELS[3:4]             # Q = 32 and Q = 1 in turn
    qu.assert_matches_twin(device_call(v, w, levels, hip_device), v, w, levels, max_edges=0)
    if k in (65, 1025, 16384):                                    # and the seven everyday levels at each instantiation
        qu.assert_matches_twin(device_call(v, w, qu.LEVELS, hip_device), v, w, qu.LEVELS, max_edges=0)


@pytest.mark.parametrize("n,k", list(enumerate(KS)))
def test_unit_weights_are_exact_everywhere(hip_device, n, k):
    m = MS[(n + 1) % 3]
    v, _ = generic(k, m)
    got = device_call(v, None, qu.LEVELS32, hip_device)
    q, lo, up, st, det = qu.twin(v, None, qu.LEVELS32)
    assert np.array_equal(got[0], q) and not got[3].any()         # C_i = i + 1 exactly: no edge can move i*
    xs = np.sort(v.astype(np.float64), axis=1)
    assert np.array_equal(got[0], xs[:, np.ceil(qu.LEVELS32 * k).astype(int) - 1, :])
    assert (np.abs(got[1] - lo) <= det["bound_lower"]).all() and (np.abs(got[2] - up) <= det["bound_upper"]).all()


def kinds(k, m):
    g = np.random.default_rng(k)
    v, w = generic(k, m)
    v, w = v[:2], w[:2]
    asc = np.sort(v, axis=1)
    one = np.zeros_like(w)
    one[:, k // 3] = 0.75
    half = w.copy()
    half[:, ::2] = 0.0
    if k == 1:
        half = w.copy()
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1e-30], dtype=np.float32)
    den = tiny[g.integers(0, len(tiny), size=v.shape)]
    return {"all equal": (np.full_like(v, 0.375), w), "ascending": (asc, w), "descending": (asc[:, ::-1].copy(), w),
            "one path holds the weight": (v, one), "half the weights zero": (v, half),
            "unnormalised": (v, 1234.5 * w), "denormals and zeros": (den, w)}


@pytest.mark.parametrize("k", (1, 2, 65, 1024, 1025, 4097, 16384))
def test_kinds_of_input(hip_device, k):
    m = 3
    for name, (v, w) in kinds(k, m).items():
        print(name)
        qu.assert_matches_twin(device_call(v, w, qu.LEVELS, hip_device), v, w, qu.LEVELS)


@pytest.mark.parametrize("k", (65, 1025, 16384))
def test_two_calls_and_scaled_weights_give_identical_bits(hip_device, k):
    v, w = generic(k, 3)
    a = device_call(v, w, qu.LEVELS32, hip_device)
    b = device_call(v, w, qu.LEVELS32, hip_device)
    c = device_call(v, 4.0 * w, qu.LEVELS32, hip_device)
    for x, y, z in zip(a[:3], b[:3], c[:3]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)) and np.array_equal(x.view(np.uint64), z.view(np.uint64))


@pytest.mark.parametrize("k", (65, 4097))
def test_status_cases(hip_device, k):
    v, w = generic(k, 3)
    v, w = v.copy(), w.copy()
    w[1, 7] = 0.0                                                 # a NaN / inf at a zero-weight path: results stay finite
    v[1, 7, 0], v[1, 7, 2] = np.nan, -np.inf
    got = device_call(v, w, qu.LEVELS, hip_device)
    assert not got[3].any() and all(np.isfinite(a).all() for a in got[:3])
    qu.assert_matches_twin(got, v, w, qu.LEVELS)
    for bad in (np.nan, np.inf, -np.inf):                         # a non-finite value at a positive weight: its column
        v1 = v.copy()
        v1[2, k - 1, 1] = bad
        got = device_call(v1, w, qu.LEVELS, hip_device)
        assert got[3].tolist() == [0, 0, qn.STATUS_NONFINITE]
        assert np.isnan(got[0][2, :, 1]).all() and np.isfinite(got[0][2, :, ::2]).all()
        qu.assert_matches_twin(got, v1, w, qu.LEVELS)
    for bad in (np.nan, np.inf, -1e-3):                           # a bad weight: the query
        w1 = w.copy()
        w1[0, k // 2] = bad
        got = device_call(v, w1, qu.LEVELS, hip_device)
        assert got[3].tolist() == [qn.STATUS_WEIGHTS, 0, 0] and all(np.isnan(a[0]).all() for a in got[:3])
        qu.assert_matches_twin(got, v, w1, qu.LEVELS)
    w1 = w.copy()
    w1[2] = 0.0                                                   # W = 0
    got = device_call(v, w1, qu.LEVELS, hip_device)
    assert got[3].tolist() == [0, 0, qn.STATUS_WEIGHTS] and all(np.isnan(a[2]).all() for a in got[:3])
    qu.assert_matches_twin(got, v, w1, qu.LEVELS)


def test_routing_of_weighted_quantiles(hip_device):
    v, w = generic(65, 3)
    ref = sa.weighted_quantiles(v, w, qu.LEVELS, cuda=False)
    up = sa.weighted_quantiles(v, w, qu.LEVELS, cuda=True)        # numpy in, uploaded
    auto = sa.weighted_quantiles(torch.from_numpy(v).to(hip_device).reshape(3, 65, 3, 1), torch.from_numpy(w), qu.LEVELS)
    assert auto.q.shape == (3, len(qu.LEVELS), 3, 1)
    for r in (up, auto):
        assert np.array_equal(r.q.reshape(ref.q.shape), ref.q) and np.array_equal(r.status, ref.status)
        assert np.allclose(r.lower.reshape(ref.q.shape), ref.lower, rtol=1e-13, atol=1e-13)
    with pytest.raises(_native.NativeLibraryError):
        sa.weighted_quantiles(np.zeros((1, 16385, 1), dtype=np.float32), None, [0.5], cuda=True)


def test_predict_quantiles_end_to_end(hip_device):
    ds = syn.dataset(64, 256, 0)
    q = syn.rolling_queries(3, 20, 1)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20))
    seen = []

    def stat(x):
        out = sa.realized_variance(x[:, :, 0, :], [5, 10, 20])
        seen.append(out)
        return out

    got = obj.predict_quantiles(q, 64, stat, qu.LEVELS, eta=0.2, cuda=True, device_predict=True)
    assert obj.last_quantile_reduction == "device" and obj.last_path == "hip"
    assert len(seen) == 1 and seen[0].is_cuda and tuple(seen[0].shape) == (3, 64, 3)
    d, _, _ = obj.shadow(q, 64, cuda=True)
    w = np.ascontiguousarray(sa.Softmax(d, 0.2).weights, dtype=np.float64)
    qu.assert_matches_twin((got.q, got.lower, got.upper, got.status), seen[0].cpu().numpy(), w, qu.LEVELS, max_edges=0)
    host = obj.predict_quantiles(q, 64, stat, qu.LEVELS, eta=0.2, cuda=False)
    assert obj.last_quantile_reduction == "host"
    for name in ("q", "lower", "upper"):
        assert np.allclose(getattr(got, name), getattr(host, name), rtol=1e-5, atol=0.0), name
