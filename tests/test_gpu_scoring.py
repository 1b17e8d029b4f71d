"""psh_score_ensemble on the MI355X against the numpy twin within the bounds of tests/_scoring.py (crps 8 (k + 4) 2^-53 span,
pit 2 (k + 2) 2^-53, mean 2 (k + 2) 2^-53 sum w |x| / W).  Sizes where the geometry changes: the three capacities (1024, 4096,
16384 entries), power-of-two padding, one entry against two a thread, a ragged last chunk.  Weight patterns that leave
whole chunks empty, every placement of the observation, ties, signed zeros, non-finite values without weight, every status
case, the bit guarantees, and PathShadowing.score() end to end."""
import functools

import numpy as np
import pytest
import torch

import _scoring as sc
import shadowing_amd as sa
from shadowing_amd import _native, scoring, synthetic as syn

pytestmark = pytest.mark.gpu

KS = (1, 2, 17, 255, 256, 257, 1024, 1025, 4096, 4097, 16384)
FIELDS = ("crps", "pit_lo", "pit_hi", "mean")
B, M = 5, 3


def threads_of(k):
    return 256 if k <= 1024 else 512 if k <= 4096 else 1024


def device_call(v, w, y, dev):
    vt = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
    yt = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(dev)
    wt = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(dev)
    return tuple(t.cpu().numpy() for t in _native.score_ensemble(vt, wt, yt))


@functools.lru_cache(maxsize=None)
def case(k):
    """(values (5, k, 3), weights (7, 5, k), obs (5, 3), the twin's results) for one k.  Queries: 0 continuous values, 1 and 2
    rounded to one decimal (ties), 2 with a -0.0 / +0.0 pair, 3 with NaN and +-inf at paths no set weighs, 4 continuous.
    Sets: dense random; the cuts k' = 1, k / 2, k - 1 (the first k' paths); only the paths of smallest and largest value (of
    column 0): every chunk between them is empty; one weighted path; only paths that sort (in column 0) into the last
    non-empty chunk of the sorted order.  Observations, column by column in turn: below every value, above every value,
    equal to path 0 (weighted by every cut), equal to path k - 1 (weightless in every cut), between two values, equal to
    the most frequent value of the column (a tied group where the values are rounded)."""
    g = np.random.default_rng(1000 + k)
    v = sc.values(B, k, M, seed=k)
    v[1:3] = np.round(v[1:3], 1)
    if k >= 4:
        v[2, 1, :], v[2, 3, :] = -0.0, 0.0
    poisoned = [k - 2] if k >= 4 else []
    for j in poisoned:
        v[3, j, 0], v[3, j, 1], v[3, j, 2] = np.nan, np.inf, -np.inf
    w = np.zeros((7, B, k))
    w[0] = 0.05 + g.random((B, k))
    for e, kc in ((1, 1), (2, max(1, k // 2)), (3, max(1, k - 1))):
        w[e, :, :kc] = np.exp(-3.0 * g.random((B, kc)))
    chunk = -(-k // threads_of(k))
    for b in range(B):
        col0 = np.where(np.isfinite(v[b, :, 0]), v[b, :, 0], 0.0)
        order = np.argsort(col0, kind="stable")
        w[4, b, order[0]], w[4, b, order[-1]] = 0.25, 0.5
        w[5, b, k // 3] = 0.75
        tail = order[((k - 1) // chunk) * chunk:]
        w[6, b, tail] = 0.1 + g.random(len(tail))
    w[:, 3, poisoned] = 0.0
    assert (w.sum(axis=2) > 0).all()
    y = np.zeros((B, M), dtype=np.float32)
    for b in range(B):
        for i in range(M):
            x = v[b, :, i][np.isfinite(v[b, :, i])]
            vals, counts = np.unique(x, return_counts=True)
            srt = np.sort(x)
            y[b, i] = (srt[0] - 1.0, srt[-1] + 1.0, v[b, 0, i], v[b, k - 1, i], 0.5 * (float(srt[len(srt) // 2]) + float(srt[-1])) + 1e-3,
                       vals[counts.argmax()])[(b * M + i) % 6]
    return v, w, y, sc.twin(v, w, y)


SHARES = {}


@pytest.mark.parametrize("k", KS)
def test_every_pattern_and_placement_against_the_twin(hip_device, k):
    v, w, y, ref = case(k)
    got = device_call(v, w, y, hip_device)                        # B = 5, m = 3, E = 7
    assert not ref[4].any()
    share = sc.assert_within_bounds(got, ref, v, w, y)
    five = device_call(v, w[:5], y, hip_device)                   # E = 5
    for a, c in zip(five, got):
        assert np.array_equal(a, c[:5], equal_nan=True)
    # B = 1, m = 1: NULL weights, and one set of weights
    v1, y1 = np.ascontiguousarray(v[:1, :, :1]), y[:1, :1]
    sc.assert_within_bounds(device_call(v1, None, y1, hip_device), sc.twin(v1, None, y1), v1, None, y1)
    unit, ones = device_call(v1, None, y1, hip_device), device_call(v1, np.ones((1, 1, k)), y1, hip_device)
    for a, c in zip(unit, ones):
        assert np.array_equal(a, c)
    w1 = w[:1, :1]
    got1 = device_call(v1, w1, y1, hip_device)
    sc.assert_within_bounds(got1, sc.twin(v1, w1, y1), v1, w1, y1)
    for n in range(4):                                            # a column's bits do not depend on B, m or E
        assert got1[n][0, 0, 0] == got[n][0, 0, 0]
    for name, s in share.items():
        SHARES[name] = max(SHARES.get(name, 0.0), s)
    print("largest share of the bounds so far:", {n: round(s, 4) for n, s in SHARES.items()})


@pytest.mark.parametrize("k", (257, 4097, 16384))
def test_identical_bits(hip_device, k):
    v, w, y, _ = case(k)
    a = device_call(v, w[:5], y, hip_device)
    b = device_call(v, w[:5], y, hip_device)
    scaled = device_call(v, w[:5] * 2.0 ** -7, y, hip_device)
    for x, x2, x3 in zip(a[:4], b[:4], scaled[:4]):
        assert np.array_equal(x.view(np.uint64), x2.view(np.uint64)) and np.array_equal(x.view(np.uint64), x3.view(np.uint64))
    s = 2                                                         # one set alone, first and last of five
    alone = device_call(v, w[s:s + 1], y, hip_device)
    first = device_call(v, w[[s, 0, 1, 3, 4]], y, hip_device)
    last = device_call(v, w[[0, 1, 3, 4, s]], y, hip_device)
    for n in range(4):
        bits = a[n][s].view(np.uint64)
        assert np.array_equal(alone[n][0].view(np.uint64), bits) and np.array_equal(first[n][0].view(np.uint64), bits)
        assert np.array_equal(last[n][4].view(np.uint64), bits)


def test_bits_do_not_depend_on_the_grid(hip_device):
    """20 queries x 3 columns x 7 sets: few enough columns that the sets are split into groups of two (the last group holds
    one); the first five queries alone, and one query alone: one set a group."""
    k = 257
    v, w, y, _ = case(k)
    V, Wt, Y = np.concatenate([v] * 4), np.concatenate([w] * 4, axis=1), np.concatenate([y] * 4)
    big = device_call(V, Wt, Y, hip_device)
    small = device_call(v, w, y, hip_device)
    single = device_call(np.ascontiguousarray(v[4:5]), w[:, 4:5], y[4:5], hip_device)
    for n in range(4):
        for rep in range(4):
            assert np.array_equal(big[n][:, 5 * rep:5 * rep + 5].view(np.uint64), small[n].view(np.uint64))
        assert np.array_equal(single[n][:, 0].view(np.uint64), small[n][:, 4].view(np.uint64))
    assert not big[4].any()


@pytest.mark.parametrize("k", (17, 4097))
def test_status_cases(hip_device, k):
    v, w, y, _ = case(k)
    W, NF, OBS = scoring.STATUS_WEIGHTS, scoring.STATUS_NONFINITE, scoring.STATUS_OBS

    def run(v1, w1, y1):
        got, ref = device_call(v1, w1, y1, hip_device), sc.twin(v1, w1, y1)
        sc.assert_within_bounds(got, ref, v1, w1, y1)             # equal status, NaN in the same places, the rest in bounds
        return got

    def untouched(got, mask):
        for n in range(4):
            assert np.isnan(got[n][mask]).all() and np.isfinite(got[n][~mask]).all()
            assert np.array_equal(got[n][~mask], base[n][~mask])  # the other sets and columns: not a bit moves

    base = device_call(v, w, y, hip_device)
    for bad in (np.nan, np.inf, -np.inf):                         # a non-finite value at a positive weight: its column
        v1 = v.copy()
        v1[1, 0, 2] = bad                                         # path 0: weighed by sets 0 .. 3, not by 4 .. 6 here
        sets = w[:, 1, 0] > 0
        got = run(v1, w, y)
        mask = np.zeros(base[0].shape, dtype=bool)
        mask[sets, 1, 2] = True
        assert sets[:4].all() and got[4][:, 1].tolist() == [NF if s else 0 for s in sets] and got[4].sum() == NF * sets.sum()
        untouched(got, mask)
    for bad in (np.nan, np.inf, -1e-3):                           # a bad weight: all of (e, b)
        w1 = w.copy()
        w1[2, 4, k // 2] = bad
        got = run(v, w1, y)
        mask = np.zeros(base[0].shape, dtype=bool)
        mask[2, 4, :] = True
        assert got[4][2, 4] == W and got[4].sum() == W
        untouched(got, mask)
    w1 = w.copy()
    w1[5, 0, :] = 0.0                                             # W = 0
    got = run(v, w1, y)
    mask = np.zeros(base[0].shape, dtype=bool)
    mask[5, 0, :] = True
    assert got[4][5, 0] == W and got[4].sum() == W
    untouched(got, mask)
    for bad in (np.nan, np.inf, -np.inf):                         # a non-finite observation: its column, every set
        y1 = y.copy()
        y1[3, 1] = bad
        got = run(v, w, y1)
        mask = np.zeros(base[0].shape, dtype=bool)
        mask[:, 3, 1] = True
        assert (got[4][:, 3] == OBS).all() and got[4].sum() == 7 * OBS
        untouched(got, mask)
    y1, w1 = y.copy(), w.copy()                                   # ... and bad weights beside it still say so
    y1[0, :], w1[1, 0, 0] = np.nan, np.nan
    got = run(v, w1, y1)
    assert got[4][:, 0].tolist() == [OBS, OBS | W] + [OBS] * 5


def test_routing_of_score_ensemble(hip_device):
    v, w, y, _ = case(257)
    ref = sa.score_ensemble(v, w, y, cuda=False)
    up = sa.score_ensemble(v, w, y, cuda=True)                    # numpy in, uploaded
    auto = sa.score_ensemble(torch.from_numpy(v).to(hip_device).reshape(B, 257, M, 1), torch.from_numpy(w[1]), y.reshape(B, M, 1))
    assert up.crps.shape == (7, B, M) and up.status.shape == (7, B) and auto.crps.shape == (B, M, 1) and auto.status.shape == (B,)
    assert np.allclose(up.crps, ref.crps, rtol=1e-12, atol=1e-13) and np.array_equal(auto.crps[..., 0], up.crps[1])
    with pytest.raises(_native.NativeLibraryError):
        sa.score_ensemble(np.zeros((1, 16385, 1), dtype=np.float32), None, np.zeros((1, 1), dtype=np.float32), cuda=True)


def test_score_end_to_end(hip_device):
    ds = syn.dataset(64, 256, 0)
    q = syn.rolling_queries(5, 20, 1)
    x_real = (0.01 * np.random.default_rng(3).standard_normal((5, 1, 20))).astype(np.float32)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20))
    seen = []

    def stat(x):
        out = sa.realized_variance(x[:, :, 0, :], [5, 20])
        seen.append(out)
        return out

    etas, ks = [0.05, 0.1, 0.5], [32, 128]
    got = obj.score(q, x_real, 128, stat, etas, ks, cuda=True, device_predict=True)
    assert obj.last_score_reduction == "device" and obj.last_path == "hip"
    assert len(seen) == 2 and all(s.is_cuda for s in seen) and tuple(seen[0].shape) == (5, 128, 2) and tuple(seen[1].shape) == (5, 1, 2)
    assert got.crps.shape == (3, 2, 5, 2) and got.status.shape == (3, 2, 5) and not got.status.any()
    assert got.etas == (0.05, 0.1, 0.5) and got.ks == (32, 128)
    # the device's own statistic and distances, scored by the twin: within the bounds
    d, _, _ = obj.shadow(q, 128, cuda=True)
    w, _, _ = obj._score_weights("softmax", d, etas, ks)
    v, y = seen[0].cpu().numpy(), seen[1][:, 0].cpu().numpy()
    flat = tuple(getattr(got, n).reshape((6,) + getattr(got, n).shape[2:]) for n in FIELDS + ("status",))
    sc.assert_within_bounds(flat, sc.twin(v, w, y), v, w, y)
    host = obj.score(q, x_real, 128, stat, etas, ks, cuda=False)
    assert obj.last_score_reduction == "host"
    for name in FIELDS:
        assert np.allclose(getattr(got, name), getattr(host, name), rtol=1e-4, atol=1e-9), name
    assert all(np.array_equal(a, c) for a, c in zip(got.best(), host.best()))
