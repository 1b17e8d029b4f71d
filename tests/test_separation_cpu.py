"""Time-separated nearest windows on the host (no GPU needed): the numpy twin of psh_separate_topk against a brute-force greedy
walk over ALL windows of small ensembles, the properties include/psh.h states, and the `separation` keyword of PathShadowing
on the generic route."""
import math

import numpy as np
import pytest

import shadowing_amd as sa
from shadowing_amd import _native, separation as sp, synthetic as syn

W, H = 8, 4
DELTAS = (0, 1, 5, 19, 2 ** 31 - 1)


def brute(idx, delta):
    kept = []
    for i, (r, t) in enumerate(idx.tolist()):
        if r >= 0 and not any(idx[j, 0] == r and abs(int(idx[j, 1]) - t) <= delta for j in kept):
            kept.append(i)
    return kept


def expect(d, idx, k, delta):
    """The five outputs from the brute-force walk, query by query."""
    B = d.shape[0]
    od, oi = np.full((B, k), np.inf, np.float32), np.full((B, k, 2), -1, np.int32)
    op, oc = np.full((B, k), -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        kept = brute(idx[b], delta)
        oc[b] = len(kept)
        kept = kept[:k]
        od[b, :len(kept)], oi[b, :len(kept)], op[b, :len(kept)] = d[b, kept], idx[b, kept], kept
    return od, oi, op, oc, (oc < k).astype(np.int32)


def same(got: sp.Separated, want):
    assert got.distances.dtype == np.float32 and got.indices.dtype == got.positions.dtype == np.int32
    assert got.count.dtype == got.status.dtype == np.int32
    for g, w in zip((got.distances.view(np.int32), got.indices, got.positions, got.count, got.status),
                    (want[0].view(np.int32),) + tuple(want[1:])):
        np.testing.assert_array_equal(g, w)


@pytest.fixture(scope="module", params=[(3, 64), (7, 131), (16, 200)], ids=lambda p: f"{p[0]}x{p[1]}")
def full_list(request, oracle_mod):
    """An ensemble, two queries and the oracle's exhaustive list of ALL its windows in the canonical order."""
    R, T = request.param
    ds = syn.dataset(R, T, seed=R)
    q = syn.rolling_queries(2, W, seed=T)
    n = R * (T - W - H + 1)
    d, idx = oracle_mod.scan_topk(ds, q, n, h=H)
    return ds, q, d, idx, n


@pytest.mark.parametrize("delta", DELTAS)
def test_twin_is_the_greedy_walk_over_all_windows(full_list, delta):
    _, _, d, idx, n = full_list
    for k in (1, 5, n):
        same(sa.separate_topk(d, idx, k, delta, cuda=False), expect(d, idx, k, delta))


@pytest.mark.parametrize("delta", (1, 5, 19))
def test_prefix_exactness_every_list_length_with_enough_kept_gives_the_full_answer(full_list, delta):
    _, _, d, idx, n = full_list
    k = 6
    full = sa.separate_topk(d, idx, k, delta, cuda=False)
    assert (full.count >= k).all()
    served = 0
    for K in sorted({k, k + 1, k + 7, 2 * k, 64, n // 3, n // 2, n - 1, n}):
        part = sa.separate_topk(d[:, :K], idx[:, :K], k, delta, cuda=False)
        for b in range(d.shape[0]):
            if part.count[b] >= k:
                served += 1
                for name in ("distances", "indices", "positions"):
                    np.testing.assert_array_equal(getattr(part, name)[b], getattr(full, name)[b])
            else:
                # a short list is a prefix of the answer, then the fill
                c = part.count[b]
                np.testing.assert_array_equal(part.positions[b, :c], full.positions[b, :c])
                assert part.status[b] == sp.STATUS_SHORT and (part.positions[b, c:] == -1).all()
                assert np.isposinf(part.distances[b, c:]).all() and (part.indices[b, c:] == -1).all()
    assert served >= 4


def made_up_list(K, seed):
    """Three rows, times drawn with repeats of neighbours, padding in the middle and at the end, rows and times at both
    ends of int32, NaN and inf among the distances."""
    g = np.random.default_rng(seed)
    idx = np.stack([g.integers(0, 3, K), g.integers(0, K, K)], axis=1).astype(np.int32)
    idx[g.random(K) < 0.1] = -1
    idx[-3:] = -1
    idx[1], idx[2], idx[3], idx[4] = (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 0), (0, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 2)
    _, first = np.unique(idx, axis=0, return_index=True)          # two entries never share (r, t)
    dup = np.ones(K, bool)
    dup[first] = False
    idx[dup] = -1
    d = np.sort(g.random(K)).astype(np.float32)
    d[5], d[6], d[7] = np.nan, np.inf, np.array([0x7fc01234], np.uint32).view(np.float32)[0]
    return d[None], idx[None]


@pytest.mark.parametrize("delta", DELTAS + (2 ** 30,))
def test_properties_of_the_definition(delta):
    d, idx = made_up_list(257, 3)
    K = d.shape[1]
    got = sa.separate_topk(d, idx, K, delta, cuda=False)
    same(got, expect(d, idx, K, delta))
    c = int(got.count[0])
    pos, r, t = got.positions[0, :c], got.indices[0, :c, 0].astype(np.int64), got.indices[0, :c, 1].astype(np.int64)
    assert (np.diff(pos) > 0).all() and (r >= 0).all()                       # list order; padding is never kept
    np.testing.assert_array_equal(got.distances[0, :c].view(np.int32), d[0, pos].view(np.int32))    # bits, NaN payloads too
    for a in range(c):                                                       # kept entries of a row: more than delta apart
        near = (r == r[a]) & (np.abs(t - t[a]) <= delta)
        assert near.sum() == 1
    kept = set(pos.tolist())
    for i in range(K):                                                       # a dropped entry: a kept one of its row before it
        ri, ti = int(idx[0, i, 0]), int(idx[0, i, 1])
        if ri >= 0 and i not in kept:
            assert any(p < i and r[a] == ri and abs(int(t[a]) - ti) <= delta for a, p in enumerate(pos))
    if delta == 0:
        np.testing.assert_array_equal(pos, np.flatnonzero(idx[0, :, 0] >= 0))
    # padding suppresses nothing: the list without it keeps the same windows
    real = idx[0, :, 0] >= 0
    bare = sa.separate_topk(d[:, real], idx[:, real], int(real.sum()), delta, cuda=False)
    assert bare.count[0] == c
    np.testing.assert_array_equal(bare.indices[0, :c], got.indices[0, :c])
    # a query's result does not depend on the others of the call, and two calls agree
    d2, idx2 = made_up_list(257, 4)
    both = sa.separate_topk(np.concatenate([d2, d]), np.concatenate([idx2, idx]), K, delta, cuda=False)
    for name in ("distances", "indices", "positions", "count", "status"):
        a, b = getattr(both, name)[1], getattr(got, name)[0]
        np.testing.assert_array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)


def test_arguments_and_routing():
    d, idx = made_up_list(33, 1)
    for bad in (dict(k=0), dict(k=34), dict(delta=-1), dict(delta=2 ** 31), dict(k=1.5), dict(delta=True)):
        with pytest.raises(ValueError):
            sa.separate_topk(d, idx, **{"k": 4, "delta": 1, **bad}, cuda=False)
    with pytest.raises(ValueError):
        sa.separate_topk(d, idx[:, :-1], 4, 1, cuda=False)
    big = _native.PSH_MAX_K + 1
    with pytest.raises(_native.NativeLibraryError):                          # the device takes K <= PSH_MAX_K; the twin any K
        sa.separate_topk(np.zeros((1, big), np.float32), np.zeros((1, big, 2), np.int32), 4, 1, cuda=True)
    many = np.stack([np.zeros(big, np.int32), np.arange(big, dtype=np.int32)], axis=1)[None]
    got = sa.separate_topk(np.zeros((1, big), np.float32), many, 4, 2, cuda=False)
    np.testing.assert_array_equal(got.positions[0], [0, 3, 6, 9])
    assert got.count[0] == math.ceil(big / 3)
    import torch
    t = sa.separate_topk(torch.from_numpy(d), torch.from_numpy(idx), 4, 1)    # host tensors: the twin, numpy out
    assert isinstance(t.positions, np.ndarray)
    import shadowing
    assert shadowing.separate_topk is sa.separate_topk and shadowing.Separated is sa.Separated


def make(ds, **kw):
    return sa.PathShadowing(sa.Identity(W), sa.RelativeMSE(), ds, sa.PredictionContext(H), **kw)


def test_the_keyword_takes_none_or_a_non_negative_int():
    ds = syn.dataset(3, 64, seed=1)
    for bad in (-1, 1.0, "1", True, 2 ** 31):
        with pytest.raises(ValueError):
            make(ds, separation=bad)
    assert make(ds).separation is None and make(ds, separation=0).separation == 0
    with pytest.raises(ValueError, match="separation"):
        make(ds, separation=3).shadow_async(syn.single_query(W), k=2)


def test_separation_none_changes_no_bit(full_list):
    ds, q, _, _, _ = full_list
    a, b = make(ds).shadow(q, k=9, cuda=False), make(ds, separation=None).shadow(q, k=9, cuda=False)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))
    assert make(ds, separation=None).last_separation is None


@pytest.mark.parametrize("delta", (0, 1, 5))
def test_the_generic_route_is_the_twin_on_an_exhaustive_shadow(full_list, delta):
    ds, q, _, _, n = full_list
    k = 5
    d, paths, idx = make(ds).shadow(q, k=n, cuda=False)
    want = sa.separate_topk(d, idx, k, delta, cuda=False)
    assert (want.count >= k).all()
    obj = make(ds, separation=delta)
    gd, gp, gi = obj.shadow(q, k=k, n_splits=1, cuda=False)
    np.testing.assert_array_equal(gd.view(np.int32), want.distances.view(np.int32))
    np.testing.assert_array_equal(gi, want.indices)
    np.testing.assert_array_equal(gp, np.take_along_axis(paths, want.positions[:, :, None, None].astype(np.int64), axis=1))
    ls = obj.last_separation
    assert ls["delta"] == delta and ls["scans"] >= 1 and (ls["count"] >= k).all() and k <= ls["K"] <= n
    bd, bi = obj.batched_distance(sa.path_shadowing._torch(sa.path_shadowing._dim_array(q)), obj._dataset_tensor(), k, 1, False)
    np.testing.assert_array_equal(bi.numpy(), want.indices)


def test_fewer_than_k_separated_windows_is_a_runtime_error():
    """R = 3 rows of T' = 53 windows, delta = 19: every row keeps at least ceil(53 / 39) = 2 windows and at most
    ceil(53 / 20) = 3, so k = 6 is always served and k = 10 never."""
    ds = syn.dataset(3, 64, seed=2)
    obj = make(ds, separation=19)
    q = syn.single_query(W)
    d, _, idx = obj.shadow(q, k=6, cuda=False)
    assert np.isfinite(d).all() and (idx >= 0).all() and (obj.last_separation["count"] >= 6).all()
    with pytest.raises(RuntimeError, match="fewer than k windows"):
        obj.shadow(q, k=10, cuda=False)
    with pytest.raises(RuntimeError, match="out of range"):
        obj.shadow(q, k=160, cuda=False)
