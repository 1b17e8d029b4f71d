"""psh_separate_topk on the device against its numpy twin, bit for bit on all five outputs (the lists are built on the host,
so the kernel is tested without a scan), and the `separation` keyword of PathShadowing end to end on the native route."""
import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, pricing, synthetic as syn

import _graph_replay as gr

pytestmark = pytest.mark.gpu

DELTAS = (0, 1, 5, 19, 2 ** 30)
TOP = 2 ** 31 - 1
KINDS = ("own_rows", "rising", "falling", "permuted", "two_rows", "extremes", "padding", "few")


def make_list(kind: str, K: int, seed: int):
    """One query's (d (K,), idx (K, 2)): distances ascending with a NaN (one with a payload) and an inf among them."""
    g = np.random.default_rng([seed, K, KINDS.index(kind)])
    i = np.arange(K)
    if kind == "own_rows":                                    # every entry a row of its own
        r, t = g.permutation(K), g.integers(0, 50, K)
    elif kind == "rising":                                    # one row, t rising with the position: the many-rounds case
        r, t = np.full(K, 7), i
    elif kind == "falling":
        r, t = np.full(K, 7), K - 1 - i
    elif kind == "permuted":
        r, t = np.full(K, TOP), g.permutation(K)
    elif kind == "two_rows":                                  # two rows interleaved, three samples between neighbours
        r, t = i % 2, 3 * (i // 2)
    elif kind == "extremes":                                  # rows and times at 2^31 - 1 and 0 in one list
        r = g.choice([0, TOP], K)
        t = g.choice([0, 1, 19, 20, TOP - 20, TOP - 19, TOP - 1, TOP], K)
    elif kind == "padding":                                   # (-1, -1) in the middle and at the end
        r, t = g.integers(0, 4, K), g.integers(0, K + 1, K)
        pad = (g.random(K) < 0.2) | (i >= K - K // 8) | ((i >= K // 3) & (i < K // 3 + K // 16))
        r, t = np.where(pad, -1, r), np.where(pad, -1, t)
    else:                                                     # few separated windows: count < k for most k
        r, t = g.integers(0, 2, K), g.integers(0, 41, K)
    d = np.sort(g.random(K)).astype(np.float32)
    if K >= 3:
        d[-1], d[-2] = np.array([0x7fc01234], np.uint32).view(np.float32)[0], np.inf
        d[K // 2] = np.nan
    return d, np.stack([r, t], axis=1).astype(np.int32)


def batch(K: int, B: int, first: int = 0):
    """B lists, query b of kind (first + b) mod 8."""
    parts = [make_list(KINDS[(first + b) % len(KINDS)], K, b) for b in range(B)]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def on_device(dev, d, idx, k, delta):
    out = _native.separate_topk(torch.from_numpy(d).to(dev), torch.from_numpy(idx).to(dev), k, delta)
    return [t.cpu().numpy() for t in out]


def assert_prefix_of(got, full: sa.Separated, k: int, what):
    """The device's five outputs at k against the twin's at k = K: the first k columns, the same count, SHORT below k."""
    gd, gi, gp, gc, gs = got
    assert gd.dtype == np.float32 and gi.dtype == gp.dtype == gc.dtype == gs.dtype == np.int32, what
    assert np.array_equal(gd.view(np.int32), full.distances[:, :k].view(np.int32)), what
    assert np.array_equal(gi, full.indices[:, :k]) and np.array_equal(gp, full.positions[:, :k]), what
    assert np.array_equal(gc, full.count) and np.array_equal(gs, (full.count < k).astype(np.int32)), what


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 1023, 1025, 4096, 16384])
def test_device_is_the_twin_bit_for_bit(hip_device, K):
    calls = [(B, 0) for B in (1, 3, 300)] if K <= 1025 else [(2, first) for first in (0, 2, 4, 6)]
    saw_short = saw_fill = False
    for B, first in calls:
        d, idx = batch(K, B, first)
        if B == 1:
            d, idx = batch(K, 1, 6)                           # (the one query: the list with padding)
        for j, delta in enumerate(DELTAS):
            full = sa.separate_topk(d, idx, K, delta, cuda=False)
            # (the long lists: one k a delta, so the many-rounds case -- "rising" at delta = 1, K = 16384 -- runs once)
            for k in sorted({1, (K + 1) // 2, K}) if K <= 1025 else [(K, (K + 1) // 2, 1, K, 1)[j]]:
                got = on_device(hip_device, d, idx, k, delta)
                assert_prefix_of(got, full, k, (K, B, first, delta, k))
                saw_short |= bool(got[4].any())
                saw_fill |= bool((got[2] == -1).any() and np.isposinf(got[0][got[2] == -1]).all())
    assert K == 1 or (saw_short and saw_fill)                 # lists with count < k were among them


def test_two_calls_and_a_query_alone_give_the_same_bits(hip_device):
    d, idx = batch(1025, 300)
    for delta in (1, 19):
        a = on_device(hip_device, d, idx, 400, delta)
        b = on_device(hip_device, d, idx, 400, delta)
        alone = on_device(hip_device, d[137:138], idx[137:138], 400, delta)
        for x, y, z in zip(a, b, alone):
            x, y, z = (v.view(np.int32) for v in (x, y, z))
            assert np.array_equal(x, y) and np.array_equal(x[137:138], z)


def test_the_entry_replays_from_a_captured_graph(hip_device):
    d, idx = batch(1025, 3, 1)
    dd, di = torch.from_numpy(d).to(hip_device), torch.from_numpy(idx).to(hip_device)
    torch.cuda.synchronize(hip_device)
    eager = gr.snapshot(gr.flatten(_native.separate_topk(dd, di, 300, 5)))
    s = torch.cuda.Stream(hip_device)
    with torch.cuda.stream(s):
        g, out = gr.capture(lambda: _native.separate_topk(dd, di, 300, 5))
    for t in out:
        t.fill_(-7)
    gr.replay(g, hip_device)
    gr.assert_same_bits(gr.flatten(out), eager, "psh_separate_topk replayed")
    want = sa.separate_topk(d, idx, 300, 5, cuda=False)
    assert np.array_equal(out[2].cpu().numpy(), want.positions) and np.array_equal(out[3].cpu().numpy(), want.count)


def test_the_functional_interface_routes_to_the_device(hip_device):
    d, idx = batch(65, 3)
    want = sa.separate_topk(d, idx, 20, 5, cuda=False)
    for got in (sa.separate_topk(torch.from_numpy(d).to(hip_device), torch.from_numpy(idx).to(hip_device), 20, 5),
                sa.separate_topk(d, idx, 20, 5, cuda=True)):
        assert isinstance(got, sa.Separated) and got.positions.is_cuda
        assert np.array_equal(got.positions.cpu().numpy(), want.positions)
        assert np.array_equal(got.distances.cpu().numpy().view(np.int32), want.distances.view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- end to end
KK, DELTA = 256, 19
SMRW = dict(K0=0.1, alpha=0.6, lam=0.2, seed=1)
_ENSEMBLES = {}


def ensemble(R, T, channels=1):
    """The SMRW twin's rows, generated once; a second channel is a second draw."""
    key = (R, T, channels)
    if key not in _ENSEMBLES:
        chans = [sa.smrw_log_returns(R, T, **{**SMRW, "seed": 1 + c}) for c in range(channels)]
        ds = np.ascontiguousarray(np.concatenate(chans, axis=1))
        ds.setflags(write=False)
        _ENSEMBLES[key] = ds
    return _ENSEMBLES[key]


def configuration(name, ds):
    if name == "identity":
        return sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(20), separation=DELTA), 20, 20
    if name == "foveal":
        return sa.PathShadowing(sa.Foveal(alpha=1.4, beta=0.9, max_context=40), sa.RelativeMSE(), ds, sa.PredictionContext(20),
                                separation=DELTA), 40, 20
    return sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.CrossChannelContext(1), separation=DELTA), 20, 0


def exhaustive_list(oracle_mod, obj, name, ds, q, W, h):
    n = ds.shape[0] * (ds.shape[-1] - W - h + 1)
    if name == "foveal":
        hx = obj.embedding(torch.tensor(q)[:, None, :])[:, 0, :].numpy()
        return oracle_mod.scan_topk_embedded(ds[:, 0, :], obj.embedding.kernel[:, 0, :].numpy(), hx, n, h=h)
    return oracle_mod.scan_topk(ds[:, 0, :], q, n, h=h)


@pytest.mark.parametrize("shape", [(64, 256), (16, 1024)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["identity", "foveal", "cross_channel"])
def test_shadow_with_the_keyword_is_the_twin_on_the_exhaustive_list(hip_device, oracle_mod, name, shape):
    ds = ensemble(*shape, channels=2 if name == "cross_channel" else 1)
    obj, W, h = configuration(name, ds)
    for B in (1, 5):
        q = (syn.rolling_queries(B, W, 3 + B) * np.float32(3.0)).astype(np.float32)
        d, idx = exhaustive_list(oracle_mod, obj, name, ds, q, W, h)
        want = sa.separate_topk(d, idx, KK, DELTA, cuda=False)
        assert (want.count >= KK).all()
        gd, gp, gi = obj.shadow(q, k=KK, cuda=True)
        assert obj.last_path == "hip"
        assert np.array_equal(gd.view(np.int32), want.distances.view(np.int32)) and np.array_equal(gi, want.indices)
        r, t = gi[..., 0].astype(np.int64), gi[..., 1].astype(np.int64)
        paths = ds[r[..., None], :, t[..., None] + np.arange(W + h)]            # (B, k, W + h, C)
        assert np.array_equal(gp, np.moveaxis(paths, -1, -2))
        ls = obj.last_separation
        assert ls["delta"] == DELTA and ls["scans"] >= 1 and KK < ls["K"] <= _native.PSH_MAX_K and (ls["count"] >= KK).all()
        bd, bi = obj.batched_distance(torch.tensor(q)[:, None, :], obj._dataset_tensor(), KK, 1, True)
        assert np.array_equal(bi.numpy(), want.indices) and np.array_equal(bd.numpy().view(np.int32), gd.view(np.int32))


def test_a_short_start_is_doubled_and_every_list_length_gives_the_same_answer(hip_device, oracle_mod):
    """The query is chosen on the CPU so that the start K1 = k + max(64, k // 4) keeps fewer than k and 2 K1 keeps enough."""
    ds = ensemble(64, 256)
    obj, W, h = configuration("identity", ds)
    q = (syn.rolling_queries(1, W, 2) * np.float32(3.0)).astype(np.float32)
    d, idx = exhaustive_list(oracle_mod, obj, "identity", ds, q, W, h)
    K1 = KK + max(64, KK // 4)
    count = lambda K: int(sa.separate_topk(d[:, :K], idx[:, :K], KK, DELTA, cuda=False).count[0])   # noqa: E731
    assert count(K1) < KK <= count(2 * K1)
    want = sa.separate_topk(d, idx, KK, DELTA, cuda=False)
    gd, _, gi = obj.shadow(q, k=KK, cuda=True)
    assert obj.last_path == "hip" and obj.last_separation["scans"] >= 2 and obj.last_separation["K"] == 2 * K1
    assert np.array_equal(gd.view(np.int32), want.distances.view(np.int32)) and np.array_equal(gi, want.indices)
    # prefix exactness on the device: every list length that keeps k gives these bits
    plain = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(20))
    for K in (2 * K1, 3 * K1, 4096, 13888):
        ld, _, li = plain.shadow(np.concatenate([q, q]), k=K, cuda=True)       # (two queries: not the one-query slot)
        got = sa.separate_topk(ld, li, KK, DELTA, cuda=True)
        assert np.array_equal(got.indices.cpu().numpy()[0], want.indices[0]), K
        assert np.array_equal(got.distances.cpu().numpy()[0].view(np.int32), want.distances[0].view(np.int32)), K


def test_an_ensemble_with_fewer_than_k_separated_windows(hip_device, oracle_mod):
    """3 rows of 53 windows, delta = 19: every row keeps 2 or 3.  k = 6 is served natively at the last list length (all 159
    windows); k = 10 is short there too, goes to the generic formulation and raises as it does on the host."""
    ds = syn.dataset(3, 64, seed=2)
    ds.setflags(write=False)
    obj = sa.PathShadowing(sa.Identity(8), sa.RelativeMSE(), ds, sa.PredictionContext(4), separation=DELTA)
    q = syn.rolling_queries(2, 8, 1)
    d, idx = oracle_mod.scan_topk(ds, q, 159, h=4)
    want = sa.separate_topk(d, idx, 6, DELTA, cuda=False)
    gd, _, gi = obj.shadow(q, k=6, cuda=True)
    assert obj.last_path == "hip" and obj.last_separation["K"] <= 159
    assert np.array_equal(gd.view(np.int32), want.distances.view(np.int32)) and np.array_equal(gi, want.indices)
    with pytest.raises(RuntimeError, match="fewer than k windows"):
        obj.shadow(q, k=10, cuda=True)
    with pytest.raises(RuntimeError, match="out of range"):
        obj.shadow(q, k=160, cuda=True)
    with pytest.raises(ValueError, match="separation"):
        obj.shadow_async(q[0], k=4)


def test_predict_and_smile_with_the_keyword_are_the_kernels_composed_by_hand(hip_device):
    ds = ensemble(64, 256)
    obj, W, h = configuration("identity", ds)
    q = (syn.rolling_queries(5, W, 8) * np.float32(3.0)).astype(np.float32)
    eta = 0.3
    d, paths, _ = obj.shadow(q, k=KK, cuda=True)
    assert obj.last_path == "hip"
    future = obj.context.select_out_context(torch.from_numpy(paths).to(hip_device))
    stat = lambda x: x[:, :, 0, :2].contiguous()                               # noqa: E731  (a pure copy)
    w = sa.softmax_weights(d, [eta], cuda=True)[0, 0]
    got = obj.predict(q, KK, stat, eta=eta, cuda=True, device_predict=True, device_weights=True)
    assert obj.last_weights == "device" and obj.last_path == "hip" and obj.last_separation["delta"] == DELTA
    for a, c in zip(got, _native.weighted_moments(stat(future), w)):
        assert a.shape == (5, 2) and (a == c.cpu().numpy()).all()
    Ts, Ms = [5, 20], [-1.0, 0.0, 1.0]
    sm = obj.smile(q, KK, Ts, Ms, eta=eta, cuda=True, device_weights=True)
    assert obj.last_weights == "device" and obj.last_path == "hip"
    hand = pricing.smile_from_log_returns(future[:, :, 0, :], w, Ts, Ms, 100.0, 0.0, degree=3, kind="otm", cuda=True)
    for name in ("prices", "ivs", "strikes", "sigma", "status"):
        assert np.array_equal(getattr(sm, name), getattr(hand, name), equal_nan=True), name
