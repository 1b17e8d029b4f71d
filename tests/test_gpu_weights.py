"""psh_softmax_weights on the MI355X against its numpy twin, and the four flows of PathShadowing with device_weights=True
against the same kernels composed by hand.

Kernel against twin: |w_dev - w_twin| <= (2 k' + 16) 2^-53 w_twin + 2^-1070.  The arguments of exp are bit-identical on the
two sides (three IEEE operations on an exact square), each exp is within 1 ulp -- what glibc and ROCm's math library document
for double exp -- so the two sides differ by 4 * 2^-53 a term; each sum of k' non-negative terms carries (k' - 1) 2^-53; one
division a side; the absolute term covers subnormal e_j under Z >= 1.  The weights past the cut-off are exactly 0.0 and the
NaN pattern is the twin's.  Sizes: one entry, both sides of a wave, of the three capacities (1024, 4096, 16384 entries) and of
their power-of-two padding; rows ascending (the network is skipped), shuffled, and with ties across every cut-off."""
import functools

import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, pricing, synthetic as syn
from shadowing_amd import weights as W

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KS = (1, 2, 63, 64, 65, 1000, 1024, 1025, 4097, 16384)
ETAS = (0.003, 0.1, 30.0, None)
SHARES = {"kernel": 0.0}


def cuts(k):
    return sorted({1, min(2, k), max(1, k - 1), k})


@functools.lru_cache(maxsize=None)
def case(k, B):
    """{kind: (distances (B, k) float32, the twin's (4, len(cuts), B, k) weights)} for ascending rows, shuffled rows and rows
    of a few levels in shuffled order (equal distances on both sides of every cut-off)."""
    g = np.random.default_rng(100 * k + B)
    asc = np.sort((np.abs(g.standard_normal((B, k))) * 0.1).astype(np.float32), axis=1)
    levels = min(8, max(1, k // 3))
    tied = np.tile((0.05 + 0.3 * np.floor(np.arange(k) * levels / k) / 8).astype(np.float32), (B, 1))
    rows = {"ascending": asc, "shuffled": g.permuted(asc, axis=1), "ties": g.permuted(tied, axis=1)}
    return {kind: (d, W.softmax_weights(d, ETAS, cuts(k), cuda=False)) for kind, d in rows.items()}


def on_device(d, etas, ks, dev):
    return _native.softmax_weights(torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).to(dev), etas, ks).cpu().numpy()


def assert_within_bound(got, ref, d, ks):
    """got, ref (A, C, B, k): zeros past each cut-off on both sides, the twin's NaN pattern, the bound elsewhere; the largest
    share of the bound."""
    order = np.argsort(d, axis=1, kind="stable")
    worst = 0.0
    for c, kc in enumerate(ks):
        past = np.broadcast_to(order[:, kc:], got[:, c].shape[:2] + (d.shape[1] - kc,))
        for x in (got, ref):
            z = np.take_along_axis(x[:, c], past, axis=-1)
            assert (z == 0.0).all() and not np.signbit(z).any(), kc
        g, r = got[:, c], ref[:, c]
        assert np.array_equal(np.isnan(g), np.isnan(r)), kc
        ok = ~np.isnan(r)
        share = np.abs(g[ok] - r[ok]) / ((2 * kc + 16) * U * r[ok] + 2.0 ** -1070)
        worst = max(worst, float(share.max(initial=0.0)))
    return worst


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("k", KS)
def test_kernel_against_the_twin(hip_device, k, B):
    ks = cuts(k)
    for kind, (d, ref) in case(k, B).items():
        got = on_device(d, ETAS, ks, hip_device).reshape(ref.shape)
        share = assert_within_bound(got, ref, d, ks)
        SHARES["kernel"] = max(SHARES["kernel"], share)
        print(f"k = {k}, B = {B}, {kind}: share of the bound {share:.4f}; largest so far {SHARES['kernel']:.4f}")
        assert share <= 1.0, (kind, share)
        uniform = got[3]                                          # eta = None: exactly 1 / k' on the kept paths
        for c, kc in enumerate(ks):
            assert np.array_equal(np.sort(uniform[c], axis=1)[:, k - kc:], np.full((B, kc), 1.0 / kc))


def test_nan_and_inf_as_the_definition_says(hip_device):
    neg_nan = np.array([0xffc00000], dtype=np.uint32).view(np.float32)[0]
    for k in (6, 65, 1030):
        g = np.random.default_rng(k)
        d = (np.abs(g.standard_normal((4, k))) * 0.1).astype(np.float32)
        d[0, [1, 4, 3]] = neg_nan, np.nan, np.inf                 # NaN of either sign behind +inf, by index
        d[1, :] = np.inf                                          # all-inf kept distances: NaN (-inf - -inf)
        d[2, 0], d[2, k // 2] = -0.0, 0.0                         # equal: the lower index first
        d[3, :] = np.sort(d[3])
        d[3, k - 1] = np.nan                                      # an ascending row that ends on a NaN skips the network too
        ks = sorted({1, 2, k - 3, k - 2, k - 1, k})
        ref = W.softmax_weights(d, (0.1, None), ks, cuda=False)
        got = on_device(d, (0.1, None), ks, hip_device).reshape(ref.shape)
        assert assert_within_bound(got, ref, d, ks) <= 1.0
        assert np.isnan(got[0, -1, 0]).all() and np.isnan(got[0, -2, 0]).sum() == k - 1 and np.isfinite(got[0, 2, 0]).all()
        assert np.isnan(got[0, -1, 1]).all() and np.isnan(got[0, 0, 1]).sum() == 1 and np.isnan(got[0, 0, 1, 0])
        assert np.isfinite(got[1]).all() and np.isfinite(got[0, :, 2]).all()
        assert got[0, 0, 2, 0] == 1.0 and got[0, 1, 2, 0] == 0.5 and got[0, 1, 2, k // 2] == 0.5


@pytest.mark.parametrize("k,B", ((1000, 3), (4097, 1), (16384, 2)))
def test_identical_bits_and_sets_that_do_not_see_each_other(hip_device, k, B):
    ks = cuts(k)
    for kind in ("shuffled", "ascending"):
        d, _ = case(k, 3)[kind]
        d = d[:B]
        a = on_device(d, ETAS, ks, hip_device)
        b = on_device(d, ETAS, ks, hip_device)
        assert a.shape == (16, B, k) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        for e in range(16):                                       # a 16-set grid equals 16 one-set calls bit for bit
            alone = on_device(d, [ETAS[e // 4]], [ks[e % 4]], hip_device)
            assert np.array_equal(alone[0].view(np.uint64), a[e].view(np.uint64)), e
    # rows that fill the chip (no split of the sets into groups) against the same rows a few at a time
    d, _ = case(1000, 3)["shuffled"]
    many = np.concatenate([d] * 90)                               # 270 rows
    big = on_device(many, ETAS, cuts(1000), hip_device)
    small = on_device(d, ETAS, cuts(1000), hip_device)
    assert np.array_equal(big[:, :3].view(np.uint64), small.view(np.uint64))
    assert np.array_equal(big[:, 267:].view(np.uint64), small.view(np.uint64))


def test_routing_of_softmax_weights(hip_device):
    d, ref = case(65, 3)["shuffled"]
    up = sa.softmax_weights(d, ETAS, cuts(65), cuda=True)         # numpy in, uploaded; a HIP tensor out
    auto = sa.softmax_weights(torch.from_numpy(d).to(hip_device), ETAS, cuts(65))
    wide = sa.softmax_weights(torch.from_numpy(d.astype(np.float64)).to(hip_device), ETAS, cuts(65), cuda=True)
    host = sa.softmax_weights(torch.from_numpy(d.astype(np.float64)).to(hip_device), ETAS, cuts(65))
    assert up.is_cuda and auto.is_cuda and tuple(up.shape) == ref.shape and up.dtype == torch.float64
    assert torch.equal(up, auto) and torch.equal(up, wide)
    assert isinstance(host, np.ndarray) and np.array_equal(host, ref)
    assert assert_within_bound(up.cpu().numpy(), ref, d, cuts(65)) <= 1.0
    with pytest.raises(_native.NativeLibraryError):
        sa.softmax_weights(np.zeros((1, 16385), dtype=np.float32), [0.1], cuda=True)
    with pytest.raises(ValueError):
        _native.softmax_weights(torch.zeros((2, 8), device=hip_device), [0.1, -1.0])
    with pytest.raises(ValueError):
        _native.softmax_weights(torch.zeros((2, 8), device=hip_device), [0.1], [9])


# ---------------------------------------------------------------------------------------------------------------- the flows
K, ETA = 64, 0.1


def pure_copy(x):
    """A statistic that is a pure copy: bit-identical whichever way the paths were gathered."""
    return x[:, :, 0, :2].contiguous()


@pytest.fixture(scope="module")
def flow(hip_device):
    """The object, its queries, and what the hand compositions start from: shadow(cuda=True)'s distances and the statistic of
    its paths, uploaded again."""
    ds = syn.dataset(64, 256, 0)
    q = syn.rolling_queries(5, 20, 1)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20))
    d, paths, _ = obj.shadow(q, K, cuda=True)
    assert obj.last_path == "hip"
    future = obj.context.select_out_context(torch.from_numpy(paths).to(hip_device))
    return obj, q, d, future


def host_weights(d, eta):
    return np.asarray(sa.Softmax(d.astype(np.float64), eta).weights, dtype=np.float64)


def test_predict_with_device_weights(hip_device, flow):
    obj, q, d, future = flow
    values = pure_copy(future)
    got = obj.predict(q, K, pure_copy, eta=ETA, cuda=True, device_predict=True, device_weights=True)
    assert obj.last_weights == "device" and obj.last_predict_reduction == "device" and obj.last_path == "hip"
    w = sa.softmax_weights(d, [ETA], cuda=True)[0, 0]
    for a, c in zip(got, _native.weighted_moments(values, w)):
        assert a.shape == (5, 2) and (a == c.cpu().numpy()).all()
    uni = obj.predict(q, K, pure_copy, proba_name="uniform", cuda=True, device_predict=True, device_weights=True)
    for a, c in zip(uni, _native.weighted_moments(values, sa.softmax_weights(d, [None], cuda=True)[0, 0])):
        assert (a == c.cpu().numpy()).all()
    # the default call: the host's weights, uploaded
    plain = obj.predict(q, K, pure_copy, eta=ETA, cuda=True, device_predict=True)
    assert obj.last_weights == "host" and obj.last_predict_reduction == "device"
    for a, c in zip(plain, _native.weighted_moments(values, torch.from_numpy(host_weights(d, ETA)).to(hip_device))):
        assert (a == c.cpu().numpy()).all()
    for a, c in zip(got, plain):
        assert np.allclose(a, c, rtol=1e-12, atol=0.0)
    obj.predict(q, K, lambda x: x[:, :, 0, :2], eta=ETA, cuda=True, device_weights=True)         # a numpy statistic: the host route
    assert obj.last_weights == "host"


def test_predict_quantiles_with_device_weights(hip_device, flow):
    obj, q, d, future = flow
    values, levels = pure_copy(future), [0.1, 0.5, 0.9]
    got = obj.predict_quantiles(q, K, pure_copy, levels, eta=ETA, cuda=True, device_predict=True, device_weights=True)
    assert obj.last_weights == "device" and obj.last_quantile_reduction == "device"
    hand = _native.weighted_quantiles(values, sa.softmax_weights(d, [ETA], cuda=True)[0, 0], levels)
    for name, c in zip(("q", "lower", "upper", "status"), hand):
        assert getattr(got, name).shape == tuple(c.shape) and (getattr(got, name) == c.cpu().numpy()).all(), name
    plain = obj.predict_quantiles(q, K, pure_copy, levels, eta=ETA, cuda=True, device_predict=True)
    assert obj.last_weights == "host" and obj.last_quantile_reduction == "device"
    hand = _native.weighted_quantiles(values, torch.from_numpy(host_weights(d, ETA)).to(hip_device), levels)
    for name, c in zip(("q", "lower", "upper", "status"), hand):
        assert (getattr(plain, name) == c.cpu().numpy()).all(), name


def test_score_with_device_weights(hip_device, flow):
    obj, q, d, future = flow
    values = pure_copy(future)
    x_real = (0.01 * np.random.default_rng(3).standard_normal((5, 1, 20))).astype(np.float32)
    obs = pure_copy(torch.from_numpy(x_real).to(hip_device)[:, None])[:, 0].contiguous()
    etas, ks = [0.05, ETA, None], [16, K]
    got = obj.score(q, x_real, K, pure_copy, etas, ks, cuda=True, device_predict=True, device_weights=True)
    assert obj.last_weights == "device" and obj.last_score_reduction == "device"
    assert got.etas == (0.05, ETA, None) and got.ks == (16, K) and got.crps.shape == (3, 2, 5, 2) and not got.status.any()
    hand = _native.score_ensemble(values, sa.softmax_weights(d, etas, ks, cuda=True).reshape(6, 5, K), obs)
    for name, c in zip(("crps", "pit_lo", "pit_hi", "mean", "status"), hand):
        assert (getattr(got, name).reshape(tuple(c.shape)) == c.cpu().numpy()).all(), name
    plain = obj.score(q, x_real, K, pure_copy, etas, ks, cuda=True, device_predict=True)
    assert obj.last_weights == "host" and obj.last_score_reduction == "device"
    w_host, _, _ = obj._score_weights("softmax", d, etas, ks)
    hand = _native.score_ensemble(values, torch.from_numpy(w_host).to(hip_device), obs)
    for name, c in zip(("crps", "pit_lo", "pit_hi", "mean", "status"), hand):
        assert (getattr(plain, name).reshape(tuple(c.shape)) == c.cpu().numpy()).all(), name
    with pytest.raises(ValueError):
        obj.score(q, x_real, K, pure_copy, [0.0], ks, cuda=True, device_predict=True, device_weights=True)
    with pytest.raises(ValueError):
        obj.score(q, x_real, K, pure_copy, etas, [K + 1], cuda=True, device_predict=True, device_weights=True)


def test_score_of_realized_variance_moves_within_the_widened_bounds(hip_device, flow):
    """device_weights=True against False: the README's bounds (crps 8 (k + 4) 2^-53 span, pit 2 (k + 2) 2^-53, mean
    2 (k + 2) 2^-53 sum w |x| / W) widened for weights that carry (2 k + 16) 2^-53 relative error each: crps within
    16 (k + 6) 2^-53 span, pit within 2 (3 k + 18) 2^-53, mean within 2 (3 k + 18) 2^-53 (sum w |x|) / W."""
    obj, q, d, _ = flow
    x_real = (0.01 * np.random.default_rng(3).standard_normal((5, 1, 20))).astype(np.float32)
    seen = []

    def stat(x):
        out = sa.realized_variance(x[:, :, 0, :], [5, 20])
        seen.append(out)
        return out

    etas, ks = [0.05, ETA, 0.5, None], [16, K]
    dev = obj.score(q, x_real, K, stat, etas, ks, cuda=True, device_predict=True, device_weights=True)
    assert obj.last_weights == "device"
    host = obj.score(q, x_real, K, stat, etas, ks, cuda=True, device_predict=True)
    assert obj.last_weights == "host" and not dev.status.any() and not host.status.any()
    v, y = seen[0].cpu().numpy().astype(np.float64), seen[1][:, 0].cpu().numpy().astype(np.float64)       # (5, K, 2), (5, 2)
    w, _, _ = obj._score_weights("softmax", d, etas, ks)
    w = w.reshape(4, 2, 5, K)
    pos = (w > 0)[..., None]
    span = (np.maximum(np.where(pos, v, -np.inf).max(axis=3), y) - np.minimum(np.where(pos, v, np.inf).min(axis=3), y))
    scale = (np.where(pos, np.abs(v), 0.0) * w[..., None]).sum(axis=3) / w.sum(axis=3)[..., None]
    bounds = {"crps": 16 * (K + 6) * U * span, "pit_lo": 2 * (3 * K + 18) * U, "pit_hi": 2 * (3 * K + 18) * U,
              "mean": 2 * (3 * K + 18) * U * scale}
    for name, b in bounds.items():
        share = float((np.abs(getattr(dev, name) - getattr(host, name)) / b).max())
        print(f"score, device_weights=True against False: {name} uses {share:.4f} of its bound")
        assert share <= 1.0, (name, share)


def test_smile_with_device_weights(hip_device, flow):
    obj, q, d, future = flow
    Ts, Ms, eta = [5, 20], [-1.0, 0.0, 1.0], 0.3                  # (at eta = 0.1 two paths carry the weight: the fit is flagged)
    got = obj.smile(q, K, Ts, Ms, eta=eta, cuda=True, device_weights=True)
    assert obj.last_weights == "device" and obj.last_path == "hip"
    hand = pricing.smile_from_log_returns(future[:, :, 0, :], sa.softmax_weights(d, [eta], cuda=True)[0, 0], Ts, Ms, 100.0, 0.0,
                                          degree=3, kind="otm", cuda=True)
    for name in ("prices", "ivs", "strikes", "sigma", "status"):
        assert np.array_equal(getattr(got, name), getattr(hand, name), equal_nan=True), name
    assert np.isfinite(got.prices).all() and not got.status.any()
    plain = obj.smile(q, K, Ts, Ms, eta=eta, cuda=True)
    assert obj.last_weights == "host"
    hand = pricing.smile_from_log_returns(future[:, :, 0, :], torch.from_numpy(host_weights(d, eta)).to(hip_device), Ts, Ms,
                                          100.0, 0.0, degree=3, kind="otm", cuda=True)
    for name in ("prices", "ivs", "strikes", "sigma", "status"):
        assert np.array_equal(getattr(plain, name), getattr(hand, name), equal_nan=True), name
