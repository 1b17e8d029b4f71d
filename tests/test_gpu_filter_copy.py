"""The one-query overlap scan on a resident f16 copy of the ensemble (psh_stream_copy.hip, psh_scan_topk_copy): the copy
only feeds the rejection test, so every result is the fp32 route's and the oracle's, bit for bit.  The "auto" policy builds
the copy on the first eligible call here (monkeypatched); every test checks that the copy scan really served (`served == 1`)."""
import numpy as np
import pytest
import torch

import _boundaries as bd
from _adversarial import make as adversarial
from shadowing_amd import synthetic as syn
from test_gpu_admitted_set import ADVERSARIAL, check_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def built(monkeypatch):
    """Policy "first", and a record of every copy the policy builds (their descriptors say whether the copy scan served)."""
    from shadowing_amd import _native
    made = []

    class Recording(_native.FilterCopy):
        def __init__(self, rows):
            super().__init__(rows)
            made.append(self)

    monkeypatch.setattr(_native, "FILTER_COPY_POLICY", "first")
    monkeypatch.setattr(_native, "_filter_copy_builder", Recording)
    monkeypatch.delenv("PSH_FILTER_COPY", raising=False)
    _native._filter_copies.clear()
    yield made
    _native._filter_copies.clear()


def _exact(d, idx, od, oidx, what):
    assert np.array_equal(d.cpu().numpy().view(np.uint32), od.view(np.uint32)), f"{what}: distances differ from the oracle"
    assert np.array_equal(idx.cpu().numpy(), oidx), f"{what}: indices differ from the oracle"


def _scan(dev, ds, q, k, h, **kw):
    from shadowing_amd import _native
    info = {}
    ds_t = ds if isinstance(ds, torch.Tensor) else torch.as_tensor(ds).to(dev)
    d, idx, st = _native.scan_topk(ds_t, torch.as_tensor(q).to(dev), k, h=h, flags=_native.FLAG_OVERLAP, info=info, **kw)
    torch.cuda.synchronize(dev)
    return d, idx, st, info


@pytest.mark.parametrize("R,T,W,h,k", [(2048, 2048, 20, 0, 200), (3072, 2300, 33, 9, 150), (3072, 2300, 7, 9, 150)])
def test_copy_scan_equals_the_oracle(hip_device, oracle_mod, R, T, W, h, k):
    """The route table's overlap case (W = 20: the compile-time instantiation) and a ragged last segment with run-time windows."""
    ds = syn.dataset(R, T, 7100 + W)[:, 0, :].copy()
    q = syn.gbm_log_returns((1, W), 7200 + W)
    d, idx, st, info = _scan(hip_device, ds, q, k, h)
    assert (info["copy_served"], info["path"], int(st[0])) == (1, 3, 0), info
    _exact(d, idx, *oracle_mod.scan_topk(ds, q, k, h=h), f"R={R} T={T} W={W}")


@pytest.mark.parametrize("geom", list(bd.GEOMETRIES))
def test_copy_scan_keeps_every_edge_plant(hip_device, oracle_mod, geom):
    c = bd.route_case("overlap", geom)
    ds, q, good, bad = bd.identity_inputs(c)
    d, idx, st, info = _scan(hip_device, ds, q, c["k"], c["h"])
    assert (info["copy_served"], info["path"], int(st[0])) == (1, 3, 0), info
    bd.check(d.cpu().numpy(), idx.cpu().numpy(), good, bad, c["T"], c["W"], c["h"], f"copy scan, {geom}")
    _exact(d, idx, *oracle_mod.scan_topk(ds, q, c["k"], h=c["h"]), geom)


@pytest.mark.parametrize("kind", ADVERSARIAL)
def test_copy_scan_admits_exactly_the_windows_below_the_level(hip_device, oracle_mod, built, kind):
    from shadowing_amd import _native
    for i, (W, h) in enumerate([(20, 20), (33, 5), (7, 11)]):
        ds, q = adversarial(kind, 4096, 2048, 1, W, h, 300 + 5 * i)
        for m in (2000, 500, 100):                       # (planted matches crowd single blocks: a shallower level then)
            try:
                check_sets(hip_device, oracle_mod, ds, q, h, m, flags=_native.FLAG_OVERLAP, k=32, what=f"copy {kind} W={W} m={m}", expect_path=3)
                break
            except AssertionError as e:
                if "overflowed" not in str(e) or m == 100:
                    raise
    assert len(built) >= 3 and all(c.desc.served == 1 for c in built), [(c.desc.served, c.desc.reason) for c in built]


def test_quiet_query_and_smooth_ensemble_take_the_dense_branch(hip_device, oracle_mod):
    """Most windows of a segment survive the test: their chains run from the staged fp32 tile."""
    W, h, k = 20, 5, 100
    ds = syn.dataset(2048, 2048, 7300)[:, 0, :].copy()
    q = (syn.gbm_log_returns((1, W), 7301) * np.float32(1e-3)).astype(np.float32)       # the query's norm is lost in the windows' energies
    d, idx, st, info = _scan(hip_device, ds, q, k, h)
    assert (info["copy_served"], info["path"], int(st[0])) == (1, 3, 0), info
    _exact(d, idx, *oracle_mod.scan_topk(ds, q, k, h=h), "quiet query")
    walk = np.cumsum(ds, axis=1, dtype=np.float64).astype(np.float32)                   # price levels: neighbours in t are neighbours in distance
    qw = (walk[77, 500:500 + W] + np.float32(1e-3)).reshape(1, W).astype(np.float32)
    d, idx, st, info = _scan(hip_device, walk, qw, k, h)
    assert (info["copy_served"], info["path"]) == (1, 3), info
    if int(st[0]) == 0:
        _exact(d, idx, *oracle_mod.scan_topk(walk, qw, k, h=h), "walk")
    else:                                                                               # (clustered matches may overflow a list: the protocol's rerun)
        d2, i2 = _native_checked(hip_device, walk, qw, k, h)
        _exact(d2, i2, *oracle_mod.scan_topk(walk, qw, k, h=h), "walk, rerun")


def _native_checked(dev, ds, q, k, h):
    from shadowing_amd import _native
    return _native.scan_topk_checked(torch.as_tensor(ds).to(dev), torch.as_tensor(q).to(dev), k, h=h, flags=_native.FLAG_OVERLAP)


def test_three_streams_share_one_copy(hip_device, oracle_mod, built):
    from shadowing_amd import _native
    ds = syn.dataset(8192, 2048, 7400)
    ds_t = torch.as_tensor(ds[:, 0, :].copy()).to(hip_device)
    qs = [syn.gbm_log_returns((1, 20), 7401 + i) for i in range(5)]
    q_t = [torch.as_tensor(q).to(hip_device) for q in qs]
    streams = [torch.cuda.Stream(hip_device) for _ in range(3)]
    wss = [_native.Workspace(hip_device) for _ in range(3)]
    torch.cuda.synchronize()
    outs = []
    for i in range(30):
        with torch.cuda.stream(streams[i % 3]):
            outs.append(_native.scan_topk(ds_t, q_t[i % 5], 256, h=20, workspace=wss[i % 3], flags=_native.FLAG_OVERLAP))
    torch.cuda.synchronize()
    assert len(built) == 1 and built[0].desc.served == 1
    want = [oracle_mod.scan_topk(ds, q, 256, h=20) for q in qs]
    for i, (d, idx, st) in enumerate(outs):
        assert int(st[0]) == 0, i
        _exact(d, idx, *want[i % 5], f"step {i}")


def test_an_edit_torch_sees_rebuilds_and_one_it_does_not_is_answered_by_retry(hip_device, oracle_mod, built):
    from shadowing_amd import _native
    W, h, k = 20, 20, 128
    a = syn.dataset(2048, 2048, 7500)[:, 0, :].copy()
    b = syn.dataset(2048, 2048, 7501)[:, 0, :].copy()
    q = syn.gbm_log_returns((1, W), 7502)
    ds_t = torch.as_tensor(a).to(hip_device)
    d, idx, st, info = _scan(hip_device, ds_t, q, k, h)
    assert info["copy_served"] == 1 and len(built) == 1
    ds_t.copy_(torch.as_tensor(b))                                    # in place: the version counter moves, the copy is rebuilt
    d, idx, st, info = _scan(hip_device, ds_t, q, k, h)
    assert info["copy_served"] == 1 and len(built) == 2 and int(st[0]) == 0
    _exact(d, idx, *oracle_mod.scan_topk(b, q, k, h=h), "after an in-place edit")
    ds_t.data.copy_(torch.as_tensor(a))                               # behind torch's back: the copy is of other data now
    d, idx, st, info = _scan(hip_device, ds_t, q, k, h)
    assert info["copy_served"] == 1 and len(built) == 2
    assert int(st[0]) == _native.PSH_STATUS_RETRY, "the audit did not catch a copy of another ensemble"
    d, idx = _native.scan_topk_checked(ds_t, torch.as_tensor(q).to(hip_device), k, h=h, flags=_native.FLAG_OVERLAP)
    torch.cuda.synchronize()
    _exact(d, idx, *oracle_mod.scan_topk(a, q, k, h=h), "scan_topk_checked after the audit's RETRY")
    assert id(ds_t) not in _native._filter_copies


def test_shadow_async_on_the_copy_equals_shadow(hip_device):
    import shadowing_amd as sa
    ds = syn.dataset(4096, 2048, 7600)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20), cache=True)
    qs = [syn.single_query(20, 7601 + j) for j in range(4)]
    hs = [obj.shadow_async(q, k=128) for q in qs]
    assert obj._async["copy"] is not None
    got = [hnd.result() for hnd in hs]
    assert any(sl._fc_desc.served == 1 for pool in obj._async["slots"] for sl in pool)
    for q, (d, paths, idx) in zip(qs, got):
        wd, wp, wi = obj.shadow(q, k=128, cuda=True)
        assert np.array_equal(d.view(np.uint32), wd.view(np.uint32)) and np.array_equal(idx, wi) and np.array_equal(paths, wp)
