"""The checked embedded scan (_native.scan_topk_embedded_checked: the sampled scan, its status read once, the queries that
overflowed redone exhaustively) and the sharded class on a dirty shard whose clean rows hold fewer windows than k -- the corner
_dirty.DirtyRows serves with the exhaustive scan -- against the oracle, bit for bit."""
import numpy as np
import pytest
import torch

from _util import assert_exact, syn

pytestmark = pytest.mark.gpu


def _foveal():
    import shadowing_amd as sa
    emb = sa.Foveal(alpha=1.3, beta=0.9, max_context=60)
    x = syn.gbm_log_returns((3, 60), 8101)
    return emb, emb.kernel[:, 0, :].numpy().copy(), emb(torch.tensor(x)[:, None, :])[:, 0, :].numpy()


def test_scan_topk_embedded_checked_equals_the_oracle(hip_device, oracle_mod, monkeypatch):
    from shadowing_amd import _native
    R, T, h, k = 256, 400, 10, 64
    _, ker, hx = _foveal()
    redone = []
    real = _native.scan_topk_embedded
    monkeypatch.setattr(_native, "scan_topk_embedded",
                        lambda *a, **kw: (redone.append(a[2].shape[0]) if kw.get("exhaustive") else None, real(*a, **kw))[1])
    ws = _native.Workspace(hip_device)
    tied = np.repeat(syn.dataset(1, T, 8103), R, axis=0)                 # identical rows: every distance tied R times over
    for name, ds in (("random rows", syn.dataset(R, T, 8102)), ("identical rows", tied)):
        n0 = len(redone)
        d, idx = _native.scan_topk_embedded_checked(torch.as_tensor(ds[:, 0, :]).to(hip_device), torch.as_tensor(ker).to(hip_device),
                                                    torch.as_tensor(hx).to(hip_device), k, h=h, workspace=ws)
        od, oidx = oracle_mod.scan_topk_embedded(ds, ker, hx, k, h=h)
        print(name, "queries redone exhaustively:", redone[n0:])
        assert_exact(d.cpu().numpy(), idx.cpu().numpy(), od, oidx, name)
    # an offset and caller's buffers, status words included
    out = (torch.empty((3, k), device=hip_device), torch.empty((3, k, 2), dtype=torch.int32, device=hip_device),
           torch.full((3,), -7, dtype=torch.int32, device=hip_device))
    d, idx = _native.scan_topk_embedded_checked(torch.as_tensor(tied[:, 0, :]).to(hip_device), torch.as_tensor(ker).to(hip_device),
                                                torch.as_tensor(hx).to(hip_device), k, h=h, r_offset=3000, workspace=ws, out=out)
    assert d.data_ptr() == out[0].data_ptr() and idx.data_ptr() == out[1].data_ptr() and int(out[2].min().item()) >= 0
    od, oidx = oracle_mod.scan_topk_embedded(tied, ker, hx, k, h=h, r_offset=3000)
    assert_exact(d.cpu().numpy(), idx.cpu().numpy(), od, oidx, "identical rows, r_offset, out")


def test_sharded_dirty_shard_with_fewer_clean_windows_than_k(hip_device, oracle_mod):
    """Rows 2 and later hold a NaN: 2 x 331 windows on clean rows < k = 3000, so the dirty rows' exhaustive leg carries the
    answer and the clean rows give every window they hold; global row numbers."""
    import shadowing_amd as sa
    from shadowing_amd.distributed import ShardedPathShadowing
    R, T, h, k = 64, 400, 10, 3000
    ds = syn.dataset(R, T, 7600)
    ds[2:, 0, 200] = np.nan
    emb, ker, hx = _foveal()
    obj = ShardedPathShadowing(emb, sa.RelativeMSE(), torch.as_tensor(ds), 3000, sa.PredictionContext(h), device=hip_device)
    d, idx, _ = obj.local_scan(torch.as_tensor(hx).to(hip_device), k)
    od, oidx = oracle_mod.scan_topk_embedded(ds, ker, hx, k, h=h, r_offset=3000)
    assert np.isfinite(od).all()
    assert_exact(d.cpu().numpy(), idx.cpu().numpy(), od, oidx, "dirty shard, few clean windows")
