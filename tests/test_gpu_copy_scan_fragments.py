"""copy_scan_kernel (psh_stream_copy.hip) feeds its MFMAs with A fragments loaded straight from the resident f16 copy.  Row 31
of A then holds the 33 - W halves that FOLLOW the segment's last window (the next segment's first samples, or the row's zero
tail): they only meet zero taps, but a NaN there -- or a value whose square leaves f16 -- turns the accumulators of windows
992 .. 1023 into NaNs.  Such windows survive the test (NaN-safe compare) and are decided by the exact fp32 chain, so every
result stays the oracle's, asked to judge a window by its own W samples (h = 0 on the rows cut by the horizon).  Also here: the rows' ends (the last row's loads end
nearest the end of the allocation) and the dense branch's audit, which now reads the copy's halves from memory.

Small ensembles: the level is given (tau_hint = the k-th distance's acc x 1.1, from the oracle) where the ensemble is too small
for the bootstrap sample, and the workspace is cut where its candidate buffer would hold every window (the exhaustive path)."""
import numpy as np
import pytest
import torch

from shadowing_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def built(monkeypatch):
    """Policy "first", and a record of every copy the policy builds (tests/test_gpu_filter_copy.py's fixture)."""
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


def _level(od, q, k):
    xn2 = (q.astype(np.float64) ** 2).sum(axis=1)
    return ((od[:, k - 1].astype(np.float64) ** 2) * xn2 * 1.1).astype(np.float32)


def _scan(dev, ds, q, k, h, **kw):
    from shadowing_amd import _native
    info = {}
    ds_t = ds if isinstance(ds, torch.Tensor) else torch.as_tensor(ds).to(dev)
    d, idx, st = _native.scan_topk(ds_t, torch.as_tensor(q).to(dev), k, h=h, flags=_native.FLAG_OVERLAP, info=info, **kw)
    torch.cuda.synchronize(dev)
    return d, idx, st, info


@pytest.mark.parametrize("W", [7, 20, 33])
def test_poison_in_the_overhang_only_makes_windows_survive(hip_device, oracle_mod, W):
    """NaN and +inf (four rows each, every half seg_start + 1024 + W - 1 .. seg_start + 1055 of segments 0 and 1) and a finite
    sample of 400 x the ensemble's rms (one row, the first of those halves in either segment: two such samples are all an
    ensemble of this size can hold at 400 x ITS rms, which they raise).  No window of that segment holds these halves, row 31 of
    its A matrix does.  Near-copies of the query end right in front of them (windows 992 .. 1023).  W = 33: the overhang is
    empty.  (The copy holds the rms in [0.5, 1): the finite sample is stored in [200, 400) and its square leaves f16 from 256
    on, before the step's 2^delta <= 1 -- whether it does or not, the result is the oracle's.)"""
    R, T, h, k = 256, 2300, 9, 64
    ds = syn.dataset(R, T, 8100 + W)[:, 0, :].copy()
    q = syn.gbm_log_returns((1, W), 8200 + W)
    g = np.random.default_rng(8300 + W)
    rows = [3 + 21 * i for i in range(9)]
    kinds = ["nan", "inf"] * 4 + ["big"]
    shifts = [(5 * i) % min(W, 32) for i in range(len(rows))]
    for row, shift in zip(rows, shifts):
        for s0 in (0, 1024):
            for p in (1023 - shift, 1023 - shift - W):
                if p >= 992:
                    ds[row, s0 + p:s0 + p + W] = q[0] * (1.0 + 1e-3 * g.standard_normal(W)).astype(np.float32)
    n_big = 2 if W < 33 else 0
    ms0 = np.mean(ds.astype(np.float64) ** 2)
    big = np.float32(400.0 * np.sqrt(ms0 / (1.0 - 400.0 ** 2 * n_big / ds.size)))       # 400 x the rms of the ensemble that holds it
    for row, kind, shift in zip(rows, kinds, shifts):
        for s0 in (0, 1024):
            lo, hi = s0 + 1024 + W - 1, s0 + 1056
            assert s0 + 1023 - shift + W - 1 < lo                                # the plants stay clear of the poison
            if kind == "big":
                ds[row, lo:min(hi, lo + 1)] = big
            else:
                ds[row, lo:hi] = np.float32(np.nan if kind == "nan" else np.inf)
    if n_big:
        fin = ds[np.isfinite(ds)].astype(np.float64)
        assert abs(big / np.sqrt(np.mean(fin ** 2)) - 400.0) < 0.5
    # (psh_scan_topk's rule -- include/psh.h, NON-FINITE SAMPLES -- is the oracle's without a horizon: with h it follows the
    #  reference, whose zero-padded conv also turns a window NaN over a non-finite sample among its h future ones; the same
    #  admissible windows t < T - W - h + 1 are those of the array cut by h samples)
    od, oidx = oracle_mod.scan_topk(np.ascontiguousarray(ds[:, :T - h]), q, k, h=0)
    assert np.isfinite(od).all(), "k reaches into the windows that hold a poisoned sample"
    planted = {(r, s0 + 1023 - sh) for r, sh in zip(rows, shifts) for s0 in (0, 1024)}
    assert planted <= {tuple(e) for e in oidx[0].tolist()}, "a planted near-copy is not among the oracle's k best"
    hint = torch.as_tensor(_level(od, q, k)).to(hip_device)
    d, idx, st, info = _scan(hip_device, ds, q, k, h, tau_hint=hint)
    assert (info["copy_served"], info["path"], int(st[0])) == (1, 3, 0), info
    _exact(d, idx, od, oidx, f"poisoned overhang, W={W}")


@pytest.mark.parametrize("T", [2299, 2048 + 20 + 9 - 1, 2048 + 20 + 9])
def test_row_ends(hip_device, oracle_mod, T):
    """T no multiple of 8; T = 2048 + W + h - 1 (two full segments of windows, nothing behind them) and one more (the last
    segment holds exactly one window).  A match at the last admissible window of the last row."""
    R, W, h, k = 64, 20, 9, 32
    ds = syn.dataset(R, T, 8400 + T)[:, 0, :].copy()
    q = syn.gbm_log_returns((1, W), 8500)
    Tp = T - W - h + 1
    ds[R - 1, Tp - 1:Tp - 1 + W] = q[0] * np.float32(1.0 + 1e-3)
    od, oidx = oracle_mod.scan_topk(ds, q, k, h=h)
    assert oidx[0, 0].tolist() == [R - 1, Tp - 1]
    hint = torch.as_tensor(_level(od, q, k)).to(hip_device)
    d, idx, st, info = _scan(hip_device, ds, q, k, h, tau_hint=hint, extra_workspace_factor=0.25)
    assert (info["copy_served"], info["path"], int(st[0])) == (1, 3, 0), info
    _exact(d, idx, od, oidx, f"row ends, T={T}")


def test_a_stale_copy_in_a_dense_segment_is_answered_by_retry(hip_device, oracle_mod, built):
    """Price levels, and a query that is one of their windows -- or one whose norm is lost in the windows' energies: most
    windows of a segment survive, their chains run from the staged fp32 tile and their audit reads the copy from memory."""
    from shadowing_amd import _native
    R, T, W, h, k = 512, 2048, 20, 5, 100
    walk_a = np.cumsum(syn.dataset(R, T, 8600)[:, 0, :], axis=1, dtype=np.float64).astype(np.float32)
    walk_b = np.cumsum(syn.dataset(R, T, 8601)[:, 0, :], axis=1, dtype=np.float64).astype(np.float32)
    queries = [(walk_a[77, 500:500 + W] + np.float32(1e-3)).reshape(1, W).astype(np.float32),
               (syn.gbm_log_returns((1, W), 8602) * np.float32(1e-3)).astype(np.float32)]
    for n, q in enumerate(queries):
        ds_t = torch.as_tensor(walk_a).to(hip_device)
        d, idx, st, info = _scan(hip_device, ds_t, q, k, h)
        assert (info["copy_served"], info["path"]) == (1, 3) and len(built) == n + 1, info
        ds_t.data.copy_(torch.as_tensor(walk_b))                      # behind torch's back: the copy is of other data now
        d, idx, st, info = _scan(hip_device, ds_t, q, k, h)
        assert (info["copy_served"], info["path"]) == (1, 3) and len(built) == n + 1, info
        assert int(st[0]) == _native.PSH_STATUS_RETRY, "the dense branch's audit did not catch a copy of another ensemble"
        d, idx = _native.scan_topk_checked(ds_t, torch.as_tensor(q).to(hip_device), k, h=h, flags=_native.FLAG_OVERLAP)
        torch.cuda.synchronize()
        _exact(d, idx, *oracle_mod.scan_topk(walk_b, q, k, h=h), f"scan_topk_checked after the audit's RETRY, query {n}")
