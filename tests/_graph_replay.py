"""What tests/test_gpu_graph_replay.py's cases share: capture one call (or one linear chain of calls) on torch.cuda.graph's
single capture stream, and compare tensors bit for bit."""
import numpy as np
import torch

_INT_OF = {torch.float32: torch.int32, torch.float64: torch.int64, torch.complex128: torch.int64}


def capture(fn):
    """(graph, what fn returned): fn's launches recorded on the capture stream, nothing run."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def replay(g, dev):
    g.replay()
    torch.cuda.synchronize(dev)


def as_bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes as integers (NaN payloads and the sign of zero count)."""
    t = t.contiguous()
    if t.dtype == torch.complex128:
        t = torch.view_as_real(t).contiguous()
        return t.view(torch.int64)
    return t.view(_INT_OF[t.dtype]) if t.dtype in _INT_OF else t


def flatten(out) -> list:
    """[(name, tensor)] of a wrapper's return value: a tensor, a tuple of tensors or a dict of them."""
    if isinstance(out, torch.Tensor):
        return [("out", out)]
    if isinstance(out, dict):
        return [(name, out[name]) for name in sorted(out)]
    return [(str(i), t) for i, t in enumerate(out)]


def snapshot(named) -> list:
    return [(name, t.clone()) for name, t in named]


def assert_same_bits(got, want, what: str):
    """Two [(name, tensor)] lists: same names, dtypes, shapes, bytes."""
    assert [n for n, _ in got] == [n for n, _ in want], what
    for (name, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name}"
        ab, bb = as_bits(a), as_bits(b)
        assert torch.equal(ab, bb), f"{what}: {name} differs in {int((ab != bb).sum())} of {ab.numel()} words"


def admission_hint(od: np.ndarray, q: np.ndarray, k: int) -> np.ndarray:
    """tests/test_gpu_routes.py's hint: 1.1 x the acc = (d ||x||)^2 of every query's k-th window."""
    xn2 = (q.astype(np.float64) ** 2).sum(axis=1)
    return ((od[:, k - 1].astype(np.float64) ** 2) * xn2 * 1.1).astype(np.float32)
