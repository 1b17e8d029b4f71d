"""The axes the host launchers turn into template arguments (psh_launch.h: pick), walked on routes where no other test
crosses them: the specialised window length W = 20 against the generic one, rows that load as aligned 16-byte quads against
rows that do not (T odd), the four K-step buckets of the long-window kernels, the one, two and three groups of four
embedding dimensions of the matrix-core embedded scan.  A launcher that picks the wrong instantiation on one combination
gives another result or another route there: every case is bit-equal to the CPU oracle, served by its first call, on the
route and with the sample recorded for the same input before the launchers were rewritten (EXPECTED).

The shapes are test_gpu_routes.py's, the smallest known to reach each branch of the dispatcher; the oracle ranks every
window once per (W, T) and the cases of a group share it (the smaller batches are the first queries of the largest)."""
import numpy as np
import pytest
import torch

from _util import assert_exact
from shadowing_amd import synthetic as syn
from test_gpu_embedded import _case_inputs
from test_gpu_routes import CASES as ROUTE_CASES

pytestmark = pytest.mark.gpu

SHORT_ROUTES = ("default", "overlap", "B2", "B4", "B32", "B32_mq_f16", "no_fuse", "copy")   # copy: the overlap route on a FilterCopy
LONG_ROUTES = ("long_W64_B1", "long_W64_B5")
EMB_ROUTES = ("emb_dense", "emb_dense_mx")
PSH_EMX_MAX_D = 12


# psh_kernels.h: lq_ksteps, lq_bucket
def lq_ksteps(W):
    return (W + 31 + 15) // 16


def lq_bucket(W):
    n = lq_ksteps(W)
    return 6 if n <= 6 else 10 if n <= 10 else 14 if n <= 14 else 18


LONG_W = {6: 64, 10: 97, 14: 130, 18: 200}          # bucket -> a window length in it


def _cases():
    """{id: dict(group, route, R, T, W, h, k, B, flags, d)}"""
    out = {}
    for route in SHORT_ROUTES:
        c = ROUTE_CASES["overlap" if route == "copy" else route]
        for W in (20, 19):
            for T in (2048, 2049):
                out[f"{route}-W{W}-T{T}"] = dict(group="short", route=route, R=2048, T=T, W=W, h=0, k=200, B=c.get("B", 1),
                                                 flags=c.get("flags", ()), d=0)
    for route in LONG_ROUTES:
        c = ROUTE_CASES[route]
        for W in LONG_W.values():
            for T in (2300, 2301):
                out[f"{route.replace('W64', f'W{W}')}-T{T}"] = dict(group="long", route=route, R=c["R"], T=T, W=W, h=c["h"], k=c["k"],
                                                                   B=c.get("B", 1), flags=c.get("flags", ()), d=0)
    for route in EMB_ROUTES:
        c = ROUTE_CASES[route]
        for d in (3, 4, 7, 8, 11, 12):                     # one, two, three groups of four, the last one partial or full
            for T in (2048, 2049):
                out[f"{route}-d{d}-T{T}"] = dict(group="emb", route=route, R=2048, T=T, W=c["emb"][2], h=c["h"], k=200, B=1,
                                                 flags=c.get("flags", ()), d=d)
    return out


CASES = _cases()

# (psh_profile.path, n_sample_rows) of each case as the launch ladders that psh_launch.h's picker replaced took it, recorded
# on an MI355X from the commit before the rewrite.  path: 0 the separate launches, 2 the fused launch, 3 the three
# overlap-friendly launches; the sample tells the matrix-core embedded scan (256 rows) from the plain one (512) on one path
EXPECTED = {
    "default-W20-T2048": (2, 512), "default-W20-T2049": (2, 512), "default-W19-T2048": (2, 512),
    "default-W19-T2049": (2, 512), "overlap-W20-T2048": (3, 512), "overlap-W20-T2049": (3, 512),
    "overlap-W19-T2048": (3, 512), "overlap-W19-T2049": (3, 512), "B2-W20-T2048": (3, 512),
    "B2-W20-T2049": (3, 512), "B2-W19-T2048": (3, 512), "B2-W19-T2049": (3, 512),
    "B4-W20-T2048": (0, 512), "B4-W20-T2049": (0, 512), "B4-W19-T2048": (0, 512),
    "B4-W19-T2049": (0, 512), "B32-W20-T2048": (0, 512), "B32-W20-T2049": (0, 512),
    "B32-W19-T2048": (0, 512), "B32-W19-T2049": (0, 512), "B32_mq_f16-W20-T2048": (0, 512),
    "B32_mq_f16-W20-T2049": (0, 512), "B32_mq_f16-W19-T2048": (0, 512), "B32_mq_f16-W19-T2049": (0, 512),
    "no_fuse-W20-T2048": (0, 51), "no_fuse-W20-T2049": (0, 51), "no_fuse-W19-T2048": (0, 51),
    "no_fuse-W19-T2049": (0, 51), "copy-W20-T2048": (3, 512), "copy-W20-T2049": (3, 512),
    "copy-W19-T2048": (3, 512), "copy-W19-T2049": (3, 512), "long_W64_B1-T2300": (3, 682),
    "long_W64_B1-T2301": (3, 682), "long_W97_B1-T2300": (3, 682), "long_W97_B1-T2301": (3, 682),
    "long_W130_B1-T2300": (3, 682), "long_W130_B1-T2301": (3, 682), "long_W200_B1-T2300": (3, 682),
    "long_W200_B1-T2301": (3, 682), "long_W64_B5-T2300": (0, 342), "long_W64_B5-T2301": (0, 342),
    "long_W97_B5-T2300": (0, 342), "long_W97_B5-T2301": (0, 342), "long_W130_B5-T2300": (0, 342),
    "long_W130_B5-T2301": (0, 342), "long_W200_B5-T2300": (0, 342), "long_W200_B5-T2301": (0, 342),
    "emb_dense-d3-T2048": (0, 512), "emb_dense-d3-T2049": (0, 512), "emb_dense-d4-T2048": (0, 512),
    "emb_dense-d4-T2049": (0, 512), "emb_dense-d7-T2048": (0, 512), "emb_dense-d7-T2049": (0, 512),
    "emb_dense-d8-T2048": (0, 512), "emb_dense-d8-T2049": (0, 512), "emb_dense-d11-T2048": (0, 512),
    "emb_dense-d11-T2049": (0, 512), "emb_dense-d12-T2048": (0, 512), "emb_dense-d12-T2049": (0, 512),
    "emb_dense_mx-d3-T2048": (0, 256), "emb_dense_mx-d3-T2049": (0, 256), "emb_dense_mx-d4-T2048": (0, 256),
    "emb_dense_mx-d4-T2049": (0, 256), "emb_dense_mx-d7-T2048": (0, 256), "emb_dense_mx-d7-T2049": (0, 256),
    "emb_dense_mx-d8-T2048": (0, 256), "emb_dense_mx-d8-T2049": (0, 256), "emb_dense_mx-d11-T2048": (0, 256),
    "emb_dense_mx-d11-T2049": (0, 256), "emb_dense_mx-d12-T2048": (0, 256), "emb_dense_mx-d12-T2049": (0, 256),
}


def test_the_window_lengths_fall_in_the_four_buckets():
    assert [lq_bucket(W) for W in LONG_W.values()] == list(LONG_W) == [6, 10, 14, 18]
    assert sorted({(c["d"] + 3) // 4 for c in CASES.values() if c["group"] == "emb"}) == [1, 2, 3]
    assert max(c["d"] for c in CASES.values()) == PSH_EMX_MAX_D
    assert set(EXPECTED) == set(CASES)


_shared = {}


def _inputs(c):
    """(ds (R, T), kernel or None, queries, oracle d, oracle idx) of a case; the oracle runs once per group, W, T and d."""
    key = (c["group"], c["W"], c["T"], c["d"])
    if key not in _shared:
        import oracle
        oracle.build()
        B = max(o["B"] for o in CASES.values() if (o["group"], o["W"], o["T"], o["d"]) == key)
        if c["group"] == "emb":
            ds, ker, q = _case_inputs(c["R"], c["T"], c["d"], c["W"], B, "dense", 9500 + c["T"] + c["d"])
            od, oidx = oracle.scan_topk_embedded(ds, ker, q, c["k"], h=c["h"])
        else:
            ds, ker = syn.dataset(c["R"], c["T"], 9600 + c["T"]), None
            q = syn.gbm_log_returns((B, c["W"]), 9700 + c["W"])
            od, oidx = oracle.scan_topk(ds, q, c["k"], h=c["h"])
        _shared[key] = (np.ascontiguousarray(ds[:, 0, :]), ker, np.ascontiguousarray(q, dtype=np.float32), od, oidx)
    ds, ker, q, od, oidx = _shared[key]
    return ds, ker, q[:c["B"]], od[:c["B"]], oidx[:c["B"]]


def run_case(dev, name):
    """One raw call: (d, idx, status, (path, n_sample_rows), copy_served, oracle d, oracle idx)."""
    from shadowing_amd import _native
    c = CASES[name]
    ds, ker, q, od, oidx = _inputs(c)
    flags = 0
    for f in c["flags"]:
        flags |= getattr(_native, "FLAG_" + f)
    ds_t, q_t = torch.as_tensor(ds).to(dev), torch.as_tensor(q).to(dev)
    info = {}
    if ker is not None:
        d, idx, st = _native.scan_topk_embedded(ds_t, torch.as_tensor(ker).to(dev), q_t, c["k"], h=c["h"], flags=flags, info=info)[:3]
    else:
        copy = _native.FilterCopy(ds_t) if c["route"] == "copy" else None
        d, idx, st = _native.scan_topk(ds_t, q_t, c["k"], h=c["h"], flags=flags, info=info, filter_copy=copy)
    torch.cuda.synchronize(dev)
    return d.cpu().numpy(), idx.cpu().numpy(), st.cpu().numpy(), (info["path"], info["n_sample_rows"]), info.get("copy_served", 0), od, oidx


@pytest.mark.parametrize("name", list(CASES))
def test_every_instantiation_gives_the_oracles_result_on_the_recorded_route(hip_device, name):
    d, idx, status, plan, copy_served, od, oidx = run_case(hip_device, name)
    assert plan == EXPECTED[name], (name, plan)
    assert copy_served == (1 if CASES[name]["route"] == "copy" else 0), (name, copy_served)
    assert not status.any(), (name, status.tolist())
    assert_exact(d, idx, od, oidx, f"launch axes: {name}")
