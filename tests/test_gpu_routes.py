"""The route table of psh_scan_topk / psh_scan_topk_embedded: which of the four routes serves a call (psh_profile.path: 0 the
separate launches, 1 exhaustive, 2 the fused launch, 3 the three overlap-friendly launches), with which sample and grid.

One call per line of CASES, each the smallest shape found that reaches its branch of the dispatcher in psh_capi.hip
(decide_route and the function of each route).  The literals in EXPECTED are (path, n_sample_rows, grid_blocks, status
words) as the 520-line scan_topk_impl gave them before it was split into those functions, recorded on a device with
CU_COUNT compute units (the grids are per-CU clamps, so the module is skipped on any other device); every case there had
status OK and the oracle's result.  Results are bit-equal to the CPU oracle.  The reserved-CU grids are test_gpu_overlap.py's."""
import numpy as np
import pytest
import torch

from _util import assert_exact
from shadowing_amd import synthetic as syn
from test_gpu_embedded import _case_inputs

pytestmark = pytest.mark.gpu

CU_COUNT = 256

DEFAULT = dict(R=2048, T=2048, W=20, h=0, k=200, B=1, flags=(), hint=False, emb=None)
LONG = dict(R=3072, T=2300, h=9, k=150)
ROWS = dict(R=65536, T=20, W=20, h=0, k=64)          # one-window rows: T == W + h

CASES = {
    "default": {},
    "default_hint": dict(hint=True),
    "no_fuse": dict(flags=("NO_FUSE",)),                      # two-class candidates around the estimate
    "no_fuse_hint": dict(flags=("NO_FUSE",), hint=True),
    "overlap": dict(flags=("OVERLAP",)),
    "filter_valu": dict(flags=("FILTER_VALU",)),
    "B2": dict(B=2),
    "B3": dict(B=3),
    "B4": dict(B=4),                                          # the batched matrix-core scan, f16 rejection test
    "B16": dict(B=16),
    "B32": dict(B=32),                                        # ... the 8-bit test
    "B32_mq_f16": dict(B=32, flags=("MQ_F16",)),
    "long_W64_B1": dict(LONG, W=64),
    "long_W64_B1_hint": dict(LONG, W=64, hint=True),          # no matrix-core sample: the exact chains' unit count
    "long_W97_B3": dict(LONG, W=97, B=3),
    "long_W129_B3": dict(LONG, W=129, B=3),                   # three tables do not ride one pass: the batched long-window scan
    "long_W64_B5": dict(LONG, W=64, B=5),
    "long_W64_B5_loop": dict(LONG, W=64, B=5, flags=("LONG_LOOP",)),    # steps of 3 + 2 queries: the profile is the last step's
    "long_W30_B7": dict(LONG, W=30, B=7),
    "long_W30_B7_loop": dict(LONG, W=30, B=7, flags=("LONG_LOOP",)),    # three-query steps of the short kernel: 3 + 3 + 1
    "large_k_estimate": dict(R=8192, T=1100, k=2048, flags=("NO_FUSE",)),
    "exhaustive_small": dict(R=64, T=300, k=10),
    "rows": dict(ROWS),
    "rows_generic": dict(ROWS, flags=("ROWS_GENERIC",)),
    "emb_foveal": dict(emb=("foveal", 0, 40), h=20),
    "emb_foveal_mx": dict(emb=("foveal", 0, 40), h=20, flags=("EMBED_MX",)),
    "emb_dense": dict(emb=("dense", 8, 24), h=20),
    "emb_dense_mx": dict(emb=("dense", 8, 24), h=20, flags=("EMBED_MX",)),
    # 260 queries are more than one call of the matrix-core embedded scan takes: two chunks of 130 inside the call (a smaller
    # ensemble: the oracle ranks every window for every query)
    "emb_dense_mx_B260": dict(emb=("dense", 8, 24), R=512, T=1100, h=20, k=100, B=260, flags=("EMBED_MX",)),
}

# (path, n_sample_rows, grid_blocks, status words)
EXPECTED = {
    'default': (2, 512, 256, [0]),
    'default_hint': (2, 512, 256, [0]),
    'no_fuse': (0, 51, 256, [0]),
    'no_fuse_hint': (0, 0, 256, [0]),
    'overlap': (3, 512, 256, [0]),
    'filter_valu': (0, 512, 256, [0]),
    'B2': (3, 512, 256, [0] * 2),
    'B3': (3, 512, 256, [0] * 3),
    'B4': (0, 512, 256, [0] * 4),
    'B16': (0, 512, 256, [0] * 16),
    'B32': (0, 512, 256, [0] * 32),
    'B32_mq_f16': (0, 512, 256, [0] * 32),
    'long_W64_B1': (3, 682, 256, [0]),
    'long_W64_B1_hint': (3, 341, 256, [0]),
    'long_W97_B3': (3, 455, 256, [0] * 3),
    'long_W129_B3': (0, 342, 256, [0] * 3),
    'long_W64_B5': (0, 342, 256, [0] * 5),
    'long_W64_B5_loop': (3, 682, 256, [0] * 5),
    'long_W30_B7': (0, 342, 256, [0] * 7),
    'long_W30_B7_loop': (2, 768, 256, [0] * 7),
    'large_k_estimate': (0, 512, 256, [0]),
    'exhaustive_small': (1, 0, 4, [0]),
    'rows': (0, 1024, 512, [0]),
    'rows_generic': (1, 0, 16, [0]),
    'emb_foveal': (0, 512, 256, [0]),
    'emb_foveal_mx': (0, 256, 256, [0]),
    'emb_dense': (0, 512, 256, [0]),
    'emb_dense_mx': (0, 256, 256, [0]),
    'emb_dense_mx_B260': (0, 6, 256, [0] * 260),
}


def _case(name):
    c = dict(DEFAULT, **CASES[name])
    c["flag_word"] = 0
    from shadowing_amd import _native
    for f in c["flags"]:
        c["flag_word"] |= getattr(_native, "FLAG_" + f)
    return c


_inputs_cache = {}


def _inputs(c):
    """(ds (R, 1, T), kernel or None, queries / embedded queries, oracle d, oracle idx): computed once per shape and flags-blind."""
    key = (c["R"], c["T"], c["W"], c["h"], c["k"], c["B"], c["emb"])
    if key not in _inputs_cache:
        import oracle
        oracle.build()
        if c["emb"]:
            kind, d, K = c["emb"]
            ds, ker, q = _case_inputs(c["R"], c["T"], d, K, c["B"], kind, 9000 + c["R"] + K)
            od, oidx = oracle.scan_topk_embedded(ds, ker, q, c["k"], h=c["h"])
        else:
            ds, ker = syn.dataset(c["R"], c["T"], 9100 + c["R"]), None
            q = syn.gbm_log_returns((c["B"], c["W"]), 9200 + c["W"])
            od, oidx = oracle.scan_topk(ds, q, c["k"], h=c["h"])
        _inputs_cache[key] = (ds, ker, q, od, oidx)
    return _inputs_cache[key]


def run_case(dev, name):
    """One raw call: (d, idx, status, (path, n_sample_rows, grid_blocks), oracle d, oracle idx)."""
    from shadowing_amd import _native
    c = _case(name)
    ds, ker, q, od, oidx = _inputs(c)
    ds_t = torch.as_tensor(np.ascontiguousarray(ds[:, 0, :])).to(dev)
    q_t = torch.as_tensor(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    hint = None
    if c["hint"]:                                 # 1.1 x the acc = (d ||x||)^2 of every query's k-th window
        xn2 = (q.astype(np.float64) ** 2).sum(axis=1)
        hint = torch.as_tensor(((od[:, c["k"] - 1].astype(np.float64) ** 2) * xn2 * 1.1).astype(np.float32)).to(dev)
    info = {}
    if ker is None:
        d, idx, st = _native.scan_topk(ds_t, q_t, c["k"], h=c["h"], flags=c["flag_word"], tau_hint=hint, info=info)
    else:
        d, idx, st = _native.scan_topk_embedded(ds_t, torch.as_tensor(ker).to(dev), q_t, c["k"], h=c["h"], flags=c["flag_word"],
                                                tau_hint=hint, info=info)[:3]
    torch.cuda.synchronize(dev)
    return (d.cpu().numpy(), idx.cpu().numpy(), st.cpu().numpy(),
            (info["path"], info["n_sample_rows"], info["grid_blocks"]), od, oidx)


@pytest.fixture(scope="module")
def route_device(hip_device):
    ncu = torch.cuda.get_device_properties(hip_device).multi_processor_count
    if ncu != CU_COUNT:
        pytest.skip(f"the recorded grids are those of a device with {CU_COUNT} compute units, this one has {ncu}")
    return hip_device


@pytest.mark.parametrize("name", list(CASES))
def test_route_sample_and_grid_are_the_recorded_ones(route_device, name):
    d, idx, status, plan, od, oidx = run_case(route_device, name)
    path, n_sample_rows, grid_blocks, want_status = EXPECTED[name]
    assert plan == (path, n_sample_rows, grid_blocks), (name, plan)
    assert status.tolist() == want_status, (name, status.tolist())
    assert not status.any(), "every case of the table is served by its first call"
    assert_exact(d, idx, od, oidx, f"route table: {name}")
