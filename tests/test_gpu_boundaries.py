"""Every route of the route table (tests/test_gpu_routes.py) on ensembles with matches planted at every row, segment and
horizon edge (tests/_boundaries.py), at three geometries of the admissible count Tp = T - W - h + 1 against a segment of 1024
windows: `full` (Tp a multiple of 1024: the inadmissible zone starts on a segment boundary, h = 0), `one` (Tp = 1 mod 1024:
the last segment holds one window, h = 5) and `short` (Tp = 1023 mod 1024, h = W + 3: a whole exact copy of the query lies
inside the horizon zone).  Every scan kernel masks that zone in its own way; an exact copy of the query in it has distance 0,
so a kernel that lets one through returns it at rank 0, and one that drops the first or last window of a lane, a segment or
a row loses a plant whose rank is known.

One raw call per case, served by its first call (no fallback: that would be another kernel), on the route the table
records for the name; the result is bit-equal to the CPU oracle's, and the plants are where they must be -- no tolerance
anywhere.  tests/test_boundaries_cpu.py shows that the oracle alone meets the same conditions on the same inputs."""
import numpy as np
import pytest
import torch

import _boundaries as bd
from _util import assert_exact
from test_gpu_routes import CASES, CU_COUNT, EXPECTED

pytestmark = pytest.mark.gpu


def _case(name, geom):
    from shadowing_amd import _native
    c = bd.route_case(name, geom)
    c["flag_word"] = 0
    for f in c["flags"]:
        c["flag_word"] |= getattr(_native, "FLAG_" + f)
    return c


_inputs_cache = {}


def _inputs(c):
    """(ds (R, T) planted, kernel or None, the scan's queries, good, bad, oracle d, oracle idx, the raw query windows): once per
    shape, flags-blind."""
    key = (c["R"], c["T"], c["W"], c["h"], c["k"], c["B"], c["emb"])
    if key not in _inputs_cache:
        import oracle
        oracle.build()
        if c["emb"]:
            ds, ker, raw, q, good, bad = bd.embedded_inputs(c)
            od, oidx = oracle.scan_topk_embedded(ds, ker, q, c["k"], h=c["h"])
        else:
            ds, q, good, bad = bd.identity_inputs(c)
            ker, raw = None, q
            od, oidx = oracle.scan_topk(ds, q, c["k"], h=c["h"])
        _inputs_cache[key] = (ds, ker, q, good, bad, od, oidx, raw)
    return _inputs_cache[key]


@pytest.fixture(scope="module")
def route_device(hip_device):
    ncu = torch.cuda.get_device_properties(hip_device).multi_processor_count
    if ncu != CU_COUNT:
        pytest.skip(f"the recorded routes are those of a device with {CU_COUNT} compute units, this one has {ncu}")
    return hip_device


@pytest.mark.parametrize("geom", list(bd.GEOMETRIES))
@pytest.mark.parametrize("name", list(CASES))
def test_route_keeps_every_edge_plant_and_no_inadmissible_one(route_device, name, geom):
    from shadowing_amd import _native
    dev = route_device
    c = _case(name, geom)
    ds, ker, q, good, bad, od, oidx, _ = _inputs(c)
    W = c["emb"][2] if c["emb"] else c["W"]
    ds_t = torch.as_tensor(ds).to(dev)
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
    d, idx, st = d.cpu().numpy(), idx.cpu().numpy(), st.cpu().numpy()
    what = f"route {name}, geometry {geom}"
    print(f"{what}: R={c['R']} T={c['T']} W={W} h={c['h']} B={c['B']} path={info['path']} sample={info['n_sample_rows']} "
          f"grid={info['grid_blocks']} status={sorted(set(st.tolist()))}")
    assert info["path"] == EXPECTED[name][0], f"{what}: path {info['path']}, the table's is {EXPECTED[name][0]}"
    assert not st.any(), f"{what}: status words {st.tolist()}: not served by its first call"
    bd.check(d, idx, good, bad, c["T"], W, c["h"], what)
    assert_exact(d, idx, od, oidx, what)


def _assert_paths(paths, idx, ds, length, what):
    """paths (B, k, 1, length) are ds[r, t : t + length] bit for bit for every returned index."""
    assert paths.shape == idx.shape[:2] + (1, length), (what, paths.shape)
    want = np.lib.stride_tricks.sliding_window_view(ds, length, axis=1)[idx[..., 0], idx[..., 1]]
    assert np.array_equal(np.ascontiguousarray(paths[:, :, 0, :]).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), what
    flat = {(int(r), int(t)) for r, t in idx.reshape(-1, 2)}
    R, T = ds.shape
    assert (0, 0) in flat and (R - 1, T - length) in flat, f"{what}: the first and the last floats of the ensemble are gathered"


def test_blocking_fused_launch_gathers_the_edge_paths(hip_device):
    """PathShadowing.shadow of one Identity query: the blocking fused launch, which gathers the winners' paths itself -- the
    paths of (0, 0) and (R - 1, Tp - 1) begin with the first and end with the last float of the ensemble."""
    import shadowing_amd as sa
    c = _case("default", "one")
    ds, _, q, good, bad, od, oidx, _ = _inputs(c)
    W, h, k = c["W"], c["h"], c["k"]
    obj = sa.PathShadowing(sa.Identity(W), sa.RelativeMSE(), torch.as_tensor(ds[:, None, :]), sa.PredictionContext(horizon=h))
    d, paths, idx = obj.shadow(q[0], k=k, cuda=True)
    assert obj.last_path == "hip" and obj._sync_slot[1].last_fused
    what = "shadow(), Identity, geometry one"
    bd.check(d, idx, good, bad, c["T"], W, h, what)
    assert_exact(d, idx, od, oidx, what)
    _assert_paths(paths, idx, ds, W + h, what)


def test_foveal_shadow_gathers_the_edge_paths(hip_device):
    """Three queries behind Foveal: the embedded scan and the separate gather launch, geometry `short`."""
    import shadowing_amd as sa
    c = _case("emb_foveal", "short")
    c["B"] = 3
    ds, ker, q, good, bad, od, oidx, x = _inputs(c)
    K, h, k = c["emb"][2], c["h"], c["k"]
    fov = sa.Foveal(alpha=1.4, beta=0.9, max_context=K)
    assert np.array_equal(fov.kernel[:, 0, :].numpy(), ker)
    obj = sa.PathShadowing(fov, sa.RelativeMSE(), torch.as_tensor(ds[:, None, :]), sa.PredictionContext(horizon=h))
    d, paths, idx = obj.shadow(x, k=k, cuda=True)
    assert obj.last_path == "hip"
    what = "shadow(), Foveal, geometry short"
    bd.check(d, idx, good, bad, c["T"], K, h, what)
    assert_exact(d, idx, od, oidx, what)
    _assert_paths(paths, idx, ds, K + h, what)
