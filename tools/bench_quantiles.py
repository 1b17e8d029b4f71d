"""psh_weighted_quantiles against what bounds it and what replaces it, all in one process: device ms per call (median of
--reps calls per round, HIP events, the cases alternating over --rounds rounds after a warm-up round; the median over rounds
is reported) for the statistic shapes B x k x m = 1 x 8192 x 3, 64 x 8192 x 3 and 256 x 1024 x 8.  The statistic is realised
variance made on the device from a generated MRW ensemble (B k paths of 64 returns), the weights are the Softmax class's.
Per shape: the kernel; psh_weighted_moments on the same input (one read: the floor); the same three quantities composed
from torch ops on the device (torch.sort, cumsum, searchsorted, gather -- written here only: what a user could do without
leaving HBM and without the kernel); and the host route, a copy down plus the numpy twin.  The kernel's results are checked
against the twin under the comparison rule of the tests, and the largest share of the error bound is reported.  One JSON
line.  PSH_LIB=... times another build."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import shadowing_amd as sa  # noqa: E402
from shadowing_amd import _native, quantiles  # noqa: E402

SHAPES = ((1, 8192, 3), (64, 8192, 3), (256, 1024, 8))
LEVELS = np.array([0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99])
N_RETURNS, ETA, SEED = 64, 0.2, 1


def _median_ms(call, reps):
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def torch_composition(v, w, levels):
    """q, lower, upper of the definition from torch ops: v (B, k, m) float32, w (B, k) float64, levels (Q,) float64."""
    B, k, m = v.shape
    xs, order = torch.sort(v, dim=1, stable=True)
    xs = xs.to(torch.float64)
    ws = w[:, :, None].expand(B, k, m).gather(1, order)
    C, S = ws.cumsum(1).transpose(1, 2).contiguous(), (ws * xs).cumsum(1).transpose(1, 2).contiguous()    # (B, m, k)
    xs = xs.transpose(1, 2).contiguous()
    W, Stot = C[:, :, -1:], S[:, :, -1:]
    t = levels[None, None, :] * W                                                                       # (B, m, Q)
    i = torch.searchsorted(C, t).clamp(max=k - 1)
    ip = (i - 1).clamp(min=0)
    xq, Ci, Si = xs.gather(2, i), C.gather(2, i), S.gather(2, i)
    Cp = torch.where(i > 0, C.gather(2, ip), torch.zeros_like(t))
    Sp = torch.where(i > 0, S.gather(2, ip), torch.zeros_like(t))
    lower = (Sp + (t - Cp) * xq) / t
    upper = ((Ci - t) * xq + (Stot - Si)) / (W - t)
    return xq.transpose(1, 2), lower.transpose(1, 2), upper.transpose(1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds after the warm-up round")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lv_dev = torch.from_numpy(LEVELS).to(dev)
    res = {"levels": LEVELS.tolist(), "reps": args.reps, "rounds": args.rounds, "kernel_ms": {}, "moments_ms": {},
           "torch_ops_ms": {}, "host_ms": {}, "kernel_over_torch_ops": {}, "max_share_of_bound": 0.0, "edges": 0, "parity": True}
    inputs = {}
    for B, k, m in SHAPES:
        ens = sa.mrw_log_returns(B * k, N_RETURNS, seed=SEED + k, cuda=True)
        Ts = [N_RETURNS * (j + 1) // m for j in range(m)]
        v = sa.realized_variance(ens.reshape(B, k, N_RETURNS), Ts).contiguous()
        g = np.random.default_rng(SEED + B)
        w = np.ascontiguousarray(sa.Softmax(0.3 + 0.2 * g.random((B, k)), ETA).weights, dtype=np.float64)
        inputs[(B, k, m)] = (v, torch.from_numpy(w).to(dev), w)

    def host_route(v, w):
        return quantiles._host_quantiles(v.cpu().numpy(), w, LEVELS)

    calls = {"kernel_ms": lambda v, wd, w: _native.weighted_quantiles(v, wd, LEVELS),
             "moments_ms": lambda v, wd, w: _native.weighted_moments(v, wd),
             "torch_ops_ms": lambda v, wd, w: torch_composition(v, wd, lv_dev)}
    ms = {(name, s): [] for name in calls for s in SHAPES}
    for rnd in range(args.rounds + 1):                                          # round 0 warms up
        for s in SHAPES:
            v, wd, w = inputs[s]
            for name, fn in calls.items():
                t = _median_ms(lambda: fn(v, wd, w), args.reps if rnd else 2)
                if rnd:
                    ms[(name, s)].append(t)
    for s in SHAPES:
        B, k, m = s
        v, wd, w = inputs[s]
        tag = f"{B}x{k}x{m}"
        for name in calls:
            res[name][tag] = round(float(np.median(ms[(name, s)])), 4)
        res["kernel_over_torch_ops"][tag] = round(res["kernel_ms"][tag] / res["torch_ops_ms"][tag], 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route(v, w)
        res["host_ms"][tag] = round((time.perf_counter() - t0) * 1e3, 2)
        # parity under the tests' rule: q equal off the edges, the tail means inside the bound
        q, lo, up, st, det = quantiles._host_quantiles(v.cpu().numpy(), w, LEVELS, detail=True)
        gq, glo, gup, gst = (a.cpu().numpy() for a in _native.weighted_quantiles(v, wd, LEVELS))
        near = det["edge"] & ((gq == det["q_prev"]) | (gq == det["q_next"]))
        share = max(float((np.abs(glo - lo) / det["bound_lower"]).max()), float((np.abs(gup - up) / det["bound_upper"]).max()))
        res["max_share_of_bound"] = round(max(res["max_share_of_bound"], share), 4)
        res["edges"] += int(det["edge"].sum())
        tq, tlo, tup = (a.cpu().numpy() for a in torch_composition(v, wd, lv_dev))
        res["parity"] = bool(res["parity"] and ((gq == q) | near).all() and share <= 1.0 and not gst.any() and not st.any()
                             and np.allclose(tlo, lo, rtol=1e-9, atol=0.0) and np.allclose(tup, up, rtol=1e-9, atol=0.0))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
