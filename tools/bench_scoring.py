"""psh_score_ensemble against what bounds it and what replaces it, all in one process: device ms per call (median of --reps
calls per round, HIP events, the cases alternating over --rounds rounds after a warm-up round; the median over rounds is
reported) for the statistic shapes B x k x m = 1 x 8192 x 3, 64 x 8192 x 3 and 256 x 1024 x 8 and E = 1, 4, 16 weight sets.
The statistic is realised variance made on the device from a generated MRW ensemble (B k paths of 64 returns), the
observation the same statistic of one more path a query, the weight sets the Softmax class's on the k' nearest of random
distances (eta in 0.05, 0.075, 0.1, 0.2; k' in k, k/2, k/4, k/8).  Per shape and E: the kernel; psh_weighted_quantiles with
seven levels on the same input and the first weight set (the cost of the sort alone); the same scores composed from torch
ops on the device (one torch.sort, then gather, cumsum and elementwise ops looped over the sets -- written here only: what a
user could do without leaving HBM and without the kernel); the host route, a copy down plus the numpy twin; and, apart, the
upload of the (E, B, k) weights.  The kernel's results are checked against the twin within the bounds of the tests, and the
largest share of each bound is reported.  One JSON line.  PSH_LIB=... times another build."""
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
from shadowing_amd import _native, scoring  # noqa: E402

SHAPES = ((1, 8192, 3), (64, 8192, 3), (256, 1024, 8))
SETS = (1, 4, 16)
LEVELS = np.array([0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99])
ETAS = (0.1, 0.05, 0.075, 0.2)
N_RETURNS, SEED = 64, 1


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


def torch_composition(v, w, y):
    """crps, pit_lo, pit_hi, mean of the definition from torch ops: v (B, k, m) float32, w (E, B, k) float64, y (B, m)
    float32.  The weightless paths stay in the chain (a gap they split is the same integral in two pieces)."""
    B, k, m = v.shape
    xs, order = torch.sort(v, dim=1, stable=True)
    xs = xs.to(torch.float64)
    yd = y.to(torch.float64)[:, None, :]
    xa, xb = xs[:, :-1], xs[:, 1:]
    c = torch.minimum(torch.maximum(yd, xa), xb)
    below, not_above = xs < yd, xs <= yd
    edge = (xs[:, 0] - yd[:, 0]).clamp(min=0) + (yd[:, 0] - xs[:, -1]).clamp(min=0)
    out = []
    for e in range(w.shape[0]):
        ws = w[e][:, :, None].expand(B, k, m).gather(1, order)
        C = ws.cumsum(1)
        W = C[:, -1:]
        Ci = C[:, :-1]
        G = (Ci * Ci * (c - xa) + (W - Ci) * (W - Ci) * (xb - c)).sum(1)
        out.append((edge + G / (W[:, 0] * W[:, 0]), (ws * below).sum(1) / W[:, 0], (ws * not_above).sum(1) / W[:, 0],
                    (ws * xs).sum(1) / W[:, 0]))
    return [torch.stack([o[n] for o in out]) for n in range(4)]


def bounds(v, w, y):
    """The tests' tolerances, (E, B, m): crps 8 (k + 4) 2^-53 span, pit 2 (k + 2) 2^-53, mean 2 (k + 2) 2^-53 sum w |x| / W."""
    k, eps = v.shape[1], 2.0 ** -53
    pos, x = (w > 0)[:, :, :, None], v.astype(np.float64)[None]
    hi = np.maximum(np.where(pos, x, -np.inf).max(axis=2), y[None])
    lo = np.minimum(np.where(pos, x, np.inf).min(axis=2), y[None])
    A = (np.where(pos, np.abs(x), 0.0) * w[:, :, :, None]).sum(axis=2)
    return 8.0 * (k + 4) * eps * (hi - lo), 2.0 * (k + 2) * eps, 2.0 * (k + 2) * eps * A / w.sum(axis=2)[:, :, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds after the warm-up round")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    names = ("kernel_ms", "quantiles_ms", "torch_ops_ms")
    res = {"reps": args.reps, "rounds": args.rounds, **{n: {} for n in names}, "host_ms": {}, "weight_upload_ms": {},
           "share_of_bound": {"crps": 0.0, "pit": 0.0, "mean": 0.0}, "parity": True}
    inputs = {}
    for B, k, m in SHAPES:
        ens = sa.mrw_log_returns(B * (k + 1), N_RETURNS, seed=SEED + k, cuda=True).reshape(B, k + 1, N_RETURNS)
        Ts = [N_RETURNS * (j + 1) // m for j in range(m)]
        stat = sa.realized_variance(ens, Ts)
        v, y = stat[:, :k].contiguous(), stat[:, k].contiguous()
        g = np.random.default_rng(SEED + B)
        d = np.sort(0.3 + 0.2 * g.random((B, k)), axis=1)
        w = np.zeros((max(SETS), B, k))
        for e in range(max(SETS)):
            kc = k >> (e // len(ETAS))
            w[e, :, :kc] = np.asarray(sa.Softmax(d[:, :kc], ETAS[e % len(ETAS)]).weights, dtype=np.float64)
        perm = g.permuted(np.tile(np.arange(k), (B, 1)), axis=1)         # the nearest paths lie anywhere in the value order
        w = np.ascontiguousarray(np.take_along_axis(w, np.broadcast_to(perm, w.shape), axis=2))
        inputs[(B, k, m)] = (v, y, torch.from_numpy(w).to(dev), w)

    cases = [(s, E) for s in SHAPES for E in SETS]
    calls = {"kernel_ms": lambda v, y, wd: _native.score_ensemble(v, wd, y),
             "quantiles_ms": lambda v, y, wd: _native.weighted_quantiles(v, wd[0], LEVELS),
             "torch_ops_ms": lambda v, y, wd: torch_composition(v, wd, y)}
    ms = {(name, c): [] for name in calls for c in cases}
    for rnd in range(args.rounds + 1):                                          # round 0 warms up
        for s, E in cases:
            v, y, wd, _ = inputs[s]
            wd = wd[:E].contiguous()
            for name, fn in calls.items():
                t = _median_ms(lambda: fn(v, y, wd), args.reps if rnd else 2)
                if rnd:
                    ms[(name, (s, E))].append(t)
    for s, E in cases:
        B, k, m = s
        v, y, wd, w = inputs[s]
        wd, w = wd[:E].contiguous(), np.ascontiguousarray(w[:E])
        tag = f"{B}x{k}x{m} E={E}"
        for name in calls:
            res[name][tag] = round(float(np.median(ms[(name, (s, E))])), 4)
        ups = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.from_numpy(w).to(dev)
            torch.cuda.synchronize()
            ups.append((time.perf_counter() - t0) * 1e3)
        res["weight_upload_ms"][tag] = round(float(np.median(ups)), 4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vh, yh = v.cpu().numpy(), y.cpu().numpy()
        ref = scoring._host_scores(vh, w, yh)
        res["host_ms"][tag] = round((time.perf_counter() - t0) * 1e3, 2)
        got = [a.cpu().numpy() for a in _native.score_ensemble(v, wd, y)]
        tor = [a.cpu().numpy() for a in torch_composition(v, wd, y)]
        b_crps, b_pit, b_mean = bounds(vh, w, yh.astype(np.float64))
        shares = {"crps": np.abs(got[0] - ref[0]) / b_crps, "pit": np.maximum(np.abs(got[1] - ref[1]), np.abs(got[2] - ref[2])) / b_pit,
                  "mean": np.abs(got[3] - ref[3]) / b_mean}
        for n, sh in shares.items():
            res["share_of_bound"][n] = round(max(res["share_of_bound"][n], float(sh.max())), 4)
        res["parity"] = bool(res["parity"] and all(float(sh.max()) <= 1.0 for sh in shares.values()) and not got[4].any()
                             and not ref[4].any() and all(np.allclose(tor[n], ref[n], rtol=1e-9, atol=1e-12) for n in range(4)))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
