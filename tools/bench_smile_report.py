"""The hedge report of a smile: device time per call (median of repeats, HIP events) of psh_hedged_mc, psh_hedged_mc_policy
and psh_hedge_replay (in-sample, without and with the per-path pnl), in one process, at the shapes of tools/bench_smile.py:
the README case (k = 8192, L = 20, Ts = 5 / 10 / 20) and the tutorial case (k = 8192, L = 252, Ts = 7 / 25 / 75), 9
strikes, B = 1, 16, 64; and a parity flag, the device report against the numpy twin at B = 1.  One JSON line."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from shadowing_amd import _native, pricing  # noqa: E402
from bench_smile import CASES, returns  # noqa: E402


def median_ms(fn, reps):
    fn()                                                                  # warm-up
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return round(float(np.median(times)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--degree", type=int, default=3)
    args = ap.parse_args()
    k, Ms, P = args.k, np.linspace(-2, 2, 9), args.degree
    res = {"k": k, "nM": len(Ms), "degree": P, "fit_ms": {}, "fit_policy_ms": {}, "replay_ms": {}, "replay_pnl_ms": {},
           "parity": True}
    for name, (L, Ts) in CASES.items():
        for B in [int(b) for b in args.batches.split(",")]:
            r = returns(B, k, L)
            w = np.random.default_rng(1).random((B, k))
            x, wt = torch.from_numpy(r).cuda(), torch.from_numpy(w).cuda()
            key = f"{name}_B{B}"
            res["fit_ms"][key] = median_ms(lambda: _native.hedged_mc(x, wt, Ts, Ms, degree=P), args.reps)
            res["fit_policy_ms"][key] = median_ms(lambda: _native.hedged_mc(x, wt, Ts, Ms, degree=P, policy=True), args.reps)
            fit = _native.hedged_mc(x, wt, Ts, Ms, degree=P, policy=True)
            replay = lambda pnl: _native.hedge_replay(x, wt, Ts, Ms, fit["policy"], fit["strike"], fit["price"], degree=P,  # noqa: E731
                                                      return_pnl=pnl)
            res["replay_ms"][key] = median_ms(lambda: replay(False), args.reps)
            res["replay_pnl_ms"][key] = median_ms(lambda: replay(True), args.reps)
            if B == 1:
                tw = pricing.hedged_mc_host(r, w, Ts, Ms, degree=P, policy=True)
                tr = pricing.replay_host(r, w, Ts, Ms, tw["policy"], tw["strike"], tw["price"], degree=P)
                ok = (np.allclose(fit["price"].cpu().numpy(), tw["price"], rtol=1e-9, atol=1e-9)
                      and np.allclose(replay(False)["sums"].cpu().numpy(), tr["sums"], rtol=1e-9, atol=1e-9))
                res["parity"] = bool(res["parity"] and ok)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
