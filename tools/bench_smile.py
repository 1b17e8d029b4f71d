"""Hedged Monte Carlo smile: device time of psh_hedged_mc per call (median of repeats, HIP events) for the README case
(k = 8192, L = 20, Ts = 5 / 10 / 20) and the tutorial case (k = 8192, L = 252, Ts = 7 / 25 / 75), 9 strikes, at
B = 1, 16, 64; the numpy host path's seconds at B = 1; and a parity flag, device against host.  One JSON line."""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from shadowing_amd import _native, pricing  # noqa: E402

CASES = {"readme": (20, [5, 10, 20]), "tutorial": (252, [7, 25, 75])}


def returns(B, k, L, seed=0):
    g = np.random.default_rng(seed)
    sig = 0.2 * (0.5 + g.random((B, k, 1)))
    return (sig * math.sqrt(1 / 252) * g.standard_normal((B, k, L)) - 0.5 * sig ** 2 / 252).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,16,64")
    args = ap.parse_args()
    k, Ms = args.k, np.linspace(-2, 2, 9)
    res = {"k": k, "nM": len(Ms), "device_ms": {}, "host_s_B1": {}, "parity": True}
    for name, (L, Ts) in CASES.items():
        for B in [int(b) for b in args.batches.split(",")]:
            r = returns(B, k, L)
            w = np.random.default_rng(1).random((B, k))
            x, wt = torch.from_numpy(r).cuda(), torch.from_numpy(w).cuda()
            _native.hedged_mc(x, wt, Ts, Ms)                              # warm-up
            times = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = _native.hedged_mc(x, wt, Ts, Ms)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            res["device_ms"][f"{name}_B{B}"] = round(float(np.median(times)), 4)
            if B == 1:
                t0 = time.perf_counter()
                host = pricing.hedged_mc_host(r, w, Ts, Ms)
                res["host_s_B1"][name] = round(time.perf_counter() - t0, 4)
                ok = (np.allclose(out["price"].cpu().numpy(), host["price"], rtol=1e-9, atol=1e-12)
                      and np.allclose(out["iv"].cpu().numpy(), host["iv"], rtol=0, atol=1e-6, equal_nan=True))
                res["parity"] = bool(res["parity"] and ok)
    for name in CASES:
        if f"{name}_B64" in res["device_ms"]:
            res[f"speedup_{name}_B64_vs_64x_host_B1"] = round(64 * res["host_s_B1"][name] * 1e3 / res["device_ms"][f"{name}_B64"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
