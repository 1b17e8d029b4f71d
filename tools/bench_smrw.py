"""Skewed MRW ensemble generation against the plain MRW's: device ms per psh_smrw_generate call (memory m = n) and per
psh_mrw_generate call (H = 0.5), both writing the (R, 1, n) float32 returns, in one process and in alternating rounds
(median of repeats per round, HIP events; the median over rounds is reported, and their ratio), for R x T = 2048 x 4097
and 32768 x 4097; plus the seconds of the numpy twin on the same seed (one run of at most 2048 paths, scaled) and a
parity flag, device against twin.  One JSON line.  PSH_LIB=... times another build of the library; --no-host skips the
twin."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from shadowing_amd import _native, mrw  # noqa: E402

CASES = [(2048, 4097), (32768, 4097)]
LAM, K0, ALPHA, SEED = 0.2, 0.1, 0.6, 1
TWIN_ROWS = 2048                  # the twin runs this many paths; its time for more is scaled (it is linear in R)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds after the warm-up round")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"lam": LAM, "K0": K0, "alpha": ALPHA, "reps": args.reps, "rounds": args.rounds, "smrw_ms": {}, "mrw_ms": {},
           "smrw_over_mrw": {}, "host_s": {}, "speedup": {}, "parity": True}
    for R, T in CASES:
        n = T - 1
        name = f"R{R}_T{T}"
        a_om, _ = mrw._device_tables(n, 0.5, LAM, float(n), dev)
        c0 = float(mrw.mrw_covariance(0, float(n), LAM))
        K = mrw.smrw_kernel(n, K0, ALPHA)
        k_hat = torch.from_numpy(mrw._k_hat(K, mrw._embedding_size(n))).to(dev)
        v = float(np.sum(K ** 2))
        buf = torch.empty((R, 1, n), dtype=torch.float32, device=dev)
        calls = {"mrw": lambda: _native.mrw_generate(R, n, mrw.DEFAULT_SIGMA, a_om, None, c0, seed=SEED, outputs=("dlnx",),
                                                     dlnx_out=buf),
                 "smrw": lambda: _native.smrw_generate(R, n, n, mrw.DEFAULT_SIGMA, a_om, k_hat, c0, v, seed=SEED,
                                                       outputs=("dlnx",), dlnx_out=buf)}
        ms = {"mrw": [], "smrw": []}
        for rnd in range(args.rounds + 1):                                      # round 0 warms up
            for key in ("mrw", "smrw"):
                t = _median_ms(calls[key], args.reps if rnd else 2)
                if rnd:
                    ms[key].append(t)
        res["mrw_ms"][name] = round(float(np.median(ms["mrw"])), 4)
        res["smrw_ms"][name] = round(float(np.median(ms["smrw"])), 4)
        res["smrw_over_mrw"][name] = round(float(np.median(ms["smrw"]) / np.median(ms["mrw"])), 3)
        if not args.no_host:
            rows = min(R, TWIN_ROWS)
            t0 = time.perf_counter()
            host = mrw.smrw_log_returns(rows, n, K0, ALPHA, lam=LAM, seed=SEED)
            res["host_s"][name] = round((time.perf_counter() - t0) * R / rows, 3)
            res["speedup"][name] = round(res["host_s"][name] * 1e3 / res["smrw_ms"][name], 1)
            calls["smrw"]()                                                     # buf holds the skewed ensemble again
            ok = np.allclose(buf[:rows].cpu().numpy(), host, rtol=2.0 ** -23, atol=1e-9 * mrw.DEFAULT_SIGMA)
            res["parity"] = bool(res["parity"] and ok)
            del host
        del buf
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
