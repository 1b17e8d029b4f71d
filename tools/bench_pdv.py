"""PDV path generation: device ms per psh_pdv_generate call writing sigma and St (median of repeats, HIP events), and the
seconds of the numpy twin on the same seed (one run), for (B, S, n_steps) = (1, 8192, 75), (64, 8192, 75) and the
ensemble-sized (1, 32768, 4096); plus a parity flag, device against twin.  One JSON line.  PSH_LIB=... times another
build of the library; --no-host skips the twin."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from shadowing_amd import _native, pdv  # noqa: E402

CASES = [(1, 8192, 75), (64, 8192, 75), (1, 32768, 4096)]
DT = 1 / 252


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--nu", type=float, default=0.0, help="Student-t degrees of freedom of the draws (0: Gaussian)")
    args = ap.parse_args()
    m = pdv.PDVModelDiscrete([60.0, 4.0], [40.0, 1.5], [0.6, 0.3], [0.04, -0.12, 0.6, 0.5], nu=args.nu or None)
    dec1, dec2 = (np.exp(-lam[None, :] / 252)[0] for lam in (m.lams1, m.lams2))
    res = {"nu": args.nu, "device_ms": {}, "host_s": {}, "speedup": {}, "parity": True}
    for B, S, n in CASES:
        name = f"B{B}_S{S}_n{n}"
        R10, R20 = np.tile([0.0, 0.01], (B, 1)), np.tile([0.04, 0.03], (B, 1))

        def call():
            return _native.pdv_generate(B, S, n, m.lams1, m.lams2, dec1, dec2, m.thetas, m.betas, 100.0, np.sqrt(DT),
                                        args.nu, R10, R20, seed=1, outputs=("sigma", "St"))
        out = call()                                                           # warm-up
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        res["device_ms"][name] = round(float(np.median(times)), 4)
        if args.no_host:
            continue
        t0 = time.perf_counter()
        host = m._host(B, S, n, 100.0, DT, R10, R20, 1, None)
        res["host_s"][name] = round(time.perf_counter() - t0, 3)
        res["speedup"][name] = round(res["host_s"][name] * 1e3 / res["device_ms"][name], 1)
        for key in ("sigma", "St"):
            d = out[key].cpu().numpy()
            ok = np.array_equal(np.isnan(d), np.isnan(host[key])) and np.allclose(d, host[key], rtol=1e-9, atol=0,
                                                                                  equal_nan=True)
            res["parity"] = bool(res["parity"] and ok)
        del out, host
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
