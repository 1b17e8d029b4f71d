"""psh_lagged_moments against its numpy twin and against two floors measured in the same run: device ms per call (median
of --reps calls per round, HIP events, the cases alternating over --rounds rounds after a warm-up round; the median over
rounds is reported) for R x n = 2048 x 4096 and 32768 x 4096, m = 40, 256, 1024, G = 64, on a skewed-MRW ensemble made on
the device; the seconds of the twin as ONE run on 256 rows SCALED to the row count (it is linear in R); the time of a
kernel that reads the ensemble once (psh_realized_variance over the full length); and the time of 4 R n (m + 1) double FMAs
at the rate a register-only FMA loop (tools/ubench_fma64.hip) reaches here.  Every case is checked against the twin on
the first 256 rows at the bound of tests/test_gpu_stylized.py.  One JSON line.  PSH_LIB=... times another build."""
import argparse
import ctypes
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
from shadowing_amd import _build, _native, mrw, stylized  # noqa: E402

ROWS, N, LAGS, G = (2048, 32768), 4096, (40, 256, 1024), 64
TWIN_ROWS, TWIN_G = 256, 4
LAM, K0, ALPHA, SEED = 0.2, 0.1, 0.6, 1


def _fma_library() -> ctypes.CDLL:
    """tools/bin/libubench_fma64.so, compiled when it is missing or was built from another source text."""
    import hashlib
    src, lib = HERE / "ubench_fma64.hip", HERE / "bin" / "libubench_fma64.so"
    stamp, digest = lib.with_suffix(".so.srchash"), hashlib.sha256(src.read_bytes()).hexdigest()
    if not lib.exists() or not stamp.exists() or stamp.read_text().strip() != digest:
        lib.parent.mkdir(exist_ok=True)
        subprocess.run([_build.hipcc_path(), "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", str(src), "-o", str(lib)],
                       check=True)
        stamp.write_text(digest + "\n")
    L = ctypes.CDLL(str(lib))
    L.fma64_rate.restype = ctypes.c_double
    L.fma64_rate.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return L


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
    ap.add_argument("--build-only", action="store_true", help="compile tools/ubench_fma64.hip and stop (no device needed)")
    args = ap.parse_args()
    fma = _fma_library()
    if args.build_only:
        return
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"n": N, "G": G, "reps": args.reps, "rounds": args.rounds, "twin_rows": TWIN_ROWS, "twin_scaled": True,
           "device_ms": {}, "twin_s": {}, "speedup": {}, "read_floor_ms": {}, "fma_floor_ms": {}, "over_larger_floor": {},
           "max_err_over_bound": 0.0, "parity": True}
    rates = [fma.fma64_rate(ncu * w, 4096, 5) for w in (2, 4, 8)]
    res["fma64_per_s"] = max(rates)
    if res["fma64_per_s"] <= 0.0:
        raise RuntimeError("the FMA loop failed to run")
    ens = {R: mrw.smrw_log_returns(R, N, K0, ALPHA, lam=LAM, seed=SEED, cuda=True) for R in ROWS}
    cases = [(R, m) for R in ROWS for m in LAGS]
    ms = {c: [] for c in cases}
    read = {R: [] for R in ROWS}
    for rnd in range(args.rounds + 1):                                          # round 0 warms up
        for R, m in cases:
            t = _median_ms(lambda: _native.lagged_moments(ens[R], m, G), args.reps if rnd else 2)
            if rnd:
                ms[(R, m)].append(t)
        for R in ROWS:
            t = _median_ms(lambda: _native.realized_variance(ens[R], [N]), args.reps if rnd else 2)
            if rnd:
                read[R].append(t)
    head = ens[ROWS[0]][:TWIN_ROWS, 0]
    host = head.cpu().numpy()
    for m in LAGS:
        t0 = time.perf_counter()
        sums, rows = stylized._host_sums(host, m, TWIN_G)
        twin_s = time.perf_counter() - t0
        mag, _ = stylized._host_sums(np.abs(host), m, TWIN_G)
        d_sums, d_rows, _ = _native.lagged_moments(head, m, TWIN_G)
        bound = 2.0 * (rows[:, None, None] * (N - np.arange(m + 1)) + 2) * 2.0 ** -53 * mag
        ratio = float((np.abs(d_sums.cpu().numpy() - sums) / bound).max())
        res["max_err_over_bound"] = max(res["max_err_over_bound"], ratio)
        res["parity"] = bool(res["parity"] and ratio <= 1.0 and np.array_equal(d_rows.cpu().numpy(), rows))
        for R in ROWS:
            name = f"R{R}_m{m}"
            dev = float(np.median(ms[(R, m)]))
            res["device_ms"][name] = round(dev, 4)
            res["twin_s"][name] = round(twin_s * R / TWIN_ROWS, 2)
            res["speedup"][name] = round(twin_s * R / TWIN_ROWS * 1e3 / dev, 1)
            res["read_floor_ms"][name] = round(float(np.median(read[R])), 4)
            res["fma_floor_ms"][name] = round(4.0 * R * N * (m + 1) / res["fma64_per_s"] * 1e3, 4)
            res["over_larger_floor"][name] = round(dev / max(res["read_floor_ms"][name], res["fma_floor_ms"][name]), 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
