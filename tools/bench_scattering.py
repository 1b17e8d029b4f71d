"""psh_scattering_spectra against its numpy twin and against two figures measured in the same process, for comparison only:
device ms per call (median of --reps calls per round, HIP events, the cases alternating over --rounds rounds after a warm-up
round; the median over rounds is reported) for R x n = 2048 x 4096 and 32768 x 4096, J = 9, G = 64, on a skewed-MRW ensemble
made on the device; the seconds of the twin as ONE run on 64 rows SCALED to the row count (it is linear in R); the time of a
kernel that reads the ensemble once (psh_realized_variance over the full length); and psh_mrw_generate on the same R at
n = 2048, which is R / 2 transforms of 4096 points plus the draws, against the R (2 J + 1) transforms of 4096 points here:
`per_transform_over_mrw` is (ms / R (2 J + 1)) / (mrw ms / (R / 2)).  The first 64 rows are checked against the twin at the
bound of tests/test_gpu_scattering.py.  One JSON line.  PSH_LIB=... times another build."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from shadowing_amd import _native, mrw, scattering  # noqa: E402

ROWS, N, J, G = (2048, 32768), 4096, 9, 64
MRW_N = 2048
TWIN_ROWS, TWIN_G = 64, 4
LAM, K0, ALPHA, SEED = 0.2, 0.1, 0.6, 1
BOUND = 1e-9


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


def _families(v):
    P3, P4 = J * (J + 1) // 2, J * (J + 1) * (J + 2) // 6
    o4 = 2 * J + 2 * P3
    return (v[:, :J], v[:, J:2 * J], v[:, 2 * J:2 * J + P3] + 1j * v[:, 2 * J + P3:o4], v[:, o4:o4 + P4] + 1j * v[:, o4 + P4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds after the warm-up round")
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"n": N, "J": J, "G": G, "reps": args.reps, "rounds": args.rounds, "twin_rows": TWIN_ROWS, "twin_scaled": True,
           "device_ms": {}, "twin_s": {}, "speedup": {}, "read_ms": {}, "mrw_generate_ms": {}, "per_transform_over_mrw": {},
           "over_read": {}, "max_err_over_bound": 0.0, "parity": True}
    ens = {R: mrw.smrw_log_returns(R, N, K0, ALPHA, lam=LAM, seed=SEED, cuda=True) for R in ROWS}
    psi = scattering._device_bank(N, J, dev)
    a_om, _ = mrw._device_tables(MRW_N, 0.5, LAM, float(MRW_N), dev)
    c0 = float(mrw.mrw_covariance(0, float(MRW_N), LAM))
    gen = {R: torch.empty((R, 1, MRW_N), dtype=torch.float32, device=dev) for R in ROWS}
    calls = {"scat": lambda R: _native.scattering_spectra(ens[R], J, G, psi),
             "read": lambda R: _native.realized_variance(ens[R], [N]),
             "mrw": lambda R: _native.mrw_generate(R, MRW_N, mrw.DEFAULT_SIGMA, a_om, None, c0, seed=SEED, outputs=("dlnx",),
                                                   dlnx_out=gen[R])}
    ms = {(name, R): [] for name in calls for R in ROWS}
    for rnd in range(args.rounds + 1):                                          # round 0 warms up
        for name, call in calls.items():
            for R in ROWS:
                t = _median_ms(lambda: call(R), args.reps if rnd else 2)
                if rnd:
                    ms[(name, R)].append(t)
    head = ens[ROWS[0]][:TWIN_ROWS, 0]
    host = head.cpu().numpy()
    t0 = time.perf_counter()
    sums, rows = scattering._host_sums(host, scattering.scattering_bank(N, J), TWIN_G)
    twin_s = time.perf_counter() - t0
    d_sums, d_rows, _ = _native.scattering_spectra(head, J, TWIN_G, psi)
    for d, t in zip(_families(d_sums.cpu().numpy()), _families(sums)):
        ratio = float((np.abs(d - t) / (BOUND * np.abs(t).max(axis=1, keepdims=True))).max())
        res["max_err_over_bound"] = max(res["max_err_over_bound"], ratio)
    res["parity"] = bool(res["max_err_over_bound"] <= 1.0 and np.array_equal(d_rows.cpu().numpy(), rows))
    for R in ROWS:
        name = f"R{R}"
        dev_ms, read, gen_ms = (float(np.median(ms[(k, R)])) for k in ("scat", "read", "mrw"))
        res["device_ms"][name] = round(dev_ms, 4)
        res["twin_s"][name] = round(twin_s * R / TWIN_ROWS, 2)
        res["speedup"][name] = round(twin_s * R / TWIN_ROWS * 1e3 / dev_ms, 1)
        res["read_ms"][name] = round(read, 4)
        res["mrw_generate_ms"][name] = round(gen_ms, 4)
        res["over_read"][name] = round(dev_ms / read, 1)
        res["per_transform_over_mrw"][name] = round((dev_ms / (R * (2 * J + 1))) / (gen_ms / (R / 2)), 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
