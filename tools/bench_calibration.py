"""psh_calibrate_weights against what it replaces, all in one process: k = 8192 paths of 75 steps, J = 30 instruments (Ts 7 / 25 /
75, 9 strikes each, the three forwards), B = 1, 64 and 252 dates (a year), eps = 1e-6 and 1e-3.  The quotes are a skewed
Black-Scholes smile (MarketQuotes(ivs=...)), the prior is uniform.
Device ms per call (median of --reps calls per round, HIP events, the cases alternating over --rounds rounds after a warm-up
round; the median over rounds is reported):
  kernel_ms     psh_calibrate_weights, both launches, with `steps`, the most Newton steps a date took;
  one_pass_ms   the same call with max_iter = 0: the terminal-price launch, the input checks, one Phi and one gradient /
                Hessian pass -- what the first launch and a single pass of the second cost (the two launches are enqueued
                back to back, so this is the nearest thing to a split that a caller can time);
  torch_ms      the same iteration composed from torch on the device, batched over dates: the (B, k, J) matrix h built from
                the returns, then `steps` full Newton steps of matmul, exp, cholesky and cholesky_solve (no line search);
  floor_ms      arithmetic, nothing measured: steps * k J^2 / 2 double FMAs on one workgroup's share (1 / 256) of the
                3.2e13 FMA/s that tools/bench_stylized.py measured from registers; `ratio` = kernel_ms / floor_ms.
Wall-clock ms (median of --host-reps):
  host_ms       the host route: the (B, k, 75) float32 paths copied down, then the numpy twin;
  calibrate_ms, calibrate_device_weights_ms   PathShadowing.calibrate() end to end (scan, gather, prior, calibration) on a
                256 x 1024 ensemble, without and with device_weights, alternating.
The kernel's lambda is checked against the twin's on the first date (`max_dlam`).  One JSON line.  PSH_LIB=... times another
build."""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import shadowing_amd as sa  # noqa: E402
from shadowing_amd import _native, calibration as cal, synthetic as syn  # noqa: E402

K, L, X0 = 8192, 75, 100.0
TS, MS = (7, 25, 75), np.linspace(-1.5, 1.5, 9)
ROWS = (1, 64, 252)
EPS = (1e-6, 1e-3)
FMA_PER_S_PER_WORKGROUP = 3.2e13 / 256


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


def _wall_ms(call, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def quotes():
    strikes = np.stack([X0 * np.exp(MS * 0.2 * math.sqrt(T / 252.0)) for T in TS])
    ivs = 0.2 - 0.15 * np.log(strikes / X0)
    return sa.MarketQuotes(TS, strikes, ivs=ivs)


def torch_newton(x, strike, target, eps, steps):
    """The iteration in torch, batched over dates: unit prior, full steps."""
    B, k, _ = x.shape
    l = torch.cumsum(x.to(torch.float64), dim=2)
    S = X0 * torch.exp(l[:, :, [T - 1 for T in TS]])                                  # (B, k, nT)
    Sj = S.repeat_interleave(len(MS), dim=2)
    call = (strike.reshape(B, 1, -1) >= X0)
    g = torch.where(call, Sj - strike.reshape(B, 1, -1), strike.reshape(B, 1, -1) - Sj).clamp_min(0.0)
    h = torch.cat([(g - target.reshape(B, 1, -1)) / X0, (S - X0) / X0], dim=2)        # (B, k, J)
    J = h.shape[2]
    lam = torch.zeros((B, J, 1), dtype=torch.float64, device=x.device)
    eye = eps * torch.eye(J, dtype=torch.float64, device=x.device)
    for _ in range(steps):
        a = torch.matmul(h, lam)
        e = torch.exp(a - a.amax(dim=1, keepdim=True))
        q = e / e.sum(dim=1, keepdim=True)
        mu = torch.matmul(h.transpose(1, 2), q)
        H = torch.matmul(h.transpose(1, 2), q * h) - torch.matmul(mu, mu.transpose(1, 2)) + eye
        lam = lam + torch.cholesky_solve(-(mu + eps * lam), torch.linalg.cholesky_ex(H).L)
    return lam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds after the warm-up round")
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    mq = quotes()
    names = ("kernel_ms", "one_pass_ms", "torch_ms")
    res = {"reps": args.reps, "rounds": args.rounds, **{n: {} for n in names}, "steps": {}, "status": {}, "floor_ms": {}, "ratio": {},
           "host_ms": {}, "calibrate_ms": {}, "calibrate_device_weights_ms": {}, "max_dlam": 0.0}
    g = np.random.default_rng(1)
    r_all = (g.standard_t(4, size=(max(ROWS), K, L)) * (0.2 / math.sqrt(252.0) / math.sqrt(2.0))).astype(np.float32)
    x_all = torch.from_numpy(r_all).to(dev)
    cases = [(B, eps) for B in ROWS for eps in EPS]
    dev_in, steps = {}, {}
    for B in ROWS:
        strike, target = mq.arrays(B, X0, 0.0)
        dev_in[B] = (x_all[:B].contiguous(), torch.from_numpy(strike).to(dev), torch.from_numpy(target).to(dev))
    run = lambda B, eps, it=100: _native.calibrate_weights(*dev_in[B][:1], None, TS, *dev_in[B][1:], X0, 0.0, 0, True, eps, 1e-8, it)  # noqa: E731
    for B, eps in cases:
        out = run(B, eps)
        steps[(B, eps)] = int(out["info"][:, 2].max())
        res["status"][f"{B}x{K} eps={eps:g}"] = sorted(set(out["status"].cpu().tolist()))
    ms = {(n, c): [] for n in names for c in cases}
    for rnd in range(args.rounds + 1):                                          # round 0 warms up
        for B, eps in cases:
            calls = (lambda: run(B, eps), lambda: run(B, eps, 0),
                     lambda: torch_newton(*dev_in[B], eps, max(steps[(B, eps)], 1)))
            for name, call in zip(names, calls):
                t = _median_ms(call, args.reps if rnd else 2)
                if rnd:
                    ms[(name, (B, eps))].append(t)

    # ---- calibrate() end to end: one object, the two routes alternating
    ds = syn.dataset(256, 1024, 0)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=L), cache=True)
    e2e = {(flag, c): [] for flag in (False, True) for c in cases}
    for rnd in range(args.rounds + 1):
        for B, eps in cases:
            q = syn.rolling_queries(B, 20, 1)
            for flag in (False, True):
                t = _wall_ms(lambda: obj.calibrate(q, K, mq, eta=0.1, eps=eps, cuda=True, device_weights=flag), args.host_reps if rnd else 1)
                assert obj.last_weights == ("device" if flag else "host") and obj.last_path == "hip"
                if rnd:
                    e2e[(flag, (B, eps))].append(t)

    for B, eps in cases:
        tag = f"{B}x{K} eps={eps:g}"
        for name in names:
            res[name][tag] = round(float(np.median(ms[(name, (B, eps))])), 4)
        res["steps"][tag] = steps[(B, eps)]
        J = len(TS) * len(MS) + len(TS)
        res["floor_ms"][tag] = round(steps[(B, eps)] * K * J * J / 2 / FMA_PER_S_PER_WORKGROUP * 1e3, 4)
        res["ratio"][tag] = round(res["kernel_ms"][tag] / max(res["floor_ms"][tag], 1e-9), 2)
        res["calibrate_ms"][tag] = round(float(np.median(e2e[(False, (B, eps))])), 3)
        res["calibrate_device_weights_ms"][tag] = round(float(np.median(e2e[(True, (B, eps))])), 3)
        strike, target = mq.arrays(B, X0, 0.0)
        host = []
        res["host_ms"][tag] = round(_wall_ms(lambda: host.append(cal.calibrate_host(dev_in[B][0].cpu().numpy(), None, TS, strike, target, X0,
                                                                                    0.0, 0, True, eps)), 1 if B > 1 else args.host_reps), 2)
        res["max_dlam"] = max(res["max_dlam"], float(np.abs(run(B, eps)["lam"][0].cpu().numpy() - host[-1]["lam"][0]).max()))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
