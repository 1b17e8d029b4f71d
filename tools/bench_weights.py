"""psh_softmax_weights against what it replaces, all in one process, for B x k = 1 x 8192, 64 x 8192 and 252 x 8192 (a year
of dates) and E = 1 and 16 weight sets (four etas x four cut-offs k, k/2, k/4, k/8; E = 1: eta = 0.1, k' = k).
Device ms per call (median of --reps calls per round, HIP events, the cases alternating over --rounds rounds after a warm-up
round; the median over rounds is reported):
  kernel_ms            psh_softmax_weights on ascending rows, as every scan returns them (the network is skipped);
  kernel_shuffled_ms   the same rows shuffled (the network runs): what the skip is worth;
  write_GBps           the (E, B, k) float64 it writes over kernel_ms.
Wall-clock ms (median of --host-reps):
  host_form_ms, upload_ms   PathShadowing._score_weights on the host's copy of the distances, and the upload of its
                            (E, B, k) weights: what every device_weights=False call pays between the scan and the kernel;
  score_ms, score_device_weights_ms   PathShadowing.score() end to end (scan, gather, realised variance, weights, scores)
                            on a 256 x 1024 ensemble, without and with device_weights, alternating.
The kernel's weights are checked against the numpy twin within (2 k' + 16) 2^-53 w + 2^-1070, and the largest share of the
bound is reported.  One JSON line.  PSH_LIB=... times another build."""
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
from shadowing_amd import _native, synthetic as syn, weights  # noqa: E402

K = 8192
ROWS = (1, 64, 252)
ETAS = (0.1, 0.05, 0.075, 0.2)


def grid(E):
    return (ETAS, (K, K // 2, K // 4, K // 8)) if E == 16 else (ETAS[:1], (K,))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds after the warm-up round")
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    names = ("kernel_ms", "kernel_shuffled_ms")
    res = {"reps": args.reps, "rounds": args.rounds, **{n: {} for n in names}, "write_GBps": {}, "host_form_ms": {}, "upload_ms": {},
           "score_ms": {}, "score_device_weights_ms": {}, "share_of_bound": 0.0, "parity": True}

    g = np.random.default_rng(1)
    inputs = {}
    for B in ROWS:
        asc = np.sort((0.3 + 0.2 * g.random((B, K))).astype(np.float32), axis=1)
        inputs[B] = (asc, torch.from_numpy(asc).to(dev), torch.from_numpy(g.permuted(asc, axis=1)).to(dev))

    # ---- the kernel
    cases = [(B, E) for B in ROWS for E in (1, 16)]
    ms = {(n, c): [] for n in names for c in cases}
    for rnd in range(args.rounds + 1):                                          # round 0 warms up
        for B, E in cases:
            etas, ks = grid(E)
            _, d_asc, d_shuf = inputs[B]
            for name, d in zip(names, (d_asc, d_shuf)):
                t = _median_ms(lambda: _native.softmax_weights(d, etas, ks), args.reps if rnd else 2)
                if rnd:
                    ms[(name, (B, E))].append(t)

    # ---- score() end to end: one object, the two routes alternating
    ds = syn.dataset(256, 1024, 0)
    obj = sa.PathShadowing(sa.Identity(20), sa.RelativeMSE(), ds, sa.PredictionContext(horizon=20), cache=True)
    stat = lambda x: sa.realized_variance(x[:, :, 0, :], [5, 20])                 # noqa: E731
    e2e = {(flag, c): [] for flag in (False, True) for c in cases}
    for rnd in range(args.rounds + 1):
        for B, E in cases:
            etas, ks = grid(E)
            q = syn.rolling_queries(B, 20, 1)
            x_real = (0.01 * np.random.default_rng(3).standard_normal((B, 1, 20))).astype(np.float32)
            for flag in (False, True):
                t = _wall_ms(lambda: obj.score(q, x_real, K, stat, etas, ks, cuda=True, device_predict=True, device_weights=flag),
                             args.host_reps if rnd else 1)
                assert obj.last_weights == ("device" if flag else "host") and obj.last_score_reduction == "device"
                if rnd:
                    e2e[(flag, (B, E))].append(t)

    for B, E in cases:
        etas, ks = grid(E)
        asc, d_asc, d_shuf = inputs[B]
        tag = f"{B}x{K} E={E}"
        for name in names:
            res[name][tag] = round(float(np.median(ms[(name, (B, E))])), 4)
        res["write_GBps"][tag] = round(E * B * K * 8 / (res["kernel_ms"][tag] * 1e-3) / 1e9, 1)
        res["score_ms"][tag] = round(float(np.median(e2e[(False, (B, E))])), 3)
        res["score_device_weights_ms"][tag] = round(float(np.median(e2e[(True, (B, E))])), 3)
        formed = []
        res["host_form_ms"][tag] = round(_wall_ms(lambda: formed.append(obj._score_weights("softmax", asc, etas, ks)[0]),
                                                  args.host_reps), 3)
        res["upload_ms"][tag] = round(_wall_ms(lambda: torch.from_numpy(formed[-1]).to(dev), args.host_reps), 4)
        ref = weights.softmax_weights(asc, etas, ks, cuda=False)
        for d in (d_asc, d_shuf):
            got = _native.softmax_weights(d, etas, ks).cpu().numpy().reshape(ref.shape)
            r = weights.softmax_weights(d.cpu().numpy(), etas, ks, cuda=False) if d is d_shuf else ref
            for c, kc in enumerate(ks):
                share = np.abs(got[:, c] - r[:, c]) / ((2 * kc + 16) * 2.0 ** -53 * r[:, c] + 2.0 ** -1070)
                res["share_of_bound"] = round(max(res["share_of_bound"], float(share.max())), 4)
                res["parity"] = bool(res["parity"] and float(share.max()) <= 1.0 and np.array_equal(got[:, c] == 0.0, r[:, c] == 0.0))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
