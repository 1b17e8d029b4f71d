"""psh_separate_topk against what it replaces and beside the scan it follows, all in one process (README "Separated
neighbours" holds the numbers).  Device ms per call: median of --reps calls per round, HIP events, the cases alternating over
--rounds rounds after a warm-up round; the median over rounds is reported.
  kernel_ms        psh_separate_topk at K = 1024, 4096, 16384 for B = 1, 64, 252, k = 4 K / 5, on two kinds of list:
                   "scan"   the Identity(20) scan's own K nearest windows of a 4096 x 1024 SMRW ensemble, delta = 19 and 1;
                   "worst"  one row whose positions rise with t at delta = 1: the most rounds the kernel can take;
  scan_ms          the scan that produced the list (psh_scan_topk at K), and kernel_over_scan = kernel_ms / scan_ms;
  host_ms          the host alternative, wall clock, once: (d, idx) copied down and the numpy twin; host_over_kernel;
  shadow_ms        PathShadowing.shadow(cuda=True) of 64 queries, k = 1024, without and with separation = 19, alternating
                   (wall clock, median of --host-reps; the one-query blocking slot is not involved): what scanning for K1
                   instead of k, separating and coming back costs; `served` says which K served and in how many scans;
  kept_share       of the 1024 and the 8192 nearest windows of four SMRW queries (seed 9) in a 32768 x 4096 SMRW ensemble
                   (K0 = 0.1, alpha = 0.6, lam = 0.2, seed 1, generated on the device), the number an exclusion zone of
                   delta = 1, 5, 19 keeps, smallest .. largest over the queries, for Identity(20) and Foveal(1.15, 0.9, 126).
Every device result is checked against the twin.  One JSON line.  PSH_LIB=... times another build."""
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
from shadowing_amd import _native  # noqa: E402

SMRW = dict(K0=0.1, alpha=0.6, lam=0.2)
KS, ROWS, H = (1024, 4096, 16384), (1, 64, 252), 20


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


def _same(dev_out, twin) -> bool:
    got = [t.cpu().numpy() for t in dev_out]
    want = (twin.distances, twin.indices, twin.positions, twin.count, twin.status)
    return all(np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds after the warm-up round")
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true", help="leave the 32768 x 4096 kept shares out")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"reps": args.reps, "rounds": args.rounds, "kernel_ms": {}, "scan_ms": {}, "kernel_over_scan": {}, "host_ms": {},
           "host_over_kernel": {}, "kept": {}, "shadow_ms": {}, "kept_share": {}, "parity": True}

    # ---- the lists: the scan's own output, and the worst case
    ens = sa.smrw_log_returns(4096, 1024, seed=1, cuda=True, **SMRW)                       # (R, 1, T) on the device
    rows = ens[:, 0, :].contiguous()
    qs = sa.smrw_log_returns(max(ROWS), H, seed=9, **SMRW)[:, 0, :]
    ws = _native.Workspace(dev)
    lists, scans = {}, {}
    for K in KS:
        for B in ROWS:
            q = torch.from_numpy(np.ascontiguousarray(qs[:B])).to(dev)
            scans[(K, B)] = lambda q=q, K=K: _native.scan_topk(rows, q, K, h=H, workspace=ws)      # (the raw call: no wait)
            d, idx = _native.scan_topk_checked(rows, q, K, h=H, workspace=ws)
            lists[("scan", K, B)] = (d.contiguous(), idx.contiguous())
            i = torch.arange(K, dtype=torch.int32, device=dev)
            worst = torch.stack([torch.full_like(i, 7), i], dim=1)[None].repeat(B, 1, 1).contiguous()
            lists[("worst", K, B)] = (d.contiguous(), worst)
    cases = [("scan", K, B, 19) for K in KS for B in ROWS] + [("scan", K, B, 1) for K in KS for B in ROWS] \
        + [("worst", K, B, 1) for K in KS for B in ROWS]
    ms = {c: [] for c in cases}
    sms = {kb: [] for kb in scans}
    for rnd in range(args.rounds + 1):                                                  # round 0 warms up
        for c in cases:
            kind, K, B, delta = c
            d, idx = lists[(kind, K, B)]
            t = _median_ms(lambda: _native.separate_topk(d, idx, 4 * K // 5, delta), args.reps if rnd else 2)
            if rnd:
                ms[c].append(t)
        for kb, scan in scans.items():
            t = _median_ms(scan, args.reps if rnd else 2)
            if rnd:
                sms[kb].append(t)
    for kb in scans:
        res["scan_ms"][f"{kb[1]}x{kb[0]}"] = round(float(np.median(sms[kb])), 4)
    for c in cases:
        kind, K, B, delta = c
        tag = f"{kind} {B}x{K} delta={delta}"
        res["kernel_ms"][tag] = round(float(np.median(ms[c])), 4)
        if kind == "scan":
            res["kernel_over_scan"][tag] = round(res["kernel_ms"][tag] / res["scan_ms"][f"{B}x{K}"], 4)

    # ---- the host alternative, and parity
    for c in cases:
        kind, K, B, delta = c
        if delta != 19 and kind == "scan":
            continue
        tag = f"{kind} {B}x{K} delta={delta}"
        d, idx = lists[(kind, K, B)]
        held = []
        res["host_ms"][tag] = round(_wall_ms(lambda: held.append(sa.separate_topk(d.cpu().numpy(), idx.cpu().numpy(), 4 * K // 5,
                                                                                  delta, cuda=False)), 1), 2)
        res["host_over_kernel"][tag] = round(res["host_ms"][tag] / res["kernel_ms"][tag], 1)
        res["kept"][tag] = [int(held[-1].count.min()), int(held[-1].count.max())]
        res["parity"] = bool(res["parity"] and _same(_native.separate_topk(d, idx, 4 * K // 5, delta), held[-1]))

    # ---- shadow() of a batch without and with the keyword
    q = qs[:64]
    objs = {sep: sa.PathShadowing(sa.Identity(H), sa.RelativeMSE(), ens, sa.PredictionContext(H), separation=sep)
            for sep in (None, 19)}
    wall = {sep: [] for sep in objs}
    for rnd in range(args.rounds + 1):
        for sep, obj in objs.items():
            t = _wall_ms(lambda: obj.shadow(q, k=1024, cuda=True), args.host_reps if rnd else 1)
            assert obj.last_path == "hip"
            if rnd:
                wall[sep].append(t)
    ls = objs[19].last_separation
    res["shadow_ms"] = {"plain": round(float(np.median(wall[None])), 3), "separation=19": round(float(np.median(wall[19])), 3),
                        "served": {"K": int(ls["K"]), "scans": int(ls["scans"]),
                                   "count": [int(ls["count"].min()), int(ls["count"].max())]}}
    del objs, lists, scans, rows, ens

    # ---- the kept share at 32768 x 4096
    if not args.skip_large:
        big = sa.smrw_log_returns(32768, 4096, seed=1, cuda=True, **SMRW)
        for name, emb, W in (("Identity(20)", sa.Identity(20), 20), ("Foveal(1.15, 0.9, 126)", sa.Foveal(1.15, 0.9, 126), 126)):
            obj = sa.PathShadowing(emb, sa.RelativeMSE(), big, sa.PredictionContext(H))
            x = torch.from_numpy(sa.smrw_log_returns(4, W, seed=9, **SMRW))
            d, idx, _ = obj._native_scan(x, obj._dataset_tensor(), 8192)
            for K in (1024, 8192):
                dk, ik = d[:, :K].contiguous(), idx[:, :K].contiguous()
                for delta in (1, 5, 19):
                    out = _native.separate_topk(dk, ik, 1, delta)
                    cnt = out[3].cpu().numpy()
                    res["kept_share"][f"{name} K={K} delta={delta}"] = [int(cnt.min()), int(cnt.max())]
                    if K == 1024:
                        twin = sa.separate_topk(dk.cpu().numpy(), ik.cpu().numpy(), 1, delta, cuda=False)
                        res["parity"] = bool(res["parity"] and _same(out, twin))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
