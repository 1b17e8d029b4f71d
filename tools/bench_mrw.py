"""MRW ensemble generation: device ms per psh_mrw_generate call writing the (R, 1, n) float32 returns (median of repeats,
HIP events) and the seconds of the numpy twin on the same seed (one run), for R x T = 2048 x 4097 (the tutorial's first
cell) and 32768 x 4097 (ensemble-sized), H = 0.5 and H = 0.3; plus a parity flag, device against twin.  --scan: the
one-query step of bench.py (W = 20, h = 20, k = 1024, three streams, the overlap-friendly launches) on the 32768 x 4096 MRW
ensemble and on synthetic.dataset of the same shape in the same process, in alternating rounds, every status word looked
at and the results checked against the CPU oracle.  One JSON line.  PSH_LIB=... times another build of the library;
--no-host skips the twin."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from shadowing_amd import _native, mrw, synthetic as syn  # noqa: E402

CASES = [(2048, 4097), (32768, 4097)]
HS = (0.5, 0.3)
LAM, SEED = 0.2, 1
TWIN_ROWS = 2048                  # the twin runs this many paths; its time for more is scaled (it is linear in R)


def generation(args, res):
    dev = torch.device("cuda", torch.cuda.current_device())
    for R, T in CASES:
        n = T - 1
        for H in HS:
            name = f"R{R}_T{T}_H{H}"
            a_om, a_eps = mrw._device_tables(n, H, LAM, float(n), dev)
            c0 = float(mrw.mrw_covariance(0, float(n), LAM))
            buf = torch.empty((R, 1, n), dtype=torch.float32, device=dev)

            def call():
                return _native.mrw_generate(R, n, mrw.DEFAULT_SIGMA, a_om, a_eps, c0, seed=SEED, outputs=("dlnx",),
                                            dlnx_out=buf)
            call()                                                             # warm-up
            times = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            res["device_ms"][name] = round(float(np.median(times)), 4)
            res["device_ms_min"][name] = round(float(np.min(times)), 4)
            if args.no_host:
                continue
            rows = min(R, TWIN_ROWS)
            t0 = time.perf_counter()
            host = mrw.mrw_log_returns(rows, n, H=H, lam=LAM, seed=SEED)
            res["host_s"][name] = round((time.perf_counter() - t0) * R / rows, 3)
            res["speedup"][name] = round(res["host_s"][name] * 1e3 / res["device_ms"][name], 1)
            ok = np.allclose(buf[:rows].cpu().numpy(), host, rtol=2.0 ** -23, atol=1e-9 * mrw.DEFAULT_SIGMA)
            res["parity"] = bool(res["parity"] and ok)
            del host
        del buf


def scan(args, res):
    import oracle
    oracle.build()
    dev = torch.device("cuda", torch.cuda.current_device())
    R, n, W, h, k, NS, NQ = 32768, 4096, 20, 20, 1024, 3, 4
    sets = {"mrw": mrw.mrw_log_returns(R, n, seed=SEED, cuda=True),
            "gaussian": torch.from_numpy(syn.dataset(R, n, 0)).to(dev)}
    # four distinct queries per ensemble, each an unseen history of the ensemble's own law
    q_hosts = {"mrw": [np.ascontiguousarray(mrw.mrw_log_returns(1, n, seed=1000 + j)[0, :, 1000:1000 + W]) for j in range(NQ)],
               "gaussian": [np.ascontiguousarray(syn.single_query(W, 1000 + j)[None, :]) for j in range(NQ)]}
    qs = {key: [torch.from_numpy(q).to(dev) for q in v] for key, v in q_hosts.items()}
    hosts = {key: v.cpu().numpy() for key, v in sets.items()}
    streams = [torch.cuda.Stream(dev) for _ in range(NS)]
    wss = [_native.Workspace(dev) for _ in range(NS)]
    outs = [(torch.empty((1, k), dtype=torch.float32, device=dev), torch.empty((1, k, 2), dtype=torch.int32, device=dev))
            for _ in range(NS)]
    ring = list(torch.zeros((args.steps + 8, 1), dtype=torch.int32, device=dev).unbind(0))

    def region(key, steps):
        last = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in range(steps):
            si, qi = c % NS, c % NQ
            last[si] = qi
            with torch.cuda.stream(streams[si]):
                _native.scan_topk(sets[key][:, 0, :], qs[key][qi], k, h=h, workspace=wss[si], flags=_native.FLAG_OVERLAP,
                                  out=(outs[si][0], outs[si][1], ring[c % len(ring)]))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / steps, last

    times = {"mrw": [], "gaussian": []}
    status, parity = 0, True
    expected = {}
    for rnd in range(args.rounds + 1):                                         # round 0 warms up
        for key in ("mrw", "gaussian"):
            for t in ring:
                t.zero_()
            us, last = region(key, args.steps)
            status = max(status, int(torch.stack(ring).max().item()))
            for si, qi in last.items():                                        # what each stream's buffers must hold
                if (key, qi) not in expected:
                    expected[(key, qi)] = oracle.scan_topk(hosts[key], q_hosts[key][qi], k, h=h)
                od, oidx = expected[(key, qi)]
                parity = parity and np.array_equal(outs[si][0].cpu().numpy().view(np.uint32), od.view(np.uint32)) and \
                    np.array_equal(outs[si][1].cpu().numpy(), oidx)
            if rnd:
                times[key].append(us)
    res["scan"] = {"R": R, "T": n, "W": W, "h": h, "k": k, "streams": NS, "steps": args.steps, "rounds": args.rounds,
                   "us_per_step": {key: round(float(np.median(v)), 2) for key, v in times.items()},
                   "us_per_step_min": {key: round(float(np.min(v)), 2) for key, v in times.items()},
                   "mrw_over_gaussian": round(float(np.median(times["mrw"]) / np.median(times["gaussian"])), 3),
                   "status_max": status, "parity_vs_oracle": bool(parity)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--scan", action="store_true", help="also time the one-query scan step on the MRW and the Gaussian ensemble")
    ap.add_argument("--steps", type=int, default=300, help="--scan: steps per timed region")
    ap.add_argument("--rounds", type=int, default=5, help="--scan: alternating rounds after the warm-up round")
    args = ap.parse_args()
    res = {"lam": LAM, "device_ms": {}, "device_ms_min": {}, "host_s": {}, "speedup": {}, "parity": True}
    generation(args, res)
    if args.scan:
        scan(args, res)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
