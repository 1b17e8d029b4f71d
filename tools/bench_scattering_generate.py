"""psh_scattering_vjp and scattering_generate on the device, with psh_scattering_spectra measured in the same process as the
yardstick: device ms per call (median of --reps calls after two warm-up calls, HIP events) of the gradient and of the forward
sums for R x n = 2048 x 4096 and 32768 x 4096, J = 9, G = 64, on a skewed-MRW ensemble made on the device, the gradient
written into a buffer allocated once; `vjp_over_forward` against the (5 J + 2) / (2 J + 1) = 2.47 of the transform counts;
then ONE generation of 256 and of 2048 rows of 4096 (batch 256, the defaults: 200 evaluations at the most, tol 1e-3) against
the spectra of the 2048-row ensemble: wall seconds, evaluations and sqrt(loss) before and after, per batch.  One JSON line.
PSH_LIB=... times another build."""
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
GEN_ROWS = (256, 2048)
LAM, K0, ALPHA, SEED = 0.2, 0.1, 0.6, 1


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
    ap.add_argument("--max-eval", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"n": N, "J": J, "G": G, "reps": args.reps, "transforms_vjp_over_forward": round((5 * J + 2) / (2 * J + 1), 2),
           "forward_ms": {}, "vjp_ms": {}, "vjp_over_forward": {}, "generate": {}}
    psi = scattering._device_bank(N, J, dev)
    cot = torch.from_numpy(np.random.default_rng(SEED).standard_normal((G, scattering.n_outputs(J)))).to(dev)
    target = None
    for R in ROWS:
        ens = mrw.smrw_log_returns(R, N, K0, ALPHA, lam=LAM, seed=SEED, cuda=True)
        grad = torch.empty((R, N), dtype=torch.float64, device=dev)
        calls = {"forward_ms": lambda: _native.scattering_spectra(ens, J, G, psi),
                 "vjp_ms": lambda: _native.scattering_vjp(ens, J, G, psi, cot, out=grad)}
        for name, call in calls.items():
            _median_ms(call, 2)
            res[name][f"R{R}"] = round(_median_ms(call, args.reps), 4)
        res["vjp_over_forward"][f"R{R}"] = round(res["vjp_ms"][f"R{R}"] / res["forward_ms"][f"R{R}"], 2)
        if target is None:
            target = scattering.scattering_spectra(ens, J=J)
        del ens, grad
    for R in GEN_ROWS:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, info = scattering.scattering_generate(target, R, max_eval=args.max_eval, seed=SEED, cuda=True, return_info=True)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        got = scattering.scattering_spectra(x, J=J)
        res["generate"][f"R{R}"] = {
            "seconds": round(wall, 3), "evaluations": info["evaluations"],
            "ms_per_evaluation": round(1e3 * wall / sum(info["evaluations"]), 3),
            "sqrt_loss_start": [round(float(np.sqrt(v)), 5) for v in info["initial_loss"]],
            "sqrt_loss_end": [round(float(np.sqrt(v)), 5) for v in info["final_loss"]],
            "im_phi3_1_3": round(float(got.phi3[0, 2].imag), 5), "target_im_phi3_1_3": round(float(target.phi3[0, 2].imag), 5),
            "target_im_phi3_1_3_se": round(float(target.phi3_se[0, 2]), 5)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
