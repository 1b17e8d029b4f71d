"""Windows the copy scan's rejection test keeps per launch at the benchmark's sizes (the tuning build counts them in
FusedHdr::pad[12]: PSH_LIB=shadowing_amd/lib/libpsh_hip_tuning.so python tools/filter_copy_survivors.py), and how many of them
are admitted below the level."""
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from shadowing_amd import _native, synthetic as syn  # noqa: E402

R, T, W, h, k = 32768, 4096, 20, 20, 1024
dev = torch.device("cuda", 0)
ds = torch.from_numpy(syn.dataset(R, T, seed=0)).to(dev)
_native.FILTER_COPY_POLICY = "first"
ws = _native.Workspace(dev)
out = []
for seed in [syn.QUERY_SEED, 1001, 1002, 1003]:
    q = torch.from_numpy(syn.single_query(W, seed)[None, :].copy()).to(dev)
    info = {}
    _native.scan_topk(ds[:, 0, :], q, k, h=h, workspace=ws, flags=_native.FLAG_OVERLAP, info=info)      # (sizes the workspace)
    torch.cuda.synchronize()
    ws.buf[60:64].zero_()                                    # FusedHdr::pad[12]
    d, idx, st = _native.scan_topk(ds[:, 0, :], q, k, h=h, workspace=ws, flags=_native.FLAG_OVERLAP, info=info)
    torch.cuda.synchronize()
    kept = int(ws.buf[60:64].view(torch.int32).item())
    lay = _native.candidates_layout(R, T, 1, W, h, k, ws.buf.numel())
    admitted = int(ws.buf[lay["hdr_stream_ncand"]: lay["hdr_stream_ncand"] + 4].view(torch.int32).item())
    out.append({"query_seed": int(seed), "copy_served": info["copy_served"], "status": int(st[0]), "windows_kept_by_the_test": kept,
                "windows_admitted": admitted, "windows": R * (T - W - h + 1)})
print(json.dumps(out))
