"""NaN / +-inf samples in an ensemble behind a linear embedding: the rows split once, the exact top-k from the two parts.

The reference's conv1d makes a window NaN when ANY tap of its zero-padded kernel meets a non-finite sample (0 * NaN; ref
path_embedding.py:48-51, :129-132).  The embedded scans' rejection tests assume finite data (prefix sums and matrix-core tiles
spread a NaN over clean windows); the dense chains of the exhaustive path multiply all K taps, zeros included, and so meet a NaN
exactly where the conv does once the horizon is smeared in.  So the rows without such a sample (almost all) keep the sampled
scan, the few that hold one go through the dense chains, and the two lists are merged by (d, r, t).  Used by PathShadowing
(one split per resident copy) and by ShardedPathShadowing (one per shard: no rank has to know about another's rows).
"""
from __future__ import annotations

import torch

from . import _native


def _numbered(idx: torch.Tensor, rows: torch.Tensor, row_offset: int) -> torch.Tensor:
    """`idx` (B, k, 2) with its row numbers -- positions in `rows` -- replaced by the ensemble's own, plus `row_offset`."""
    idx = idx.clone()
    idx[..., 0] = (rows[idx[..., 0].long()] + row_offset).to(torch.int32)
    return idx


class DirtyRows:
    """The split of a resident (R, C, T) ensemble: `clean_idx` / `dirty_idx` (row numbers, ascending), `clean_rows` (a contiguous
    (Rc, T) copy of channel 0) and `dirty_rows` (channel 0 with every non-finite sample written back over the `back` samples in
    front of it; None without a dirty row)."""

    def __init__(self, ds: torch.Tensor, back: int):
        flags = _native.rows_nonfinite(ds)
        self.back = back
        self.T = int(ds.shape[-1])
        self.dirty_idx = torch.nonzero(flags).flatten()
        self.clean_idx = torch.nonzero(flags == 0).flatten()
        self.clean_rows = ds[self.clean_idx, 0, :].contiguous()
        self.dirty_rows = _native.smear_nonfinite(ds[self.dirty_idx].contiguous(), back, 0) if self.dirty_idx.numel() else None

    def topk(self, hx: torch.Tensor, ker: torch.Tensor, k: int, h: int, workspace, flags: int, row_offset: int = 0,
             one_window: bool = False):
        """The exact (d (B, k), idx (B, k, 2)) of the k best windows for the embedded queries `hx` (B, d) behind `ker` (d, K), NaN
        windows last (ref path_shadowing.py:165), row numbers the ensemble's plus `row_offset`.  `flags`: what the clean rows'
        scan takes (FLAG_EMBED_MX).  `one_window`: rows one window long, scanned as R pre-embedded points."""
        Tp = self.T - ker.shape[-1] - h + 1
        n_clean, n_dirty = int(self.clean_idx.numel()) * Tp, int(self.dirty_idx.numel()) * Tp
        parts = []
        if n_clean > 0:
            kc = min(k, n_clean)
            if one_window:
                dc, ic = _native.scan_topk_checked(_native.embed_rows(self.clean_rows, ker), hx, kc, h=0, workspace=workspace)
            elif kc == k:
                dc, ic = _native.scan_topk_embedded_checked(self.clean_rows, ker, hx, kc, h=h, workspace=workspace, flags=flags)
            else:   # every clean window is wanted: nothing to sample for
                dc, ic, _ = _native.scan_topk_embedded(self.clean_rows, ker, hx, kc, h=h, workspace=workspace, exhaustive=True,
                                                       flags=flags)
            parts.append((dc, _numbered(ic, self.clean_idx, row_offset)))
        if n_dirty > 0 and (n_clean < k or not one_window):
            kd = min(k, n_dirty)
            if one_window:
                # a dirty row IS its one window: NaN, ranked behind every clean one
                dd = torch.full((hx.shape[0], kd), float("nan"), dtype=torch.float32, device=hx.device)
                idd = torch.zeros((hx.shape[0], kd, 2), dtype=torch.int32, device=hx.device)
                idd[..., 0] = (self.dirty_idx[:kd] + row_offset).to(torch.int32)[None, :]
            else:
                # (EMBED_DENSE: every one of the K taps is multiplied, zeros included -- the suffix-rows walk would skip the
                #  taps in front of Foveal's longest row, where the conv still meets a NaN)
                dd, idd, _ = _native.scan_topk_embedded(self.dirty_rows, ker, hx, kd, h=h, workspace=workspace, exhaustive=True,
                                                        flags=_native.FLAG_EMBED_DENSE)
                idd = _numbered(idd, self.dirty_idx, row_offset)
            parts.append((dd, idd))
        if len(parts) == 1 and parts[0][0].shape[1] == k:
            return parts[0]
        return _native.merge_topk(torch.cat([p[0] for p in parts], dim=1).contiguous(),
                                  torch.cat([p[1] for p in parts], dim=1).contiguous(), k)
