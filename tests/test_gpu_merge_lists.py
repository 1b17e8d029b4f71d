"""The merges behind every sharded run (psh_select.hip: select_kernel through psh_merge_topk and psh_merge_topk_gathered,
merge_sorted_kernel through psh_merge_sorted_gathered) at the sizes of many ranks, emulated on one GPU: generated per-rank
lists (tests/_merge_lists.py) against a numpy lexsort on (distance bits, r, t), bit for bit over ALL k outputs.

Every general case names the branch of launch_select / select_kernel it is for in its id -- ordering stage (thread,
lds_ranking, network) and where the distance keys are read from (lds, global) -- and tests/test_merge_lists_cpu.py proves
that its input forces that branch: floods and single values make the second radix select over (r, t) happen, `few` puts
equal distances among the selected (pass 1 of the thread path, the full comparison elsewhere), `distinct` cannot.

Not covered: psh_exchange_merge on more than one rank.  With one rank G * k <= 32768 always holds, so its hand-over to the
general merge (G > 64 or G * k > 32768) is never taken end to end; the merges it would call are run here at such sizes
(65 x 1024 and 64 x 1024 lists)."""
import numpy as np
import pytest
import torch

import _merge_lists as ml
from shadowing_amd import _native

pytestmark = pytest.mark.gpu


def _host(*tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def _gathered(c, dev):
    return torch.from_numpy(ml.pack(*ml.case_lists(c))).to(dev)


def _reference(c):
    return ml.reference(*ml.flat(*ml.case_lists(c)), c.k)


def _check_general(c, dev):
    d, idx = ml.case_lists(c)
    rd, ri = _reference(c)
    sd, si = ml.flat_shuffled(d, idx, seed=c.k)
    md, mi = _host(*_native.merge_topk(torch.from_numpy(sd).to(dev), torch.from_numpy(si).to(dev), c.k))
    ml.assert_same(md, mi, rd, ri, "merge_topk (flat, shuffled)")
    gd, gi = _host(*_native.merge_topk_gathered(_gathered(c, dev), c.G, c.B, c.k_in, c.k))
    ml.assert_same(gd, gi, rd, ri, "merge_topk_gathered (rank-major)")
    return rd, ri


@pytest.mark.parametrize("c", ml.GENERAL, ids=[ml.case_id(c) for c in ml.GENERAL])
def test_general_merge_equals_the_lexsort(hip_device, c):
    rd, ri = _check_general(c, hip_device)
    n_real = sum(ml.real_counts(c.G, c.k_in, c.padding, dict(c.opts).get("empty")))
    if c.padding in ("short", "all"):                      # the real entries in order, then (+inf, -1, -1) only
        assert n_real < c.k and (ri[:, :n_real, 0] >= 0).all() and (ri[:, n_real:] == -1).all() and np.isposinf(rd[:, n_real:]).all()


@pytest.mark.parametrize("c", ml.SORTED, ids=[ml.case_id(c, False) for c in ml.SORTED])
def test_sorted_merge_equals_the_lexsort_and_the_general_merge(hip_device, c):
    assert _native.merge_sorted_supported(c.G, c.k_in)
    g = _gathered(c, hip_device)
    md, mi = _host(*_native.merge_sorted_gathered(g, c.G, c.B, c.k_in, c.k))
    ml.assert_same(md, mi, *_reference(c), "merge_sorted_gathered")
    if c.k <= 16384:                                       # PSH_MAX_K: where the general merge applies too
        gd, gi = _host(*_native.merge_topk_gathered(g, c.G, c.B, c.k_in, c.k))
        ml.assert_same(md, mi, gd, gi, "merge_sorted_gathered vs merge_topk_gathered")


@pytest.mark.parametrize("c", ml.INF_REAL, ids=[ml.case_id(c) for c in ml.INF_REAL])
def test_real_entries_at_inf_precede_padding_in_the_general_merge(hip_device, c):
    """A real entry (r >= 0) whose distance is +inf is a candidate like any other: skip_negative_rows leaves it in, so
    it follows the finite entries in (r, t) order and precedes the padding."""
    _check_general(c, hip_device)


@pytest.mark.parametrize("c", ml.INF_REAL, ids=[ml.case_id(c, False) for c in ml.INF_REAL])
def test_real_entries_at_inf_precede_padding_in_the_sorted_merge(hip_device, c):
    """The first list is padding only and the other two end in five real entries at +inf each.  merge_sorted_kernel
    ranks equal keys of a lower list first, so with padding keyed as +inf the first list's 64 padding entries came out
    before every real +inf entry.  Seen on the MI355X before the fix: of the 10 real +inf entries of a query, (-1, -1) in
    the place of 4 at k = 90 (ranks 86 .. 89) and of all 10 at k = 150, the general merge giving the reference's answer.
    Padding now takes a key above +inf when it is loaded."""
    g = _gathered(c, hip_device)
    md, mi = _host(*_native.merge_sorted_gathered(g, c.G, c.B, c.k_in, c.k))
    rd, ri = _reference(c)
    print("ranks holding padding before a real entry:",
          [int(((mi[b, :, 0] < 0) & (ri[b, :, 0] >= 0)).sum()) for b in range(c.B)])
    ml.assert_same(md, mi, rd, ri, "merge_sorted_gathered")
    gd, gi = _host(*_native.merge_topk_gathered(g, c.G, c.B, c.k_in, c.k))
    ml.assert_same(md, mi, gd, gi, "merge_sorted_gathered vs merge_topk_gathered")


@pytest.mark.parametrize("G,k_in,ok", [(64, 512, True), (65, 512, False), (64, 513, False)])
def test_sorted_merge_limits_are_refused_by_the_c_entry_as_the_wrapper_says(hip_device, G, k_in, ok):
    B, k = 2, 100
    assert _native.merge_sorted_supported(G, k_in) is ok
    d = np.full((G, B, k_in), np.inf, np.float32)
    g = torch.from_numpy(ml.pack(d, np.full((G, B, k_in, 2), -1, np.int32))).to(hip_device)
    if ok:
        md, mi = _host(*_native.merge_sorted_gathered(g, G, B, k_in, k))
        assert np.isposinf(md).all() and (mi == -1).all()
    else:
        with pytest.raises(_native.NativeLibraryError, match=r"code -2"):
            _native.merge_sorted_gathered(g, G, B, k_in, k)
