"""What tests/test_gpu_merge_lists.py asks of the merges are properties of its INPUTS and of its reference, not of the code
under test: every generated case meets the conditions the kernels rely on (sorted lists, row blocks, unique (r, t)), the
flood cases force the second radix select, the distinct cases cannot reach it, reference() equals the project's oracle on
lists cut from real scans, the comparison has teeth, and plan() gives the launcher's literals."""
import numpy as np
import pytest

import _merge_lists as ml
from shadowing_amd import synthetic as syn

ALL = [(c, True) for c in ml.GENERAL + ml.INF_REAL] + [(c, False) for c in ml.SORTED + ml.INF_REAL]
IDS = [("general-" if g else "sorted-") + ml.case_id(c, g) for c, g in ALL]


@pytest.mark.parametrize("c", [c for c, _ in ALL], ids=IDS)
def test_every_case_meets_the_conditions(c):
    d, idx = ml.case_lists(c)
    assert d.shape == (c.G, c.B, c.k_in) and idx.shape == (c.G, c.B, c.k_in, 2)
    assert d.dtype == np.float32 and idx.dtype == np.int32
    assert not np.isnan(d).any() and (d >= 0).all()
    r, t = idx[..., 0].astype(np.int64), idx[..., 1].astype(np.int64)
    real = r >= 0
    assert np.array_equal(idx[~real], np.full((int((~real).sum()), 2), -1)) and np.isposinf(d[~real]).all()     # padding is (+inf, -1, -1)
    assert (t[real] >= 0).all()
    # real entries first, and every list ascending by (d bits, r, t): strictly, so no (r, t) twice within a list ...
    assert not (real[..., 1:] & ~real[..., :-1]).any()
    db = ml.bits(d).astype(np.int64)
    key_rt = r * (1 << 31) + t
    both = real[..., 1:] & real[..., :-1]
    up = (db[..., 1:] > db[..., :-1]) | ((db[..., 1:] == db[..., :-1]) & (key_rt[..., 1:] > key_rt[..., :-1]))
    assert up[both].all()
    # ... list g holds rows of its own block only, so none twice within a query either
    lo = (np.arange(c.G) * ml.ROWS)[:, None, None]
    assert ((r >= lo) & (r < lo + ml.ROWS))[real].all()
    for b in range(c.B):
        k = key_rt[:, b][real[:, b]]
        assert np.unique(k).size == k.size
    counts = ml.real_counts(c.G, c.k_in, c.padding, dict(c.opts).get("empty"))
    assert all(np.array_equal(real[g].sum(-1), np.full(c.B, counts[g])) for g in range(c.G))
    if c.padding == "tails":
        pads = [c.k_in - n for n in counts]
        assert len(set(pads)) == c.G and pads.count(c.k_in) == 1 and min(pads) >= 1
    if c.padding == "short":
        assert 0 < sum(counts) < c.k
    if dict(c.opts).get("same_sequence"):
        assert all(np.array_equal(ml.bits(d[g]), ml.bits(d[0])) for g in range(c.G))
        assert (np.diff(db, axis=-1) > 0).all()
    n_inf = dict(c.opts).get("inf_real", 0)
    assert np.array_equal((np.isposinf(d) & real).sum(-1), np.array([[n_inf if n >= max(n_inf, 1) else 0] * c.B for n in counts]))


def _kth_value_counts(c):
    """Per query: (candidates at the k-th distance value, how many of them are selected)."""
    d, idx = ml.flat(*ml.case_lists(c))
    out = []
    for b in range(c.B):
        db = np.sort(ml.bits(d[b][idx[b, :, 0] >= 0]))
        at = db == db[c.k - 1]
        out.append((int(at.sum()), int(at[:c.k].sum())))
    return out


FLOODS = [(c, g) for c, g in ALL if c.ties == "flood"]


@pytest.mark.parametrize("c", [c for c, _ in FLOODS], ids=[i for i, (c, _) in zip(IDS, ALL) if c.ties == "flood"])
def test_a_flood_shares_the_kth_value_on_both_sides_of_k(c):
    """At least 2 selected and 2 unselected real candidates carry the k-th distance value: the radix select on the
    distance cannot be exact and tie_select has to happen."""
    for total, taken in _kth_value_counts(c):
        assert taken >= 2 and total - taken >= 2, (total, taken)


def test_the_flood_of_the_largest_merge_is_hundreds_wide():
    c = next(c for c in ml.GENERAL if (c.G, c.k_in, c.k, c.ties) == (64, 1024, 16384, "flood"))
    for total, taken in _kth_value_counts(c):
        assert total >= 1000 and taken >= 2 and total - taken >= 2, (total, taken)      # 65536 / 40 = 1638 expected a value


@pytest.mark.parametrize("c", [c for c, _ in ALL if c.ties == "one_value"], ids=[i for i, (c, _) in zip(IDS, ALL) if c.ties == "one_value"])
def test_one_value_leaves_the_order_to_r_and_t(c):
    d, idx = ml.case_lists(c)
    assert np.unique(ml.bits(d[idx[..., 0] >= 0])).size == 1 and c.k < c.G * c.k_in


DISTINCT = [(i, c) for i, (c, _) in zip(IDS, ALL) if c.ties == "distinct" and not dict(c.opts).get("same_sequence")]


@pytest.mark.parametrize("c", [c for _, c in DISTINCT], ids=[i for i, _ in DISTINCT])
def test_distinct_has_no_equal_distances(c):
    d, idx = ml.flat(*ml.case_lists(c))
    for b in range(c.B):
        db = ml.bits(d[b][idx[b, :, 0] >= 0])
        assert np.unique(db).size == db.size


@pytest.mark.parametrize("c", [c for c, _ in ALL if c.ties == "few" and c.padding == "none"],
                         ids=[i for i, (c, _) in zip(IDS, ALL) if c.ties == "few" and c.padding == "none"])
def test_few_has_equal_distances(c):
    """A few percent of equal pairs among the candidates; from k = 1000 on some of them are among the selected, so the thread
    path's pass 1 and the full comparison of the ranking sort and of the network run (below that the flood cases do it)."""
    d, idx = ml.flat(*ml.case_lists(c))
    rd, _ = ml.reference(d, idx, c.G * c.k_in if c.k < 1000 else min(c.k, c.G * c.k_in))
    for b in range(c.B):
        pairs = int((np.diff(ml.bits(rd[b])) == 0).sum())
        assert 1 <= pairs <= rd.shape[1] // 8, pairs


def test_the_real_inf_entries_follow_the_finite_ones_and_precede_padding():
    for c in ml.INF_REAL:
        d, idx = ml.flat(*ml.case_lists(c))
        rd, ri = ml.reference(d, idx, c.k)
        for b in range(c.B):
            real = idx[b, :, 0] >= 0
            n_fin, n_inf = int((np.isfinite(d[b]) & real).sum()), int((np.isposinf(d[b]) & real).sum())
            assert n_inf == 10 and n_fin < c.k
            assert np.isfinite(rd[b, :n_fin]).all() and np.isposinf(rd[b, n_fin:]).all()
            m = min(c.k, n_fin + n_inf)
            assert (ri[b, :m, 0] >= 0).all() and (ri[b, m:] == -1).all()
    assert [c.k < 96 for c in ml.INF_REAL] == [True, False]          # one k cuts through the real +inf entries, one takes them all


# ---- reference() against the project's oracle: lists cut by oracle.scan_topk from three row shards ----
@pytest.fixture(scope="module")
def shards(oracle_mod):
    rows, T, W, h, k_in, B = 300, 400, 20, 5, 64, 2
    base = syn.dataset(rows, T, 4100)
    ds = np.concatenate([base[:100], base[100:200], base[100:200]], 0)          # the third shard repeats the second: exact ties
    q = syn.gbm_log_returns((B, W), 4101)
    cut = [oracle_mod.scan_topk(ds[100 * g:100 * (g + 1)], q, k_in, h=h, r_offset=100 * g) for g in range(3)]
    d = np.stack([c[0] for c in cut]).astype(np.float32)
    idx = np.stack([c[1] for c in cut]).astype(np.int32)
    return ds, q, h, d, idx


@pytest.mark.parametrize("k", [1, 37, 64])
def test_reference_equals_the_oracle_on_lists_cut_from_scans(oracle_mod, shards, k):
    ds, q, h, d, idx = shards
    od, oidx = oracle_mod.scan_topk(ds, q, k, h=h)
    rd, ri = ml.reference(*ml.flat(d, idx), k)
    ml.assert_same(rd, ri, od, oidx, "reference vs oracle")
    assert (np.diff(ml.bits(od), axis=1) == 0).any() or k == 1                   # the duplicated shard gives ties among the best
    sd, si = ml.flat_shuffled(d, idx, seed=k)
    ml.assert_same(*ml.reference(sd, si, k), od, oidx, "reference of the shuffled lists vs oracle")


def test_the_comparison_has_teeth(shards):
    _, _, _, d, idx = shards
    fd, fi = ml.flat(d, idx)
    k = 64
    rd, ri = ml.reference(fd, fi, k)
    ml.assert_same(rd.copy(), ri.copy(), rd, ri)
    # two tied neighbours swapped: the distances still agree, the indices do not
    b, j = np.argwhere(np.diff(ml.bits(rd), axis=1) == 0)[0]
    wrong = ri.copy()
    wrong[b, [j, j + 1]] = wrong[b, [j + 1, j]]
    with pytest.raises(AssertionError, match=rf"2 indices differ, first at \(b, rank\) = \({b}, {j}\)"):
        ml.assert_same(rd, wrong, rd, ri, "swapped ties")
    # one candidate dropped from the input: everything behind it moves up
    drop = int(np.flatnonzero((fi[0] == ri[0, 10]).all(-1))[0])
    keep = np.arange(fd.shape[1]) != drop
    wd, wi = ml.reference(fd[:, keep], fi[:, keep], k)
    with pytest.raises(AssertionError, match=r"first at \(b, rank\) = \(0, 10\)"):
        ml.assert_same(wd, wi, rd, ri, "dropped candidate")
    # a padding entry reported before a real one
    wd, wi = rd.copy(), ri.copy()
    wd[1, -2], wi[1, -2] = np.inf, -1
    with pytest.raises(AssertionError, match="distances differ"):
        ml.assert_same(wd, wi, rd, ri, "padding before a real entry")


def test_plan_gives_the_literals_of_the_launcher():
    assert ml.plan(1, 30720, 1024) == (1024, 30720, True, "thread")
    assert ml.plan(1, 30721, 1024) == (1024, 30720, False, "thread")
    assert ml.plan(2, 16384, 8192) == (8192, 16384, True, "lds_ranking")
    assert ml.plan(2, 16385, 5000) == (8192, 16384, False, "lds_ranking")
    assert ml.plan(1, 1, 16384) == (16384, 0, False, "network")
    assert ml.plan(1, 1, 8193).ordering == "network" and ml.plan(1, 1, 1025).ordering == "lds_ranking"
    assert ml.plan(257, 8192, 100) == (128, 8192, True, "thread") and not ml.plan(257, 8193, 100).in_lds
    assert ml.plan(256, 8193, 100).in_lds and ml.plan(256, 8193, 100).key_cap == (131072 - 8 * 128) // 4
    assert ml.plan(257, 16384, 1025).key_cap == (131072 - 8 * 2048) // 4           # the clamp is for kpad <= 1024 only


def test_every_branch_has_a_named_case():
    seen = {(ml.plan(c.B, c.G * c.k_in, c.k).ordering, ml.plan(c.B, c.G * c.k_in, c.k).in_lds, c.ties) for c in ml.GENERAL}
    for ordering, in_lds in (("thread", True), ("thread", False), ("lds_ranking", True), ("lds_ranking", False), ("network", False)):
        assert (ordering, in_lds, "distinct") in seen and (ordering, in_lds, "few") in seen, (ordering, in_lds)
    for ordering in ("thread", "lds_ranking", "network"):                        # tie_select in each ordering branch
        assert any(o == ordering and t == "flood" for o, _, t in seen) and any(o == ordering and t == "one_value" for o, _, t in seen)
    assert any(ml.plan(c.B, c.G * c.k_in, c.k).kpad <= 64 for c in ml.GENERAL)
    # the B > 256 clamp decides: the same sizes with 256 queries would stage their keys
    clamp = [c for c in ml.GENERAL if c.B > 256]
    assert sorted(ml.plan(c.B, c.G * c.k_in, c.k).in_lds for c in clamp) == [False, True]
    assert all(ml.plan(256, c.G * c.k_in, c.k).in_lds for c in clamp)
    # sizes at which psh_exchange_merge hands over to the general merge
    assert any(ml.exchange_takes_general_merge(c.G, c.k) and c.G > 64 for c in ml.GENERAL)
    assert any(ml.exchange_takes_general_merge(c.G, c.k) and c.G == 64 and c.k == c.k_in for c in ml.GENERAL)
    # the sorted merge: its three LDS limits exactly, the clipped cut index, k on every side of k_in and G * k_in
    shapes = {(c.G, c.k_in) for c in ml.SORTED}
    assert {(64, 512), (2, 16384), (8, 4096)} <= shapes and {1, 2, 3, 64} <= {c.G for c in ml.SORTED}
    assert all(G <= 64 and G * k_in * 4 <= 128 * 1024 for G, k_in in shapes)
    for G, k_in in ((64, 512), (2, 16384), (8, 4096)):
        assert G == 64 or G * k_in * 4 == 128 * 1024
        assert any(ml.cut_is_clipped(c) and c.k < G * k_in for c in ml.SORTED if (c.G, c.k_in) == (G, k_in)) or G == 64
    assert any(ml.cut_is_clipped(c) and c.k < c.G * c.k_in for c in ml.SORTED)
    for rel in (lambda c: c.k < c.k_in, lambda c: c.k == c.k_in, lambda c: c.k == c.G * c.k_in, lambda c: c.k > c.G * c.k_in):
        assert any(rel(c) for c in ml.SORTED)
    empties = {dict(c.opts).get("empty") for c in ml.SORTED if c.padding == "tails"}
    assert empties == {0, 7}
