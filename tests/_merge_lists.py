"""Per-rank top-k lists for the merges of psh_select.hip (shared by tests/test_merge_lists_cpu.py and
tests/test_gpu_merge_lists.py; numpy only): generators, the reference, and the launcher's plan arithmetic.

A merge is a pure ordering: reference() is a numpy lexsort on (distance bits, r, t) and every comparison is bit for bit over
all k outputs.  lists() builds what G ranks would send: every list ascending by (d, r, t), list g holding rows of its own
row block [g * ROWS, (g + 1) * ROWS) only, distances non-negative (finite or +inf), and no (r, t) pair twice within a query
-- the kernels rank with a strict comparison, two identical entries would claim one slot, and real scans never produce them.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

ROWS, WINDOWS = 37, 1000             # rows a list owns, windows a row: 37 000 (r, t) pairs to draw a list's entries from
TIES = ("distinct", "few", "flood", "one_value")
PADDING = ("none", "tails", "short", "all")
ONE_VALUE = np.float32(0.75)
INF = np.float32(np.inf)


def bits(d: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)


def flood_values(n: int) -> int:
    """How many values j / 64 a flood of n candidates is drawn from: 40, fewer where n is small (48 candidates a value)."""
    return int(min(40, max(2, n // 48)))


def real_counts(G: int, k_in: int, padding: str, empty: int | None = None) -> list:
    """Real entries of each list.  tails: list g ends in 1 + g * step padding entries (all different), list `empty`
    (default: the last) is padding only; short: k_in // (4 G) + (g odd) entries a list; all: none."""
    if padding == "none":
        return [k_in] * G
    if padding == "all":
        return [0] * G
    if padding == "short":
        return [k_in // (4 * G) + (g & 1) for g in range(G)]
    assert padding == "tails" and G >= 2
    step = max(1, (k_in // 2) // G)
    assert 1 + (G - 1) * step < k_in
    n = [k_in - 1 - g * step for g in range(G)]
    n[G - 1 if empty is None else empty] = 0
    return n


def lists(G: int, k_in: int, B: int, ties: str = "distinct", padding: str = "none", seed: int = 0, *, empty: int | None = None,
          same_sequence: bool = False, inf_real: int = 0):
    """(G, B, k_in) float32 distances and (G, B, k_in, 2) int32 (r, t) under the conditions of the module docstring.
    same_sequence: every list of a query carries the same distances (distinct within a list).  inf_real: the last
    `inf_real` REAL entries of every list that has that many get d = +inf (r >= 0: not padding; they sit after the
    list's finite entries and before its padding)."""
    assert ties in TIES and padding in PADDING and k_in <= ROWS * WINDOWS
    rng = np.random.default_rng([seed, G, k_in, B])
    d = np.full((G, B, k_in), INF, np.float32)
    idx = np.full((G, B, k_in, 2), -1, np.int32)
    counts = real_counts(G, k_in, padding, empty)
    N = sum(counts)
    for b in range(B):
        if ties in ("distinct", "few"):
            # distinct multiples of 2^-23 in (0, 1]: exact in float32
            pool = (rng.choice(1 << 23, size=k_in if same_sequence else max(N, 1), replace=False) + 1).astype(np.float32) * np.float32(2.0 ** -23)
            if ties == "few" and N > 1 and not same_sequence:
                dup = rng.choice(N, size=max(1, N // 32), replace=False)         # ~3 %: each takes another entry's value
                pool[dup] = pool[rng.integers(0, N, size=dup.size)]
        elif ties == "flood":
            pool = (rng.integers(0, flood_values(G * k_in), size=max(N, 1)) / 64.0).astype(np.float32)
        else:
            pool = np.full(max(N, 1), ONE_VALUE, np.float32)
        at = 0
        for g in range(G):
            n = counts[g]
            if n == 0:
                continue
            dv = np.sort(pool[:k_in])[:n].copy() if same_sequence else pool[at:at + n].copy()
            at += n
            if inf_real and n >= inf_real:
                dv[np.argsort(dv, kind="stable")[n - inf_real:]] = INF
            code = rng.choice(ROWS * WINDOWS, size=n, replace=False)
            r, t = (g * ROWS + code // WINDOWS).astype(np.int32), (code % WINDOWS).astype(np.int32)
            o = np.lexsort((t, r, bits(dv)))
            d[g, b, :n], idx[g, b, :n, 0], idx[g, b, :n, 1] = dv[o], r[o], t[o]
    return d, idx


def flat(d: np.ndarray, idx: np.ndarray):
    """(B, G * k_in) and (B, G * k_in, 2): the lists of a query one after the other."""
    G, B, k_in = d.shape
    return (np.ascontiguousarray(d.transpose(1, 0, 2)).reshape(B, G * k_in),
            np.ascontiguousarray(idx.transpose(1, 0, 2, 3)).reshape(B, G * k_in, 2))


def flat_shuffled(d: np.ndarray, idx: np.ndarray, seed: int = 0):
    """flat() with the candidates of every query in a random order (psh_merge_topk does not ask for sorted input)."""
    fd, fi = flat(d, idx)
    rng = np.random.default_rng([seed, 77])
    order = [rng.permutation(fd.shape[1]) for _ in range(fd.shape[0])]
    return np.stack([fd[b, o] for b, o in enumerate(order)]), np.stack([fi[b, o] for b, o in enumerate(order)])


def pack(d: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """int32 (G, 3 * B * k_in): per rank the (B, k_in) distance bits, then the (B, k_in, 2) indices -- what one all-gather
    delivers (merge_topk_gathered, merge_sorted_gathered)."""
    G, B, k_in = d.shape
    return np.concatenate([bits(d).view(np.int32).reshape(G, B * k_in), idx.reshape(G, 2 * B * k_in)], axis=1)


def reference(d: np.ndarray, idx: np.ndarray, k: int):
    """d (B, n), idx (B, n, 2) -> the k first of the entries with r >= 0 by (distance bits, r, t), padded with (+inf, -1, -1):
    (B, k) float32 and (B, k, 2) int32."""
    B = d.shape[0]
    out_d = np.full((B, k), INF, np.float32)
    out_idx = np.full((B, k, 2), -1, np.int32)
    for b in range(B):
        real = np.flatnonzero(idx[b, :, 0] >= 0)
        r, t, db = idx[b, real, 0], idx[b, real, 1], bits(d[b, real])
        o = real[np.lexsort((t, r, db))][:k]
        out_d[b, :o.size], out_idx[b, :o.size] = d[b, o], idx[b, o]
    return out_d, out_idx


def assert_same(d, idx, ref_d, ref_idx, what=""):
    """All k entries: identical distance bits and identical (r, t)."""
    d, idx = np.asarray(d), np.asarray(idx)
    assert d.shape == ref_d.shape and idx.shape == ref_idx.shape, f"{what}: shapes {d.shape} {idx.shape}"
    bad_d, bad_i = bits(d) != bits(ref_d), np.any(idx != ref_idx, axis=-1)
    first = lambda bad: tuple(int(v) for v in np.argwhere(bad)[0])                       # noqa: E731
    assert not bad_d.any(), f"{what}: {int(bad_d.sum())} distances differ, first at (b, rank) = {first(bad_d)}"
    assert not bad_i.any(), f"{what}: {int(bad_i.sum())} indices differ, first at (b, rank) = {first(bad_i)}"


# ---- what launch_select (psh_select.hip) decides for a merge: no slices, skip_negative_rows = 1, sort_scratch = nullptr ----
Plan = namedtuple("Plan", "kpad key_cap in_lds ordering")
LDS_BUDGET, SELECT_THREADS = 128 * 1024, 1024


def plan(B: int, n_in: int, k: int) -> Plan:
    """kpad = next_pow2(k); key_cap: the distance keys that fit behind the kpad 8-byte items in the 128 KiB budget, clamped
    to 8192 for B > 256 blocks with kpad <= 1024; keys are staged in LDS when n_in <= key_cap (the launcher also clips
    key_cap to n_in, which does not change that); ordering: one item per thread for kpad <= 1024, the ranking merge sort
    in LDS for 2048 <= kpad <= 8192 (its second buffer fits), the plain bitonic network at kpad = 16384."""
    kpad = 1
    while kpad < k:
        kpad <<= 1
    key_cap = (LDS_BUDGET - 8 * kpad) // 4 if 8 * kpad < LDS_BUDGET else 0
    if B > 256 and kpad <= 1024 and key_cap > 8192:
        key_cap = 8192
    ordering = "thread" if kpad <= SELECT_THREADS else "lds_ranking" if 2 * 8 * kpad <= LDS_BUDGET else "network"
    return Plan(kpad, key_cap, n_in <= key_cap, ordering)


def exchange_takes_general_merge(G: int, k: int) -> bool:
    """psh_exchange_merge (psh_comm.hip) merges with the sorted kernel unless G > 64 or G * k > 32768."""
    return G > 64 or G * k > 32768


# ---- the cases of the GPU module; the CPU module proves that their inputs force the branch they are named for ----
Case = namedtuple("Case", "B G k_in k ties padding opts")


def _case(B, G, k_in, k, ties="distinct", padding="none", **opts):
    return Case(B, G, k_in, k, ties, padding, tuple(sorted(opts.items())))


def case_id(c: Case, general: bool = True) -> str:
    s = f"B{c.B}-{c.G}x{c.k_in}-k{c.k}-{c.ties}-{c.padding}" + "".join(f"-{n}{v}" for n, v in c.opts)
    if general:
        p = plan(c.B, c.G * c.k_in, c.k)
        s = f"{p.ordering}-{'lds' if p.in_lds else 'global'}-" + s
    return s


@functools.lru_cache(maxsize=None)
def case_lists(c: Case):
    d, idx = lists(c.G, c.k_in, c.B, c.ties, c.padding, seed=c.k, **dict(c.opts))
    d.setflags(write=False)
    idx.setflags(write=False)
    return d, idx


GENERAL = (
    # thread path, kpad <= 64
    [_case(2, 3, 64, k, t) for k in (1, 37, 64) for t in ("distinct", "few")]
    # thread path: pass 0 only (distinct) and pass 1 (few)
    + [_case(3, 8, 512, k, t) for k in (65, 1000, 1024) for t in ("distinct", "few")]
    # keys in LDS against keys from global memory at kpad = 1024: n_in = 30720 = key_cap, and 1024 more
    + [_case(1, G, 1024, 1024, t) for G in (30, 31) for t in ("distinct", "few")]
    # the B > 256 clamp: n_in = 8192 = the clamped key_cap, and 1024 more
    + [_case(257, G, 1024, 100) for G in (8, 9)]
    # the ranking merge sort in LDS; n_in = 16384 = key_cap at kpad = 8192, and 4096 more
    + [_case(2, G, 4096, k, "few" if k == 5000 else "distinct") for G in (4, 5) for k in (1025, 5000, 8192)]
    # the bitonic network at kpad = 16384; 65 lists, and 64 lists with 64 * k > 32768: where psh_exchange_merge merges with this kernel
    + [_case(1, 4, 16384, k, "few" if k == 10000 else "distinct") for k in (8193, 10000, 16384)]
    + [_case(2, G, 1024, k, "few" if k == 10000 else "distinct") for G in (65, 64) for k in (8193, 10000, 16384)]
    # ... and its smallest such size, 64 ranks with k = k_in = 1024: one item per thread, 65536 keys read from global memory
    + [_case(2, 64, 1024, 1024, "few")]
    # tie_select in every ordering branch (and with keys in LDS and from global memory)
    + [_case(2, 3, 64, 37, t) for t in ("flood", "one_value")]
    + [_case(2, 8, 512, 1000, t) for t in ("flood", "one_value")]
    + [_case(2, G, 4096, 5000, t) for G in (4, 5) for t in ("flood", "one_value")]
    + [_case(2, 64, 1024, 16384, t) for t in ("flood", "one_value")]
    + [_case(1, 4, 16384, 16384, t) for t in ("flood", "one_value")]
    # padding
    + [_case(2, 8, 512, k, "few", p) for p in ("tails", "short", "all") for k in (300, 5000)]
)

# real entries at +inf (r >= 0): after the finite entries of their list, before its padding.  3 x 64 with the first list
# padding only: 53 and 43 real entries in the other two, 5 of each at +inf -> 86 finite and 10 real +inf entries a query;
# k = 90 cuts through the real +inf entries, k = 150 takes them all and pads
INF_REAL = [_case(2, 3, 64, k, "few", "tails", empty=0, inf_real=5) for k in (90, 150)]

SORTED = (
    [_case(2, 1, 128, k) for k in (100, 128, 200)]
    + [_case(4, 2, 64, k, "few") for k in (50, 64, 128, 200)]
    + [_case(2, 3, 500, k, "few") for k in (37, 700, 1500, 1600)]
    # the three LDS limits: G = 64 and G * k_in * 4 = 128 KiB; k < k_in, = k_in, = G * k_in, beyond; a clipped cut index
    + [_case(2, 64, 512, k, "few") for k in (300, 512, 16384, 32768, 33000)]
    + [_case(1, 2, 16384, k, "few") for k in (16383, 16384, 30000, 32768)]
    + [_case(2, 8, 4096, k, "few") for k in (4096, 30000, 32768)]
    # ties across lists
    + [_case(2, 8, 512, 1000, t) for t in ("flood", "one_value")]
    + [_case(2, 64, 512, 16384, "flood"), _case(2, 3, 64, 100, "one_value")]
    # every list the same distances
    + [_case(2, 5, 100, k, same_sequence=True) for k in (37, 333, 500)]
    + [_case(2, 64, 512, 5000, same_sequence=True)]
    # padding: a list that is padding only placed first and placed last
    + [_case(2, 8, 512, k, "few", "tails", empty=e) for e in (0, 7) for k in (300, 3000, 4096, 5000)]
    + [_case(2, 8, 512, 300, "few", p) for p in ("short", "all")]
)


def cut_is_clipped(c: Case) -> bool:
    """merge_sorted_kernel: the cut index ceil(1.25 k / G) is clipped to k_in - 1."""
    return (5 * c.k + 4 * c.G - 1) // (4 * c.G) > c.k_in - 1
