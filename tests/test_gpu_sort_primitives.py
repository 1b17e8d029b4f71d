"""The primitives of psh_sort_lds.h, each on its own through the probe library (tests/csrc/psh_probe.hip), BIT FOR BIT:
the key map against its bit formulas, qnt_sort's three instantiations against np.sort at every power-of-two size, and
qnt_scan against the twin of its stated order (tests/_wave_twin.py)."""
import numpy as np
import pytest

import _probe as P
import _probe_cases as cases
import _wave_twin as tw

pytestmark = pytest.mark.gpu

NIN = 256                                # inputs per launch of the sort, one block each
SENTINEL = np.uint64(0xffffffff) << np.uint64(32)


@pytest.fixture(scope="module")
def probe(hip_device):
    return P.load()


def test_qnt_key_and_value(probe):
    x = cases.key_floats()
    xs = np.concatenate([x, np.float32([-0.0]), np.array([0x7fc00000], dtype=np.uint32).view(np.float32)])
    n = xs.size
    xs = np.concatenate([xs, np.zeros(-n % 64, dtype=np.float32)])
    dx, key, back = P.dev(xs), P.words(xs.size, 4, -1), P.words(xs.size, 4, -1)
    P.check(probe.psh_probe_key(dx.data_ptr(), key.data_ptr(), back.data_ptr(), xs.size, P.stream()), "psh_probe_key")
    key, back = P.host(key, np.uint32)[:n], P.host(back, np.uint32)[:n]
    assert np.array_equal(key, tw.qnt_key(xs[:n])) and np.array_equal(back, tw.qnt_value(tw.qnt_key(xs[:n])).view(np.uint32))
    assert np.all(np.diff(key[:x.size].astype(np.int64)) > 0)                       # strictly increasing over -inf .. +inf
    assert np.array_equal(back[:x.size], x.view(np.uint32))                         # and back to the same bits
    assert key[x.size] == key[x.size // 2] == 0x80000000 and back[x.size] == 0      # -0 takes +0's key and comes back as +0
    assert key[x.size + 1] > key[x.size - 1]                                        # a (positive quiet) NaN lies above +inf


def sort_inputs(n2: int, NB: int, seed: int) -> np.ndarray:
    """NIN inputs of n2 entries key << 32 | j, as the callers build them on the device."""
    g = np.random.default_rng(seed)
    vals = (g.standard_normal((NIN, n2)) * 10.0 ** g.integers(-2, 3, (NIN, 1))).astype(np.float32)
    vals[NIN // 2:] = np.round(vals[NIN // 2:])                                      # many equal values (and +-0)
    vals[0] = np.sort(vals[0])                                                       # already sorted
    vals[1] = np.sort(vals[1])[::-1]                                                 # reversed
    up = np.sort(vals[2])
    vals[2] = np.concatenate([up[0::2], up[1::2][::-1]])                             # organ pipe
    vals[3] = np.float32(1.25)                                                       # all equal: ties by index only
    vals[4, : n2 // 2], vals[4, n2 // 2:] = np.float32(-0.0), np.float32(0.0)        # one key, both zeros
    vals[5, 0::2], vals[5, 1::2] = np.float32(0.0), np.float32(-0.0)
    key = tw.qnt_key(vals).astype(np.uint64)
    # random 0-1 inputs, the density of ones running from 0 to 1
    zo = slice(8, 8 + 64)
    key[zo] = g.random((64, n2)) < np.linspace(0.0, 1.0, 64)[:, None]
    ent = (key << np.uint64(32)) | np.arange(n2, dtype=np.uint64)[None, :]
    # sentinel-padded tails as the callers pad: k live entries, then ~0 keys, for every class of k
    ks = sorted({1, 2, (1 << NB) - 1, 1 << NB, (1 << NB) + 1, n2 // 2 - 1, n2 // 2, n2 // 2 + 1, n2 - (1 << NB), n2 - 2, n2 - 1} & set(range(1, n2)))
    for row, k in zip(range(80, 80 + len(ks)), ks):
        ent[row, k:] = SENTINEL | np.arange(k, n2, dtype=np.uint64)
    return ent


@pytest.mark.parametrize("NB,cap", [(2, 1024), (3, 4096), (4, 16384)])       # qnt_sort<2, 256>, <3, 512>, <4, 1024>
def test_qnt_sort(probe, NB, cap):
    n2 = 1 << NB
    while n2 <= cap:
        ent = sort_inputs(n2, NB, 100 * NB + n2.bit_length())
        din, out = P.dev(ent), P.words(ent.size, 8, 0)
        P.check(probe.psh_probe_sort(NB, din.data_ptr(), out.data_ptr(), n2, NIN, P.stream()), "psh_probe_sort")
        got = P.host(out, np.uint64).reshape(NIN, n2)
        assert np.array_equal(got, np.sort(ent, axis=1)), n2
        n2 <<= 1


def scan_inputs(threads: int, is_max: bool, seed: int) -> np.ndarray:
    """Mixed magnitudes, so that another order of the additions gives other bits (the maximum takes values >= 0)."""
    g = np.random.default_rng(seed)
    v = g.standard_normal((64, threads)) * 10.0 ** g.integers(-8, 9, (64, threads))
    v[0] = g.integers(0, 1000, threads)                                              # exact in any order
    v[1] = 0.0
    v[2] = 0.1                                                                       # every partial sum rounds
    return np.abs(v) if is_max else v


@pytest.mark.parametrize("threads", [256, 512, 1024])
@pytest.mark.parametrize("is_max", [False, True])
def test_qnt_scan(probe, threads, is_max):
    """Each thread's exclusive prefix and the total in g[GROUPS]; two scans back to back on the same arrays, the second of
    other data (the leading barrier)."""
    a, b = scan_inputs(threads, is_max, threads), scan_inputs(threads, is_max, threads + 1)[::-1].copy()
    da, db = P.dev(a), P.dev(b)
    outs = [P.words(a.size, 8, -1) for _ in range(4)]
    P.check(probe.psh_probe_scan(threads, int(is_max), da.data_ptr(), db.data_ptr(), *(o.data_ptr() for o in outs), a.shape[0], P.stream()),
            "psh_probe_scan")
    pre1, tot1, pre2, tot2 = (P.host(o, np.float64).reshape(a.shape) for o in outs)
    for blk in range(a.shape[0]):
        for data, pre, tot in ((a, pre1, tot1), (b, pre2, tot2)):
            wpre, wtot = tw.qnt_scan(data[blk], is_max)
            assert np.array_equal(tw.bits(pre[blk]), tw.bits(wpre)), (blk, "prefix")
            assert np.array_equal(tw.bits(tot[blk]), tw.bits(np.full(threads, wtot))), (blk, "total")      # the same word in every thread
    if not is_max:      # the order shows on this data: the plain cumulative sum gives other bits somewhere
        assert any(not np.array_equal(pre1[blk], np.cumsum(a[blk]) - a[blk]) for blk in range(3, a.shape[0]))
