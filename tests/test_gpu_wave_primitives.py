"""The primitives of psh_wave.h (and fast_div, unit_queue), each called on its own through the probe library
(tests/csrc/psh_probe.hip) and compared BIT FOR BIT with the numpy twin of its stated order (tests/_wave_twin.py), at the
inputs where a wrong lane, row mask, seed, boundary or signedness shows.  Whole waves only: the header assumes 64 active
lanes.  NaN results are compared as "a NaN here" (tw.bits: IEEE leaves a NaN's sign and payload open), everything else
by its raw words; where a result is documented as uniform, all 64 lanes must hold the same bits."""
import numpy as np
import pytest

import _probe as P
import _probe_cases as cases
import _wave_twin as tw

pytestmark = pytest.mark.gpu

NW = 256                                 # waves per launch of the reductions and scans: 64 blocks of 256 threads
INF, NAN = np.inf, np.nan


@pytest.fixture(scope="module")
def probe(hip_device):
    return P.load()


def same(got, want):
    return np.array_equal(tw.bits(got), tw.bits(want))


def uniform(a):
    """[waves, 64]: every lane of a wave holds lane 0's bits."""
    b = tw.bits(a)
    return np.array_equal(b, np.broadcast_to(b[..., :1], b.shape))


def run_wave(probe, typ, op, a, b=None):
    a = np.ascontiguousarray(a)
    da, db = P.dev(a), P.dev(a if b is None else b)
    o1, o2 = P.words(a.size, a.dtype.itemsize, -1), P.words(a.size, a.dtype.itemsize, -1)
    P.check(probe.psh_probe_wave(typ, op, da.data_ptr(), db.data_ptr(), o1.data_ptr(), o2.data_ptr(), a.size, P.stream()), "psh_probe_wave")
    return P.host(o1, a.dtype).reshape(a.shape), P.host(o2, a.dtype).reshape(a.shape)


def run_dpp(probe, op, a):
    a = np.ascontiguousarray(a)
    da, o = P.dev(a), P.words(a.size, 4, -1)
    P.check(probe.psh_probe_dpp(op, da.data_ptr(), o.data_ptr(), a.size, P.stream()), "psh_probe_dpp")
    return P.host(o, a.dtype).reshape(a.shape)


# ------------------------------------------------------------------------------------------ inputs
def mixed(g, shape, dtype):
    """Mixed magnitude and sign, so that another order of the additions gives other bits: terms at the scale of 1 beside
    terms at the scale where a unit is a few ulps (1e8 in float32, 1e16 in float64), and a cancelling pair per wave."""
    big = 1e8 if dtype == np.float32 else 1e16
    v = g.standard_normal(shape) * np.where(g.random(shape) < 0.25, big, 1.0)
    v = v.astype(dtype).reshape(-1, 64)
    rows, first = np.arange(v.shape[0]), g.integers(0, 64, v.shape[0])
    v[rows, first] = dtype(big * 3)
    v[rows, (first + g.integers(1, 64, v.shape[0])) % 64] = dtype(-big * 3)
    return v.reshape(shape)


def sum_waves(dtype, seed=0):
    g = np.random.default_rng(seed)
    v = mixed(g, (NW, 64), dtype)
    v[:64] = 0
    v[np.arange(64), np.arange(64)] = dtype(3.0) * mixed(g, (64,), dtype)        # one-hot at each lane
    v[64] = dtype(-0.0)                                                           # all -0.0: the sum is -0.0
    v[65, 17] = INF                                                               # one lane +inf
    v[66, 5], v[66, 40] = INF, -INF                                               # NaN
    v[67] = dtype(-0.0)
    v[67, 63] = dtype(0.0)                                                        # one +0 among -0: +0
    return v


def minmax_waves(dtype, seed=1):
    g = np.random.default_rng(seed)
    v = (g.standard_normal((NW, 64)) * 10.0 ** g.integers(-3, 4, (NW, 64))).astype(dtype)
    v[:64][g.random((64, 64)) < 0.5] = NAN                                        # NaN in some lanes: dropped
    v[np.arange(64), np.arange(64)] = g.standard_normal(64).astype(dtype)         # (never a whole wave of them here)
    v[64] = NAN                                                                   # NaN in all lanes: NaN out
    v[65] = dtype(0.0)
    v[65, ::3] = dtype(-0.0)                                                      # +-0 mixed
    v[66] = dtype(-0.0)
    v[66, 31] = dtype(0.0)
    v[67, 3], v[67, 60] = INF, -INF
    v[68] = INF
    v[69] = -INF
    v[70] = NAN
    v[70, 33] = dtype(-0.0)                                                       # the one number among NaNs
    return v


def int_waves(dtype, seed=2):
    """Words on both sides of 2^31 (a signed / unsigned mix-up orders them the other way round), sums that wrap."""
    g = np.random.default_rng(seed)
    v = g.integers(0, 1 << 32, size=(NW, 64), dtype=np.uint64).astype(np.uint32)
    v[:64] = 0
    v[np.arange(64), np.arange(64)] = g.integers(1, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)      # one-hot
    v[64] = 0x7fffffff
    v[64, 9] = 0x80000000
    v[65] = 0x80000000
    v[65, 50] = 0x7fffffff
    v[66] = 0xffffffff
    v[67] = g.integers(0, 1 << 31, 64)                                             # one side only
    v[68] = g.integers(1 << 31, 1 << 32, 64, dtype=np.uint64)
    v[69] = 1 << np.arange(64, dtype=np.uint64) % 32                               # (or: one bit per lane)
    return v.view(dtype)


# ------------------------------------------------------------------------------------------ wave_reduce
@pytest.mark.parametrize("dtype,typ", [(np.float32, P.F32), (np.float64, P.F64)])
def test_wave_sum(probe, dtype, typ):
    v = sum_waves(dtype)
    got, _ = run_wave(probe, typ, P.SUM, v)
    assert same(got, tw.wave_reduce(v, tw.op_sum))
    assert uniform(got)
    assert np.array_equal(tw.bits(got[64]), tw.bits(np.full(64, -0.0, dtype)))     # the -0.0 survives
    assert np.isnan(got[66]).all() and np.isposinf(got[65]).all() and not np.signbit(got[67]).any()


@pytest.mark.parametrize("dtype,typ", [(np.float32, P.F32), (np.float64, P.F64)])
def test_wave_min_max_float(probe, dtype, typ):
    v = minmax_waves(dtype)
    lo, _ = run_wave(probe, typ, P.MIN, v)
    hi, _ = run_wave(probe, typ, P.MAX, v)
    assert same(lo, tw.wave_reduce(v, tw.fmin_)) and same(hi, tw.wave_reduce(v, tw.fmax_))
    assert uniform(lo) and uniform(hi)
    assert not np.isnan(lo[:64]).any() and not np.isnan(hi[:64]).any()             # NaN operands are dropped
    assert np.array_equal(lo[:64, 0], np.nanmin(v[:64], axis=1)) and np.array_equal(hi[:64, 0], np.nanmax(v[:64], axis=1))
    assert np.isnan(lo[64]).all() and np.isnan(hi[64]).all()                       # nothing but NaN: NaN
    assert np.signbit(lo[70]).all() and (lo[70] == 0).all() and (hi[70] == 0).all()
    # both in one butterfly, lo and hi from different data
    w = minmax_waves(dtype, seed=11)
    lo2, hi2 = run_wave(probe, typ, P.MINMAX, v, w)
    tlo, thi = tw.wave_minmax(v, w)
    assert same(lo2, tlo) and same(hi2, thi) and same(lo2, lo) and uniform(lo2) and uniform(hi2)


@pytest.mark.parametrize("dtype,typ", [(np.int32, P.I32), (np.uint32, P.U32)])
def test_wave_reduce_integers(probe, dtype, typ):
    v = int_waves(dtype)
    w = int_waves(dtype, seed=12)
    for op, twin in ((P.SUM, tw.op_sum), (P.MIN, tw.fmin_), (P.MAX, tw.fmax_), (P.OR, tw.op_or)):
        got, _ = run_wave(probe, typ, op, v)
        assert same(got, tw.wave_reduce(v, twin)) and uniform(got), op
    lo, _ = run_wave(probe, typ, P.MIN, v)
    hi, _ = run_wave(probe, typ, P.MAX, v)
    assert np.array_equal(lo[:, 0], v.min(axis=1)) and np.array_equal(hi[:, 0], v.max(axis=1))      # in the operand's OWN order
    lo2, hi2 = run_wave(probe, typ, P.MINMAX, v, w)
    assert np.array_equal(lo2, lo) and np.array_equal(hi2[:, 0], w.max(axis=1)) and uniform(hi2)


# ------------------------------------------------------------------------------------------ the DPP forms
LEVELS = np.array([0x00000000, 0x00000001, 0x3f800000, 0x7f7fffff, 0x7f800000], dtype=np.uint32)   # +0, smallest denormal, 1.0, FLT_MAX, +inf


def test_wave_max_nonneg(probe):
    # the maximum at each lane, over each neighbouring pair of levels: wave 4 l + j holds LEVELS[j + 1] at lane l, LEVELS[j] elsewhere
    v = np.repeat(np.tile(LEVELS[:4], 64)[:, None], 64, axis=1)
    l, j = np.divmod(np.arange(NW), 4)
    v[np.arange(NW), l] = LEVELS[j + 1]
    got = run_dpp(probe, P.DPP_MAX_NONNEG, v.view(np.float32))
    assert same(got, np.broadcast_to(tw.wave_max_nonneg(v.view(np.float32))[:, None], got.shape))
    assert np.array_equal(got.view(np.uint32)[:, 0], LEVELS[j + 1]) and uniform(got)
    # all lanes +0; the maximum over a +0 background; random non-negative values with denormals among them
    g = np.random.default_rng(4)
    w = np.zeros((NW, 64), dtype=np.uint32)
    w[1:65, :][np.arange(64), np.arange(64)] = LEVELS[1 + np.arange(64) % 4]
    w[65:] = g.integers(0, 0x7f800001, (NW - 65, 64))
    w[65:][g.random((NW - 65, 64)) < 0.2] >>= 9                                    # denormals
    got = run_dpp(probe, P.DPP_MAX_NONNEG, w.view(np.float32))
    assert same(got, np.broadcast_to(tw.wave_max_nonneg(w.view(np.float32))[:, None], got.shape)) and uniform(got)
    assert not got[0].view(np.uint32).any()


def test_wave_sum_dpp(probe):
    v = sum_waves(np.float32, seed=5)
    got = run_dpp(probe, P.DPP_SUM, v)
    want = tw.wave_sum_dpp(v)
    assert same(got, np.broadcast_to(want[:, None], got.shape)) and uniform(got)
    assert np.array_equal(tw.bits(got[64]), tw.bits(np.full(64, -0.0, np.float32)))
    # the order is the stated tree and no other: on this data the butterfly's and the left-to-right sums differ from it
    seq = np.zeros(NW, np.float32)
    with np.errstate(invalid="ignore"):
        for lane in range(64):
            seq = seq + v[:, lane]
    finite = np.isfinite(want)
    assert (tw.bits(want) != tw.bits(seq))[finite].any() and (tw.bits(want) != tw.bits(tw.wave_reduce(v, tw.op_sum)[:, 0]))[finite].any()


def scan_int_waves(seed=6):
    g = np.random.default_rng(seed)
    v = g.integers(-(1 << 31), 1 << 31, (NW, 64)).astype(np.int32)                # sums that wrap int32
    v[:64] = 0
    v[np.arange(64), np.arange(64)] = g.integers(1, 1 << 31, 64)                  # one-hot at each lane
    v[64] = 1                                                                     # all ones: lane l gives l + 1
    v[65:97] = tw.pack16(g.integers(0, 9, (32, 64)))                              # the callers' packed counters, c <= 8
    v[97] = tw.pack16(np.full(64, 8))
    v[98] = 0x7fffffff
    v[99] = -1
    return v


def test_wave_scan_inclusive_dpp(probe):
    v = scan_int_waves()
    got = run_dpp(probe, P.DPP_SCAN, v)
    assert np.array_equal(got, tw.wave_scan_inclusive_dpp(v))
    assert np.array_equal(got[64], np.arange(1, 65))                               # (lanes 15/16, 31/32, 47/48, 63: the row broadcasts)
    assert np.array_equal(got[97].view(np.uint32), np.arange(1, 65, dtype=np.uint32) * np.uint32(8 * 0x10001))
    tot = run_dpp(probe, P.DPP_TOTAL, v)
    assert np.array_equal(tot, np.broadcast_to(tw.wave_total_dpp(v)[:, None], tot.shape)) and uniform(tot)


@pytest.mark.parametrize("dtype,typ", [(np.float32, P.F32), (np.float64, P.F64), (np.int32, P.I32), (np.uint32, P.U32)])
def test_wave_scan_inclusive(probe, dtype, typ):
    v = sum_waves(dtype, seed=7) if np.dtype(dtype).kind == "f" else scan_int_waves(seed=8).view(dtype)
    got, _ = run_wave(probe, typ, P.SCAN, v)
    assert same(got, tw.wave_scan_inclusive(v))
    if np.dtype(dtype).kind != "f":
        assert np.array_equal(got.view(np.int32), tw.wave_scan_inclusive_dpp(v.view(np.int32)))     # the two scans agree on integers


# ------------------------------------------------------------------------------------------ block_reduce
def block_data(dtype, nblocks, waves, seed):
    g = np.random.default_rng(seed)
    v = mixed(g, (nblocks, waves, 64), dtype)
    s = seed % 4                                         # (the second reduction's special blocks lie elsewhere)
    v[s] = dtype(-0.0)                                   # a total of -0.0: the fold starts at red[0], not at a zero
    v[s + 4, min(1, waves - 1)] = NAN                    # a NaN confined to one wave: the maximum drops it
    v[s + 8, 0] = NAN                                    # ... to the wave the fold starts with
    v[s + 12][g.random((waves, 64)) < 0.3] = NAN         # scattered
    v[s + 16] = NAN
    v[s + 20] = dtype(-0.0)
    v[s + 20, waves - 1, 63] = dtype(0.0)
    return v


@pytest.mark.parametrize("waves", [1, 2, 4, 8, 16])
def test_block_reduce(probe, waves):
    """WAVES = 1 .. 16 (CAL_WAVES = 4 and the weights kernels' values among them), both TAIL_BARRIER settings; with the
    tail barrier two reductions back to back through the same red[], on 1024 blocks, both results in every thread."""
    for dtype, typ in ((np.float32, P.F32), (np.float64, P.F64)):
        for tail, nblocks in ((0, 64), (1, 1024)):
            a, b = block_data(dtype, nblocks, waves, 20 + waves), block_data(dtype, nblocks, waves, 41 + waves)
            da, db = P.dev(a), P.dev(b)
            for op, twin in ((P.SUM, tw.op_sum), (P.MAX, tw.fmax_), (P.MIN, tw.fmin_)):
                o1, o2 = P.words(a.size, a.dtype.itemsize, -1), P.words(a.size, a.dtype.itemsize, -1)
                P.check(probe.psh_probe_block_reduce(typ, op, waves, tail, da.data_ptr(), db.data_ptr(), o1.data_ptr(), o2.data_ptr(),
                                                     nblocks, P.stream()), "psh_probe_block_reduce")
                r1 = P.host(o1, dtype).reshape(nblocks, waves * 64)
                want = tw.block_reduce(a, twin)
                assert same(r1, np.broadcast_to(want[:, None], r1.shape)), (dtype, tail, op)      # every thread of every block
                if tail:
                    r2 = P.host(o2, dtype).reshape(nblocks, waves * 64)
                    want2 = tw.block_reduce(b, twin)
                    assert same(r2, np.broadcast_to(want2[:, None], r2.shape)), (dtype, op)
                s = (20 + waves) % 4
                if op == P.SUM:
                    assert np.signbit(r1[s]).all() and (r1[s] == 0).all() and not np.signbit(r1[s + 20]).any()
                if op == P.MAX and waves > 1:
                    assert not np.isnan(r1[s + 4]).any() and not np.isnan(r1[s + 8]).any()
                if op != P.SUM:
                    assert np.isnan(r1[s + 16]).all()


# ------------------------------------------------------------------------------------------ rank_bucket / RankHist
FILL = 0xffffffff


@pytest.mark.parametrize("per", [1, 16, 32])          # 1, and what the kernels instantiate: 1024 / 64, 2048 / 64 (fused and select)
def test_rank_bucket(probe, per):
    hists = cases.rank_histograms(per)
    ranks = [cases.rank_list(h) for h in hists]
    nr = max(r.size for r in ranks)
    ranks = np.stack([np.concatenate([r, np.full(nr - r.size, FILL, np.uint32)]) for r in ranks])
    H = np.stack(hists)
    assert int(H[-1].astype(np.uint64).sum()) > 1 << 31
    want = np.empty((len(hists), nr, 5), dtype=np.uint32)
    for i, h in enumerate(hists):
        for j, r in enumerate(ranks[i]):
            f = tw.rank_find(h, int(r))
            want[i, j] = (FILL, FILL, FILL, 0, FILL) if f is None else (f[0], f[1], f[2], 1, f[0] // per)
    assert (want[:, :, 3] == 1).any() and (want[-1][:, 3] == 0).any() and not want[5][:, 3].any()       # (the all-zero histogram owns nothing)
    dh, dr = P.dev(H), P.dev(ranks)
    for one_hist in (0, 1):                           # a fresh rank_bucket per rank; every rank from ONE RankHist
        out = P.words(len(hists) * 4 * nr * 5, 4, -1)
        P.check(probe.psh_probe_rank(per, dh.data_ptr(), len(hists), dr.data_ptr(), nr, one_hist, out.data_ptr(), P.stream()), "psh_probe_rank")
        got = P.host(out, np.uint32).reshape(len(hists), 4, nr, 5)
        for wave in range(4):                         # called by each wave of the block in turn
            assert np.array_equal(got[:, wave], want), (one_hist, wave)
        owned = got[..., 3] == 1
        assert set(np.unique(got[..., 3])) <= {0, 1}                                # exactly one lane, or none
        assert (got[..., 2][owned] > 0).all()                                       # an empty counter is never the answer
        assert np.array_equal(H[np.nonzero(owned)[0], got[..., 0][owned]], got[..., 2][owned])


def test_bucket_upper_edge(probe):
    rows = []
    for kmin, kmax in ((0, 0xffffffff), (0xfffffc00, 0xffffffff), (0xffffffff, 0xffffffff), (0x80000000, 0xc0000000), (7, 7), (0, 0),
                       (0x3f800000, 0x7f800000), (0xfff00000, 0xfffffffe)):
        for shift in (0, 1, 10, 21, 22):              # 22: the largest the callers use (a 32-bit range over 1024 buckets)
            for bucket in (0, 1, 2, 511, 1022, 1023, 2047):
                rows.append((kmin, kmax, bucket, shift))
    while len(rows) % 64:
        rows.append(rows[-1])
    r = np.array(rows, dtype=np.uint64)
    want = np.array([tw.bucket_upper_edge(*row) for row in rows], dtype=np.uint64)
    unclamped = r[:, 0] + ((r[:, 2] + 1) << r[:, 3]) - 1
    assert (unclamped > 0xffffffff).any() and ((unclamped > r[:, 1]) & (unclamped <= 0xffffffff)).any() and (unclamped <= r[:, 1]).any()
    out = P.words(len(rows), 4, -1)
    cols = [P.dev(r[:, c].astype(np.uint32)) for c in range(4)]
    P.check(probe.psh_probe_bucket_edge(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), out.data_ptr(),
                                        len(rows), P.stream()), "psh_probe_bucket_edge")
    got = P.host(out, np.uint32)
    assert np.array_equal(got, want.astype(np.uint32))
    assert (got.astype(np.uint64) <= r[:, 1]).all()                                 # clamped to kmax, never wrapped


# ------------------------------------------------------------------------------------------ fast_div, unit_queue
def test_fast_div(probe):
    ds = {1, 2, 3, 7}
    for k in range(2, 32):
        ds |= {d for d in ((1 << k) - 1, 1 << k, (1 << k) + 1) if d <= (1 << 31) - 1}
    us, dd = [], []
    for d in sorted(ds):
        top = (1 << 32) - 1
        cand = {0, d - 1, d, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, top}
        for m in (2, 3, 1000, 65537, top // d):
            cand |= {m * d - 1, m * d, m * d + 1}
        for u in sorted(c for c in cand if 0 <= c <= top):
            us.append(u)
            dd.append(d)
    while len(us) % 64:
        us.append(us[-1])
        dd.append(dd[-1])
    u, d = np.array(us, dtype=np.uint32), np.array(dd, dtype=np.uint32)
    magic = np.array([tw.fast_div_magic(x) for x in dd], dtype=np.uint32)
    out, du, dm, dd_ = P.words(u.size, 4, -1), P.dev(u), P.dev(magic), P.dev(d)
    P.check(probe.psh_probe_fast_div(du.data_ptr(), dm.data_ptr(), dd_.data_ptr(), out.data_ptr(), u.size, P.stream()), "psh_probe_fast_div")
    assert np.array_equal(P.host(out, np.uint32), np.array([tw.fast_div(a, b) for a, b in zip(us, dd)], dtype=np.uint32))


@pytest.mark.parametrize("grid", [1, 255, 256, 1024])
def test_unit_queue(probe, grid):
    ns = np.array(sorted({0, 1, max(grid - 1, 0), grid, grid + 1, (1 << 31) - 1}), dtype=np.uint32)
    lo, hi, dn = P.words(ns.size * grid, 4, -1), P.words(ns.size * grid, 4, -1), P.dev(ns)
    P.check(probe.psh_probe_unit_queue(dn.data_ptr(), ns.size, lo.data_ptr(), hi.data_ptr(), grid, P.stream()), "psh_probe_unit_queue")
    lo, hi = P.host(lo, np.uint32).reshape(ns.size, grid), P.host(hi, np.uint32).reshape(ns.size, grid)
    for k, n in enumerate(ns):
        tlo, thi = tw.unit_queue(int(n), grid)
        assert np.array_equal(lo[k], tlo.astype(np.uint32)) and np.array_equal(hi[k], thi.astype(np.uint32))
        assert lo[k, 0] == 0 and hi[k, -1] == n and np.array_equal(lo[k, 1:], hi[k, :-1]) and (lo[k] <= hi[k]).all()    # contiguous, ordered, covering
