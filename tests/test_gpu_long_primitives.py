"""The pieces of the long-window front end (psh_long.h), each called on its own through the probe library
(tests/csrc/psh_probe.hip) and compared BIT FOR BIT with its numpy twin (tests/_long_twin.py): one wave per case, all cases
of a test in one launch.  Where the twin holds a NaN the device must hold a NaN (tw.bits); everywhere else the words are
equal.  The segment's conversion and the C operand's mask have no function of their own (psh_long.h says why) and no
test here."""
import numpy as np
import pytest

import _long_twin as lt
import _probe as P
import _probe_cases as cases
import _wave_twin as tw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(hip_device):
    return P.load()


def params(rows):
    """[ncases, LONG_PARAMS] int32 from the cases' leading ints"""
    par = np.zeros((len(rows), P.LONG_PARAMS), dtype=np.int32)
    for c, row in enumerate(rows):
        par[c, :len(row)] = row
    return par


def run(probe, what, a, b, par, nout, itemsize=4, fill=-1):
    """`nout` words per case back from one launch; a, b: float32 arrays (or None)"""
    da = P.dev(np.zeros(1, np.float32) if a is None else np.ascontiguousarray(a, dtype=np.float32))
    db = P.dev(np.zeros(1, np.float32) if b is None else np.ascontiguousarray(b, dtype=np.float32))
    dp = P.dev(par)
    n = par.shape[0] * nout
    out = P.words(n if itemsize == 4 else (n + 1) // 2, 4, fill)
    P.check(probe.psh_probe_long(what, da.data_ptr(), db.data_ptr(), dp.data_ptr(), out.data_ptr(), par.shape[0], P.stream()), "psh_probe_long")
    return P.host(out, np.uint32 if itemsize == 4 else np.uint16)[:n].reshape(par.shape[0], nout)


def same(got, want):
    return np.array_equal(tw.bits(np.ascontiguousarray(got)), tw.bits(np.ascontiguousarray(want)))


def test_stage_row_both_cache_policies(probe):
    for ds, T, cs in cases.long_stage_cases():
        buf = np.concatenate([ds.ravel(), np.full(1024 + 1280, 7.0, dtype=np.float32)])      # a margin behind the last row
        par = params([(row, T, seg, nfloat) for row, seg, nfloat in cs])
        want = np.stack([lt.stage_row(ds, T, row, seg, nfloat) for row, seg, nfloat in cs])
        for what in (P.L_STAGE0, P.L_STAGE2):
            got = run(probe, what, buf, None, par, 1280)
            assert np.array_equal(got, want), (T, what)


def test_energy_operand_both_signs(probe):
    sps = [cases.long_prefix_sums(20 + i) for i in range(len(cases.LONG_OPERAND_W))]
    sps[1][700:] = np.inf                                                     # an inf sample: every later prefix
    sps[2][900:] = np.nan
    par = params([(W,) for W in cases.LONG_OPERAND_W])
    for upper in (False, True):
        got = run(probe, P.L_OPERAND_HI if upper else P.L_OPERAND_LO, np.stack(sps), None, par, 1024).view(np.float32)
        for c, W in enumerate(cases.LONG_OPERAND_W):
            assert same(got[c].reshape(64, 16), lt.energy_operand(sps[c], W, upper)), (W, upper)


def test_tile_min(probe):
    tiles = cases.long_tiles()
    got = run(probe, P.L_TILE_MIN, np.stack([t for t, _ in tiles]), None, params([(nv,) for _, nv in tiles]), 64).view(np.float32)
    for c, (t, nv) in enumerate(tiles):
        assert same(got[c], lt.tile_min(t, nv)), nv
        assert not np.isnan(got[c]).any()                                     # the NaN slots are dropped, never returned


def test_query_tables(probe):
    g = np.random.default_rng(31)
    cs = list(cases.LONG_TABLE_CASES) + [(3, cases.LONG_TABLE_W14)]
    xs = np.zeros((len(cs), 3, 256), dtype=np.float32)
    rows, scales = [], []
    for c, (nq, W) in enumerate(cs):
        x = g.standard_normal((nq, W)).astype(np.float32)
        x[0, W // 2] = 40000.0 if c == 2 else x[0, W // 2]                   # beyond the f16 range after -2 x: inf in the table
        xs[c].reshape(-1)[:nq * W] = x.ravel()                               # [query][W], packed as the kernels stage them
        scale = np.float32(2.0 ** (c % 3 - 1))
        scales.append(scale)
        rows.append((lt.bucket(W), nq, W, int(scale.view(np.int32))))
    got = run(probe, P.L_TABLES, xs, None, params(rows), 3 * lt.query_halves(18), itemsize=2)
    for c, (nq, W) in enumerate(cs):
        nks = lt.bucket(W)
        x = xs[c].reshape(-1)[:nq * W].reshape(nq, W)
        want = lt.query_tables(x, W, scales[c], nks).view(np.uint16).ravel()
        assert np.array_equal(got[c, :want.size], want), (nq, W)
        assert np.all(got[c, want.size:] == np.float16(1.0).view(np.uint16))  # nothing written behind the last query's table


def test_exact_window_both_pointer_kinds(probe):
    g = np.random.default_rng(32)
    y = (g.standard_normal(4096) * 0.01).astype(np.float32)
    x = (g.standard_normal(1024) * 0.01).astype(np.float32)
    y[100], y[2000] = np.nan, np.inf
    rows = []
    for c, W in enumerate(cases.LONG_EXACT_W):
        qn = (64, 37, 1, 64, 5)[c]
        t = (np.arange(64) * 53 + c) % (4096 - 256)                          # window starts of every residue mod 4
        xo = (np.arange(64) * 11 + c) % (1024 - 256)
        rows.append([W, qn, (3 * c + 1) % 4, 0, 0, 0, 0, 0] + list(t) + list(xo))
    par = params(rows)
    for vector in (False, True):
        got = run(probe, P.L_EXACT_VECTOR if vector else P.L_EXACT_SCALAR, y, x, par, 64).view(np.float32)
        for c, row in enumerate(rows):
            W, qn, xoff = row[0], row[1], row[2]
            want = np.zeros(64, dtype=np.float32)                            # lanes at and past qn run no chain
            for lane in range(qn):
                xs = x[row[72 + lane]:] if vector else x[xoff:]
                want[lane] = lt.exact_window(y[row[8 + lane]:], xs, W)
            assert same(got[c], want), (W, vector)


def test_upper_bound(probe):
    est, nx = cases.long_bound_inputs()
    cs = [(W, sexp) for W in (34, 256) for sexp in cases.LONG_BOUND_SEXP]
    got = run(probe, P.L_BOUND, np.tile(est, (len(cs), 1)), np.tile(nx, (len(cs), 1)), params(cs), 64).view(np.float32)
    for c, (W, sexp) in enumerate(cs):
        want = lt.upper_bound(est, nx, W, sexp)
        assert np.array_equal(got[c].view(np.uint32), want.view(np.uint32)), (W, sexp)     # a NaN estimate: +inf bits
        assert got[c, 2].view(np.uint32) == 0x7f800000


def test_zero_rows(probe):
    ws = [lt.long_rows(nks) * lt.ROW // 2 for nks in (6, 10, 14, 18)] + [1, 64, 65]
    got = run(probe, P.L_ZERO, None, None, params([(w,) for w in ws]), 1024)
    for c, w in enumerate(ws):
        assert w <= 1024 and not got[c, :w].any() and np.all(got[c, w:] == 0xffffffff), w
