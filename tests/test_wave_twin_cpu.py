"""The numpy twins of the device primitives (tests/_wave_twin.py) are the reference of tests/test_gpu_wave_primitives.py
and tests/test_gpu_sort_primitives.py, so they are held here against plain definitions: the sort network sorts (0-1
principle), sums and scans are exact where every order is, the key map is monotone, the rank search equals a brute-force
expansion.  And the probe library is what it says: built with the product's flags, exporting what its binding declares,
stale when a header changes, and no part of the product."""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _probe
import _probe_cases as cases
import _wave_twin as tw

REPO = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------ the sort network
def _n2s(NB):
    return [1 << e for e in range(NB, 15)]


@pytest.mark.parametrize("NB", [2, 3, 4])
def test_sort_twin_sorts_random_entries(NB):
    g = np.random.default_rng(NB)
    for n2 in _n2s(NB):
        ent = g.integers(0, 1 << 63, size=(4, n2), dtype=np.uint64)
        ent[1] = ent[1] >> np.uint64(60)                  # many ties
        assert np.array_equal(tw.qnt_sort(ent, NB), np.sort(ent, axis=1)), n2


@pytest.mark.parametrize("NB", [2, 3, 4])
def test_sort_twin_zero_one_principle(NB):
    """A comparison network sorts every input iff it sorts every 0-1 input: all of them for n2 <= 16, beyond that 2048
    random ones per size, the density of ones running from 0 to 1 across them."""
    g = np.random.default_rng(10 + NB)
    for n2 in _n2s(NB):
        if n2 <= 16:
            x = ((np.arange(1 << n2, dtype=np.uint32)[:, None] >> np.arange(n2, dtype=np.uint32)[None, :]) & 1).astype(np.uint8)
        else:
            x = (g.random((2048, n2), dtype=np.float32) < np.linspace(0.0, 1.0, 2048, dtype=np.float32)[:, None]).astype(np.uint8)
        assert np.array_equal(tw.qnt_sort(x, NB), np.sort(x, axis=1)), n2


# ------------------------------------------------------------------------------------------ sums and scans
def _ints(g, shape, dtype):
    return g.integers(-1000, 1001, size=shape).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sum_twins_are_exact_on_integers(dtype):
    g = np.random.default_rng(1)
    v = _ints(g, (8, 64), dtype)
    want = np.array([math.fsum(row) for row in v.astype(np.float64)])
    got = tw.wave_reduce(v, tw.op_sum)
    assert got.dtype == dtype and np.array_equal(got, np.broadcast_to(want[:, None], got.shape).astype(dtype))
    if dtype == np.float32:
        assert np.array_equal(tw.wave_sum_dpp(v), want.astype(np.float32))
    blk = _ints(g, (5, 16, 64), dtype)
    for waves in (1, 2, 4, 8, 16):
        want = np.array([math.fsum(b.ravel()) for b in blk[:, :waves].astype(np.float64)])
        assert np.array_equal(tw.block_reduce(blk[:, :waves], tw.op_sum), want.astype(dtype))


def test_scan_twins_are_exact_on_integers():
    g = np.random.default_rng(2)
    for dtype in (np.float32, np.float64):
        v = _ints(g, (8, 64), dtype)
        assert np.array_equal(tw.wave_scan_inclusive(v), np.cumsum(v.astype(np.int64), axis=1).astype(dtype))
    u = g.integers(0, 1 << 32, size=(8, 64), dtype=np.uint64).astype(np.uint32)          # wraps
    want = (np.cumsum(u.astype(np.uint64), axis=1) & np.uint64(0xffffffff)).astype(np.uint32)
    assert np.array_equal(tw.wave_scan_inclusive(u), want)
    assert np.array_equal(tw.wave_scan_inclusive(u.view(np.int32)).view(np.uint32), want)
    assert np.array_equal(tw.wave_scan_inclusive_dpp(u.view(np.int32)).view(np.uint32), want)
    assert np.array_equal(tw.wave_total_dpp(u.view(np.int32)).view(np.uint32), want[:, 63])
    c = g.integers(0, 9, size=(4, 64))
    packed = tw.wave_scan_inclusive_dpp(tw.pack16(c)).view(np.uint32)
    assert np.array_equal(packed & 0xffff, np.cumsum(c, axis=1)) and np.array_equal(packed >> 16, np.cumsum(c, axis=1))


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_qnt_scan_twin_is_exact_on_integers(threads):
    g = np.random.default_rng(threads)
    x = g.integers(0, 1000, threads).astype(np.float64)
    pre, total = tw.qnt_scan(x, False)
    assert np.array_equal(pre, np.cumsum(x) - x) and total == math.fsum(x)
    pre, total = tw.qnt_scan(x, True)
    assert np.array_equal(pre, np.concatenate([[0.0], np.maximum.accumulate(x)[:-1]])) and total == x.max()


def test_min_max_operators():
    g = np.random.default_rng(3)
    a, b = g.standard_normal(1000).astype(np.float32), g.standard_normal(1000).astype(np.float32)
    a[::7], b[::11] = np.nan, np.nan
    assert np.array_equal(tw.bits(tw.fmin_(a, b)), tw.bits(np.fmin(a, b)))      # no +-0 tie here: numpy's fmin is the definition
    assert np.array_equal(tw.bits(tw.fmax_(a, b)), tw.bits(np.fmax(a, b)))
    pz, nz = np.float32([0.0]), np.float32([-0.0])
    for x, y in ((pz, nz), (nz, pz)):                                           # -0 orders below +0, whichever side it is on
        assert np.signbit(tw.fmin_(x, y))[0] and not np.signbit(tw.fmax_(x, y))[0]
    i = np.array([-2**31, -1, 0, 2**31 - 1], dtype=np.int32)
    assert tw.wave_reduce(np.resize(i, 64), tw.fmin_)[0] == -2**31 and tw.wave_reduce(np.resize(i.view(np.uint32), 64), tw.fmin_)[0] == 0
    assert tw.wave_reduce(np.resize(i, 64), tw.fmax_)[0] == 2**31 - 1 and tw.wave_reduce(np.resize(i.view(np.uint32), 64), tw.fmax_)[0] == 0xffffffff


# ------------------------------------------------------------------------------------------ keys
def test_key_twin():
    x = cases.key_floats()
    k = tw.qnt_key(x)
    assert np.all(np.diff(k.astype(np.int64)) > 0)                              # strictly increasing with the value
    assert np.array_equal(tw.qnt_value(k).view(np.uint32), x.view(np.uint32))
    nz = np.float32([-0.0])
    assert tw.qnt_key(nz)[0] == tw.qnt_key(np.float32([0.0]))[0] == 0x80000000
    assert tw.qnt_value(tw.qnt_key(nz)).view(np.uint32)[0] == 0                 # -0 comes back as +0


# ------------------------------------------------------------------------------------------ the rank search
@pytest.mark.parametrize("per", [1, 16, 32])
def test_rank_twin_equals_brute_force(per):
    for h in cases.rank_histograms(per):
        if int(h.astype(np.uint64).sum()) > 1 << 20:
            continue                                                            # (not expandable; the boundaries below cover it)
        expanded = np.repeat(np.arange(h.size), h)
        for rank in cases.rank_list(h):
            got = tw.rank_find(h, int(rank))
            if rank < 1 or rank > expanded.size:
                assert got is None
            else:
                b = int(expanded[int(rank) - 1])
                assert got == (b, int((expanded < b).sum()), int(h[b])) and h[b] > 0


def test_rank_twin_above_2_31():
    h = cases.rank_histograms(1)[-1]
    total = int(h.astype(np.uint64).sum())
    assert total > 1 << 31
    assert tw.rank_find(h, 1 << 30) == (0, 0, 1 << 30) and tw.rank_find(h, (1 << 30) + 1) == (21, 1 << 30, (1 << 30) + 5)
    assert tw.rank_find(h, total) == (63, total - ((1 << 30) - 1), (1 << 30) - 1) and tw.rank_find(h, total + 1) is None


def test_bucket_upper_edge_twin():
    for kmin, kmax, shift in ((0, 0xffffffff, 22), (0xfffffff0, 0xffffffff, 0), (0x80000000, 0xc0000000, 21), (5, 5, 0)):
        for bucket in (0, 1, 7, 1023, 2047):
            e = tw.bucket_upper_edge(kmin, kmax, bucket, shift)
            keys = [k for k in (kmin + (bucket << shift), kmin + ((bucket + 1) << shift) - 1) if k <= kmax]
            assert e <= kmax and all(((k - kmin) >> shift) == bucket and k <= e for k in keys)


def test_fast_div_and_unit_queue_twins():
    assert tw.fast_div_magic(1) == 0 and tw.fast_div_magic(3) == 1431655765 and tw.fast_div_magic(1 << 31) == 2
    for n in (0, 1, 255, 256, 257, 2**31 - 1):
        for grid in (1, 255, 256, 1024):
            lo, hi = tw.unit_queue(n, grid)
            assert lo[0] == 0 and hi[-1] == n and np.array_equal(lo[1:], hi[:-1]) and np.all(lo <= hi)


# ------------------------------------------------------------------------------------------ the probe library
@pytest.fixture(scope="module")
def probe_lib():
    return _probe.build()


def test_probe_builds_with_the_products_flags(probe_lib):
    from shadowing_amd import _build
    cmd = _probe.command(probe_lib)
    assert cmd[1:1 + len(_build.HIPCC_FLAGS)] == _build.HIPCC_FLAGS
    assert {"--offload-arch=gfx950", "-O3", "-ffp-contract=off"} <= set(cmd)
    assert [c for c in cmd[1:] if c.startswith("-") and c not in _build.HIPCC_FLAGS and not c.startswith("-I")] == ["-o"]
    assert probe_lib.exists() and not _probe.is_stale()
    src = _probe.SOURCE.read_text()
    for h in _probe.HEADERS:
        assert f'#include "{h.name}"' in src


def test_probe_exports_what_the_binding_declares(probe_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(probe_lib)], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (psh_probe_\w+)", out))
    assert exported == set(_probe.EXPORTS)
    L = _probe.load()
    assert L.psh_probe_version() == _probe.PROBE_VERSION
    assert L.psh_probe_wave(0, 0, None, None, None, None, 100, None) == -1          # no partial block, let alone a partial wave
    assert L.psh_probe_sort(2, None, None, 2048, 1, None) == -1                     # beyond <2, 256>'s capacity


def test_probe_is_stale_when_a_headers_bytes_change(tmp_path, monkeypatch):
    copies = []
    for p in _probe.DEPS:
        (tmp_path / p.name).write_bytes(p.read_bytes())
        copies.append(tmp_path / p.name)
    monkeypatch.setattr(_probe, "DEPS", copies)
    lib = tmp_path / "libpsh_probe.so"
    lib.write_bytes(b"")
    assert _probe.is_stale(lib)                                                     # no stamp
    _probe._stamp(lib).write_text(_probe.source_hash() + "\n")
    assert not _probe.is_stale(lib)
    for c in copies:
        before = c.read_bytes()
        c.write_bytes(before + b"\n")
        assert _probe.is_stale(lib), c.name
        c.write_bytes(before)
        assert not _probe.is_stale(lib)


def test_product_library_exports_no_probe_symbol():
    from shadowing_amd import _build
    _build.build()
    out = subprocess.run(["nm", "-D", str(_build.LIB)], check=True, capture_output=True, text=True).stdout
    assert "psh_version" in out and "probe" not in out


def test_product_never_mentions_the_probe():
    from shadowing_amd import _build
    for p in (REPO / "shadowing_amd").rglob("*"):
        if p.is_file() and p.suffix in (".py", ".hip", ".h", ".cpp", ".c"):
            assert not re.search(r"\b_probe\b|psh_probe", p.read_text()), p      # (the module tests/_probe.py, the library)
    assert not any("probe" in p.name for p in _build.SOURCES + _build.DEPS)


# ------------------------------------------------------------------------------------------ the long-window twins
import _long_twin as lt  # noqa: E402
from fractions import Fraction  # noqa: E402


def test_round_f32_is_round_to_nearest_even():
    one, ulp = Fraction(1), Fraction(2) ** -23
    assert lt.round_f32(one + ulp / 2) == np.float32(1.0)                           # a tie: to the even neighbour
    assert lt.round_f32(one + ulp * 3 / 2) == np.float32(1.0) + np.float32(2.0 ** -22)
    assert lt.round_f32(one + ulp / 2 + Fraction(2) ** -80) == np.float32(1.0) + np.float32(2.0 ** -23)
    assert lt.round_f32(Fraction(2) ** -150) == 0 and lt.round_f32(Fraction(2) ** -150 * 3) == np.float32(2.0 ** -148)
    assert lt.round_f32(Fraction(2) ** 128 - Fraction(2) ** 103) == np.inf and lt.round_f32(-(Fraction(2) ** 128)) == -np.inf
    g = np.random.default_rng(5)
    for x in g.standard_normal(200) * 10.0 ** g.integers(-30, 30, 200):
        assert lt.round_f32(Fraction(float(x))) == np.float32(x)                    # float64 -> float32 is one rounding too
    # an fma a float64 product-and-add gets wrong: the product's low bits decide a tie
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** 30)
    assert lt.fma32(a, b, c) == lt.round_f32(Fraction(float(a)) ** 2 + Fraction(float(c)))


def test_energy_operand_twin_against_the_formula():
    sp = cases.long_prefix_sums(3)
    for W in cases.LONG_OPERAND_W:
        for upper in (False, True):
            ce = lt.energy_operand(sp, W, upper)
            lane, r = np.meshgrid(np.arange(64), np.arange(16), indexing="ij")
            p = lt.mx_window(r, lane)
            assert sorted(p.ravel()) == list(range(1024))                             # the map covers the segment once
            S = sp.astype(np.float64)
            want = S[p + W] * (1.0 + (2.0 ** -17 if upper else -(2.0 ** -17))) - S[p]
            assert np.all(np.abs(ce - want) <= 2.0 ** -24 * np.abs(want) * 1.0000001 + 1e-30)       # half an ulp of the result
            E = S[p + W] - S[p]
            assert np.all(ce >= E) if upper else np.all(ce <= E)


def test_tile_min_twin_against_a_plain_minimum():
    for tile, nv in cases.long_tiles():
        lane, r = np.meshgrid(np.arange(64), np.arange(16), indexing="ij")
        valid = lt.mx_window(r, lane) < nv
        want = np.nanmin(np.where(valid, tile, np.inf))
        got = lt.tile_min(tile, nv)
        assert np.all(got == np.float32(want)), nv


def test_query_tables_twin_against_the_formula():
    g = np.random.default_rng(6)
    for nq, W in cases.LONG_TABLE_CASES + ((3, cases.LONG_TABLE_W14),):
        nks = lt.bucket(W)
        xs = g.standard_normal((nq, W)).astype(np.float32)
        tab = lt.query_tables(xs, W, 0.5, nks)
        assert tab.shape == (nq, 8, lt.copy_chunks(nks), 8) and tab.size == nq * lt.query_halves(nks)
        # the fragment of lane (n, hk), K-step s is chunk 2 s + hk - (n >> 3) + 3 of copy n & 7: -2 x~[16 s + 8 hk + i - n]
        for n in (0, 7, 8, 31):
            for hk in (0, 1):
                for s in range(lt.ksteps(W)):
                    frag = tab[:, n & 7, 2 * s + hk - (n >> 3) + 3, :]
                    j = 16 * s + 8 * hk + np.arange(8) - n
                    want = np.where((j >= 0) & (j < W), -2.0 * (xs[:, np.clip(j, 0, W - 1)] * np.float32(0.5)), 0.0)
                    assert np.array_equal(frag, want.astype(np.float16))
    assert sorted({lt.bucket(W) for _, W in cases.LONG_TABLE_CASES} | {lt.bucket(cases.LONG_TABLE_W14)}) == [6, 10, 14, 18]


def test_exact_window_and_upper_bound_twins():
    g = np.random.default_rng(7)
    x, y = g.standard_normal(40).astype(np.float32), g.standard_normal(40).astype(np.float32)
    v = lt.exact_window(y, x, 40)
    want = ((x.astype(np.float64) - y.astype(np.float64)) ** 2).sum()
    assert abs(float(v) - want) <= 41 * 2.0 ** -24 * want
    est, nx = cases.long_bound_inputs()
    for sexp in cases.LONG_BOUND_SEXP:
        ub = lt.upper_bound(est, nx, 126, sexp)
        assert ub.dtype == np.float32 and np.isposinf(ub[1]) and np.isposinf(ub[2])
        fin = np.isfinite(ub)
        plain = (est.astype(np.float64) + nx * (3.0 / 900.0) + 254.0 / 64.0 / 262144.0) * (1.0 + 2.0 / 900.0 + 1e-5 + 6.0 * 2.0 ** -17) * (1.0 + 1e-6) * 4.0 ** -sexp
        assert np.allclose(ub[fin], plain[fin], rtol=1e-6)


def test_stage_row_twin_reads_zero_past_the_row():
    ds, T, cs = cases.long_stage_cases()[0]
    w = lt.stage_row(ds, T, 0, 1024, 1023 + 64)
    assert np.array_equal(w[:5].view(np.float32), ds[0, 1024:]) and not w[5:4 * 272].any()       # ... although row 1 follows
    assert np.all(w[4 * 272:] == 0xffffffff)                                                       # ceil(1087 / 4) = 272 pieces
