"""tests/_filter_copy.py is what the device's copy and step words are held to (tests/test_gpu_filter_copy_bytes.py,
tests/test_gpu_step_words.py): here the reference itself is held to statements that share no code with it -- `encode` to
struct.pack('<e') (round to nearest even, OverflowError beyond f16), e_c to a correctly rounded sum and to exact powers of
two, the words' offsets to a ctypes mirror of StreamCtl, `threshold` to the level in rational arithmetic."""
import ctypes
import struct
from fractions import Fraction

import numpy as np
import pytest

import _filter_copy as fc
from test_filter_copy_bound_cpu import CASES, adversarial, exact_acc
from test_gpu_filter_copy_bytes import (FP32_MAX, SHAPES, VALUE_KINDS, VALUE_SHAPE, base_ensemble, plant, positions, probe_rounds,
                                        tie_probes)

f32, f16 = np.float32, np.float16


def _pack_e(v):
    """The independent encoder: struct's binary16 (nearest even; raises where f16 has no finite value); non-finite -> the copy's NaN."""
    if not np.isfinite(v):
        return fc.COPY_NAN
    try:
        return struct.unpack("<H", struct.pack("<e", float(v)))[0]
    except OverflowError:
        return fc.COPY_NAN


def _encode_inputs():
    allh = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(f16).astype(f32)          # every f16 value
    pos = np.arange(0x7c00, dtype=np.uint32).astype(np.uint16).view(f16).astype(np.float64)    # 0 .. 65504, ascending
    mids = ((pos[:-1] + pos[1:]) / 2).astype(f32)                                              # every midpoint: subnormal and normal
    assert np.array_equal(mids.astype(np.float64), (pos[:-1] + pos[1:]) / 2)
    sub = np.array([0x00000001, 0x00000400, 0x007fffff, 0x80000001, 0x807fffff], np.uint32).view(f32)
    extra = np.array([65504, 65519, 65520, -65504, -65519, -65520, FP32_MAX, -FP32_MAX, 0.0, -0.0, np.nan, np.inf, -np.inf], f32)
    return np.concatenate([allh, mids, -mids, sub, extra])


@pytest.mark.parametrize("e_c", [0, 6, -7, 60, -60])
def test_encode_is_round_to_nearest_even_with_one_nan(e_c):
    c = _encode_inputs()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        y = (c.astype(np.float64) * 2.0 ** -e_c).astype(f32)
        exact = np.isnan(c) | (y.astype(np.float64) * 2.0 ** e_c == c.astype(np.float64))         # (y 2^e_c is c again: no fp32 rounding on the way)
    assert exact.sum() >= (c.size - 8 if abs(e_c) < 60 else 60000), (e_c, int(exact.sum()), c.size)
    got = fc.encode(y[exact], e_c).view(np.uint16)
    want = np.array([_pack_e(v) for v in c[exact]], np.uint16)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(c[exact][i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]
    assert set(got[(got & 0x7c00) == 0x7c00].tolist()) <= {fc.COPY_NAN}


def test_every_probe_of_the_gpu_test_is_a_tie_or_one_step_beside_it():
    for name, c in tie_probes():
        lo, hi = f16(np.nextafter(f16(c), f16(-np.inf))), f16(np.nextafter(f16(c), f16(np.inf)))
        near = [float(f16(c)), float(lo), float(hi)]
        mids = {(near[0] + near[1]) / 2, (near[0] + near[2]) / 2}
        if "ulp32" in name:
            assert any(abs(c - m) in (abs(float(np.spacing(f32(m)))), abs(float(np.spacing(f32(m)))) / 2) for m in mids), (name, c)
        else:
            assert c in mids, (name, c)


@pytest.mark.parametrize("R,T", SHAPES, ids=[f"{r}x{t}" for r, t in SHAPES])
def test_the_shapes_ensembles_are_decidable(R, T):
    base = base_ensemble("returns", R, T)
    rounds = probe_rounds("returns", R, T)
    for probes in (rounds if R * T <= 1 << 16 else rounds[SHAPES.index((R, T)) % len(rounds):][:1]):
        assert len(probes) <= len(positions(R, T))
        ds, e_c, _ = plant(base, probes, "returns")                    # (asserts: decidable, e_c unchanged, both exponents agree)
        hdr, halves, e2 = fc.reference_copy(ds)
        assert e2 == e_c and hdr.size == 64 and halves.shape == (R, fc.copy_pitch(T))
        assert not halves[:, T:].any() and struct.unpack("<4siqqq", hdr[:32].tobytes()) == (b"PSHC", e_c, R, T, fc.copy_pitch(T))
        assert not hdr[32:].any()
        m = fc.exponent_margin(ds)
        if R * T >= 4096:
            assert 0.62 <= m <= 0.89 and e_c == 6, (m, e_c)


@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_the_value_kinds_are_decidable_and_their_exponents_are_the_stated_ones(kind):
    R, T = VALUE_SHAPE
    base = base_ensemble(kind, R, T)
    assert fc.decidable(base), (kind, fc.exponent_margin(base))
    seen = set()
    for probes in probe_rounds(kind, R, T):
        ds, e_c, placed = plant(base, probes, kind)
        seen |= {n for _, _, n, _ in placed}
        _, halves, _ = fc.reference_copy(ds)
        nonfin = ~np.isfinite(ds)
        assert (halves[:, :T][nonfin] == fc.COPY_NAN).all()
        # NaN and +-inf are excluded from the rms and from the count: the exponent is the finite samples' alone
        fin = ds[np.isfinite(ds)]
        assert fc.reference_exponent(fin.reshape(1, -1)) == e_c if fin.size else e_c == 0
    p = fc.power_of_two_exponent(base)
    if kind.startswith("pow2_"):
        assert p == int(kind[5:]) and e_c == -(p + 1) and fc.exponent_margin(ds) == 0.5
    else:
        assert p is None or kind == "one_finite"
    want = {"returns": 6, "rms_2^-80": 60, "rms_2^+80": -60, "zeros": 0, "all_nan": 0, "one_finite": 5}
    if kind in want:
        assert e_c == want[kind]
    if kind in ("scale_up", "scale_down", "prices"):
        assert (e_c > 20) if kind == "scale_down" else (e_c < 0)
    if kind == "rms_2^+80":
        assert {"+65504", "-65519", "+65520", "fp32 max", "nan", "+inf", "-inf"} <= seen
    if kind == "returns":
        assert {n for n, _ in tie_probes()} <= seen and {"+0", "-0", "fp32 subnormal", "nan", "+inf", "-inf"} <= seen


def test_the_sum_of_squares_is_math_fsums():
    import math
    rng = np.random.default_rng(5)
    for ds in (base_ensemble("returns", 5, 2047), base_ensemble("scale_down", 3, 1023), base_ensemble("prices", 7, 300),
               (rng.standard_normal(4000) * 10.0 ** rng.integers(-18, 18, 4000)).astype(f32), np.array([2.0 ** -149, 3.0, np.nan], f32)):
        fin = ds[np.isfinite(ds)].astype(np.float64)
        assert fc._finite_sumsq(ds) == (math.fsum((fin * fin).tolist()), fin.size)


def test_the_clamps_hold_at_60_and_nothing_finite_gives_0():
    one = np.ones((2, 9), f32)
    for p, want in ((-61, 60), (-60, 59), (-62, 60), (-100, 60), (59, -60), (58, -59), (60, -60), (100, -60)):
        ds = one * f32(2.0 ** p)
        assert fc.copy_exponent(ds) == fc.reference_exponent(ds) == want, (p, want)
    for ds in (np.zeros((3, 5), f32), np.full((3, 5), np.nan, f32), np.full((1, 1), np.inf, f32), np.zeros((0, 4), f32)):
        assert fc.copy_exponent(ds) == fc.reference_exponent(ds) == 0 and fc.exponent_margin(ds) is None
    # an undecidable ensemble is an error of the test that made it, not a case to skip
    ds = np.ones((1, 4), f32)
    ds[0, 0] = f32(1 - 2.0 ** -22)
    assert not fc.decidable(ds)
    with pytest.raises(AssertionError, match="summation order"):
        fc.reference_exponent(ds)


def test_word_offsets_agree_with_a_ctypes_mirror():
    class StreamCtl(ctypes.Structure):
        _fields_ = [("ticket", ctypes.c_uint32), ("ovf", ctypes.c_uint32), ("armed", ctypes.c_uint32), ("scale_bits", ctypes.c_uint32),
                    ("ncand", ctypes.c_uint32 * 4), ("tau2_bits", ctypes.c_uint32 * 4), ("thr2_bits", ctypes.c_uint32 * 4),
                    ("xn_bits", ctypes.c_uint32 * 4)]

    off = fc.step_word_offsets()
    assert set(off) == {"ticket", "ovf", "armed", "scale_bits", "tau2_bits", "thr2_bits", "xn_bits"}
    for name, o in off.items():
        assert o == getattr(StreamCtl, name).offset - StreamCtl.ncand.offset, name
    assert sum(4 * w for _, w in fc.stream_ctl_fields()) == ctypes.sizeof(StreamCtl) == 80


def test_the_routes_constants_are_the_sources():
    assert fc.ROUTE_CONSTANTS == {"fp32": (Fraction(1, 512), Fraction(1, 262144)), "long": (Fraction(1, 900), Fraction(1, 262144)),
                                  "copy": (Fraction(1, 320), Fraction(1, 131072))}
    x = np.full(40, 0.5, f32)
    req, dev = fc.exact_threshold(x, 40, f32(3.0), 1, "long")
    a, b = Fraction(1, 900), Fraction(1, 262144) * Fraction(82, 64)
    assert req == 12 * (1 + Fraction(1, 131072)) * (1 + 2 * a) - 40 * (1 - 3 * a) + b
    assert dev - req == 40 * (1 - 3 * a) * Fraction(1e-12)
    assert fc.f32_round_up(Fraction(1, 3)) == f32(1 / 3) and float(f32(1 / 3)) > 1 / 3 and fc.f32_round_up(Fraction(-1, 3)) == np.nextafter(f32(-1 / 3), f32(0))
    assert fc.f32_round_up(Fraction(5, 4)) == f32(1.25)


def test_threshold_brackets_the_exact_level_on_the_bound_tests_cases():
    """threshold() -- the emulation's level, which the proof shows safe -- is at or above what the proof needs, T_req, and at most one
    fp32 step above the round-up of what the kernel aims at, T_dev, on all 351 cases of the bound test."""
    assert len(CASES) == 351
    n = flood = unarmed = 0
    for i, (kind, W, scale, qfac) in enumerate(CASES):
        ds, q = adversarial(kind, 6, fc.SEG + W - 1, 1, W, 0, 1000 + i)
        ds = (ds * f32(scale)).astype(f32)
        x = (q[0] * f32(scale) * f32(qfac)).astype(f32)
        if not np.isfinite(x).all():
            unarmed += 1
            continue
        acc = np.stack([exact_acc(r, x) for r in ds])
        fin = np.sort(acc[np.isfinite(acc)].ravel())
        tau = f32(fin[min(200, fin.size - 1)]) if fin.size else None
        allowed = fc.sexp_of(x, tau) if fin.size else None
        if allowed is None:
            unarmed += 1
            continue
        e_c = fc.copy_exponent(ds)
        flood += allowed < e_c - 14
        s = min(allowed, e_c)
        thr = fc.threshold(x, W, tau, f32(2.0 ** s), fc.A_COPY, fc.B_COPY)
        assert thr is not None
        req, dev = fc.exact_threshold(x, W, tau, s, "copy")
        assert req < dev or not x.any()
        assert Fraction(float(thr)) >= req, (kind, W, scale, qfac)
        up = fc.f32_round_up(dev)
        assert thr <= np.nextafter(up, f32(np.inf)), (kind, W, scale, qfac, thr, up)
        n += 1
    assert n + unarmed == 351 and n >= 300 and flood >= 1, (n, unarmed, flood)
