"""The bytes psh_filter_copy_build writes, held bit for bit to tests/_filter_copy.py::reference_copy -- the code the bound's
proof runs on (tests/test_filter_copy_bound_cpu.py).  Every other GPU test of the copy route looks at results that are exact
whatever the copy holds; here the 64 header bytes, every half of every row (the zero tails included) and 4 KiB guard zones
around `out` and `scratch` are read back after ONE synchronise.

Shapes: the smallest that cross each piece of the three launches' bookkeeping (SHAPES).  Values: VALUE_KINDS, each on a base
ensemble whose e_c is DECIDABLE (tests/_filter_copy.py::decidable: two summation orders in double cannot disagree on it; a
case that is not is an error of this file and fails, it is never skipped).  Probes -- with s = 2^-e_c: s x every kind of f16
tie, +-0, fp32 subnormals, NaN and +-inf -- are planted at the first, middle and last sample of the first and last row and
next to T - 1; the reference says beforehand that they leave e_c where it was.

Where the probes at f16's upper edge can live: a sample is at most sqrt(N) times the rms of its N-sample ensemble, so
y 2^e_c >= 65504 needs N > 4.29e9 samples unless e_c is CLAMPED.  s x 65504, 65519, 65520 (both signs) and fp32's largest
value are therefore planted in the ensemble whose rms is 2^80 (e_c clamped at -60, s = 2^60: the probes are quiet samples
there, and most of the ensemble is out of f16's range -> NaN); in every other ensemble they would move e_c and miss the edge."""
import struct

import numpy as np
import pytest
import torch

import _filter_copy as fc
from _adversarial import make as adversarial
from shadowing_amd import synthetic as syn

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 4096
FILL = 0xA5

# (R, T), what they cross: T odd, T not a multiple of 8, either side of a segment, pitch = T + 32
# exactly; one block of the sum of squares; the first pass's 1024-block cap on either side; every thread of the first pass
# striding twice; the write pass's 8192-block cap (17 039 360 halves against 16 777 216; 64 MB: the largest case)
SHAPES = [(1, 1), (1, 7), (3, 1023), (2, 1024), (2, 1025), (5, 2047), (3, 2049), (1, 255), (1, 257), (256, 1024), (257, 1024),
          (520, 1024), (8192, 2048)]
VALUE_KINDS = ["returns", "prices", "scale_up", "scale_down", "rms_2^-80", "rms_2^+80", "pow2_-3", "pow2_0", "pow2_5", "zeros",
               "all_nan", "one_finite"]
VALUE_SHAPE = (3, 2049)                 # odd T, two segments and a sample, three rows: every position of a probe exists


def tie_probes():
    """[(name, c)]: c is exactly representable in float32 and sits ON or one float32 step beside a midpoint of two neighbouring
    f16 values; |c| < 2."""
    out = []
    # normal ties: between mantissas k and k + 1 of binade e -- k even (down to even), k odd (up to even), k = 1023 (up into the next binade)
    for e in (-14, -1, 0):
        for k in (0, 1, 2, 511, 1022, 1023):
            out.append((f"tie e={e} k={k}", (1024 + k) * 2.0 ** (e - 10) + 2.0 ** (e - 11)))
    # subnormal ties: (k + 1/2) 2^-24 -- k = 0 goes to zero, k = 1023 to the smallest normal
    for k in (0, 1, 2, 511, 1022, 1023):
        out.append((f"subnormal tie k={k}", (k + 0.5) * 2.0 ** -24))
    # one float32 step off a tie: truncation, round-half-up and round-half-away all differ from nearest-even somewhere in this list
    for name, c in list(out):
        if name in ("tie e=0 k=0", "tie e=0 k=1", "subnormal tie k=0", "subnormal tie k=1", "tie e=-14 k=0"):
            out.append((name + " + ulp32", float(np.nextafter(f32(c), f32(np.inf)))))
            out.append((name + " - ulp32", float(np.nextafter(f32(c), f32(-np.inf)))))
    out = out + [(n + " negated", -v) for n, v in out]
    for _, c in out:
        assert float(f32(c)) == c and abs(c) < 2
    return out


def edge_probes():
    """f16's upper edge: the largest half, the last value that rounds to it, the tie that does not; both signs."""
    return [(f"{sign}{c}", float(c) if sign == "+" else -float(c)) for c in (65504, 65519, 65520) for sign in "+-"]


SMALL_ABSOLUTE = [("+0", 0.0), ("-0", -0.0), ("fp32 subnormal", 2.0 ** -149), ("-fp32 subnormal", -(2.0 ** -140)),
                  ("largest fp32 subnormal", float(np.frombuffer(struct.pack("<I", 0x007fffff), f32)[0]))]
NONFINITE = [("nan", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf"))]
FP32_MAX = float(np.finfo(f32).max)


def base_ensemble(kind, R, T, seed=4100):
    rng = np.random.default_rng(seed)
    ret = syn.dataset(R, T, seed + R + T)[:, 0, :].copy()
    if kind == "returns":
        ds = ret
    elif kind == "prices":                                            # levels around 100: e_c < 0
        ds = (100.0 * np.exp(np.cumsum(ret.astype(np.float64), axis=1))).astype(f32)
    elif kind in ("scale_up", "scale_down"):
        ds = adversarial(kind, R, T, 1, 20, 0, seed + 1)[0]
    elif kind == "rms_2^-80":                                         # the true exponent is +80: clamped at +60
        ds = (ret * f32(2.0 ** -74)).astype(f32)
    elif kind == "rms_2^+80":                                         # ... -81: clamped at -60
        ds = (ret * f32(2.0 ** 86)).astype(f32)
    elif kind.startswith("pow2_"):
        p = int(kind[5:])
        ds = (rng.choice([-1.0, 1.0], size=(R, T)) * 2.0 ** p).astype(f32)
    elif kind == "zeros":
        ds = np.zeros((R, T), f32)
    elif kind == "all_nan":
        ds = np.full((R, T), np.nan, f32)
    elif kind == "one_finite":
        ds = np.full((R, T), np.nan, f32)
        ds[R // 2, T // 3] = f32(0.02)
    else:
        raise AssertionError(kind)
    return np.ascontiguousarray(ds, dtype=f32)


def positions(R, T):
    """(r, t) of the probes: first, middle and last sample of the first and last row, and T - 2 beside T - 1 for odd T."""
    ts = [0, T // 2, T - 1] + ([T - 2] if T % 2 and T >= 2 else [])
    pos = []
    for r in (0, R - 1):
        for t in ts:
            if 0 <= t < T and (r, t) not in pos:
                pos.append((r, t))
    return pos


def probe_rounds(kind, R, T):
    """The probe lists of one ensemble's builds, each at most as long as the positions: [[(name, multiple of s or None, absolute
    value)]].  A finite probe of |c| < 2 in place of a sample moves the mean square by at most 16 / N of itself: at most N / 128
    of them per build keep the mantissa of the rms inside (0.55, 0.96) when the base's is inside [0.62, 0.89].  What is not
    finite moves nothing: one of those rides every round.  An ensemble too small for a finite probe gets none, or NaN and inf."""
    npos = len(positions(R, T))
    budget = (R * T) // 128
    nonfinite = [(n, None, v) for n, v in NONFINITE]
    if kind.startswith("pow2_") or kind in ("zeros", "all_nan", "one_finite"):
        # (a finite probe would take the exactness these ensembles are about: what is not finite is left out of rms AND count)
        return [nonfinite]
    if budget == 0:
        return [[], nonfinite[:max(npos - 1, 0)]]
    finite = [(n, c, None) for n, c in tie_probes()] + [(n, None, v) for n, v in SMALL_ABSOLUTE]
    if kind == "rms_2^+80":
        finite += [(n, c, None) for n, c in edge_probes()]
    per = max(1, min(npos - 1, budget))
    rounds = [finite[i:i + per] + [nonfinite[(i // per) % 3]] for i in range(0, len(finite), per)]
    if kind == "rms_2^+80":
        rounds.append([("fp32 max", None, FP32_MAX)] + nonfinite)      # (it makes the rms alone: e_c stays clamped)
    return rounds


def plant(base, probes, kind):
    """(the ensemble with the probes in, e_c, [(r, t, name, value)]).  The reference says that the probes leave e_c where the base
    had it (so s x c meets its tie) and that the margin is still decidable; fp32's largest value may move a clamped e_c nowhere."""
    R, T = base.shape
    e0 = fc.reference_exponent(base)
    s = 2.0 ** -e0
    ds = base.copy()
    placed = []
    finite = 0
    for (r, t), (name, c, v) in zip(positions(R, T), probes):
        val = f32(c * s) if c is not None else f32(v)
        if c is not None:
            assert float(val) == c * s and np.isfinite(val), (name, c, s)       # (a power of two times a float32: exact)
        finite += bool(np.isfinite(val)) and name != "fp32 max"
        ds[r, t] = val
        placed.append((r, t, name, val))
    assert finite <= max(R * T // 128, 0), "more finite probes than the margin's argument allows"
    e1 = fc.reference_exponent(ds)                                    # (asserts decidability)
    assert e1 == fc.copy_exponent(ds), (kind, e1, fc.copy_exponent(ds), fc.exponent_margin(ds))
    if any(c is not None for _, c, _ in probes):                      # (s x c meets its tie only under the exponent s came from)
        assert e1 == e0, (kind, e0, e1, fc.exponent_margin(ds))
    return ds, e1, placed


def guarded(dev, nbytes):
    """A byte tensor of `nbytes` filled with 0xA5 inside an allocation with GUARD bytes of 0xA5 on both sides."""
    whole = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + nbytes]


def raw_build(dev, ds_t, out, scratch, stream=None):
    from shadowing_amd import _native
    R, T = ds_t.shape
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    rc = _native.load().psh_filter_copy_build(dev.index, st.cuda_stream, ds_t.data_ptr(), R, T, out.data_ptr(), out.numel(),
                                              scratch.data_ptr(), scratch.numel())
    assert rc == 0, rc


def build_and_read(dev, ds, stream=None, out_pair=None):
    """One build on the caller's own guarded buffers, ONE synchronise: (the copy's bytes, both allocations as numpy)."""
    from shadowing_amd import _native
    R, T = ds.shape
    nbytes, pitch = _native.filter_copy_bytes(R, T)
    assert pitch == fc.copy_pitch(T) and nbytes == 64 + 2 * R * pitch, (nbytes, pitch)
    ds_t = torch.as_tensor(ds).to(dev)
    whole_o, out = out_pair if out_pair is not None else guarded(dev, nbytes)
    whole_s, scratch = guarded(dev, _native.PSH_FILTER_COPY_SCRATCH_BYTES)
    assert out.data_ptr() % 16 == 0 and out.numel() == nbytes
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    raw_build(dev, ds_t, out, scratch, stream)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), whole_o.cpu().numpy(), whole_s.cpu().numpy()


def check_bytes(got, whole_o, whole_s, ds, what, placed=()):
    """Header, rows and guards against the reference; the first difference is named with its sample."""
    hdr, halves, e_c = fc.reference_copy(ds)
    R, T = ds.shape
    pitch = halves.shape[1]
    e_dev = int(got[4:8].view(np.int32)[0])
    assert e_dev == e_c, f"{what}: the device's e_c is {e_dev}, the reference's {e_c} (m = {fc.exponent_margin(ds)!r})"
    assert np.array_equal(got[:64], hdr), f"{what}: header bytes {got[:64].tolist()} != {hdr.tolist()}"
    rows = got[64:].view(np.uint16).reshape(R, pitch)
    if not np.array_equal(rows, halves):
        r, t = (int(v[0]) for v in np.nonzero(rows != halves))
        src = f"sample {ds[r, t]!r} (bits {int(ds[r, t].view(np.uint32)):#010x})" if t < T else "the row's zero tail"
        names = [n for (pr, pt, n, _) in placed if (pr, pt) == (r, t)]
        raise AssertionError(f"{what}: {int((rows != halves).sum())} halves differ; first at row {r}, half {t}: device "
                             f"{int(rows[r, t]):#06x}, reference {int(halves[r, t]):#06x}, {src}, e_c {e_c} {names}")
    for name, whole, n in (("out", whole_o, got.size), ("scratch", whole_s, whole_s.size - 2 * GUARD)):
        assert (whole[:GUARD] == FILL).all(), f"{what}: the guard in front of `{name}` was written"
        assert (whole[GUARD + n:] == FILL).all(), f"{what}: the guard behind `{name}` was written"
    return e_c


@pytest.mark.parametrize("R,T", SHAPES, ids=[f"{r}x{t}" for r, t in SHAPES])
def test_every_byte_of_the_copy_at_the_bookkeeping_shapes(hip_device, R, T):
    """Log-returns with one round of probes, rotated by the shape so that the shapes together plant every probe."""
    base = base_ensemble("returns", R, T)
    rounds = probe_rounds("returns", R, T)
    probes = rounds[SHAPES.index((R, T)) % len(rounds)] if rounds else []
    ds, e_c, placed = plant(base, probes, "returns")
    got, wo, ws = build_and_read(hip_device, ds)
    check_bytes(got, wo, ws, ds, f"returns {R}x{T}", placed)
    if R * T >= 4096:
        assert e_c == 6                                               # (sigma sqrt(dt) = 0.0126: rms 2^6 = 0.81)


@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_every_byte_of_the_copy_for_every_kind_of_value(hip_device, kind):
    R, T = VALUE_SHAPE
    base = base_ensemble(kind, R, T)
    n_probes = 0
    for i, probes in enumerate(probe_rounds(kind, R, T)):
        ds, e_c, placed = plant(base, probes, kind)
        got, wo, ws = build_and_read(hip_device, ds)
        check_bytes(got, wo, ws, ds, f"{kind} round {i}", placed)
        n_probes += len(placed)
        # what the probes are for, said by the reference (the device equals it): ties to even, the edge, NaN for what is not finite
        _, halves, _ = fc.reference_copy(ds)
        for r, t, name, val in placed:
            h = int(halves[r, t])
            if not np.isfinite(val) or name in ("+65520", "-65520", "fp32 max"):
                assert h == fc.COPY_NAN, (name, hex(h))
            elif name in ("+65504", "+65519"):
                assert h == 0x7bff, (name, hex(h))
            elif name in ("-65504", "-65519"):
                assert h == 0xfbff, (name, hex(h))
            elif name.startswith(("tie", "subnormal tie")) and "ulp32" not in name:
                assert h & 1 == 0, f"{name}: a tie went to the odd neighbour {h:#06x}"
    assert n_probes >= 3
    want = {"returns": 6, "rms_2^-80": 60, "rms_2^+80": -60, "pow2_-3": 2, "pow2_0": -1, "pow2_5": -6, "zeros": 0, "all_nan": 0,
            "one_finite": 5}
    if kind in want:
        assert e_c == want[kind], (kind, e_c)
    if kind == "prices":
        assert e_c < 0


def test_two_builds_another_stream_a_used_buffer_and_FilterCopy_give_the_same_bytes(hip_device):
    from shadowing_amd import _native
    dev = hip_device
    R, T = 5, 2047
    ds, _, placed = plant(base_ensemble("returns", R, T), probe_rounds("returns", R, T)[1], "returns")
    first, wo, ws = build_and_read(dev, ds)
    check_bytes(first, wo, ws, ds, "first build", placed)
    again, wo, ws = build_and_read(dev, ds)
    assert np.array_equal(first, again), "two builds of one ensemble differ"
    side, wo, ws = build_and_read(dev, ds, stream=torch.cuda.Stream(dev))
    check_bytes(side, wo, ws, ds, "a build on a non-default stream", placed)
    # a buffer that still holds the copy of another shape (more rows, a shorter pitch: old halves lie under the new zero tails)
    other = base_ensemble("prices", 11, 1000)
    nbytes, _ = _native.filter_copy_bytes(R, T)
    onbytes, _ = _native.filter_copy_bytes(*other.shape)
    assert onbytes >= nbytes
    whole = torch.full((GUARD + onbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    scratch = torch.empty(_native.PSH_FILTER_COPY_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
    raw_build(dev, torch.as_tensor(other).to(dev), whole[GUARD:GUARD + onbytes], scratch)
    torch.cuda.synchronize(dev)
    old = whole[GUARD:GUARD + onbytes].cpu().numpy()
    assert (old[64:nbytes] != 0).mean() > 0.5                          # (the new copy's zero tails do land on old values)
    used, wo, ws = build_and_read(dev, ds, out_pair=(whole, whole[GUARD:GUARD + nbytes]))
    assert np.array_equal(used, first), "a build into a used buffer kept some of its bytes"
    assert np.array_equal(wo[GUARD + nbytes:GUARD + onbytes], old[nbytes:]), "the build wrote behind its own bytes"
    assert (wo[:GUARD] == FILL).all() and (wo[GUARD + onbytes:] == FILL).all()
    # the Python owner of a copy
    obj = _native.FilterCopy(torch.as_tensor(ds).to(dev))
    torch.cuda.synchronize(dev)
    assert obj.buf.numel() == nbytes and np.array_equal(obj.buf.cpu().numpy(), first), "FilterCopy.buf differs from the raw call"
