"""The ONE statement of what the resident f16 filter copy and the scan step built on it compute (numpy and stdlib only).

The first half is the numpy emulation the bound's proof runs on (tests/test_filter_copy_bound_cpu.py): the build
(`copy_exponent`, `encode`), the step's exponent (`sexp_of`), the level (`threshold`) and the per-window test (`rejects`).
The second half is what the device is held to, derived from the same functions: the copy's bytes (`reference_copy`), whether
two summation orders can disagree on e_c (`exponent_margin`, `decidable`), the level in exact rational arithmetic
(`exact_threshold`) and where the sample launch leaves its words (`step_word_offsets`).  Constants and layouts are parsed
out of the sources: nothing is written a second time.

tests/test_filter_copy_reference_cpu.py tests this module; tests/test_gpu_filter_copy_bytes.py and tests/test_gpu_step_words.py
hold the device to it."""
import math
import re
import struct
from fractions import Fraction
from pathlib import Path

import numpy as np

f32, f16 = np.float32, np.float16
SEG = 1024
CSRC = Path(__file__).resolve().parent.parent / "shadowing_amd" / "csrc"
SRC = (CSRC / "psh_segment.h").read_text()
KERNELS_H = (CSRC / "psh_kernels.h").read_text()
STREAM_HIP = (CSRC / "psh_stream.hip").read_text()


def _const(name):
    m = re.search(r"#define %s \(1\.0 / ([0-9.]+)\)" % name, SRC)
    assert m, name
    return 1.0 / float(m.group(1))


A_COPY, B_COPY = _const("PSH_COPY_A"), _const("PSH_COPY_B")


# ---------------------------------------------------------------------------------------------------------------------
# the emulation the proof runs on
# ---------------------------------------------------------------------------------------------------------------------
def copy_exponent(ds):
    fin = ds[np.isfinite(ds)].astype(np.float64)
    ms = float((fin * fin).sum() / fin.size) if fin.size else 0.0
    if not (ms > 0.0 and ms < 1e300):
        return 0
    _, ex = np.frexp(np.sqrt(ms))
    return int(np.clip(-int(ex), -60, 60))


def encode(y, e_c):
    with np.errstate(over="ignore", invalid="ignore"):
        h = (y.astype(f32) * f32(2.0 ** e_c)).astype(f32).astype(f16)
    h[~np.isfinite(h)] = f16(np.nan)
    return h


def sexp_of(x, tau):
    """stream_sexp_of: None when the step is not armed."""
    qbits = int(np.abs(x).max().view(np.uint32))
    tbits = int(f32(tau).view(np.uint32))
    if not (tau > 0 and np.isfinite(tau) and qbits < 0x7f800000):
        return None
    et = ((tbits >> 23) & 255) - 126
    sexp = (12 - et) // 2 if 12 - et >= 0 else -((et - 12 + 1) // 2)
    if qbits >= 0x00800000:
        eq = ((qbits >> 23) & 255) - 126
        sexp = min(sexp, 3 - eq)
    if not (-60 <= sexp <= 60 and tbits >= 0x00800000):
        return None
    return sexp


def threshold(x, W, tau, sc, a, b):
    nxs = float(((x.astype(np.float64) * float(sc)) ** 2).sum())
    bm = b * ((2 * W + 2) / 64.0 if W > 31 else 1.0)
    T = float(tau) * float(sc) ** 2 * (1.0 + 1.0 / 131072.0) * (1.0 + 2.0 * a) - nxs * (1.0 - 3.0 * a) * (1.0 - 1e-12) + bm
    Tf = f32(T)
    if float(Tf) < T:
        Tf = np.nextafter(Tf, f32(np.inf))
    return Tf if np.isfinite(Tf) else None


def rejects(crow, x, W, s, e_c, thr):
    """The reject mask of one segment's SEG windows from the copy's halves."""
    delta = s - e_c
    assert -14 <= delta <= 0
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        yh = (crow * f16(2.0 ** delta)).astype(f16)                  # numpy multiplies halves in float and rounds once
        y2 = (yh * yh).astype(f16)
        xh = (f32(-2.0) * (x.astype(f32) * f32(2.0 ** s)).astype(f32)).astype(f32).astype(f16)
        n = len(crow) - W + 1
        t = np.zeros(n, f32)
        for j in range(W):                                            # fp32 accumulation of exact products, energies first
            t = (t.astype(np.float64) + y2[j:j + n].astype(np.float64)).astype(f32)
        for j in range(W):
            t = (t.astype(np.float64) + yh[j:j + n].astype(np.float64) * float(xh[j])).astype(f32)
        return t > thr                                                # (NaN > thr is False: kept)


# ---------------------------------------------------------------------------------------------------------------------
# the copy's bytes
# ---------------------------------------------------------------------------------------------------------------------
COPY_NAN = 0x7e00                       # every non-finite f16 of the copy is this one pattern


def _define(name, text=KERNELS_H):
    m = re.search(r"#define %s\s+\(?([0-9a-fx]+)u?\)?" % name, text)
    assert m, name
    return int(m.group(1), 0)


def copy_pitch(T):
    """filter_copy_pitch (psh_kernels.h), its formula read from the source: T rounded up to whole segments, plus 32."""
    m = re.search(r"filter_copy_pitch\(long long T\) \{ return \(T \+ PSH_SEG - 1\) / PSH_SEG \* PSH_SEG \+ (\d+); \}", KERNELS_H)
    assert m, "filter_copy_pitch"
    assert re.search(r"#define PSH_L 16\b", KERNELS_H) and re.search(r"#define PSH_SEG \(64 \* PSH_L\)", KERNELS_H)
    return (T + SEG - 1) // SEG * SEG + int(m.group(1))


def copy_header(e_c, R, T, pitch):
    """The 64 bytes of CopyHdr (psh_kernels.h): the fields in the struct's own order, parsed from the source."""
    body = re.search(r"struct CopyHdr \{(.*?)\};", KERNELS_H, re.S)
    assert body, "struct CopyHdr"
    decl = re.sub(r"//[^\n]*", "", body.group(1))
    values = {"magic": _define("PSH_COPY_MAGIC"), "e_c": e_c, "R": R, "T": T, "pitch": pitch}
    fmt, args = "<", []
    for ty, names in re.findall(r"(unsigned|int|long long)\s+([^;]+);", decl):
        for name in (n.strip() for n in names.split(",")):
            arr = re.fullmatch(r"(\w+)\[(\d+)\]", name)
            code = {"unsigned": "I", "int": "i", "long long": "q"}[ty]
            if arr:                                                   # (the pad words: zero)
                fmt += code * int(arr.group(2))
                args += [0] * int(arr.group(2))
            else:
                fmt += code
                args.append(values[name])
    raw = struct.pack(fmt, *args)
    assert len(raw) == 64 and raw[:4] == b"PSHC", raw[:4]
    return np.frombuffer(raw, np.uint8).copy()


def reference_copy(ds):
    """(header bytes (64,) uint8, halves (R, pitch) uint16, e_c) of the copy psh_filter_copy_build makes of `ds` (R, T) float32."""
    ds = np.ascontiguousarray(ds, dtype=f32)
    R, T = ds.shape
    pitch = copy_pitch(T)
    e_c = copy_exponent(ds)
    halves = np.zeros((R, pitch), np.uint16)                          # the tail of every row is zero
    for r0 in range(0, R, 1024):
        halves[r0:r0 + 1024, :T] = encode(ds[r0:r0 + 1024], e_c).view(np.uint16)
    halves[:, :T][(halves[:, :T] & 0x7c00) == 0x7c00] = COPY_NAN
    return copy_header(e_c, R, T, pitch), halves, e_c


def _finite_sumsq(ds):
    """(the correctly rounded sum of squares of the finite samples, their number): what math.fsum gives (the reference test holds
    it to that), taken in integers so that 2^24 samples cost a second.  The square of a float32 is exact in double: m 2^e with a
    53-bit integer m; the halves of m are summed per exponent (at most 2^27 x 2^24 < 2^53: exact in a double's bincount), the
    exact rational total is rounded once."""
    fin = np.ascontiguousarray(ds, dtype=f32).ravel()
    fin = fin[np.isfinite(fin)].astype(np.float64)
    n = int(fin.size)
    assert n <= 1 << 24
    sq = fin * fin
    sq = sq[sq > 0]
    if sq.size == 0:
        return 0.0, n
    mant, ex = np.frexp(sq)
    mi = np.ldexp(mant, 53).astype(np.int64)
    e0 = int(ex.min())
    idx = (ex - e0).astype(np.int64)
    hi = np.bincount(idx, weights=(mi >> 27).astype(np.float64))
    lo = np.bincount(idx, weights=(mi & ((1 << 27) - 1)).astype(np.float64))
    total = sum(((int(h) << 27) + int(l)) << i for i, (h, l) in enumerate(zip(hi, lo)) if h or l)
    return float(Fraction(total) * Fraction(2) ** (e0 - 53)), n


def exponent_margin(ds):
    """The mantissa m in [0.5, 1) of the reference rms = m 2^ex of the finite samples (the sum of squares correctly rounded:
    math.fsum's value); None when there is no positive finite rms (e_c = 0 by definition, nothing to decide)."""
    s, n = _finite_sumsq(ds)
    ms = s / n if n else 0.0
    if not (ms > 0.0 and ms < 1e300):
        return None
    m, _ = math.frexp(math.sqrt(ms))
    return m


def power_of_two_exponent(ds):
    """p when every finite sample is +-2^p for ONE p (all sums are then exact, m = 0.5 and e_c = -(p + 1) exactly), else None."""
    fin = np.ascontiguousarray(ds, dtype=f32).ravel()
    fin = np.abs(fin[np.isfinite(fin)])
    if fin.size == 0 or not (fin == fin[0]).all() or fin[0] == 0:
        return None
    m, ex = math.frexp(float(fin[0]))
    return ex - 1 if m == 0.5 else None


MARGIN_LO, MARGIN_HI = 0.5 * (1 + 2.0 ** -20), 1 - 2.0 ** -20


def decidable(ds):
    """Whether two summation orders in double cannot disagree on e_c: m well inside [0.5, 1) -- a double sum of n <= 2^24 exact
    squares is within n 2^-53 < 2^-29 of the true one, relatively --, or the exact case of one power of two, or no rms at all."""
    m = exponent_margin(ds)
    return m is None or power_of_two_exponent(ds) is not None or MARGIN_LO <= m <= MARGIN_HI


def reference_exponent(ds):
    """e_c from the correctly rounded sum (a second statement of copy_exponent, to hold it against): asserts decidability."""
    assert decidable(ds), f"the test's ensemble leaves e_c to the summation order: m = {exponent_margin(ds)!r}"
    s, n = _finite_sumsq(ds)
    ms = s / n if n else 0.0
    if not (ms > 0.0 and ms < 1e300):
        return 0
    _, ex = math.frexp(math.sqrt(ms))
    return max(-60, min(60, -ex))


# ---------------------------------------------------------------------------------------------------------------------
# the level, exactly
# ---------------------------------------------------------------------------------------------------------------------
def _route_constants():
    """{route: (a, b)} as Fractions, from stream_threshold_of's two lines in psh_stream.hip and PSH_COPY_A / PSH_COPY_B."""
    ma = re.search(r"const double am = copy \? PSH_COPY_A : \(W > 33 \? 1\.0 / ([0-9.]+) : 1\.0 / ([0-9.]+)\);", STREAM_HIP)
    mb = re.search(r"const double bm = \(copy \? PSH_COPY_B : 1\.0 / ([0-9.]+)\) \* \(W > 31 \? \(double\)\(2 \* W \+ 2\) / 64\.0 : 1\.0\);", STREAM_HIP)
    assert ma and mb, "stream_threshold_of's constants are not where they were"
    assert re.search(r"taus \* \(1\.0 \+ 1\.0 / 131072\.0\) \* \(1\.0 \+ 2\.0 \* am\) - nxs \* \(1\.0 - 3\.0 \* am\) \* \(1\.0 - 1e-12\) \+ bm", STREAM_HIP), \
        "stream_threshold_of's formula is not what exact_threshold restates"
    inv = lambda s: Fraction(1, int(float(s)))                        # noqa: E731
    copy = tuple(inv(re.search(r"#define %s \(1\.0 / ([0-9.]+)\)" % n, SRC).group(1)) for n in ("PSH_COPY_A", "PSH_COPY_B"))
    assert (float(copy[0]), float(copy[1])) == (A_COPY, B_COPY)
    return {"fp32": (inv(ma.group(2)), inv(mb.group(1))), "long": (inv(ma.group(1)), inv(mb.group(1))), "copy": copy}


ROUTE_CONSTANTS = _route_constants()


def exact_threshold(x, W, tau, s, route):
    """(T_req, T_dev) as Fractions for the query x (float32), the level tau (float32) and the step's exponent s:
        T_req = tau~ (1 + 2^-17)(1 + 2 a) - nx~ (1 - 3 a) + b          what the proof needs (psh_stream_copy.hip, psh_scan.hip)
        T_dev = the same with the kernel's (1 - 1e-12) on the nx~ term   what stream_threshold_of aims at
    tau~ = tau 4^s, nx~ = sum (x_j 2^s)^2, (a, b) the route's pair -- "fp32" (W <= 33), "long" (W > 33), "copy" (W <= 33) --, b
    times (2 W + 2) / 64 for W > 31."""
    assert (route == "long") == (W > 33), (route, W)
    a, b = ROUTE_CONSTANTS[route]
    if W > 31:
        b = b * Fraction(2 * W + 2, 64)
    x = np.asarray(x, dtype=f32).reshape(-1)
    assert x.size == W
    s2 = Fraction(4) ** s
    taus = Fraction(float(f32(tau))) * s2
    nxs = sum(Fraction(float(v)) ** 2 for v in x) * s2
    head = taus * (1 + Fraction(1, 131072)) * (1 + 2 * a)
    return head - nxs * (1 - 3 * a) + b, head - nxs * (1 - 3 * a) * (1 - Fraction(1e-12)) + b


def scaled_level_and_norm(x, tau, s):
    """(tau~, nx~) as Fractions: the two magnitudes the kernel's roundings are relative to."""
    s2 = Fraction(4) ** s
    return Fraction(float(f32(tau))) * s2, sum(Fraction(float(v)) ** 2 for v in np.asarray(x, dtype=f32).reshape(-1)) * s2


def f32_round_up(q):
    """The smallest float32 >= the Fraction q (finite q inside float32's range)."""
    c = f32(float(q))
    while Fraction(float(c)) < q:
        c = np.nextafter(c, f32(np.inf))
    while Fraction(float(np.nextafter(c, f32(-np.inf)))) >= q:
        c = np.nextafter(c, f32(-np.inf))
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the sample launch's words
# ---------------------------------------------------------------------------------------------------------------------
def stream_ctl_fields():
    """[(name, words)] of struct StreamCtl (psh_kernels.h) in declaration order; every member is `unsigned`."""
    body = re.search(r"struct StreamCtl \{(.*?)\};", KERNELS_H, re.S)
    assert body, "struct StreamCtl"
    decl = re.sub(r"//[^\n]*", "", body.group(1))
    fields = []
    for stmt in decl.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        m = re.fullmatch(r"unsigned\s+(.+)", stmt, re.S)
        assert m, f"StreamCtl holds something that is not an unsigned word: {stmt!r}"
        for name in (n.strip() for n in m.group(1).split(",")):
            arr = re.fullmatch(r"(\w+)\[(\d+)\]", name)
            fields.append((arr.group(1), int(arr.group(2))) if arr else (name, 1))
    return fields


def step_word_offsets():
    """Byte offsets of StreamCtl's words RELATIVE TO `ncand` (psh_candidates_layout's out[8] is the offset of ncand)."""
    off, at = {}, 0
    for name, words in stream_ctl_fields():
        off[name] = at
        at += 4 * words
    want = ("ticket", "ovf", "armed", "scale_bits", "tau2_bits", "thr2_bits", "xn_bits")
    assert all(n in off for n in want + ("ncand",)), off
    return {n: off[n] - off["ncand"] for n in want}
