"""The copy route's rejection test (copy_scan_kernel, psh_stream_copy.hip) EMULATED in numpy float16 and run over the
adversarial ensembles on the CPU.

What is restated, rounding for rounding:
    the build   : e_c from the rms of the finite samples (rms 2^e_c in [0.5, 1)), c = (f16)(y 2^e_c) to nearest even, what is
                  not a finite f16 stored as NaN
    the step    : the exponent the query's proof allows (stream_sexp_of: max|x| 2^s < 8, tau 4^s <= 4096), s = min(that, e_c),
                  delta = s - e_c <= 0; below e_c - 14 the test is switched off
    the scan    : y^ = fl16(c 2^delta), (y^2)^ = fl16(y^ y^), x^ = fl16(-2 (x 2^s)), t^ = sum (y^2)^ + sum y^ x^ in fp32
    the level   : stream_threshold_of with the copy route's constants PSH_COPY_A / PSH_COPY_B (read from psh_segment.h)
    per window  : reject iff t^ > thr (a NaN keeps the window)
The property: NO window whose exact fp32 chain lies below the level is ever rejected.  The GPU side of it is
tests/test_gpu_filter_copy.py (the admitted sets).  The five restated functions live in tests/_filter_copy.py: the device's
bytes and step words are held to the very code this proof runs on (tests/test_gpu_filter_copy_bytes.py,
tests/test_gpu_step_words.py)."""
import numpy as np
import pytest

from _adversarial import KINDS, make as adversarial
from _filter_copy import A_COPY, B_COPY, SEG, copy_exponent, encode, rejects, sexp_of, threshold

f32, f16 = np.float32, np.float16


def exact_acc(yrow, x):
    W = len(x)
    n = len(yrow) - W + 1
    acc = np.zeros(n, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(W):
            D = (f32(x[j]) - yrow[j:j + n].astype(f32)).astype(f32).astype(np.float64)
            acc = (D * D + acc.astype(np.float64)).astype(f32)
    return acc


def run_case(kind, W, scale, qfac, seed, a=A_COPY, b=B_COPY, depth=200, stats=None):
    ds, q = adversarial(kind, 6, SEG + W - 1, 1, W, 0, seed)
    ds = (ds * f32(scale)).astype(f32)
    x = (q[0] * f32(scale) * f32(qfac)).astype(f32)
    if not np.isfinite(x).all():
        return 0
    e_c = copy_exponent(ds)
    acc = np.stack([exact_acc(r, x) for r in ds])
    fin = np.sort(acc[np.isfinite(acc)].ravel())
    if fin.size == 0:
        return 0
    tau = f32(fin[min(depth, fin.size - 1)])
    allowed = sexp_of(x, tau)
    if allowed is None or allowed < e_c - 14:
        return 0                                                      # not armed / the test is switched off: nothing is rejected
    s = min(allowed, e_c)
    if stats is not None:
        stats["delta<0"] += s < e_c
        stats["e_c<<allowed"] += e_c <= allowed - 4
    thr = threshold(x, W, tau, f32(2.0 ** s), a, b)
    if thr is None:
        return 0
    n_rej = 0
    for r in range(ds.shape[0]):
        rej = rejects(encode(ds[r], e_c), x, W, s, e_c, thr)
        bad = np.nonzero(rej & (acc[r] < tau))[0]
        assert bad.size == 0, (f"{kind} W={W} scale={scale} qfac={qfac}: windows {bad[:5].tolist()} of row {r} with acc "
                               f"{acc[r][bad[:5]].tolist()} < tau {tau!r} were REJECTED by the copy route's test")
        n_rej += int(rej.sum())
    return n_rej


CASES = [(kind, W, scale, qfac) for kind in KINDS for W in (7, 20, 33) for scale in (1.0, 2.0 ** 20, 2.0 ** -20)
         for qfac in (1.0, 2.0 ** 9, 2.0 ** -9)]


def test_copy_route_never_rejects_a_window_below_the_level():
    stats = {"delta<0": 0, "e_c<<allowed": 0}
    rejected = 0
    for i, (kind, W, scale, qfac) in enumerate(CASES):
        rejected += run_case(kind, W, scale, qfac, 1000 + i, stats=stats)
    # queries louder than the data scale the copy down, quieter ones leave the step at e_c well below what they allow
    assert stats["delta<0"] >= 20 and stats["e_c<<allowed"] >= 20, stats
    assert rejected > 0


@pytest.mark.parametrize("a,b", [(0.0, B_COPY), (A_COPY, 0.0)], ids=["no_relative_part", "no_absolute_part"])
def test_a_weakened_constant_is_caught(a, b):
    """The cases have teeth: without the relative part of the bound (the copy's three roundings are then nowhere in the level) and
    without the absolute one (f16 subnormals: an ensemble whose rms a few spikes make) some window below the level is rejected."""
    with pytest.raises(AssertionError, match="REJECTED by the copy route's test"):
        for i, (kind, W, scale, qfac) in enumerate(CASES):
            run_case(kind, W, scale, qfac, 1000 + i, a=a, b=b)


def test_most_windows_are_rejected_at_the_benchmarks_statistics():
    """An emulation that kept everything would make the property vacuous: i.i.d. Gaussian log-returns, a query of the same
    kind, a level a few windows deep."""
    rng = np.random.default_rng(0)
    W = 20
    ds = (rng.standard_normal((8, SEG + W - 1)) * 0.0126).astype(f32)
    x = (rng.standard_normal(W) * 0.0126).astype(f32)
    e_c = copy_exponent(ds)
    acc = np.stack([exact_acc(r, x) for r in ds])
    tau = f32(np.sort(acc.ravel())[8])
    s = min(sexp_of(x, tau), e_c)
    thr = threshold(x, W, tau, f32(2.0 ** s), A_COPY, B_COPY)
    kept = total = 0
    for r in range(8):
        rej = rejects(encode(ds[r], e_c), x, W, s, e_c, thr)
        assert not (rej & (acc[r] < tau)).any()
        kept += int((~rej).sum()); total += rej.size
    assert kept < 0.05 * total, (kept, total)
