"""The words stream_sample_finish (psh_stream.hip) leaves for the scan -- StreamCtl's armed, scale_bits, tau2_bits, thr2_bits,
xn_bits -- read back from the caller's workspace (psh_candidates_layout out[8] + tests/_filter_copy.py::step_word_offsets) and
held to the reference the bound's proof runs on (tests/_filter_copy.py: sexp_of, threshold, exact_threshold).  Every other
test sees these numbers through outcomes only: a level a little too low shows there for a thin band of windows at most.

Per case, BEFORE the device is asked, the reference says which regime the case is in (armed or not; on the copy route
delta = s - e_c: 0, -14 .. -1, or the flood below e_c - 14).  Then:
    tau2_bits   the hint's bits when hinted; without a hint the device's word is taken as tau and the rest derives from it
    xn_bits     the oracle's qnorm, or the caller's
    armed, scale_bits   2^s, s = the minimum over the queries of sexp_of(x, tau); the copy route: min(that, e_c)
    thr2_bits   +inf exactly in the flood; otherwise, for the device's Tf and the exact rationals T_req, T_dev, tau~, nx~:
        safe       Tf >= T_req - 8 x 2^-53 (tau~ + nx~)
                   The kernel's formula tau~ c1 c2 - nx~ c3 c4 + b has EIGHT roundings in double of its own -- 1 + 2a, 1 - 3a,
                   the four products, the difference, the sum with b -- each at most 2^-53 of an intermediate no larger than
                   tau~ (1 + 2^-17)(1 + 2a) + nx~ + b; what the sum nx~ itself loses in double (2 W + 1 roundings, 10^-14 nx~) is
                   under the 10^-12 nx~ the kernel's factor (1 - 1e-12) puts on the safe side; the conversion to fp32 rounds up.
        not loose  Tf is at most two fp32 steps above the fp32 round-up of T_dev (one for the roundings above moving T across
                   an fp32 value, one to spare).
        Whether Tf equals threshold() bit for bit is printed and tallied, not asserted (a long window's nx~ is summed a
        lane a sample).
Every case keeps the end condition of the other tests: results bit-equal to the oracle, directly or through the status
protocol."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import _filter_copy as fc
from _adversarial import make as adversarial
from shadowing_amd import synthetic as syn

pytestmark = pytest.mark.gpu

f32 = np.float32
OVERLAP = dict(R=2048, T=2048, h=0, k=200)                # the route table's `overlap` shape (tests/test_gpu_routes.py)
LONG = dict(R=3072, T=2300, h=9, k=150, W=64)             # ... and its `long_W64_B1`
TALLY = {"bit-equal to threshold()": 0, "inside the two conditions only": 0, "flood (+inf)": 0, "not armed": 0}

_ens, _oracle_cache, _acc_cache = {}, {}, {}


def _bits(v):
    return int(np.asarray(v, f32).reshape(-1)[0].view(np.uint32))


def ensemble(dev, key):
    """{ds, ds_t, copy (a FilterCopy, built once), e_c}: the copy's exponent is read from its header and must be the reference's."""
    from shadowing_amd import _native
    if key not in _ens:
        if key == "overlap":
            ds = syn.dataset(OVERLAP["R"], OVERLAP["T"], 9100 + OVERLAP["R"])[:, 0, :].copy()
        elif key == "long":
            ds = syn.dataset(LONG["R"], LONG["T"], 9100 + LONG["R"])[:, 0, :].copy()
        else:
            ds, q_adv = adversarial(key, OVERLAP["R"], OVERLAP["T"], 1, 20, 0, 7700)
        ds = np.ascontiguousarray(ds, dtype=f32)
        ds_t = torch.as_tensor(ds).to(dev)
        copy = _native.FilterCopy(ds_t)
        torch.cuda.synchronize(dev)
        e_c = int(copy.buf[4:8].cpu().numpy().view(np.int32)[0])
        assert e_c == fc.reference_exponent(ds) == fc.copy_exponent(ds), (key, e_c)      # (asserts decidability)
        _ens[key] = dict(ds=ds, ds_t=ds_t, copy=copy, e_c=e_c, q=None if key in ("overlap", "long") else q_adv)
    return _ens[key]


def query(W):
    return syn.gbm_log_returns((1, W), 9200 + W)


def oracle_topk(oracle_mod, key, ds, q, k, h, qn=None):
    ck = (key, q.tobytes(), k, h, None if qn is None else qn.tobytes())
    if ck not in _oracle_cache:
        _oracle_cache[ck] = oracle_mod.scan_topk(ds, q, k, h=h, qn=qn)
    return _oracle_cache[ck]


def level(oracle_mod, key, ds, x, h, m, xn=None, floor=0):
    """Just above the m-th smallest finite acc of the oracle's chain -- moved up to the end of the run of windows whose DISTANCE
    sqrt(acc) / ||x|| equals the m-th's: a level inside such a run (a loud query: every acc is ||x||^2 to five digits) would admit
    some of a tie and leave the rest of it out, and the k best by (d, r, t) would not all be candidates."""
    ck = (key, x.tobytes(), h)
    if ck not in _acc_cache:
        a = oracle_mod.all_acc(ds, x, h=h).ravel()
        a = a[np.isfinite(a)]
        _acc_cache[ck] = np.sort(np.partition(a, 2048)[:2048])
    a = _acc_cache[ck]
    xn = f32(oracle_mod.qnorm(x)[0]) if xn is None else f32(xn)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (np.sqrt(a, dtype=f32) / xn).astype(f32)
    j = m
    while j + 1 < a.size and d[j + 1] == d[m]:
        j += 1
    if j + 1 < a.size:
        return np.nextafter(f32(a[j]), f32(np.inf))
    # (the run does not end among the 2048 nearest windows: the level goes in FRONT of it, where more than `floor` windows remain)
    j = int(np.searchsorted(d, d[m], "left"))
    assert j > floor, "a run of equal distances holds the k-th window and more than 2048 others: no level serves this query"
    return f32(a[j])


def read_words(ws, lay, B):
    off = fc.step_word_offsets()
    base = lay["hdr_stream_ncand"]
    lo, hi = base + min(off.values()), base + max(off.values()) + 16
    raw = ws.buf[lo:hi].cpu().numpy()
    word = lambda name, n: raw[base + off[name] - lo: base + off[name] - lo + 4 * n].copy().view(np.uint32)     # noqa: E731
    out = {n: int(word(n, 1)[0]) for n in ("ticket", "ovf", "armed", "scale_bits")}
    out.update({n: word(n, 4)[:B].copy() for n in ("tau2_bits", "thr2_bits", "xn_bits")})
    return out


def run_step(dev, oracle_mod, key, q, route, hint=None, qnorm=None, k=None, h=None, what="", rerun=True):
    """One raw call on the caller's own Workspace: the words, checked against the reference; then the end condition.
    `hint`: None, "k", "4k" (levels at about the k-th / 4k-th acc of every query) or B floats.  Returns the regime's facts."""
    from shadowing_amd import _native
    ens = ensemble(dev, key)
    ds, ds_t = ens["ds"], ens["ds_t"]
    R, T = ds.shape
    q = np.ascontiguousarray(q, dtype=f32)
    B, W = q.shape
    shape = LONG if route == "long" else OVERLAP
    k = shape["k"] if k is None else k
    h = shape["h"] if h is None else h
    if isinstance(hint, str):
        m = {"k": k, "4k": 4 * k}[hint]
        hint = np.array([level(oracle_mod, key, ds, q[b], h, m, None if qnorm is None else qnorm[b], floor=k) for b in range(B)], f32)
    hint_t = None if hint is None else torch.as_tensor(np.asarray(hint, f32)).to(dev)
    qn_t = None if qnorm is None else torch.as_tensor(np.asarray(qnorm, f32)).to(dev)
    flags = _native.FLAG_OVERLAP if route != "long" and B == 1 else 0
    ws, info = _native.Workspace(dev), {}
    d, idx, st = _native.scan_topk(ds_t, torch.as_tensor(q).to(dev), k, h=h, workspace=ws, flags=flags, tau_hint=hint_t, qnorm=qn_t,
                                   info=info, filter_copy=ens["copy"] if route == "copy" else None)
    torch.cuda.synchronize(dev)
    assert info["path"] == 3 and info["copy_served"] == (1 if route == "copy" else 0), (what, info)
    words = read_words(ws, _native.candidates_layout(R, T, B, W, h, k, ws.buf.numel()), B)
    st = st.cpu().numpy()

    # ---- the reference's statement of the case
    if hint is not None:
        assert [int(v) for v in words["tau2_bits"]] == [_bits(v) for v in hint], f"{what}: tau2_bits is not the hint"
    taus = words["tau2_bits"].view(f32)
    sexps = [fc.sexp_of(q[b], taus[b]) for b in range(B)]
    want_qn = oracle_mod.qnorm(q) if qnorm is None else np.asarray(qnorm, f32)
    facts = dict(armed=None not in sexps, sexps=sexps, e_c=ens["e_c"] if route == "copy" else None, status=st.tolist(), taus=taus.tolist())
    line = f"step words: {what}: route {route} W {W} B {B} tau {['%.6g' % t for t in taus]} sexp {sexps}"
    if not facts["armed"]:
        TALLY["not armed"] += 1
        print(line + " -> NOT ARMED")
        assert (words["armed"], words["scale_bits"]) == (0, 0), (what, words)
        assert (st != 0).all(), (what, st)
        assert np.isnan(d.cpu().numpy()).all() and (idx.cpu().numpy() == -1).all(), f"{what}: results of a step that was not armed are not poisoned"
        if rerun:                                         # the same call without the hint, then the rest of the status protocol
            d, idx, st = _native.scan_topk(ds_t, torch.as_tensor(q).to(dev), k, h=h, workspace=ws, flags=flags, qnorm=qn_t,
                                           filter_copy=ens["copy"] if route == "copy" else None)
            torch.cuda.synchronize(dev)
            if int(st.cpu().numpy().any()):
                assert qnorm is None, (what, st)
                d, idx = _native.scan_topk_checked(ds_t, torch.as_tensor(q).to(dev), k, h=h, workspace=ws, flags=flags)
                torch.cuda.synchronize(dev)
            od, oidx = oracle_topk(oracle_mod, key, ds, q, k, h, None if qnorm is None else np.asarray(qnorm, f32))
            assert np.array_equal(d.cpu().numpy().view(np.uint32), od.view(np.uint32)) and np.array_equal(idx.cpu().numpy(), oidx), \
                f"{what}: the rerun without the hint differs from the oracle"
        return facts
    s = min(sexps)
    flood = False
    if route == "copy":
        flood = s < ens["e_c"] - 14
        s = min(s, ens["e_c"])
        facts["delta"] = None if flood else s - ens["e_c"]
    facts["s"], facts["flood"] = s, flood
    assert words["armed"] == 1 and words["scale_bits"] == _bits(f32(2.0 ** s)), \
        f"{what}: armed {words['armed']}, scale_bits {words['scale_bits']:#010x}; the reference: 2^{s} = {_bits(f32(2.0 ** s)):#010x}"
    assert words["ticket"] == 0
    assert [int(v) for v in words["xn_bits"]] == [_bits(v) for v in want_qn], f"{what}: xn_bits {words['xn_bits']} != {want_qn}"
    a, b = fc.ROUTE_CONSTANTS[route]
    for i in range(B):
        tf_bits = int(words["thr2_bits"][i])
        if flood:
            TALLY["flood (+inf)"] += 1
            print(line + f" q{i} -> FLOOD")
            assert tf_bits == 0x7f800000, f"{what}: the flood's threshold is {tf_bits:#010x}, not +inf"
            continue
        tf = words["thr2_bits"][i:i + 1].view(f32)[0]
        assert np.isfinite(tf), (what, tf_bits)
        t_req, t_dev = fc.exact_threshold(q[i], W, taus[i], s, route)
        tau_s, nx_s = fc.scaled_level_and_norm(q[i], taus[i], s)
        emu = fc.threshold(q[i], W, taus[i], f32(2.0 ** s), float(a), float(b))
        equal = emu is not None and _bits(emu) == tf_bits
        TALLY["bit-equal to threshold()" if equal else "inside the two conditions only"] += 1
        up = fc.f32_round_up(t_dev)
        print(line + f" q{i} s {s} delta {facts.get('delta')} Tf {tf!r} ({tf_bits:#010x}) threshold() {emu!r} round-up(T_dev) {up!r} "
              f"Tf - T_req {float(Fraction(float(tf)) - t_req):.3e} -> {'BIT-EQUAL' if equal else 'inside'}")
        assert Fraction(float(tf)) >= t_req - 8 * Fraction(2) ** -53 * (tau_s + nx_s), \
            f"{what}: q{i}: NOT SAFE: Tf = {tf!r} lies {float(t_req - Fraction(float(tf))):.3e} below T_req (tau~ {float(tau_s):.6g}, nx~ {float(nx_s):.6g})"
        assert tf <= np.nextafter(np.nextafter(up, f32(np.inf)), f32(np.inf)), \
            f"{what}: q{i}: LOOSE: Tf = {tf!r} is more than two fp32 steps above round-up(T_dev) = {up!r}"

    # ---- the end condition: the oracle's results, directly or through the status protocol
    od, oidx = oracle_topk(oracle_mod, key, ds, q, k, h, None if qnorm is None else np.asarray(qnorm, f32))
    if (st == 0).all():
        got_d, got_i = d.cpu().numpy(), idx.cpu().numpy()
    elif qnorm is None:
        got = _native.scan_topk_checked(ds_t, torch.as_tensor(q).to(dev), k, h=h, workspace=ws, flags=flags, tau_hint=hint_t)
        torch.cuda.synchronize(dev)
        got_d, got_i = got[0].cpu().numpy(), got[1].cpu().numpy()
    else:
        raise AssertionError(f"{what}: status {st}")
    assert np.array_equal(got_d.view(np.uint32), od.view(np.uint32)) and np.array_equal(got_i, oidx), f"{what}: results differ from the oracle"
    return facts


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hint", [None, "k", "4k"], ids=["sampled", "hint_k", "hint_4k"])
@pytest.mark.parametrize("W", [7, 20, 33])
@pytest.mark.parametrize("route", ["fp32", "copy"])
def test_ordinary_queries_on_both_routes(hip_device, oracle_mod, route, W, hint):
    """delta = 0 on the copy route; W = 33 takes the (2 W + 2) / 64 share of b."""
    q = query(W)
    facts = run_step(hip_device, oracle_mod, "overlap", q, route, hint=hint, what=f"ordinary {hint}")
    assert facts["armed"] and not facts["flood"] and facts.get("delta", 0) == 0, facts
    if hint is not None:
        assert facts["status"] == [0], facts
    if W == 20:                                           # (the query's largest |x| binds: 3 - eq < (12 - et) / 2)
        tb = _bits(f32(facts["taus"][0]))
        et = ((tb >> 23) & 255) - 126
        assert facts["sexps"][0] < (12 - et) // 2, facts


LOUD = [3, 9, 12, 15, 16, 17, 20]


@pytest.mark.parametrize("hint", ["k", "4k", None], ids=["hint_k", "hint_4k", "sampled"])
@pytest.mark.parametrize("p", LOUD)
def test_copy_route_scales_the_copy_down_and_floods_below_14(hip_device, oracle_mod, p, hint):
    """The query 2^p times louder: delta < 0 down to -14 exactly, the flood beyond; the reference says which before the device runs."""
    e_c = ensemble(hip_device, "overlap")["e_c"]
    q = (query(20) * f32(2.0 ** p)).astype(f32)
    eq = ((_bits(np.abs(q).max()) >> 23) & 255) - 126
    want_delta = min(3 - eq, e_c) - e_c                  # (the level of a loud query is about ||x||^2: its own rule binds)
    assert want_delta == {3: -1, 9: -7, 12: -10, 15: -13, 16: -14, 17: -15, 20: -18}[p]
    facts = run_step(hip_device, oracle_mod, "overlap", q, "copy", hint=hint, what=f"loud 2^{p} {hint}")
    assert facts["armed"] and facts["sexps"][0] == 3 - eq, facts
    assert facts["flood"] == (want_delta < -14) and facts["delta"] == (None if want_delta < -14 else want_delta), facts


@pytest.mark.parametrize("route", ["fp32", "copy"])
@pytest.mark.parametrize("et", [-8, -7, 11, 12, 13, 14, 15])
def test_hints_at_both_parities_and_both_sides_of_the_halving(hip_device, oracle_mod, route, et):
    """A quiet query, so that tau's rule binds: s = (12 - et) / 2 rounded towards -inf on either side of 12 - et = 0."""
    q = (query(20) * f32(2.0 ** -20)).astype(f32)
    hint = np.array([1.5 * 2.0 ** (et - 1)], f32)         # in [2^(et-1), 2^et)
    want = {-8: 10, -7: 9, 11: 0, 12: 0, 13: -1, 14: -1, 15: -2}[et]
    assert fc.sexp_of(q[0], hint[0]) == want
    facts = run_step(hip_device, oracle_mod, "overlap", q, route, hint=hint, what=f"hint with et = {et}")
    assert facts["armed"] and facts["sexps"] == [want], facts


@pytest.mark.parametrize("route", ["fp32", "copy"])
@pytest.mark.parametrize("kind", ["tau_binds", "subnormal_query", "caller_qnorm"])
def test_which_rule_binds(hip_device, oracle_mod, route, kind):
    q = query(20)
    qn = None
    if kind == "tau_binds":
        q = (q * f32(2.0 ** -6)).astype(f32)
    elif kind == "subnormal_query":                      # no sample is a normal float: the query's rule is not even looked at
        q = (q * f32(2.0 ** -122)).astype(f32)
        assert 0 < _bits(np.abs(q).max()) < 0x00800000
        qn = np.array([1.0], f32)                         # (its own norm is 0 in fp32: every distance would be inf)
    else:
        qn = (oracle_mod.qnorm(q) * f32(1.5)).astype(f32)
    facts = run_step(hip_device, oracle_mod, "overlap", q, route, hint="4k", qnorm=qn, what=kind)
    assert facts["armed"], facts
    tb = _bits(f32(facts["taus"][0]))
    et = ((tb >> 23) & 255) - 126
    halved = (12 - et) // 2 if 12 - et >= 0 else -((et - 12 + 1) // 2)
    assert (facts["sexps"][0] == halved) == (kind != "caller_qnorm"), facts


NOT_ARMED = {"zero": 0.0, "negative": -1.0, "nan": float("nan"), "inf": float("inf"), "subnormal": 1e-40, "s_past_60": 2.0 ** -126,
             "inf_in_query": None}


@pytest.mark.parametrize("route", ["fp32", "copy"])
@pytest.mark.parametrize("kind", list(NOT_ARMED))
def test_a_step_that_is_not_armed_says_so_and_the_rerun_is_the_oracles(hip_device, oracle_mod, route, kind):
    """armed == 0, scale_bits == 0, a status that is not OK, NaN distances and (-1, -1) indices; then the call without the hint."""
    dev = hip_device
    q, qn = query(20), None
    hint = np.array([NOT_ARMED[kind]], f32) if kind != "inf_in_query" else None
    if kind == "s_past_60":                               # the smallest normal level, a query of subnormals: (12 + 125) / 2 = 68 > 60
        q = (q * f32(2.0 ** -122)).astype(f32)
        qn = np.array([1.0], f32)                         # (its own norm is 0 in fp32: every distance would be inf)
        assert fc.sexp_of(q[0], hint[0]) is None and hint[0] > 0 and 0 < _bits(np.abs(q).max()) < 0x00800000
    if kind == "inf_in_query":                            # (no window of such a query has a finite distance: nothing to rerun)
        hint = np.array([level(oracle_mod, "overlap", ensemble(dev, "overlap")["ds"], q[0], 0, 800)], f32)
        q = q.copy()
        q[0, 5] = np.inf
    facts = run_step(dev, oracle_mod, "overlap", q, route, hint=hint, qnorm=qn, what=f"not armed: {kind}", rerun=kind != "inf_in_query")
    assert not facts["armed"], facts


@pytest.mark.parametrize("hint", [None, "4k"], ids=["sampled", "hint_4k"])
def test_three_queries_of_mixed_amplitude_share_one_scale(hip_device, oracle_mod, hint):
    q = syn.gbm_log_returns((3, 20), 9300)
    q = (q * np.array([[1.0], [2.0 ** 6], [2.0 ** -6]], f32)).astype(f32)
    facts = run_step(hip_device, oracle_mod, "overlap", q, "fp32", hint=hint, what=f"three queries {hint}")
    assert facts["armed"] and facts["s"] == facts["sexps"][1] and facts["sexps"][1] < min(facts["sexps"][0], facts["sexps"][2]), facts


@pytest.mark.parametrize("hint", [None, "k"], ids=["sampled", "hint_k"])
def test_long_window_takes_its_own_constants(hip_device, oracle_mod, hint):
    """a = 1 / 900, b = 2^-18 (2 W + 2) / 64; without a hint the query is staged in LDS and nx~ summed a lane a sample."""
    assert fc.ROUTE_CONSTANTS["long"] == (Fraction(1, 900), Fraction(1, 2 ** 18))
    q = query(LONG["W"])
    facts = run_step(hip_device, oracle_mod, "long", q, "long", hint=hint, what=f"long window {hint}")
    assert facts["armed"], facts


@pytest.mark.parametrize("route", ["fp32", "copy"])
@pytest.mark.parametrize("kind", ["spikes", "scale_up", "scale_down", "quiet_one_loud"])
def test_sampled_levels_on_adversarial_ensembles(hip_device, oracle_mod, route, kind):
    """The level comes from the device; scale, threshold and norm are checked from it (armed or not: the reference says)."""
    run_step(hip_device, oracle_mod, kind, ensemble(hip_device, kind)["q"], route, what=f"adversarial {kind}")


def test_tally_of_the_threshold_cases():
    """(last in the file) How many thresholds were bit-equal to threshold() and how many only inside the two conditions."""
    print("step words tally: " + ", ".join(f"{v} {k}" for k, v in TALLY.items()))
    assert TALLY["bit-equal to threshold()"] + TALLY["inside the two conditions only"] > 0
