"""Every stream-ordered entry of the library, replayed from a captured graph and compared bit for bit.

One pattern throughout: static input and output buffers and a Workspace; one eager call as warm-up (and, where no oracle
exists, as the reference); ONE call -- or one linear chain of calls -- captured by torch.cuda.graph on its single capture
stream; three replays with other inputs written into the same buffers by copy_; every replay compared bit for bit, the
scans with the CPU oracle, the rest with the same calls made eagerly on the same inputs.  No tolerance anywhere: every kernel
involved promises repeatable bits.

What a replay can get wrong that an eager call cannot: a per-call value computed on the host and frozen into the graph (the
fused launch's epoch lives in the workspace header for that reason), a Python-side guard that ran at capture time only (the
"auto" filter copy's version check), an event or allocator call that is illegal while a stream captures (FilterCopy.use).

Which wrappers may be captured was decided by reading them (no .item(), .cpu(), synchronize, pageable host-to-device copy):
everything below.  pdv_generate uploads R10 / R20 when they are host arrays, so it is captured with device tensors.  Not
capturable, and not captured: anything with profile=True (stage timings synchronise), scan_topk_checked and
scan_topk_embedded_checked (they read the status words), embed_plan and count_nonfinite (they read a result), the blocking
and the multi-rank entries."""
import numpy as np
import pytest
import torch

from _graph_replay import admission_hint, assert_same_bits, capture, flatten, replay, snapshot
from _util import assert_exact
from shadowing_amd import synthetic as syn
from test_gpu_routes import EXPECTED, _case, _inputs

pytestmark = pytest.mark.gpu

# a one-query case of the route table -> the table's case whose inputs hold its three queries (same ensemble, same window,
# same k: the oracle's rows of the first three queries), or None: the case's own shape with B = 3
ONE_QUERY = {"default": "B3", "default_hint": "B3", "overlap": "B3", "no_fuse": "B3", "long_W64_B1": "long_W64_B5",
             "exhaustive_small": None, "rows": None, "emb_foveal": None, "emb_dense_mx": None}
BATCHED = ["B3", "B4", "B32", "long_W64_B5"]


def _three_queries(name):
    """(case, ds, kernel, [three (1, .) queries], [their oracle d], [their oracle idx])"""
    c = _case(name)
    src = ONE_QUERY[name]
    ds, ker, q, od, oidx = _inputs(_case(src) if src else dict(c, B=3))
    return c, ds, ker, [q[j:j + 1] for j in range(3)], [od[j:j + 1] for j in range(3)], [oidx[j:j + 1] for j in range(3)]


def _rolled(name):
    """A batched case: replay j scans the queries rolled by j rows, and expects the oracle's rows rolled alike."""
    c = _case(name)
    ds, ker, q, od, oidx = _inputs(c)
    return c, ds, ker, [np.roll(q, j, axis=0) for j in range(3)], [np.roll(od, j, axis=0) for j in range(3)], \
        [np.roll(oidx, j, axis=0) for j in range(3)]


class Scan:
    """The static buffers of one scan call, and the call."""

    def __init__(self, dev, c, ds, ker, B, qlen, ds_t=None, q_t=None, **kw):
        self.c, self.dev, self.kw = c, dev, kw
        self.ds = torch.as_tensor(np.ascontiguousarray(ds[:, 0, :] if ds.ndim == 3 else ds)).to(dev) if ds_t is None else ds_t
        self.ker = None if ker is None else torch.as_tensor(ker).to(dev)
        self.q = torch.zeros((B, qlen), dtype=torch.float32, device=dev) if q_t is None else q_t
        self.hint = torch.zeros((B,), dtype=torch.float32, device=dev) if c["hint"] else None
        k = c["k"]
        self.out = (torch.zeros((B, k), dtype=torch.float32, device=dev), torch.zeros((B, k, 2), dtype=torch.int32, device=dev),
                    torch.zeros((B,), dtype=torch.int32, device=dev))
        self.info = {}

    def call(self):
        from shadowing_amd import _native
        c = self.c
        kw = dict(h=c["h"], flags=c["flag_word"], tau_hint=self.hint, info=self.info, out=self.out, **self.kw)
        if self.ker is None:
            return _native.scan_topk(self.ds, self.q, c["k"], **kw)
        return _native.scan_topk_embedded(self.ds, self.ker, self.q, c["k"], **kw)

    def set(self, q, od):
        self.q.copy_(torch.as_tensor(np.ascontiguousarray(q, dtype=np.float32)))
        if self.hint is not None:
            self.hint.copy_(torch.as_tensor(admission_hint(od, np.asarray(q), self.c["k"])))

    def smudge(self):
        """Plausible numbers of another call in the outputs: what a replay that wrote nothing would leave behind."""
        self.out[0].fill_(1.0)
        self.out[1].fill_(7)
        self.out[2].fill_(-1)

    def results(self):
        torch.cuda.synchronize(self.dev)
        return tuple(t.cpu().numpy() for t in self.out)

    def check(self, od, oidx, what):
        d, idx, st = self.results()
        assert st.tolist() == [0] * len(st), f"{what}: status {st.tolist()}"
        assert_exact(d, idx, od, oidx, what)


def _replay_case(dev, name, c, ds, ker, Q, OD, OIDX, workspace=True, **kw):
    from shadowing_amd import _native
    if workspace:
        kw["workspace"] = _native.Workspace(dev)
    s = Scan(dev, c, ds, ker, Q[0].shape[0], Q[0].shape[1], **kw)
    s.set(Q[0], OD[0])
    s.call()
    s.check(OD[0], OIDX[0], f"{name}: the eager call")
    s.info.clear()
    g, _ = capture(s.call)
    assert s.info["path"] == EXPECTED[name][0], (name, s.info)
    for j in range(3):
        s.set(Q[j], OD[j])
        s.smudge()
        replay(g, dev)
        s.check(OD[j], OIDX[j], f"{name}: replay {j}")
    return s, g


# ---------------------------------------------------------------------------------------------------------- A. scans
@pytest.mark.parametrize("name", list(ONE_QUERY))
def test_a_captured_one_query_scan_follows_its_query_buffer(hip_device, name):
    c, ds, ker, Q, OD, OIDX = _three_queries(name)
    kw = dict(filter_copy=None) if name == "overlap" else {}
    _replay_case(hip_device, name, c, ds, ker, Q, OD, OIDX, **kw)


@pytest.mark.parametrize("name", BATCHED)
def test_a_captured_batched_scan_follows_its_query_buffer(hip_device, name):
    c, ds, ker, Q, OD, OIDX = _rolled(name)
    _replay_case(hip_device, name, c, ds, ker, Q, OD, OIDX)


def test_a_workspace_made_inside_the_capture(hip_device):
    """scan_topk without a `workspace`: the allocation (from the graph's pool) and psh_workspace_init are part of the graph,
    so every replay arms the header again before the fused launch reads it."""
    c, ds, ker, Q, OD, OIDX = _three_queries("default")
    _replay_case(hip_device, "default", c, ds, ker, Q, OD, OIDX, workspace=False)


def test_two_graphs_share_one_workspace(hip_device):
    """The fused launch and the overlap launches captured on ONE Workspace and replayed alternately on one stream: the epoch
    the fused launch advances lives in the header, not in either graph."""
    from shadowing_amd import _native
    dev = hip_device
    c1, ds, _, Q, OD, OIDX = _three_queries("default")
    c2 = _case("overlap")
    ws = _native.Workspace(dev)
    s1 = Scan(dev, c1, ds, None, 1, Q[0].shape[1], workspace=ws)
    s2 = Scan(dev, c2, ds, None, 1, Q[0].shape[1], ds_t=s1.ds, q_t=s1.q, workspace=ws, filter_copy=None)
    graphs = []
    for s, name in ((s1, "default"), (s2, "overlap")):
        s.set(Q[0], OD[0])
        s.call()
        s.check(OD[0], OIDX[0], f"{name}: the eager call")
        g, _ = capture(s.call)
        assert s.info["path"] == EXPECTED[name][0]
        graphs.append(g)
    for turn, j in enumerate((0, 1, 2, 0)):
        s, g = (s1, graphs[0]) if turn % 2 == 0 else (s2, graphs[1])
        s.set(Q[j], OD[j])
        s.smudge()
        replay(g, dev)
        s.check(OD[j], OIDX[j], f"turn {turn}")


def test_retry_inside_a_replay_and_the_replay_after_it(hip_device):
    """Constant rows (every window ties: the block lists overflow, the by-design give-up of tests/test_gpu_fused.py and
    tests/test_gpu_overlap.py) in the static ensemble buffer: every replay says RETRY and leaves NaN distances and (-1, -1)
    indices, not the numbers that were there.  The ordinary ensemble copied into the same buffer: the next replay is OK and
    exact -- this give-up leaves the header armed and only advances the epoch, nothing is re-armed from the host."""
    from shadowing_amd import _native
    dev = hip_device
    c1, ds, _, Q, OD, OIDX = _three_queries("default")
    flat = np.full_like(ds[:, 0, :], 0.01)
    s1 = Scan(dev, c1, flat, None, 1, Q[0].shape[1], workspace=_native.Workspace(dev))
    s2 = Scan(dev, _case("overlap"), flat, None, 1, Q[0].shape[1], ds_t=s1.ds, q_t=s1.q, workspace=_native.Workspace(dev),
              filter_copy=None)
    cases = []
    for s, name in ((s1, "default"), (s2, "overlap")):
        s.set(Q[0], OD[0])
        s.call()
        torch.cuda.synchronize(dev)
        g, _ = capture(s.call)
        assert s.info["path"] == EXPECTED[name][0]
        cases.append((s, g, name))
    for s, g, name in cases:
        for j in range(3):
            s.set(Q[j], OD[j])
            s.smudge()
            replay(g, dev)
            d, idx, st = s.results()
            assert st.tolist() == [_native.PSH_STATUS_RETRY], (name, j, st.tolist())
            assert np.isnan(d).all() and (idx == -1).all(), (name, j)
    s1.ds.copy_(torch.as_tensor(np.ascontiguousarray(ds[:, 0, :])))
    for s, g, name in cases:
        s.set(Q[1], OD[1])
        s.smudge()
        replay(g, dev)
        s.check(OD[1], OIDX[1], f"{name}: the replay after the give-ups")


# ------------------------------------------------------------------------------------- B. the filter copy under capture
@pytest.fixture()
def first_policy(monkeypatch):
    """Policy "first", and a record of every copy the policy builds (tests/test_gpu_copy_scan_fragments.py's fixture)."""
    from shadowing_amd import _native
    made = []

    class Recording(_native.FilterCopy):
        def __init__(self, rows):
            super().__init__(rows)
            made.append(self)

    monkeypatch.setattr(_native, "FILTER_COPY_POLICY", "first")
    monkeypatch.setattr(_native, "_filter_copy_builder", Recording)
    monkeypatch.delenv("PSH_FILTER_COPY", raising=False)
    _native._filter_copies.clear()
    yield made
    _native._filter_copies.clear()


def test_the_auto_copy_steps_aside_in_a_capture(hip_device, oracle_mod, first_policy):
    """The "auto" copy's staleness guard is the tensor's version counter, read when scan_topk runs -- at capture time only.
    A graph that streamed that copy would reject, on every later replay, a row edited into a near-copy of the query (only
    survivors of the f16 test are audited): status OK, wrong top-k.  So the policy serves nothing to a capturing stream."""
    from shadowing_amd import _native
    dev = hip_device
    c, ds, _, Q, OD, OIDX = _three_queries("overlap")
    q, W, k = Q[0], c["W"], c["k"]
    s = Scan(dev, c, ds, None, 1, W, workspace=_native.Workspace(dev), filter_copy="auto")
    s.set(q, OD[0])
    s.call()
    s.check(OD[0], OIDX[0], "the eager call")
    assert (s.info["copy_served"], s.info["path"], len(first_policy)) == (1, 3, 1), s.info
    s.info.clear()
    g, _ = capture(s.call)
    info = dict(s.info)
    s.smudge()
    replay(g, dev)
    s.check(OD[0], OIDX[0], "replay on the unchanged ensemble")
    # a near-copy of the query written in place over a row the top-k did not hold
    r = min(set(range(c["R"])) - set(OIDX[0][0, :, 0].tolist()))
    t = 100
    plant = (q[0] * np.float32(1.0 + 2.0 ** -6)).astype(np.float32)
    s.ds[r, t:t + W] = torch.as_tensor(plant).to(dev)
    edited = np.ascontiguousarray(ds[:, 0, :]).copy()
    edited[r, t:t + W] = plant
    od2, oidx2 = oracle_mod.scan_topk(edited, q, k, h=c["h"])
    assert oidx2[0, 0].tolist() == [r, t], "the plant is not the oracle's best window"
    s.smudge()
    replay(g, dev)
    d, idx, st = s.results()
    assert st.tolist() == [0] and idx[0, 0].tolist() == [r, t], (st.tolist(), idx[0, 0].tolist())
    assert_exact(d, idx, od2, oidx2, "replay on the edited ensemble")
    assert (info["copy_served"], info["path"]) == (0, 3), info


def test_an_explicit_copy_is_served_in_a_capture(hip_device, first_policy):
    """A FilterCopy handed in is the caller's: built and seen complete (wait()) before the capture, it is streamed by every
    replay; use() asks nothing of the event while the stream captures."""
    from shadowing_amd import _native
    dev = hip_device
    c, ds, _, Q, OD, OIDX = _three_queries("overlap")
    rows = torch.as_tensor(np.ascontiguousarray(ds[:, 0, :])).to(dev)
    fc = _native.FilterCopy(rows)
    fc.wait()
    s, g = _replay_case(dev, "overlap", c, ds, None, Q, OD, OIDX, ds_t=rows, filter_copy=fc)
    assert (s.info["copy_served"], s.info["path"]) == (1, 3) and not first_policy, s.info


# --------------------------------------------------------------------------- C. the reductions and the pricing chain
def test_the_reductions_and_pricing_chain_in_one_graph(hip_device):
    """gather_paths -> realized_variance (on the strided out-context view) -> softmax_weights -> weighted_moments ->
    weighted_quantiles -> score_ensemble -> hedged_mc(policy) -> hedge_replay -> calibrate_weights as ONE linear graph on
    static buffers, B = 3 and k = 257 (one past a block and a wave edge); d, idx, obs and the quotes are refreshed between the
    replays.  Every output, status words included, has the bits of the same calls made eagerly on the same inputs."""
    from shadowing_amd import _native
    dev = hip_device
    B, k, W, h = 3, 257, 20, 20
    ds = _inputs(_case("B3"))[0]
    ds3 = torch.as_tensor(ds).to(dev)
    rows = ds3[:, 0, :].contiguous()
    TS_RV, ETAS, KS, LEVELS, TS, MS = [5, 10, 20], [0.5, None], [129, 257], [0.05, 0.5, 0.95], [5, 20], [-1.0, 0.0, 1.0]
    OTM = _native.PSH_HMC_OTM
    d = torch.zeros((B, k), dtype=torch.float32, device=dev)
    idx = torch.zeros((B, k, 2), dtype=torch.int32, device=dev)
    obs = torch.zeros((B, len(TS_RV)), dtype=torch.float32, device=dev)
    quotes = torch.zeros((B, len(TS), len(MS)), dtype=torch.float64, device=dev)

    def future():
        return _native.gather_paths(ds3, idx, W + h)[:, :, 0, W:]

    def chain():
        outs = {}
        paths = _native.gather_paths(ds3, idx, W + h)
        fut = paths[:, :, 0, W:]
        rv = _native.realized_variance(fut, TS_RV)
        assert rv is not None and not fut.is_contiguous()
        w = _native.softmax_weights(d, ETAS, KS)
        outs.update(paths=paths, rv=rv, w=w)
        outs["mean"], outs["std"] = _native.weighted_moments(rv, w[0])
        outs["q"], outs["q_lo"], outs["q_hi"], outs["q_status"] = _native.weighted_quantiles(rv, w[1], LEVELS)
        outs["crps"], outs["pit_lo"], outs["pit_hi"], outs["s_mean"], outs["s_status"] = _native.score_ensemble(rv, w, obs)
        fit = _native.hedged_mc(fut, w[3], TS, MS, 100.0, 0.01, 3, OTM, policy=True)
        rep = _native.hedge_replay(fut, w[1], TS, MS, fit["policy"], fit["strike"], fit["price"], 100.0, 0.01, 3, OTM,
                                   return_pnl=True)
        cal = _native.calibrate_weights(fut, w[3], TS, fit["strike"], quotes, 100.0, 0.01, OTM, True, 1e-6, 1e-8, 100)
        for tag, res in (("fit", fit), ("rep", rep), ("cal", cal)):
            outs.update({f"{tag}_{name}": t for name, t in res.items()})
        return outs

    inputs = []
    g = np.random.default_rng(9700)
    for j in range(3):
        qj = torch.as_tensor(syn.gbm_log_returns((B, W), 9710 + j)).to(dev)
        dj, ij = _native.scan_topk_checked(rows, qj, k, h=h)
        idx.copy_(ij)
        price = _native.hedged_mc(future(), None, TS, MS, 100.0, 0.01, 3, OTM)["price"]
        inputs.append((dj.clone(), ij.clone(), torch.as_tensor((1e-4 * g.standard_normal((B, len(TS_RV))) ** 2).astype(np.float32)).to(dev),
                       price * torch.as_tensor(1.0 + 0.02 * g.standard_normal((B, len(TS), len(MS)))).to(dev)))
    torch.cuda.synchronize(dev)

    def load(j):
        for buf, val in zip((d, idx, obs, quotes), inputs[j]):
            buf.copy_(val)

    want = []
    for j in range(3):
        load(j)
        want.append(snapshot(flatten(chain())))
    torch.cuda.synchronize(dev)
    status = {name: t.flatten().tolist() for name, t in want[0] if name.endswith("status")}
    assert not any(any(v) for name, v in status.items() if name != "cal_status"), f"the chain's inputs are meant to be ordinary ones: {status}"
    for name in ("paths", "w", "crps", "fit_price", "rep_sums", "cal_weights"):
        assert not torch.equal(dict(want[0])[name], dict(want[1])[name]), f"{name}: the refreshed inputs are meant to change it"
    load(0)
    graph, outs = capture(chain)
    for j in (1, 2, 0):
        load(j)
        replay(graph, dev)
        assert_same_bits(flatten(outs), want[j], f"replay with inputs {j}")


# ---------------------------------------------------------------------------------------- D. generators and spectra
def _generator_calls(dev):
    from shadowing_amd import _native, mrw, pdv
    R, n, m, lam = 5, 64, 7, 0.2
    a_om, _ = mrw._device_tables(n, 0.5, lam, float(n), dev)
    _, a_eps = mrw._device_tables(n, 0.7, lam, float(n), dev)
    c0 = float(mrw.mrw_covariance(0, float(n), lam))
    K = mrw.smrw_kernel(m, 0.1, 0.6)
    k_hat = torch.from_numpy(mrw._k_hat(K, mrw._embedding_size(n))).to(dev)
    model = pdv.PDVModelDiscrete(lams1=[60.0, 4.0], lams2=[40.0, 1.5], thetas=[0.6, 0.3], betas=[0.04, -0.12, 0.6, 0.5], nu=None)
    dec = lambda v: np.exp(-np.asarray(v)[None, :] / 252)[0]   # noqa: E731
    # (device tensors: a host array would be uploaded by the wrapper, a pageable copy no capture may hold)
    R10 = torch.tensor([[0.0, 0.01], [0.05, -0.02], [-0.03, 0.0]], dtype=torch.float64, device=dev)
    R20 = torch.tensor([[0.04, 0.03], [0.02, 0.05], [0.09, 0.01]], dtype=torch.float64, device=dev)
    return {
        "mrw_generate": lambda: _native.mrw_generate(R, n, mrw.DEFAULT_SIGMA, a_om, a_eps, c0, seed=4242, outputs=_native.MRW_OUTPUTS),
        "smrw_generate": lambda: _native.smrw_generate(R, n, m, mrw.DEFAULT_SIGMA, a_om, k_hat, c0, float(np.sum(K ** 2)), seed=4243,
                                                       outputs=_native.SMRW_OUTPUTS),
        "pdv_generate": lambda: _native.pdv_generate(3, 33, 21, model.lams1, model.lams2, dec(model.lams1), dec(model.lams2),
                                                     model.thetas, model.betas, 100.0, np.sqrt(1 / 252), model._draw_nu(), R10, R20,
                                                     seed=4244, outputs=_native.PDV_OUTPUTS, device=dev),
    }


@pytest.mark.parametrize("entry", ["mrw_generate", "smrw_generate", "pdv_generate"])
def test_a_captured_generator_repeats_its_draws(hip_device, entry):
    """The seed is an argument of the launch: a graph holds it, so every replay makes the eager call's paths again (the
    documented behaviour: a caller who wants fresh paths per step captures nothing here, or draws them and passes `draws`)."""
    call = _generator_calls(hip_device)[entry]
    want = snapshot(flatten(call()))
    torch.cuda.synchronize(hip_device)
    g, outs = capture(call)
    for turn in range(2):
        for _, t in flatten(outs):
            t.zero_()
        replay(g, hip_device)
        assert_same_bits(flatten(outs), want, f"{entry}: replay {turn}")


@pytest.mark.parametrize("entry", ["lagged_moments", "scattering_spectra", "scattering_vjp"])
def test_a_captured_measurement_follows_its_input_buffer(hip_device, entry):
    """The three measuring entries with their workspaces allocated inside the capture, `x` refreshed between the replays."""
    from shadowing_amd import _native, scattering
    dev = hip_device
    if entry == "lagged_moments":
        R, n, m, G = 9, 256, 8, 2
        x = torch.zeros((R, n), dtype=torch.float32, device=dev)
        call = lambda: _native.lagged_moments(x, m, G)   # noqa: E731
    else:
        n, J, R, G = 64, 4, 9, 4
        x = torch.zeros((R, n), dtype=torch.float32, device=dev)
        psi = scattering._device_bank(n, J, dev)
        if entry == "scattering_spectra":
            call = lambda: _native.scattering_spectra(x, J, G, psi)   # noqa: E731
        else:
            cot = torch.as_tensor(np.random.default_rng(9800).standard_normal((G, _native.scattering_nout(J)))).to(dev)
            call = lambda: _native.scattering_vjp(x, J, G, psi, cot)   # noqa: E731
    xs = [torch.as_tensor(syn.gbm_log_returns(tuple(x.shape), 9810 + j)).to(dev) for j in range(3)]
    want = []
    for j in range(3):
        x.copy_(xs[j])
        want.append(snapshot(flatten(call())))
    torch.cuda.synchronize(dev)
    assert not any(torch.equal(a, b) for (_, a), (_, b) in zip(want[0][:1], want[1][:1])), "the inputs are meant to differ"
    g, outs = capture(call)
    for j in (1, 2, 0):
        x.copy_(xs[j])
        replay(g, dev)
        assert_same_bits(flatten(outs), want[j], f"{entry}: replay with input {j}")


# -------------------------------------------------------------------------------------------------- E. epoch wrap
@pytest.mark.parametrize("start", [0x7fffffff, 0xffffffff])
def test_the_fused_launch_across_the_wrap_of_its_tags(hip_device, start):
    """The fused launch tags what its blocks exchange with 2 * epoch (the sample's flags) and 2 * epoch + 1 (the blocks' end
    records) in 32 bits: the tags wrap after 2^31 launches of one workspace (two and a half days at 100 us a step) and the
    epoch itself after 2^32; the second wrap meets tag 0, which is also what a zeroed header holds.

    Why a wrap is safe whatever a tag matches (psh_fused.hip, psh_capi.hip's try_fused_step):
      * nothing read from FusedHdr indexes memory unbounded.  The grid is <= PSH_FUSED_MAX_BLOCKS and the sample <=
        PSH_FUSED_MAX_UNITS (try_fused_step refuses the route otherwise); flags, end records and minima are read by lane /
        thread number through buffer resources sized to their arrays; a histogram bucket comes from (key - kmin) >> shift
        with kmin, kmax and shift derived from the very keys staged in LDS.  The one header VALUE used as an index is a
        block's candidate count: every word the kernel ever stores there is min(count, PSH_FUSED_FRONT), a zeroed word is 0,
        so the prefix sums stay <= grid * PSH_FUSED_FRONT = the size of `cand`; the sum must be <= 8192 before any candidate
        is loaded, and the loads go through a buffer resource of sizeof(cand) besides (out of range reads 0, never faults);
      * a poll that is not satisfied ends: both barriers leave their loop at spin_ticks (2 ms), set C_BAIL, disarm the header
        and report RETRY;
      * a tag that matches a STALE record cannot produce a wrong OK.  Every launch rewrites the records of all its blocks, so
        with one grid per workspace a stale tag is always the previous launch's, never the current one.  Where the grid has
        grown since a record was written (or the record was never written and the tag is 0), a block may pass the first
        barrier early and read minima of an older sample: it then admits with another level than its peers -- every block
        checks that all end records carry ITS tau2 bits and the call says RETRY -- or with the same level, and any common level
        under which >= k windows were found gives the exact top-k.  An end record (odd tag) never matches a zeroed word.
    So nothing is skipped at the wrap; the launches below run straight through it."""
    from shadowing_amd import _native
    dev = hip_device
    c, ds, _, Q, OD, OIDX = _three_queries("default")
    ws = _native.Workspace(dev)
    s = Scan(dev, c, ds, None, 1, Q[0].shape[1], workspace=ws)
    s.set(Q[0], OD[0])
    s.call()
    s.check(OD[0], OIDX[0], "the ordinary launch")
    assert s.info["path"] == 2
    epoch = ws.buf[8:12].view(torch.int32)
    assert int(epoch.item()) == 2, "bytes 8..11 of an armed workspace after one fused launch"
    epoch.fill_(start - (1 << 32) if start >= 1 << 31 else start)
    for i in range(4):
        j = (i + 1) % 3
        s.set(Q[j], OD[j])
        s.smudge()
        s.call()
        s.check(OD[j], OIDX[j], f"launch {i} from epoch {start:#x}")
    assert int(epoch.item()) & 0xffffffff == (start + 4) & 0xffffffff
