"""scan_topk's filter_copy="auto" policy (shadowing_amd/_native.py) with a fake builder: which call builds a copy, what makes
the policy start over, what drops an entry.  CPU tensors stand in for the ensemble: the policy looks at a tensor's identity,
pointer, shape, strides, device and version counter, never at its contents."""
import gc

import pytest
import torch

from shadowing_amd import _native


class Fake:
    def __init__(self, rows):
        self.shape = tuple(rows.shape)


@pytest.fixture()
def policy(monkeypatch):
    built = []

    def builder(rows):
        built.append(Fake(rows))
        return built[-1]

    state = {"capturing": False, "free": 1 << 40}
    monkeypatch.setattr(_native, "_filter_copy_builder", builder)
    monkeypatch.setattr(_native, "_filter_copy_capturing", lambda: state["capturing"])
    monkeypatch.setattr(_native, "_filter_copy_free_bytes", lambda device: state["free"])
    monkeypatch.setattr(_native, "filter_copy_bytes", lambda R, T: (64 + R * ((T + 1023) // 1024 * 1024 + 32) * 2, 0))
    monkeypatch.setattr(_native, "FILTER_COPY_POLICY", "second")
    monkeypatch.delenv("PSH_FILTER_COPY", raising=False)
    _native._filter_copies.clear()
    yield built, state
    _native._filter_copies.clear()


def auto(ds):
    return _native._filter_copy_auto(ds) if _native._filter_copy_enabled() else None


def test_the_copy_is_built_on_the_second_consecutive_call(policy):
    built, _ = policy
    ds = torch.zeros(64, 2048)
    assert auto(ds) is None and not built                 # a one-off call pays nothing
    c = auto(ds)
    assert c is built[0] and len(built) == 1
    assert auto(ds) is c and auto(ds) is c and len(built) == 1


def test_a_version_bump_starts_over(policy):
    built, _ = policy
    ds = torch.zeros(64, 2048)
    auto(ds); c = auto(ds)
    ds.add_(1.0)                                           # an in-place edit torch sees
    assert auto(ds) is None and len(built) == 1            # the stale copy is not handed out, the count starts again
    c2 = auto(ds)
    assert c2 is built[1] and c2 is not c


def test_views_of_one_base_share_the_entry_and_other_views_do_not(policy):
    built, _ = policy
    base = torch.zeros(64, 1, 2048)
    assert auto(base[:, 0, :]) is None
    c = auto(base[:, 0, :])                                # a new view object of the same rows each call (bench.py's ds[:, 0, :])
    assert c is built[0] and auto(base[:, 0, :]) is c
    assert auto(base[:32, 0, :]) is None                   # other rows of the same base: another key
    assert len(_native._filter_copies) == 1


def test_a_new_tensor_has_its_own_entry(policy):
    built, _ = policy
    a, b = torch.zeros(64, 2048), torch.zeros(64, 2048)
    auto(a); ca = auto(a)
    assert auto(b) is None
    cb = auto(b)
    assert ca is built[0] and cb is built[1] and auto(a) is ca


def test_the_entry_dies_with_the_tensor(policy):
    built, _ = policy
    ds = torch.zeros(64, 2048)
    auto(ds); auto(ds)
    assert len(_native._filter_copies) == 1
    del ds
    gc.collect()
    assert len(_native._filter_copies) == 0


def test_forget_drops_the_entry(policy):
    built, _ = policy
    base = torch.zeros(64, 1, 2048)
    auto(base[:, 0, :]); auto(base[:, 0, :])
    _native.filter_copy_forget(base[:, 0, :])              # (through a view: the entry is the base's)
    assert len(_native._filter_copies) == 0
    assert auto(base[:, 0, :]) is None and len(built) == 1


def test_policy_and_environment_switches(policy, monkeypatch):
    built, _ = policy
    ds = torch.zeros(64, 2048)
    monkeypatch.setattr(_native, "FILTER_COPY_POLICY", "off")
    assert auto(ds) is None and auto(ds) is None and auto(ds) is None and not built
    monkeypatch.setattr(_native, "FILTER_COPY_POLICY", "first")
    assert auto(ds) is built[0]
    monkeypatch.setenv("PSH_FILTER_COPY", "0")
    assert auto(ds) is None and auto(torch.zeros(8, 2048)) is None and len(built) == 1
    monkeypatch.delenv("PSH_FILTER_COPY")
    assert auto(ds) is built[0]


def test_the_copy_needs_its_bytes_and_a_gibibyte_free(policy):
    built, state = policy
    ds = torch.zeros(64, 2048)
    need = 64 + 64 * (2048 + 32) * 2
    state["free"] = need + (1 << 30) - 1
    assert auto(ds) is None and auto(ds) is None and auto(ds) is None and not built
    ds2 = torch.zeros(64, 2048)
    state["free"] = need + (1 << 30)
    auto(ds2)
    assert auto(ds2) is built[0]


def test_nothing_is_built_while_the_stream_captures(policy):
    built, state = policy
    ds = torch.zeros(64, 2048)
    state["capturing"] = True
    assert auto(ds) is None and auto(ds) is None and auto(ds) is None and not built
    state["capturing"] = False
    assert auto(ds) is built[0]                            # the calls were counted: the first one outside a capture builds


def test_nothing_is_served_while_the_stream_captures(policy):
    """A graph is replayed after the capture-time look at the version counter: an entry that exists is not handed to a
    capturing stream, and is there again once the capture is over (nothing was dropped, nothing rebuilt)."""
    built, state = policy
    ds = torch.zeros(64, 2048)
    auto(ds)
    c = auto(ds)
    assert c is built[0]
    state["capturing"] = True
    assert auto(ds) is None and auto(ds) is None and len(built) == 1
    state["capturing"] = False
    assert auto(ds) is c and len(built) == 1


class FakeEvent:
    def __init__(self, done):
        self.done, self.calls = done, []

    def query(self):
        self.calls.append("query")
        return self.done

    def synchronize(self):
        self.calls.append("synchronize")
        self.done = True


class FakeBuf:
    def __init__(self):
        self.recorded = []

    def record_stream(self, stream):
        self.recorded.append(stream.cuda_stream)


class FakeStream:
    def __init__(self, ptr):
        self.cuda_stream, self.waits = ptr, []

    def wait_event(self, ev):
        self.waits.append(ev)


def _copy(done, builder=1):
    """A FilterCopy as its constructor leaves it, without a device: built on stream `builder`, event complete or not."""
    c = object.__new__(_native.FilterCopy)
    c.event, c.buf, c._builder, c._streams, c._built = FakeEvent(done), FakeBuf(), builder, {builder}, False
    return c


def test_use_makes_no_event_or_allocator_call_while_the_stream_captures(policy):
    _, state = policy
    # outside a capture: a new stream is made known to the allocator and asks the event (complete: remembered; not: waits)
    c, s2 = _copy(True), FakeStream(2)
    c.use(s2)
    assert c.event.calls == ["query"] and c.buf.recorded == [2] and c._built and not s2.waits
    c, s2 = _copy(False), FakeStream(2)
    c.use(s2)
    assert c.event.calls == ["query"] and s2.waits == [c.event] and not c._built
    # capturing, the build not seen complete: a Python error before any call, and nothing has changed
    state["capturing"] = True
    c, s3 = _copy(True), FakeStream(3)
    with pytest.raises(_native.NativeLibraryError, match=r"wait\(\)"):
        c.use(s3)
    assert c.event.calls == [] and c.buf.recorded == [] and not s3.waits and c._streams == {1}
    # ... seen complete (wait(), outside the capture): used as it is, on any stream, without a call
    state["capturing"] = False
    c.wait()
    assert c.event.calls == ["synchronize"] and c._built
    state["capturing"] = True
    c.use(s3)
    c.use(FakeStream(1))
    assert c.event.calls == ["synchronize"] and c.buf.recorded == [] and not s3.waits
    # ... and a capture on the builder's own stream is in stream order behind the build
    c = _copy(False)
    c.use(FakeStream(1))
    assert c.event.calls == [] and c.buf.recorded == []
    # after the capture the new stream registers as ever
    state["capturing"] = False
    c, s3 = _copy(True), FakeStream(3)
    c.wait()
    c.use(s3)
    assert c.buf.recorded == [3] and c.event.calls == ["synchronize"]
