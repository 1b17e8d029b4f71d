"""ctypes binding of libpsh_hip.so (include/psh.h) on PyTorch-ROCm tensors.

PyTorch is plumbing here: device memory, streams, the caching allocator.  All
compute goes through the C ABI.  There is NO CPU fallback in this module: if the
library cannot be loaded, or a tensor is not on a HIP device, calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
from pathlib import Path

import torch

from . import _build

PSH_OK = 0
PSH_VERSION = 3          # include/psh.h: 2: psh_profile.tau_hint, psh_candidates_layout; 3: psh_shadow_blocking
PSH_STATUS_OK, PSH_STATUS_OVERFLOW, PSH_STATUS_RETRY = 0, 1, 2
PSH_MAX_W, PSH_MAX_K, PSH_MAX_B_PER_LAUNCH = 256, 16384, 1024
# psh_hedged_mc (include/psh.h)
PSH_HMC_OTM, PSH_HMC_CALL, PSH_HMC_PUT = 0, 1, 2
PSH_HMC_STATUS_OK, PSH_HMC_STATUS_NONFINITE, PSH_HMC_STATUS_WEIGHTS, PSH_HMC_STATUS_ILL_CONDITIONED = 0, 1, 2, 4
PSH_HMC_MAX_T = PSH_HMC_MAX_M = 64
# psh_profile.flags (include/psh.h)
FLAG_UNSORTED, FLAG_FILTER_VALU, FLAG_EMBED_DENSE, FLAG_ROWS_GENERIC, FLAG_NO_FUSE, FLAG_RESERVE_CUS, FLAG_EMBED_MX, FLAG_EMBED_TAPS, FLAG_EMBED_PLAN_KEEP, FLAG_EMBED_MX_SPLIT, FLAG_SELECT_ONE_BLOCK, FLAG_OVERLAP, FLAG_MQ_F16, FLAG_LONG_LOOP = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192


# psh_filter_copy.reason (include/psh.h)
PSH_COPY_SERVED, PSH_COPY_NOT_ROUTE, PSH_COPY_MISMATCH = 0, 1, 2
PSH_FILTER_COPY_SCRATCH_BYTES = 16384


class NativeLibraryError(RuntimeError):
    """The HIP extension is missing or failed."""


class PshProfile(C.Structure):
    _fields_ = [("mode", C.c_int), ("flags", C.c_int), ("ev_scan_begin", C.c_void_p), ("ev_scan_end", C.c_void_p),
                ("prep_ms", C.c_float), ("sample_ms", C.c_float), ("threshold_ms", C.c_float),
                ("scan_ms", C.c_float), ("select_ms", C.c_float), ("total_ms", C.c_float),
                ("path", C.c_int), ("n_sample_rows", C.c_int), ("grid_blocks", C.c_int),
                ("n_candidates", C.c_int), ("tau_hint", C.c_void_p)]

    def as_dict(self) -> dict:
        skip = ("mode", "flags", "ev_scan_begin", "ev_scan_end", "tau_hint")
        return {name: getattr(self, name) for name, _ in self._fields_ if name not in skip}


class PshFilterCopy(C.Structure):
    _fields_ = [("copy", C.c_void_p), ("pitch_halves", C.c_int64), ("R", C.c_int64), ("T", C.c_int64),
                ("served", C.c_int), ("reason", C.c_int)]


def _signatures() -> dict:
    """The argument types of every entry point include/psh.h declares, by name (tests/test_capi_abi_cpu.py holds the
    table against the header's prototypes)."""
    vp, i64, i32, f64, u64, sz, P = C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_uint64, C.c_size_t, C.POINTER
    scan_args = [i32, vp, vp, i64, i64, i64, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, sz, P(PshProfile)]
    emb_args = [i32, vp, vp, i64, i64, i64, vp, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, sz, P(PshProfile)]
    hmc_args = [i32, vp, vp, i64, i32, i32, i32, vp, f64, f64, P(i32), i32, P(f64), i32, i32, i32]
    hedged_mc = hmc_args + [vp, vp, vp, vp, vp]
    return {
        "psh_version": [],
        "psh_strerror": [i32],
        "psh_last_hip_error": [],
        "psh_workspace_bytes": [i64, i64, i32, i32, i32, i32, P(sz)],
        "psh_workspace_init": [i32, vp, vp, sz],
        "psh_query_norm": [i32, vp, vp, i32, i32, vp],
        "psh_scan_topk": scan_args,
        "psh_scan_topk_exhaustive": scan_args,
        "psh_scan_topk_copy": scan_args + [P(PshFilterCopy)],
        "psh_filter_copy_bytes": [i64, i64, P(sz), P(i64)],
        "psh_filter_copy_build": [i32, vp, vp, i64, i64, vp, sz, vp, sz],
        "psh_scan_topk_embedded": emb_args,
        "psh_scan_topk_embedded_exhaustive": emb_args,
        "psh_embedded_supported": [i32, i32],
        "psh_embed_plan_offset": [],
        "psh_embed_rows": [i32, vp, vp, i64, i64, vp, i32, i32, vp],
        "psh_candidates_layout": [i64, i64, i32, i32, i32, i32, sz, P(i64)],
        "psh_merge_workspace_bytes": [i32, i32, P(sz)],
        "psh_merge_topk": [i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, sz],
        "psh_merge_topk_gathered": [i32, vp, vp, vp, i32, i64, i64, i32, i32, i32, vp, vp, vp, sz],
        "psh_merge_sorted_gathered": [i32, vp, vp, vp, i32, i64, i64, i32, i32, i32, vp, vp],
        "psh_gather_paths": [i32, vp, vp, i64, i64, i64, i64, vp, i64, i32, vp],
        "psh_last_comm_error": [],
        "psh_comm_unique_id": [C.c_char_p, vp],
        "psh_comm_create": [C.c_char_p, i32, i32, i32, vp, P(vp)],
        "psh_comm_destroy": [vp],
        "psh_comm_world": [vp],
        "psh_exchange_merge": [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, sz, vp, vp],
        "psh_stream_create_reserving": [i32, i32, P(vp), P(i32)],
        "psh_stream_destroy": [i32, vp],
        "psh_shadow_block_layout": [i32, i32, i32, i64, P(sz)],
        "psh_shadow_blocking": [i32, vp, vp, i64, i64, i64, vp, i64, i32, i32, i32, vp, sz, i32, vp, sz, P(PshProfile)],
        "psh_count_nonfinite": [i32, vp, vp, i64, vp],
        "psh_rows_nonfinite": [i32, vp, vp, i64, i64, i64, vp],
        "psh_smear_nonfinite": [i32, vp, vp, i64, i64, i64, i32, i32, vp],
        "psh_weighted_moments": [i32, vp, vp, vp, i32, i32, i32, vp, vp],
        "psh_weighted_quantiles": [i32, vp, vp, vp, i32, i32, i32, P(f64), i32, vp, vp, vp, vp],
        "psh_score_ensemble": [i32, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp],
        "psh_softmax_weights": [i32, vp, vp, i32, i32, P(f64), i32, P(i32), i32, vp],
        "psh_separate_topk": [i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp],
        "psh_realized_variance": [i32, vp, vp, i64, i64, i32, P(i32), i32, i32, vp],
        "psh_calibrate_workspace_bytes": [i32, i32, i32, P(sz)],
        "psh_calibrate_weights": [i32, vp, vp, i64, i32, i32, i32, vp, f64, f64, P(i32), i32, vp, vp, i32, i32, i32, f64, f64, i32,
                                  vp, vp, vp, vp, vp, vp, sz],
        "psh_hedged_mc": hedged_mc,
        "psh_hedged_mc_policy": hedged_mc + [vp],
        "psh_hmc_policy_doubles": [i32, i32, i32, i32, i32, P(sz)],
        "psh_hedge_replay_workspace_bytes": [i32, i32, i32, i32, P(sz)],
        "psh_hedge_replay": hmc_args + [vp, vp, vp, vp, vp, vp, vp, sz],
        "psh_pdv_generate": [i32, vp, i32, i64, i32] + [P(f64)] * 6 + [i32, f64, f64, f64, vp, vp, vp, u64, vp, vp, vp, vp, vp],
        "psh_mrw_generate": [i32, vp, i64, i32, f64, vp, vp, f64, u64, vp, i64, vp, vp],
        "psh_smrw_generate": [i32, vp, i64, i32, i32, f64, vp, vp, f64, f64, u64, vp, i64, vp, vp],
        "psh_lagged_moments_workspace_bytes": [i64, i32, i64, P(sz)],
        "psh_lagged_moments": [i32, vp, vp, i64, i64, i32, i32, i64, vp, vp, vp, vp, sz],
        "psh_scattering_spectra_workspace_bytes": [i64, i32, i64, P(sz)],
        "psh_scattering_spectra": [i32, vp, vp, i64, i64, i32, i32, vp, i64, vp, vp, vp, vp, sz],
        "psh_scattering_vjp_workspace_bytes": [i64, i32, i32, i64, P(sz)],
        "psh_scattering_vjp": [i32, vp, vp, i64, i64, i32, i32, vp, i64, vp, vp, i64, vp, vp, sz],
    }


SIGNATURES = _signatures()
# every entry point returns int (a PSH_* code), but:
RESTYPES = {"psh_strerror": C.c_char_p, "psh_last_hip_error": C.c_char_p, "psh_last_comm_error": C.c_char_p,
            "psh_embed_plan_offset": C.c_size_t}
EXPORTS = tuple(SIGNATURES)

_lib = None


def library_path() -> Path:
    import os
    override = os.environ.get("PSH_LIB")          # tuning aid: load an experimental build
    return Path(override) if override else _build.LIB


def load() -> C.CDLL:
    """dlopen the in-tree library (never builds implicitly on a GPU box: the built
    .so travels with the tree; __graft_entry__.build() / `python -m shadowing_amd._build`
    produce it)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.exists():
        raise NativeLibraryError(
            f"{path} is missing: build it with `python -m shadowing_amd._build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for cuda=True.")
    if path == _build.LIB and _build.is_stale():
        raise NativeLibraryError(
            f"{path} was built from other sources than the ones in shadowing_amd/csrc (content hash differs): "
            "rebuild it with `python -m shadowing_amd._build`")
    try:
        L = C.CDLL(str(path))
    except OSError as e:  # pragma: no cover
        raise NativeLibraryError(f"cannot load {path}: {e}") from e
    for name, argtypes in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = RESTYPES.get(name, C.c_int), argtypes
    if L.psh_version() != PSH_VERSION:
        raise NativeLibraryError(f"{path} speaks version {L.psh_version()} of the C ABI, this binding version {PSH_VERSION} "
                                 "(psh_profile differs): rebuild it with `python -m shadowing_amd._build`")
    _lib = L
    return L


def _check(rc: int, what: str):
    if rc == PSH_OK:
        return
    L = load()
    msg = L.psh_strerror(rc).decode()
    if rc == -4:
        msg += ": " + L.psh_last_hip_error().decode()
    if rc == -5:
        msg += ": " + L.psh_last_comm_error().decode()
    if rc == -1:
        raise ValueError(f"{what}: {msg}")
    raise NativeLibraryError(f"{what}: {msg} (code {rc})")


def _dev_tensor(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NativeLibraryError(f"{name} must be a tensor on a HIP device (got {type(t).__name__} "
                                 f"on {getattr(t, 'device', '?')}); there is no CPU path here")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t: torch.Tensor | None):
    return None if t is None else t.data_ptr()


def _workspace_bytes(bytes_fn, *sizes) -> int:
    out = C.c_size_t(0)
    _check(bytes_fn(*sizes, C.byref(out)), bytes_fn.__name__)
    return out.value


def _workspace(bytes_fn, *sizes, device) -> torch.Tensor:
    """The workspace an entry point asks for through its *_workspace_bytes companion, as int64 words on `device`."""
    return torch.empty((max(_workspace_bytes(bytes_fn, *sizes), 8) + 7) // 8, dtype=torch.int64, device=device)


def workspace_bytes(R: int, T: int, B: int, W: int, h: int, k: int) -> int:
    return _workspace_bytes(load().psh_workspace_bytes, R, T, B, W, h, k)


class Workspace:
    """Caller-owned scratch of the scan (a torch uint8 tensor), grown on demand.  A fresh buffer is armed for the
    fused single-launch scan (psh_workspace_init, enqueued on the current stream).  The header at its start keeps an
    epoch from launch to launch: one Workspace serves one stream at a time."""

    def __init__(self, device: torch.device):
        self.device = device
        self.buf = None
        self.plan_of = None        # (kernel tensor, its version, B): whose plan the last embedded call left in `buf`

    def get(self, nbytes: int) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.plan_of = None
            self.arm()
        return self.buf

    def arm(self) -> None:
        """(Re-)initialise the fused scan's header: after allocation, and after a PSH_STATUS_RETRY (a time-out inside
        the fused launch disarms the header on the device)."""
        if self.buf is not None:
            _check(load().psh_workspace_init(self.device.index, _stream_ptr(self.device), self.buf.data_ptr(),
                                             self.buf.numel()), "psh_workspace_init")


def query_norm(queries: torch.Tensor) -> torch.Tensor:
    q = _dev_tensor(queries, torch.float32, "queries")
    B, W = q.shape
    out = torch.empty(B, dtype=torch.float32, device=q.device)
    _check(load().psh_query_norm(q.device.index, _stream_ptr(q.device), q.data_ptr(), B, W, out.data_ptr()),
           "psh_query_norm")
    return out


def filter_copy_bytes(R: int, T: int) -> tuple[int, int]:
    """(bytes, pitch_halves) of the resident f16 filter copy of an (R, T) ensemble (psh_filter_copy_bytes: host arithmetic)."""
    nbytes, pitch = C.c_size_t(0), C.c_int64(0)
    _check(load().psh_filter_copy_bytes(R, T, C.byref(nbytes), C.byref(pitch)), "psh_filter_copy_bytes")
    return int(nbytes.value), int(pitch.value)


class FilterCopy:
    """A resident f16 copy of an (R, T) float32 ensemble for the one-query overlap scan (psh_filter_copy_build, include/psh.h):
    R * T * 2 bytes of device memory more, half the bytes of every such scan.  Owns the buffer and the completion event of its
    build; a stream other than the builder's waits on that event until it has completed, and every stream is made known to
    the caching allocator on first use (record_stream).  The copy knows nothing of later edits of the ensemble: whoever keeps
    it decides when it is stale (the "auto" policy of scan_topk watches the tensor's version counter)."""

    def __init__(self, rows: torch.Tensor):
        rows = _dev_tensor(rows, torch.float32, "rows")
        if rows.dim() != 2:
            raise ValueError("rows must be (R, T)")
        R, T = rows.shape
        dev = rows.device
        nbytes, pitch = filter_copy_bytes(R, T)
        self.R, self.T, self.pitch_halves, self.nbytes, self.device = R, T, pitch, nbytes, dev
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        scratch = torch.empty(PSH_FILTER_COPY_SCRATCH_BYTES, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _check(load().psh_filter_copy_build(dev.index, stream.cuda_stream, rows.data_ptr(), R, T, self.buf.data_ptr(), nbytes,
                                            scratch.data_ptr(), scratch.numel()), "psh_filter_copy_build")
        self.event = torch.cuda.Event()
        self.event.record(stream)
        self._builder = stream.cuda_stream
        self._streams = {self._builder}
        self._built = False                  # the event has been seen complete: nobody waits any more
        self.desc = PshFilterCopy(self.buf.data_ptr(), pitch, R, T, 0, 0)

    def wait(self) -> None:
        """Block the host until the build has completed and remember that it has: from then on use() issues no event call on
        any stream.  Call it (outside a capture) before a scan that reads the copy is captured into a graph."""
        if not self._built:
            self.event.synchronize()
            self._built = True

    def use(self, stream: "torch.cuda.Stream") -> None:
        """Call before enqueueing a scan that reads the copy on `stream`.  While `stream` captures a graph nothing is asked
        of the event or the allocator (an event query is illegal then, and the graph is replayed on other streams anyway): a
        copy seen complete -- wait() -- or captured on its builder's stream is used as it is, any other raises here, before
        anything reaches HIP.  Whoever replays the graph keeps the copy alive and current as long as the graph."""
        sp = stream.cuda_stream
        if sp in self._streams and (self._built or sp == self._builder):
            return
        if _filter_copy_capturing():
            if not self._built and sp != self._builder:
                raise NativeLibraryError("a FilterCopy whose build has not been seen complete cannot be used while the stream "
                                         "captures a graph: call its wait() before the capture begins")
            return
        if sp not in self._streams:
            self.buf.record_stream(stream)
            self._streams.add(sp)
        if not self._built and sp != self._builder:
            if self.event.query():
                self._built = True
            else:
                stream.wait_event(self.event)


# ---- scan_topk(filter_copy="auto"): one entry per ensemble, kept as long as the tensor lives
FILTER_COPY_POLICY = "second"      # "off" | "second" (build on the second consecutive eligible call) | "first"
_FILTER_COPY_HEADROOM = 1 << 30    # device memory that must stay free beside a new copy
_filter_copies: dict = {}          # id(base tensor) -> entry
_filter_copy_builder = FilterCopy  # (tests put fakes here and in the two probes below)
_filter_copy_capturing = lambda: torch.cuda.is_current_stream_capturing()         # noqa: E731
_filter_copy_free_bytes = lambda device: torch.cuda.mem_get_info(device)[0]       # noqa: E731


def _filter_copy_enabled() -> bool:
    import os
    return FILTER_COPY_POLICY in ("second", "first") and os.environ.get("PSH_FILTER_COPY", "1") != "0"


def _filter_copy_key(ds: torch.Tensor):
    base = ds._base if ds._base is not None else ds
    return base, (ds.data_ptr(), tuple(ds.shape), tuple(ds.stride()), str(ds.device), ds._version)


def filter_copy_forget(tensor: torch.Tensor) -> None:
    """Drop the "auto" copy of `tensor`'s ensemble: after an edit torch cannot see (.data, DLPack, raw pointers)."""
    base = tensor._base if tensor._base is not None else tensor
    _filter_copies.pop(id(base), None)


def _filter_copy_auto(ds: torch.Tensor):
    """The "auto" policy: the FilterCopy that serves this call, or None.  One entry per base tensor (it dies with the
    tensor); a call whose key -- data pointer, shape, strides, device, version counter -- differs from the entry's starts over.
    The copy is built on the second consecutive eligible call with one key ("second"; "first": at once), if the device has
    room for it and 1 GiB more, and never while the stream is capturing.  Nor is an existing copy SERVED to a capturing stream:
    the version counter is read now, the graph is replayed later, on an ensemble its owner may have refreshed in place since."""
    import weakref
    base, key = _filter_copy_key(ds)
    ent = _filter_copies.get(id(base))
    if ent is not None and ent["ref"]() is base and ent["key"] == key:
        if ent["copy"] is not None:
            return None if _filter_copy_capturing() else ent["copy"]
        ent["calls"] += 1
    else:
        bid = id(base)
        ent = {"key": key, "calls": 1, "copy": None, "denied": False,
               "ref": weakref.ref(base, lambda _r, bid=bid: _filter_copies.pop(bid, None))}
        _filter_copies[bid] = ent
    if ent["denied"] or ent["calls"] < (1 if FILTER_COPY_POLICY == "first" else 2):
        return None
    if _filter_copy_capturing():
        return None
    nbytes, _ = filter_copy_bytes(ds.shape[0], ds.shape[1])
    if _filter_copy_free_bytes(ds.device) < nbytes + _FILTER_COPY_HEADROOM:
        ent["denied"] = True               # (asked once per key: mem_get_info is a driver call)
        return None
    ent["copy"] = _filter_copy_builder(ds)
    return ent["copy"]


def _per_launch(B: int, out, call):
    """(d, idx, status) of `call(queries' slice, that slice of out)` over PSH_MAX_B_PER_LAUNCH queries at a time, concatenated: one
    launch keeps a per-block append cursor per query in LDS."""
    cuts = [slice(i, i + PSH_MAX_B_PER_LAUNCH) for i in range(0, B, PSH_MAX_B_PER_LAUNCH)]
    parts = [call(c, None if out is None else tuple(o[c] for o in out)) for c in cuts]
    return tuple(torch.cat([p[j] for p in parts], dim=0) for j in range(3))


def _cut(t, c):
    return None if t is None else t[c].contiguous()


def _scan_outputs(out, B: int, k: int, dev):
    """(d (B,k) f32, idx (B,k,2) i32, status (B,) i32) of a scan: the caller's contiguous device tensors (e.g. views of a send
    buffer; the status words optionally, as out[2] -- no allocation at all in the call then) or fresh ones."""
    status = None
    if out is not None:
        out_d = _dev_tensor(out[0], torch.float32, "out[0]")
        out_idx = _dev_tensor(out[1], torch.int32, "out[1]")
        if tuple(out_d.shape) != (B, k) or tuple(out_idx.shape) != (B, k, 2):
            raise ValueError("out must be ((B,k) float32, (B,k,2) int32)")
        if len(out) > 2:
            status = _dev_tensor(out[2], torch.int32, "out[2]")
            if tuple(status.shape) != (B,):
                raise ValueError("out[2] must be (B,) int32")
    else:
        out_d = torch.empty((B, k), dtype=torch.float32, device=dev)
        out_idx = torch.empty((B, k, 2), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty((B,), dtype=torch.int32, device=dev)
    return out_d, out_idx, status


def _scan_profile(B: int, profile: bool, scan_events, flags: int, info, tau_hint):
    """The PshProfile a scan hands to the library (None: nothing to say): stage timings (`profile`), the two events around the
    scan kernel, PSH_FLAG_* bits, the launch plan's facts for `info`, the caller's admission levels."""
    prof = None
    if profile:
        prof = PshProfile()
        prof.mode = 0
    elif scan_events is not None:
        prof = PshProfile()
        prof.mode = 1
        prof.ev_scan_begin = scan_events[0].cuda_event
        prof.ev_scan_end = scan_events[1].cuda_event
    if tau_hint is not None:
        tau_hint = _dev_tensor(tau_hint, torch.float32, "tau_hint")
        if tuple(tau_hint.shape) != (B,):
            raise ValueError("tau_hint must be (B,) float32")
    if flags or info is not None or tau_hint is not None:
        if prof is None:
            prof = PshProfile()
            prof.mode = 1                 # no events given: nothing is recorded, nothing is synchronised
        prof.flags = flags
        prof.tau_hint = None if tau_hint is None else tau_hint.data_ptr()
    return prof


def scan_topk(dataset: torch.Tensor, queries: torch.Tensor, k: int, h: int = 0, r_offset: int = 0,
              qnorm: torch.Tensor | None = None, workspace: Workspace | None = None,
              exhaustive: bool = False, profile: bool = False, extra_workspace_factor: float = 1.0,
              scan_events: tuple | None = None, out: tuple | None = None, unsorted: bool = False, flags: int = 0,
              info: dict | None = None, tau_hint: torch.Tensor | None = None, filter_copy="auto"):
    """Enqueue the scan on the current stream.

    dataset (R, T) float32 device, queries (B, W) float32 device.  Returns
    (d (B,k) f32, idx (B,k,2) i32, status (B,) i32[, profile dict]) -- device tensors,
    NOT synchronised; status must be inspected (after a sync) unless exhaustive=True.
    `profile=True` synchronises and adds the per-stage HIP-event timings;
    `scan_events=(begin, end)` (two torch.cuda.Event(enable_timing=True), each recorded
    once beforehand so that the handle exists) are re-recorded on the current stream
    right around the dominant scan kernel, without any synchronisation.
    `unsorted=True`: the k best come back in arbitrary order (PSH_FLAG_UNSORTED; for callers that
    merge afterwards).  `flags`: further PSH_FLAG_* bits (A/B switches of tests and tools).
    `info`: a dict that receives the launch plan's facts (path: 0 separate launches, 1 exhaustive, 2 fused, 3 the
    overlap-friendly launches; ...) without any synchronisation.
    `tau_hint`: (B,) float32 device tensor, the caller's admission levels on acc = (d ||x||)^2 (psh_profile.tau_hint): no
    bootstrap sample; a status other than OK then means "rerun without the hint".
    `filter_copy`: a FilterCopy of `dataset`, None, or "auto" (default) -- the one-query overlap scan (B = 1, W <= 33,
    FLAG_OVERLAP) streams a resident f16 copy of the ensemble, built on the second consecutive such call on the same
    unchanged tensor (FILTER_COPY_POLICY, PSH_FILTER_COPY=0, filter_copy_forget).  Results do not depend on it;
    `info` receives `copy_served` / `copy_reason`.  While the stream captures a graph "auto" neither builds nor serves a copy
    (a replay may meet an ensemble edited since); a FilterCopy passed in is served, its staleness being the caller's business.
    """
    ds = _dev_tensor(dataset, torch.float32, "dataset")
    q = _dev_tensor(queries, torch.float32, "queries")
    if ds.dim() != 2 or q.dim() != 2:
        raise ValueError("dataset must be (R, T) and queries (B, W)")
    if q.device != ds.device:
        raise ValueError("dataset and queries must live on the same device")
    R, T = ds.shape
    B, W = q.shape
    dev = ds.device
    if qnorm is not None:
        qnorm = _dev_tensor(qnorm, torch.float32, "qnorm")
    if B > PSH_MAX_B_PER_LAUNCH and not profile and scan_events is None:
        return _per_launch(B, out, lambda c, o: scan_topk(
            ds, q[c].contiguous(), k, h=h, r_offset=r_offset, qnorm=_cut(qnorm, c), workspace=workspace, exhaustive=exhaustive,
            extra_workspace_factor=extra_workspace_factor, out=o, unsorted=unsorted, flags=flags, tau_hint=_cut(tau_hint, c)))
    nbytes = int(workspace_bytes(R, T, B, W, h, k) * extra_workspace_factor)
    ws = (workspace or Workspace(dev)).get(nbytes)
    out_d, out_idx, status = _scan_outputs(out, B, k, dev)
    if unsorted and not exhaustive:
        flags |= FLAG_UNSORTED
    prof = _scan_profile(B, profile, scan_events, flags, info, tau_hint)
    # the resident f16 copy serves one route only: everything else does not even look for one
    fc = None
    if filter_copy is not None and B == 1 and W <= 33 and (flags & FLAG_OVERLAP) and not (flags & (FLAG_FILTER_VALU | FLAG_NO_FUSE)) \
            and not exhaustive and not profile and r_offset == 0:
        if isinstance(filter_copy, FilterCopy):
            fc = filter_copy
        elif filter_copy == "auto":
            fc = _filter_copy_auto(ds) if _filter_copy_enabled() else None
        else:
            raise ValueError('filter_copy must be "auto", None or a FilterCopy')
    args = (dev.index, _stream_ptr(dev), ds.data_ptr(), R, T, r_offset, q.data_ptr(),
            None if qnorm is None else qnorm.data_ptr(), B, W, h, k,
            out_d.data_ptr(), out_idx.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
            C.byref(prof) if prof is not None else None)
    if fc is not None:
        fc.use(torch.cuda.current_stream(dev))
        _check(load().psh_scan_topk_copy(*args, C.byref(fc.desc)), "psh_scan_topk_copy")
    else:
        fn = load().psh_scan_topk_exhaustive if exhaustive else load().psh_scan_topk
        _check(fn(*args), "psh_scan_topk_exhaustive" if exhaustive else "psh_scan_topk")
    if info is not None:
        info.update(path=prof.path, n_sample_rows=prof.n_sample_rows, grid_blocks=prof.grid_blocks,
                    copy_served=0 if fc is None else fc.desc.served, copy_reason=None if fc is None else fc.desc.reason)
    if profile:
        return out_d, out_idx, status, prof.as_dict()
    return out_d, out_idx, status


def scan_topk_checked(dataset: torch.Tensor, queries: torch.Tensor, k: int, h: int = 0, r_offset: int = 0,
                      workspace: Workspace | None = None, out: tuple | None = None, unsorted: bool = False, flags: int = 0,
                      tau_hint: torch.Tensor | None = None):
    """scan_topk + the status protocol of include/psh.h, with ONE host synchronisation in the normal case:
    a call with `tau_hint` whose status is not OK everywhere (the hint fell short of k windows, or was useless) -> the same
    call without the hint, then as below;
    PSH_STATUS_RETRY (the fused launch gave up) -> the same call through the separate launches (PSH_FLAG_NO_FUSE);
    PSH_STATUS_OVERFLOW (candidate slices overflowed: ties en masse) -> those queries through the exhaustive path.
    Returns (d, idx) device tensors holding valid results for every query."""
    ws = workspace or Workspace(dataset.device)
    d, idx, status = scan_topk(dataset, queries, k, h=h, r_offset=r_offset, workspace=ws, out=out, unsorted=unsorted, flags=flags,
                               tau_hint=tau_hint)
    st = status.cpu()
    if tau_hint is not None and bool((st != PSH_STATUS_OK).any()):
        if bool((st == PSH_STATUS_RETRY).any()):
            ws.arm()
        d, idx, status = scan_topk(dataset, queries, k, h=h, r_offset=r_offset, workspace=ws, out=out, unsorted=unsorted, flags=flags)
        st = status.cpu()
    if bool((st == PSH_STATUS_RETRY).any()):
        ws.arm()
        filter_copy_forget(dataset)        # (the copy scan's audit raises RETRY too: a copy that may be stale is not kept)
        d, idx, status = scan_topk(dataset, queries, k, h=h, r_offset=r_offset, workspace=ws, out=out, unsorted=unsorted,
                                   flags=(flags & ~FLAG_OVERLAP) | FLAG_NO_FUSE)
        st = status.cpu()
    if bool((st != PSH_STATUS_OK).any()):      # (nothing is uploaded in the normal case)
        bad = torch.nonzero(st != PSH_STATUS_OK).flatten().to(dataset.device)
        d2, i2, _ = scan_topk(dataset, queries[bad].contiguous(), k, h=h, r_offset=r_offset, workspace=ws, exhaustive=True)
        d[bad] = d2
        idx[bad] = i2
    return d, idx


def scan_topk_embedded_checked(dataset: torch.Tensor, kernel: torch.Tensor, hx: torch.Tensor, k: int, h: int = 0, r_offset: int = 0,
                               workspace: Workspace | None = None, out: tuple | None = None, flags: int = 0,
                               keep_plan: bool = False):
    """scan_topk_embedded + its status protocol, ONE host synchronisation: the queries whose status is not OK (candidate slices
    overflowed: massive ties / adversarial data) are redone through the exhaustive scan with the same `flags`.
    Returns (d, idx) device tensors holding valid results for every query."""
    ws = workspace or Workspace(dataset.device)
    d, idx, status = scan_topk_embedded(dataset, kernel, hx, k, h=h, r_offset=r_offset, workspace=ws, out=out, flags=flags,
                                        keep_plan=keep_plan)
    bad = torch.nonzero(status != PSH_STATUS_OK).flatten()
    if bad.numel():
        d2, i2, _ = scan_topk_embedded(dataset, kernel, hx[bad].contiguous(), k, h=h, r_offset=r_offset, workspace=ws,
                                       exhaustive=True, flags=flags)
        d[bad] = d2
        idx[bad] = i2
    return d, idx


PSH_EMB_MAX_D = 128


def embed_plan(workspace: "Workspace") -> dict:
    """What the last sampled scan_topk_embedded call on `workspace` found in its kernel matrix (synchronises)."""
    off = int(load().psh_embed_plan_offset())
    v = workspace.buf[off:off + 16].view(torch.int32).cpu().tolist()
    return {"one_interval": bool(v[0]), "ktop": v[1], "merged_rows": v[2], "d": v[3]}


def embedding_supported(d: int, K: int) -> bool:
    """Whether psh_scan_topk_embedded takes a (d, K) kernel (it lives in LDS beside the wave tiles)."""
    if not (0 < d <= PSH_EMB_MAX_D and 0 < K <= PSH_MAX_W):
        return False
    return bool(load().psh_embedded_supported(int(d), int(K)))


def scan_topk_embedded(dataset: torch.Tensor, kernel: torch.Tensor, hx: torch.Tensor, k: int, h: int = 0,
                       r_offset: int = 0, hxnorm: torch.Tensor | None = None, workspace: Workspace | None = None,
                       exhaustive: bool = False, profile: bool = False, out: tuple | None = None, flags: int = 0,
                       keep_plan: bool = False, tau_hint: torch.Tensor | None = None, info: dict | None = None):
    """The scan behind a linear embedding: kernel (d, K) float32 device (unpadded), hx (B, d)
    embedded queries.  Same returns and conventions as scan_topk.
    keep_plan: the caller changes `kernel` only through torch (in-place edits bump its version): when the last sampled call
    on `workspace` scanned with this very tensor at this version, what the library found in the matrix is used again
    (PSH_FLAG_EMBED_PLAN_KEEP) instead of being worked out by one more launch."""
    ds = _dev_tensor(dataset, torch.float32, "dataset")
    ker = _dev_tensor(kernel, torch.float32, "kernel")
    q = _dev_tensor(hx, torch.float32, "hx")
    if ds.dim() != 2 or ker.dim() != 2 or q.dim() != 2 or q.shape[1] != ker.shape[0]:
        raise ValueError("dataset must be (R, T), kernel (d, K) and hx (B, d)")
    if q.device != ds.device or ker.device != ds.device:
        raise ValueError("dataset, kernel and hx must live on the same device")
    R, T = ds.shape
    d, K = ker.shape
    B = q.shape[0]
    dev = ds.device
    if hxnorm is not None:
        hxnorm = _dev_tensor(hxnorm, torch.float32, "hxnorm")
    if B > PSH_MAX_B_PER_LAUNCH and not profile:
        return _per_launch(B, out, lambda c, o: scan_topk_embedded(
            ds, ker, q[c].contiguous(), k, h=h, r_offset=r_offset, hxnorm=_cut(hxnorm, c), workspace=workspace,
            exhaustive=exhaustive, out=o, flags=flags, keep_plan=keep_plan, tau_hint=_cut(tau_hint, c)))
    wsobj = workspace or Workspace(dev)
    ws = wsobj.get(workspace_bytes(R, T, B, K, h, k))
    if not exhaustive:
        po = wsobj.plan_of
        planned = not (flags & (FLAG_EMBED_DENSE | FLAG_EMBED_TAPS | FLAG_EMBED_MX))     # the library works the plan out at all
        if keep_plan and planned and po is not None and po[0] is kernel and po[1:] == (kernel._version, B):
            flags |= FLAG_EMBED_PLAN_KEEP
        # (a call of the non-exhaustive entry point leaves the plan of ITS kernel in the workspace, unless it kept one)
        wsobj.plan_of = (kernel, kernel._version, B) if planned else None
    out_d, out_idx, status = _scan_outputs(out, B, k, dev)
    prof = _scan_profile(B, profile, None, flags, info, tau_hint)
    name = "psh_scan_topk_embedded_exhaustive" if exhaustive else "psh_scan_topk_embedded"
    rc = getattr(load(), name)(dev.index, _stream_ptr(dev), ds.data_ptr(), R, T, r_offset, ker.data_ptr(), d, K,
                               q.data_ptr(), None if hxnorm is None else hxnorm.data_ptr(), B, h, k,
                               out_d.data_ptr(), out_idx.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                               C.byref(prof) if prof is not None else None)
    _check(rc, name)
    if info is not None:
        info.update(path=prof.path, n_sample_rows=prof.n_sample_rows, grid_blocks=prof.grid_blocks)
    if profile:
        return out_d, out_idx, status, prof.as_dict()
    return out_d, out_idx, status


def candidates_layout(R: int, T: int, B: int, W: int, h: int, k: int, nbytes: int) -> dict:
    """psh_candidates_layout: where a scan with these sizes on a workspace of `nbytes` leaves the windows it admitted
    (diagnostics: tests/test_gpu_admitted_set.py reads the admitted SET back and compares it with the oracle's)."""
    out = (C.c_int64 * 14)()
    _check(load().psh_candidates_layout(R, T, B, W, h, k, nbytes, out), "psh_candidates_layout")
    names = ("qstate", "bcount", "bcount2", "cand_d", "cand_rt", "cap", "hdr_cand", "hdr_blk", "hdr_stream_ncand", "max_blocks",
             "fused_max_blocks", "fused_front", "stream_list", "stream_cap")
    return dict(zip(names, (int(v) for v in out)))


def embed_rows(dataset: torch.Tensor, kernel: torch.Tensor) -> torch.Tensor:
    """(R, d): the embedding of the FIRST window of every row (one-window rows behind a linear embedding)."""
    ds = _dev_tensor(dataset, torch.float32, "dataset")
    ker = _dev_tensor(kernel, torch.float32, "kernel")
    R, T = ds.shape
    d, K = ker.shape
    out = torch.empty((R, d), dtype=torch.float32, device=ds.device)
    _check(load().psh_embed_rows(ds.device.index, _stream_ptr(ds.device), ds.data_ptr(), R, T, ker.data_ptr(), d, K,
                                 out.data_ptr()), "psh_embed_rows")
    return out


# ---- multi-GPU exchange under the C ABI (psh_comm.hip) ----------------------------------------------------------
PSH_COMM_ID_BYTES = 128


def rccl_library_path() -> str:
    """The RCCL this process already uses: the one bundled with PyTorch-ROCm (torch/lib/librccl.so)."""
    import os
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    return cand if os.path.exists(cand) else "librccl.so"


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(PSH_COMM_ID_BYTES)
    _check(load().psh_comm_unique_id(rccl_library_path().encode(), buf), "psh_comm_unique_id")
    return buf.raw


class Comm:
    """An RCCL communicator owned by libpsh_hip.so (psh_comm_create): one per rank, created collectively."""

    def __init__(self, device: torch.device, world: int, rank: int, unique_id: bytes):
        self.device, self.world, self.rank = device, world, rank
        h = C.c_void_p()
        _check(load().psh_comm_create(rccl_library_path().encode(), device.index, world, rank, unique_id, C.byref(h)),
               "psh_comm_create")
        self._h = h

    def close(self):
        if self._h:
            load().psh_comm_destroy(self._h)
            self._h = None

    def exchange_merge(self, send: torch.Tensor, gathered: torch.Tensor, B: int, k: int, out_d: torch.Tensor,
                       out_idx: torch.Tensor, merge_ws: torch.Tensor | None, side: "torch.cuda.Stream",
                       ev_scan_done: "torch.cuda.Event", ev_merged: "torch.cuda.Event"):
        """psh_exchange_merge: all-gather + merge on `side`, behind ONE event on the current stream; nothing is
        synchronised.  The events must have been recorded once (their handles exist)."""
        _dev_tensor(send, torch.int32, "send")
        _dev_tensor(gathered, torch.int32, "gathered")
        rc = load().psh_exchange_merge(self._h, _stream_ptr(self.device), side.cuda_stream, send.data_ptr(), gathered.data_ptr(),
                                       B, k, out_d.data_ptr(), out_idx.data_ptr(),
                                       None if merge_ws is None else merge_ws.data_ptr(), 0 if merge_ws is None else merge_ws.numel(),
                                       ev_scan_done.cuda_event, ev_merged.cuda_event)
        _check(rc, "psh_exchange_merge")


PSH_STREAM_RESERVED_CUS = 8


def reserving_stream(device: torch.device, reserve_cus: int = PSH_STREAM_RESERVED_CUS):
    """(torch stream, CUs reserved): a stream whose kernels leave `reserve_cus` compute units alone
    (psh_stream_create_reserving), wrapped for torch.  The raw stream lives as long as the process (a handful per object)."""
    h, got = C.c_void_p(), C.c_int(0)
    _check(load().psh_stream_create_reserving(device.index, int(reserve_cus), C.byref(h), C.byref(got)), "psh_stream_create_reserving")
    return torch.cuda.ExternalStream(h.value, device=device), int(got.value)


class PreparedShadow:
    """One single-query shadow() on the device -- psh_scan_topk as the overlap-friendly launches, then psh_gather_paths -- with
    everything but the stream fixed beforehand: argument lists built once, the query staged through a pinned buffer of its own,
    results in buffers the slot owns.  The per-call host cost is one small copy and two ctypes calls (the general path spends
    ~250 us of Python per call, three times what the device needs).  One slot serves one call at a time: the caller hands it
    out again only after the previous call's results have been taken."""

    def __init__(self, rows: torch.Tensor, ds3: torch.Tensor, W: int, k: int, h: int, workspace: "Workspace", flags: int,
                 host_direct: bool = False, filter_copy: "FilterCopy | None" = None):
        """`filter_copy`: a FilterCopy of `rows` the owner keeps for its resident ensemble: the scan goes through
        psh_scan_topk_copy (the copy serves the overlap launches of a query with W <= 33; any other call is psh_scan_topk's).
        `host_direct`: the kernels read the query from the pinned staging buffer and write their results into the pinned
        result buffer themselves (host memory mapped into the device's address space: ~170 KB over PCIe as posted writes) --
        no copy engine in the chain of a BLOCKING call, whose latency is what counts."""
        self.host_direct = host_direct
        rows = _dev_tensor(rows, torch.float32, "rows")
        dev = rows.device
        R, T = rows.shape
        C_ = ds3.shape[1]
        # the query and, behind it at a 16-byte boundary, the caller's admission hint (psh_profile.tau_hint: one float)
        self._Wp = (W + 3) // 4 * 4
        self._stage_pin = torch.zeros((self._Wp + 4,), dtype=torch.float32, pin_memory=True)
        self._stage_dev = torch.zeros((self._Wp + 4,), dtype=torch.float32, device=dev)
        self.q_pin = self._stage_pin[:W].view(1, W)
        self.q_dev = self._stage_dev[:W].view(1, W)
        # results packed in ONE device buffer and one pinned host buffer (status | d | idx | paths): one D2H copy per call
        n_d, n_i, n_p = 4 * k, 8 * k, 4 * k * C_ * (W + h)
        o_d = 256
        o_i = o_d + (n_d + 255) // 256 * 256
        o_p = o_i + (n_i + 255) // 256 * 256
        self._res = torch.zeros(o_p + n_p, dtype=torch.uint8, device=dev)
        self._res_host = torch.zeros(self._res.numel(), dtype=torch.uint8, pin_memory=True)

        def carve(buf):
            return (buf[o_d:o_d + n_d].view(torch.float32).view(1, k),
                    buf[o_p:o_p + n_p].view(torch.float32).view(1, k, C_, W + h),
                    buf[o_i:o_i + n_i].view(torch.int32).view(1, k, 2),
                    buf[0:4].view(torch.int32))
        self._carve = carve
        self.host = carve(self._res_host)
        self.d, self.paths, self.idx, self.status = self.host if host_direct else carve(self._res)
        if host_direct:
            self.q_dev = self.q_pin
            self._stage_dev = self._stage_pin
        self._hint_ptr = self._stage_dev.data_ptr() + 4 * self._Wp
        self._stage_np = self._stage_pin.numpy()             # (numpy views: element stores / reads without a torch dispatch)
        self._q_np = self._stage_np[:W]
        self._refresh_status_view()
        self.event = torch.cuda.Event()
        ws = workspace.get(workspace_bytes(R, T, 1, W, h, k))
        self._keep = (rows, ds3, ws, workspace)
        self.prof = PshProfile()
        self.prof.mode = 1
        self.prof.flags = flags
        L = load()
        self._scan_fn, self._gather_fn = L.psh_scan_topk, L.psh_gather_paths
        self._scan_args = [dev.index, None, rows.data_ptr(), R, T, 0, self.q_dev.data_ptr(), None, 1, W, h, k, self.d.data_ptr(),
                           self.idx.data_ptr(), self.status.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(self.prof)]
        self.filter_copy = filter_copy
        if filter_copy is not None:
            if (filter_copy.R, filter_copy.T) != (R, T):
                raise ValueError("filter_copy was built from an ensemble of another shape")
            self._fc_desc = PshFilterCopy(filter_copy.buf.data_ptr(), filter_copy.pitch_halves, R, T, 0, 0)   # (served / reason: this slot's)
            self._scan_fn = L.psh_scan_topk_copy
            self._scan_args.append(C.byref(self._fc_desc))
        self._gather_args = [dev.index, None, ds3.data_ptr(), ds3.shape[0], C_, ds3.shape[2], 0, self.idx.data_ptr(), k, W + h,
                             self.paths.data_ptr()]

    def _refresh_status_view(self):
        self.status_np = self.host[3].numpy()                # the call's status word as the host sees it (after the event)

    # results of this size and more are HANDED to the caller instead of copied out of the slot's pinned buffer (host_direct
    # slots): at k = 8192 the four numpy copies were 100 us of a 340 us shadow() call
    HANDOVER_BYTES = 256 * 1024

    def take(self):
        """(d, paths, idx, status) of the finished call as numpy arrays the caller owns.  Small results are copied out of the
        pinned buffer (12 us at k = 1024); large ones keep the buffer -- the arrays view it, it lives as long as they do -- and
        the slot gets a fresh pinned buffer for its next call (torch's pinned-memory cache hands back the block a dropped
        result returned: no allocation in a steady loop)."""
        if self._res_host.numel() < self.HANDOVER_BYTES:
            return tuple(t.numpy().copy() for t in self.host)
        out = tuple(t.numpy() for t in self.host)
        self._res_host = torch.empty(self._res_host.numel(), dtype=torch.uint8, pin_memory=True)
        self.host = self._carve(self._res_host)
        self._refresh_status_view()
        if self.host_direct:                                 # the kernels write the pinned buffer themselves: new addresses
            self.host[3].zero_()
            self.d, self.paths, self.idx, self.status = self.host
            self._scan_args[12], self._scan_args[13], self._scan_args[14] = self.d.data_ptr(), self.idx.data_ptr(), self.status.data_ptr()
            self._gather_args[7], self._gather_args[10] = self.idx.data_ptr(), self.paths.data_ptr()
        return out

    def launch(self, stream: "torch.cuda.Stream", x_row: torch.Tensor, hint: float | None = None) -> None:
        """x_row: (1, W) float32 CPU tensor.  Everything is enqueued on `stream`, the D2H copies of the results included.
        `hint`: the caller's admission level on acc (psh_profile.tau_hint) -- a status other than OK then means "again without"."""
        # (a CUDA query, or one that requires grad -- the reference's `_torch` passes tensors through as they are: a detached host copy)
        self._q_np[:] = x_row.detach().cpu().numpy().reshape(-1) if isinstance(x_row, torch.Tensor) else x_row
        if hint is not None:
            self._stage_np[self._Wp] = hint
        self.prof.tau_hint = self._hint_ptr if hint is not None else None
        sp = stream.cuda_stream
        if self.filter_copy is not None:
            self.filter_copy.use(stream)
        if self.host_direct:
            # nothing here is a torch operation: the kernels read the pinned staging buffer and write the pinned result buffer
            # themselves -- two library calls and the event, no stream context to enter and leave (5 us of a blocking call)
            a = self._scan_args
            a[1] = sp
            rc = self._scan_fn(*a)
            if rc:
                _check(rc, "psh_scan_topk")
            g = self._gather_args
            g[1] = sp
            rc = self._gather_fn(*g)
            if rc:
                _check(rc, "psh_gather_paths")
            self.event.record(stream)
            return
        with torch.cuda.stream(stream):
            self._stage_dev.copy_(self._stage_pin, non_blocking=True)
            a = self._scan_args
            a[1] = sp
            rc = self._scan_fn(*a)
            if rc:
                _check(rc, "psh_scan_topk")
            g = self._gather_args
            g[1] = sp
            rc = self._gather_fn(*g)
            if rc:
                _check(rc, "psh_gather_paths")
            self._res_host.copy_(self._res, non_blocking=True)
            self.event.record()


class _HostBlock:
    """One pinned block of psh_shadow_blocking (query in, status / d / idx / paths out).  `root` is the numpy view every array
    handed to a caller is based on: while the caller keeps one of them, root's reference count says so and the block is not
    written again."""

    def __init__(self, owner: "BlockingShadow"):
        import sys
        import numpy as np
        self.t = torch.zeros(owner.nbytes, dtype=torch.uint8, pin_memory=True)
        self.root = self.t.numpy()
        W = owner.W
        self.q = self.root[owner.o_query:owner.o_query + 4 * W].view(np.float32)
        self.hint = self.root[owner.o_hint:owner.o_hint + 4].view(np.float32)
        self.status = self.root[owner.o_status:owner.o_status + 4].view(np.int32)
        self.times = self.root[16:32].view(np.float32)        # PSH_SHADOW_OFF_TIMES: us enqueueing / waiting / until the launch started, last call
        self.prof = PshProfile()
        self.prof.flags = owner.flags
        rows, ds3 = owner.rows, owner.ds3
        self.args = [rows.device.index, None, rows.data_ptr(), rows.shape[0], rows.shape[1], 0, ds3.data_ptr(), ds3.shape[1],
                     W, owner.h, owner.k, self.t.data_ptr(), owner.nbytes, 0, owner.ws.data_ptr(), owner.ws.numel(), C.byref(self.prof)]
        self._getrc = sys.getrefcount
        self.rc0 = self._getrc(self.root)

    def busy(self) -> bool:
        return self._getrc(self.root) != self.rc0


class BlockingShadow:
    """shadow() of ONE Identity query as ONE blocking library call (psh_shadow_blocking): the fused launch reads the query
    from a pinned block and writes distances, indices AND the gathered paths into it, the call returns when the launch's
    completion words have landed there.  Results are handed to the caller as numpy arrays that VIEW the block (no copy out:
    11 us at k = 1024); a block is written again only once the caller has dropped every array of it -- callers that keep
    their results get a fresh block per call, up to POOL of them, after which results are copied out of a scratch block."""

    POOL = 8

    def __init__(self, rows: torch.Tensor, ds3: torch.Tensor, W: int, k: int, h: int, workspace: "Workspace", flags: int = 0):
        import numpy as np
        self._np = np
        self.rows = _dev_tensor(rows, torch.float32, "rows")
        self.ds3 = _dev_tensor(ds3, torch.float32, "dataset")
        self.W, self.k, self.h, self.flags = W, k, h, flags
        self.C = ds3.shape[1]
        L = load()
        lay = (C.c_size_t * 7)()
        _check(L.psh_shadow_block_layout(W, h, k, self.C, lay), "psh_shadow_block_layout")
        self.nbytes, self.o_status, self.o_query, self.o_hint, self.o_d, self.o_i, self.o_p = (int(v) for v in lay)
        R, T = self.rows.shape
        self.ws = workspace.get(workspace_bytes(R, T, 1, W, h, k))
        self._keep = workspace
        self._fn = L.psh_shadow_blocking
        self.blocks = [_HostBlock(self)]
        self.scratch = None
        self.last_fused = False

    def _block(self):
        for b in self.blocks:
            if not b.busy():
                return b, False
        if len(self.blocks) < self.POOL:
            b = _HostBlock(self)
            self.blocks.append(b)
            return b, False
        if self.scratch is None:
            self.scratch = _HostBlock(self)
        return self.scratch, True

    def call(self, stream_ptr: int, x, hint: float | None = None):
        """x: W float32 values (numpy).  Returns (status, None) or (0, (d (1,k), paths (1,k,C,W+h), idx (1,k,2)))."""
        np = self._np
        b, copy = self._block()
        b.q[:] = x
        a = b.args
        a[1] = stream_ptr
        if hint is not None:
            b.hint[0] = hint
            a[13] = 1
        else:
            a[13] = 0
        rc = self._fn(*a)
        if rc:
            _check(rc, "psh_shadow_blocking")
        self.last_fused = b.prof.path == 2
        st = int(b.status[0])
        if st != PSH_STATUS_OK:
            return st, None
        k, W, h, Cc = self.k, self.W, self.h, self.C
        d = np.ndarray((1, k), np.float32, b.root, self.o_d)
        idx = np.ndarray((1, k, 2), np.int32, b.root, self.o_i)
        paths = np.ndarray((1, k, Cc, W + h), np.float32, b.root, self.o_p)
        if copy:
            return 0, (d.copy(), paths.copy(), idx.copy())
        return 0, (d, paths, idx)


class PreparedStep:
    """One step of the row-sharded scan with everything but the stream and the query pointer fixed beforehand: the local
    psh_scan_topk into the send buffer, then psh_exchange_merge (all-gather + merge on the side stream).  The per-step host
    cost is two ctypes calls over pre-built argument lists -- no tensor is allocated, no Python-side check repeated (a rank
    that spends 100 us of Python per 85 us step is host-bound).  Buffers are owned here and REUSED by the next launch()."""

    def __init__(self, comm: "Comm", dataset: torch.Tensor, r_offset: int, B: int, W: int, k: int, h: int, workspace: "Workspace",
                 side: "torch.cuda.Stream", flags: int, sorted_merge: bool):
        ds = _dev_tensor(dataset, torch.float32, "dataset")
        dev = ds.device
        R, T = ds.shape
        G = comm.world
        self.B, self.W, self.k = B, W, k
        self.send = torch.empty(3 * B * k, dtype=torch.int32, device=dev)
        self.gathered = torch.empty((G, 3 * B * k), dtype=torch.int32, device=dev)
        self.out_d = torch.empty((B, k), dtype=torch.float32, device=dev)
        self.out_idx = torch.empty((B, k, 2), dtype=torch.int32, device=dev)
        # a status row PER LAUNCH (round-robin over STATUS_ROWS): a PSH_STATUS_RETRY of any step stays visible after later
        # launches of this slot have reused every other buffer (`status` is the row of the latest launch)
        self.status_all = torch.zeros((self.STATUS_ROWS, B), dtype=torch.int32, device=dev)
        self.status = self.status_all[0]
        self._launches = 0
        self.merge_ws = None
        if not sorted_merge:
            self.merge_ws = torch.empty(merge_workspace_bytes(B, k), dtype=torch.uint8, device=dev)
        self.ev_a, self.ev_b = torch.cuda.Event(), torch.cuda.Event()
        self.ev_a.record(); self.ev_b.record()                  # materialise the hipEvent handles
        ws = workspace.get(workspace_bytes(R, T, B, W, h, k))
        self._keep = (ds, ws, side, comm, workspace)
        self.prof = PshProfile()
        self.prof.mode = 1
        self.prof.flags = flags | (0 if sorted_merge else FLAG_UNSORTED)
        L = load()
        self._scan_fn, self._exch_fn = L.psh_scan_topk, L.psh_exchange_merge
        self._scan_args = [dev.index, None, ds.data_ptr(), R, T, r_offset, None, None, B, W, h, k, self.send.data_ptr(),
                           self.send.data_ptr() + 4 * B * k, self.status_all.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(self.prof)]
        self._status_base = self.status_all.data_ptr()
        self._exch_args = [comm._h, None, side.cuda_stream, self.send.data_ptr(), self.gathered.data_ptr(), B, k,
                           self.out_d.data_ptr(), self.out_idx.data_ptr(),
                           None if self.merge_ws is None else self.merge_ws.data_ptr(), 0 if self.merge_ws is None else self.merge_ws.numel(),
                           self.ev_a.cuda_event, self.ev_b.cuda_event]

    STATUS_ROWS = 1024

    def launch(self, stream_ptr: int, q_ptr: int) -> None:
        a = self._scan_args
        a[1] = stream_ptr
        a[6] = q_ptr
        row = self._launches % self.STATUS_ROWS
        self._launches += 1
        a[14] = self._status_base + 4 * self.B * row
        self.status = self.status_all[row]
        rc = self._scan_fn(*a)
        if rc:
            _check(rc, "psh_scan_topk")
        e = self._exch_args
        e[1] = stream_ptr
        rc = self._exch_fn(*e)
        if rc:
            _check(rc, "psh_exchange_merge")


def merge_topk(d_lists: torch.Tensor, idx_lists: torch.Tensor, k: int):
    """k best by (d, r, t) out of (B, n) candidates; entries with r < 0 are padding."""
    d = _dev_tensor(d_lists, torch.float32, "d_lists")
    ix = _dev_tensor(idx_lists, torch.int32, "idx_lists")
    B, n = d.shape
    if tuple(ix.shape) != (B, n, 2):
        raise ValueError("idx_lists must be (B, n, 2)")
    ws = torch.empty(merge_workspace_bytes(B, k), dtype=torch.uint8, device=d.device)
    out_d = torch.empty((B, k), dtype=torch.float32, device=d.device)
    out_idx = torch.empty((B, k, 2), dtype=torch.int32, device=d.device)
    _check(load().psh_merge_topk(d.device.index, _stream_ptr(d.device), d.data_ptr(), ix.data_ptr(), B, n, k,
                                 out_d.data_ptr(), out_idx.data_ptr(), ws.data_ptr(), ws.numel()),
           "psh_merge_topk")
    return out_d, out_idx


def merge_topk_gathered(gathered: torch.Tensor, G: int, B: int, k_in: int, k: int):
    """Merge what one all-gather delivered.  `gathered`: int32 (G, 3*B*k_in): per rank the
    (B,k_in) float32 distances (bit pattern) followed by the (B,k_in,2) int32 indices."""
    g = _dev_tensor(gathered, torch.int32, "gathered")
    if tuple(g.shape) != (G, 3 * B * k_in):
        raise ValueError("gathered must be (G, 3*B*k_in) int32")
    ws = torch.empty(merge_workspace_bytes(B, k), dtype=torch.uint8, device=g.device)
    out_d = torch.empty((B, k), dtype=torch.float32, device=g.device)
    out_idx = torch.empty((B, k, 2), dtype=torch.int32, device=g.device)
    base = g.data_ptr()
    # distances: rank stride 3*B*k_in floats; indices: the (r,t) pairs start B*k_in ints in
    # and their rank stride is 3*B*k_in/2 pairs -- whole (and 8-byte aligned) when B*k_in is even
    if (B * k_in) % 2:
        raise ValueError("B*k_in must be even for the in-place gathered merge")
    _check(load().psh_merge_topk_gathered(g.device.index, _stream_ptr(g.device), base, base + 4 * B * k_in,
                                          G, 3 * B * k_in, (3 * B * k_in) // 2, B, k_in, k,
                                          out_d.data_ptr(), out_idx.data_ptr(),
                                          ws.data_ptr(), ws.numel()), "psh_merge_topk_gathered")
    return out_d, out_idx


def merge_workspace_bytes(B: int, k: int) -> int:
    return _workspace_bytes(load().psh_merge_workspace_bytes, B, k)


def merge_sorted_supported(G: int, k_in: int) -> bool:
    return G <= 64 and G * k_in <= 32768


def merge_sorted_gathered(gathered: torch.Tensor, G: int, B: int, k_in: int, k: int):
    """merge_topk_gathered for lists that are SORTED by (d, r, t), rank g owning smaller rows than rank g+1
    (psh_merge_sorted_gathered: positions by binary search, no selection, no sort)."""
    g = _dev_tensor(gathered, torch.int32, "gathered")
    if tuple(g.shape) != (G, 3 * B * k_in):
        raise ValueError("gathered must be (G, 3*B*k_in) int32")
    if (B * k_in) % 2:
        raise ValueError("B*k_in must be even for the in-place gathered merge")
    out_d = torch.empty((B, k), dtype=torch.float32, device=g.device)
    out_idx = torch.empty((B, k, 2), dtype=torch.int32, device=g.device)
    base = g.data_ptr()
    _check(load().psh_merge_sorted_gathered(g.device.index, _stream_ptr(g.device), base, base + 4 * B * k_in,
                                            G, 3 * B * k_in, (3 * B * k_in) // 2, B, k_in, k,
                                            out_d.data_ptr(), out_idx.data_ptr()), "psh_merge_sorted_gathered")
    return out_d, out_idx


def gather_paths(dataset: torch.Tensor, idx: torch.Tensor, length: int, r_offset: int = 0,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """out[b, i, c, :] = dataset[idx[b,i,0] - r_offset, c, idx[b,i,1] : +length]; dataset (R, C, T)."""
    ds = _dev_tensor(dataset, torch.float32, "dataset")
    ix = _dev_tensor(idx, torch.int32, "idx")
    if ds.dim() != 3:
        raise ValueError("dataset must be (R, C, T)")
    R, Cc, T = ds.shape
    n = ix.numel() // 2
    if out is None:
        out = torch.zeros(tuple(ix.shape[:-1]) + (Cc, length), dtype=torch.float32, device=ds.device)
    _check(load().psh_gather_paths(ds.device.index, _stream_ptr(ds.device), ds.data_ptr(), R, Cc, T, r_offset,
                                   ix.data_ptr(), n, length, out.data_ptr()), "psh_gather_paths")
    return out


def _values(values):
    """(v, B, k, m): the (B, k, ...) float32 statistic and its m values per path."""
    v = _dev_tensor(values, torch.float32, "values")
    if v.dim() < 2:
        raise ValueError("values must be (B, k, ...)")
    B, k = v.shape[:2]
    m = v.numel() // (B * k) if B * k else 0
    if m == 0:
        raise ValueError("values is empty")
    return v, B, k, m


def _weights(weights, B: int, k: int, sets: bool = False):
    """The (B, k) float64 weights of a statistic -- with sets=True (E, B, k) weight sets -- or None for unit weights."""
    if weights is None:
        return None
    w = _dev_tensor(weights, torch.float64, "weights")
    if sets and (w.dim() != 3 or tuple(w.shape[1:]) != (B, k)):
        raise ValueError(f"weights must be (E, B, k) with (B, k) = ({B}, {k}), got {tuple(w.shape)}")
    if not sets and tuple(w.shape) != (B, k):
        raise ValueError(f"weights must be (B, k) = ({B}, {k}), got {tuple(w.shape)}")
    return w


def weighted_moments(values: torch.Tensor, weights: torch.Tensor | None):
    """(mean, std) over axis 1 of a (B, k, ...) float32 statistic with (B, k) float64 weights (None: uniform) --
    predict_from_paths()'s `proba.avg(values, axis=1)`, `proba.std(values, axis=1)` on the device; float64 (B, ...)."""
    v, B, k, m = _values(values)
    w = _weights(weights, B, k)
    mean = torch.empty((B,) + tuple(v.shape[2:]), dtype=torch.float64, device=v.device)
    std = torch.empty_like(mean)
    _check(load().psh_weighted_moments(v.device.index, _stream_ptr(v.device), v.data_ptr(), _ptr(w), B, k, m,
                                       mean.data_ptr(), std.data_ptr()), "psh_weighted_moments")
    return mean, std


PSH_QUANTILE_MAX_LEVELS = 32
PSH_QUANTILE_STATUS_OK, PSH_QUANTILE_STATUS_NONFINITE, PSH_QUANTILE_STATUS_WEIGHTS = 0, 1, 2


def weighted_quantiles(values: torch.Tensor, weights: torch.Tensor | None, levels):
    """psh_weighted_quantiles over axis 1 of a (B, k, ...) float32 statistic with (B, k) float64 weights (None: unit
    weights) at the levels 0 < p < 1: (q, lower, upper), each (B, Q, ...) float64, and status (B,) int32, all on the device;
    nothing is synchronised here."""
    v, B, k, m = _values(values)
    lv = [float(p) for p in levels]
    w = _weights(weights, B, k)
    shape = (B, len(lv)) + tuple(v.shape[2:])
    q, lower, upper = (torch.empty(shape, dtype=torch.float64, device=v.device) for _ in range(3))
    status = torch.empty((B,), dtype=torch.int32, device=v.device)
    arr = (C.c_double * max(len(lv), 1))(*lv)
    _check(load().psh_weighted_quantiles(v.device.index, _stream_ptr(v.device), v.data_ptr(), _ptr(w), B, k, m, arr, len(lv),
                                         q.data_ptr(), lower.data_ptr(), upper.data_ptr(), status.data_ptr()),
           "psh_weighted_quantiles")
    return q, lower, upper, status


PSH_SCORE_MAX_SETS = 64
PSH_SCORE_STATUS_OK, PSH_SCORE_STATUS_NONFINITE, PSH_SCORE_STATUS_WEIGHTS, PSH_SCORE_STATUS_OBS = 0, 1, 2, 4


def score_ensemble(values: torch.Tensor, weights: torch.Tensor | None, obs: torch.Tensor):
    """psh_score_ensemble over axis 1 of a (B, k, ...) float32 statistic against the (B, ...) float32 observations, under
    (E, B, k) float64 weight sets (None: one set of unit weights): (crps, pit_lo, pit_hi, mean), each (E, B, ...) float64,
    and status (E, B) int32, all on the device; nothing is synchronised here."""
    v, B, k, m = _values(values)
    y = _dev_tensor(obs, torch.float32, "obs")
    if tuple(y.shape) != (B,) + tuple(v.shape[2:]):
        raise ValueError(f"obs must be {(B,) + tuple(v.shape[2:])}, got {tuple(y.shape)}")
    w = _weights(weights, B, k, sets=True)
    E = 1 if w is None else int(w.shape[0])
    shape = (E, B) + tuple(v.shape[2:])
    crps, pit_lo, pit_hi, mean = (torch.empty(shape, dtype=torch.float64, device=v.device) for _ in range(4))
    status = torch.empty((E, B), dtype=torch.int32, device=v.device)
    _check(load().psh_score_ensemble(v.device.index, _stream_ptr(v.device), v.data_ptr(), _ptr(w), y.data_ptr(), B, k, m, E,
                                     crps.data_ptr(), pit_lo.data_ptr(), pit_hi.data_ptr(), mean.data_ptr(),
                                     status.data_ptr()), "psh_score_ensemble")
    return crps, pit_lo, pit_hi, mean, status


def softmax_weights(distances: torch.Tensor, etas, ks=None) -> torch.Tensor:
    """psh_softmax_weights on the (B, k) float32 distances of a scan, where they lie: the (len(etas) * len(ks), B, k) float64
    weights of the grid, set a * len(ks) + c being (etas[a], ks[c]), on the device; nothing is synchronised here.  An eta of
    None is the uniform weighting 1 / k'; ks=None is the one cut-off k."""
    d = _dev_tensor(distances, torch.float32, "distances")
    if d.dim() != 2 or d.numel() == 0:
        raise ValueError(f"distances must be (B, k) and not empty, got {tuple(d.shape)}")
    B, k = d.shape
    es = [math.inf if eta is None else float(eta) for eta in etas]
    kk = None if ks is None else [int(n) for n in ks]
    n_ks = 1 if kk is None else len(kk)
    if not es or n_ks < 1 or len(es) * n_ks > PSH_SCORE_MAX_SETS:
        raise ValueError(f"{len(es)} etas x {n_ks} ks weight sets: 1 to {PSH_SCORE_MAX_SETS} a call")
    if k > PSH_MAX_K:
        raise NativeLibraryError(f"psh_softmax_weights takes k <= {PSH_MAX_K} paths, got {k}")
    out = torch.empty((len(es) * n_ks, B, k), dtype=torch.float64, device=d.device)
    _check(load().psh_softmax_weights(d.device.index, _stream_ptr(d.device), d.data_ptr(), B, k, (C.c_double * len(es))(*es),
                                      len(es), None if kk is None else (C.c_int * n_ks)(*kk), n_ks, out.data_ptr()),
           "psh_softmax_weights")
    return out


PSH_SEPARATE_STATUS_OK, PSH_SEPARATE_STATUS_SHORT = 0, 1


def separate_topk(distances: torch.Tensor, indices: torch.Tensor, k: int, delta: int):
    """psh_separate_topk on the (B, K) float32 distances and (B, K, 2) int32 indices of a scan, where they lie: the first k
    entries an exclusion zone of `delta` samples keeps, as device tensors (distances (B, k), indices (B, k, 2), positions
    (B, k) int32, count (B,) int32, status (B,) int32); nothing is synchronised here."""
    d = _dev_tensor(distances, torch.float32, "distances")
    idx = _dev_tensor(indices, torch.int32, "indices")
    if d.dim() != 2 or d.numel() == 0 or tuple(idx.shape) != tuple(d.shape) + (2,):
        raise ValueError(f"distances must be (B, K), not empty, and indices (B, K, 2); got {tuple(d.shape)} and {tuple(idx.shape)}")
    B, K = d.shape
    k, delta = int(k), int(delta)
    if not (1 <= k <= K) or not (0 <= delta < 2 ** 31):
        raise ValueError(f"separate_topk: 1 <= k <= K = {K} and 0 <= delta < 2^31, got k = {k}, delta = {delta}")
    if K > PSH_MAX_K:
        raise NativeLibraryError(f"psh_separate_topk takes lists of K <= {PSH_MAX_K} entries, got {K}")
    od = torch.empty((B, k), dtype=torch.float32, device=d.device)
    oi = torch.empty((B, k, 2), dtype=torch.int32, device=d.device)
    op = torch.empty((B, k), dtype=torch.int32, device=d.device)
    oc = torch.empty(B, dtype=torch.int32, device=d.device)
    os_ = torch.empty(B, dtype=torch.int32, device=d.device)
    _check(load().psh_separate_topk(d.device.index, _stream_ptr(d.device), d.data_ptr(), idx.data_ptr(), B, K, k, delta,
                                    od.data_ptr(), oi.data_ptr(), op.data_ptr(), oc.data_ptr(), os_.data_ptr()),
           "psh_separate_topk")
    return od, oi, op, oc, os_


def _uniform_rows(x: torch.Tensor):
    """(n_rows, row_stride) when x (..., L) -- last dim contiguous -- is n_rows rows a constant stride apart (a contiguous
    tensor, or a slice of the last dimension of one: the out-context view of gathered paths), else None."""
    if x.dim() == 0 or x.stride(-1) != 1:
        return None
    if x.dim() == 1:
        return 1, x.shape[0]
    rs = x.stride(-2) if x.shape[-2] > 1 else None
    n = 1
    for dim in range(x.dim() - 2, -1, -1):
        if x.shape[dim] > 1:
            if rs is None:
                rs = x.stride(dim) // n if n else x.stride(dim)
            if x.stride(dim) != rs * n:
                return None
        n *= x.shape[dim]
    return n, (rs if rs is not None else x.shape[-1])


def _strided_rows(x, name: str):
    """(n_rows, row_stride) of a non-empty float32 HIP tensor (..., n) whose rows lie a constant stride apart."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise NativeLibraryError(f"{name} must be a tensor on a HIP device (got {type(x).__name__} on "
                                 f"{getattr(x, 'device', '?')}); there is no CPU path here")
    if x.dtype != torch.float32:
        raise TypeError(f"{name} must be torch.float32, got {x.dtype}")
    rows = _uniform_rows(x) if x.numel() else None
    if rows is None:
        raise ValueError(f"{name} must be non-empty rows of samples a constant stride apart, the last dimension contiguous")
    return rows


def _psi_hat(psi_hat, J: int, n: int, device):
    """The check of the scattering entry points' (J, n / 2) float64 multipliers."""
    if not (isinstance(psi_hat, torch.Tensor) and psi_hat.device == device and psi_hat.dtype == torch.float64
            and psi_hat.is_contiguous() and tuple(psi_hat.shape) == (J, n // 2)):
        raise ValueError(f"psi_hat must be a contiguous ({J}, {n // 2}) float64 tensor on {device}")


def realized_variance(x: torch.Tensor, Ts, vol: bool = False) -> torch.Tensor | None:
    """statistics.realized_variance on a float32 HIP tensor (..., L): (..., len(Ts)) float32, or None when this tensor's
    layout is not rows a constant stride apart (the caller then uses torch ops)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.numel() > 0):
        return None
    Ts = [int(T) for T in Ts]
    rows = _uniform_rows(x)
    if rows is None or not Ts or len(Ts) > 64 or min(Ts) <= 0:
        return None
    n_rows, row_stride = rows
    L = x.shape[-1]
    if row_stride < L:
        return None
    out = torch.empty(tuple(x.shape[:-1]) + (len(Ts),), dtype=torch.float32, device=x.device)
    arr = (C.c_int * len(Ts))(*Ts)
    _check(load().psh_realized_variance(x.device.index, _stream_ptr(x.device), x.data_ptr(), n_rows, row_stride, L, arr, len(Ts),
                                        1 if vol else 0, out.data_ptr()), "psh_realized_variance")
    return out


PSH_MOMENTS_MAX_LAG = 1024
PSH_MOMENTS_STATUS_ROWS_EXCLUDED = 1


def lagged_moments_workspace_bytes(R: int, m: int, G: int) -> int:
    return _workspace_bytes(load().psh_lagged_moments_workspace_bytes, int(R), int(m), int(G))


def lagged_moments(x: torch.Tensor, m: int, G: int):
    """psh_lagged_moments on a float32 HIP tensor (..., n) whose rows lie a constant stride apart (contiguous, a (R, 1, n)
    ensemble, or a slice of the last dimension of one -- no copy): (sums (G, 4, m + 1) float64, rows_used (G,) int64,
    status (1,) int32), all on the device; nothing is synchronised here."""
    R, row_stride = _strided_rows(x, "x")
    n = x.shape[-1]
    sums = torch.empty((int(G), 4, int(m) + 1), dtype=torch.float64, device=x.device)
    rows_used = torch.empty((int(G),), dtype=torch.int64, device=x.device)
    status = torch.empty((1,), dtype=torch.int32, device=x.device)
    L = load()
    ws = _workspace(L.psh_lagged_moments_workspace_bytes, R, int(m), int(G), device=x.device)
    _check(L.psh_lagged_moments(x.device.index, _stream_ptr(x.device), x.data_ptr(), R, row_stride, n, int(m), int(G),
                                sums.data_ptr(), rows_used.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel() * 8),
           "psh_lagged_moments")
    return sums, rows_used, status


PSH_SCATTERING_MAX_N = 4096
PSH_SCATTERING_STATUS_ROWS_EXCLUDED = 1


def scattering_nout(J: int) -> int:
    """NOUT = 2 J + 2 P3 + 2 P4 of psh_scattering_spectra."""
    return 2 * J + J * (J + 1) + J * (J + 1) * (J + 2) // 3


def scattering_spectra_workspace_bytes(R: int, J: int, G: int) -> int:
    return _workspace_bytes(load().psh_scattering_spectra_workspace_bytes, int(R), int(J), int(G))


def scattering_spectra(x: torch.Tensor, J: int, G: int, psi_hat: torch.Tensor):
    """psh_scattering_spectra on a float32 HIP tensor (..., n) whose rows lie a constant stride apart (contiguous, a
    (R, 1, n) ensemble, or a slice of the last dimension of one -- no copy) with the (J, n / 2) float64 multipliers psi_hat
    on the same device: (sums (G, NOUT) float64, rows_used (G,) int64, status (1,) int32), all on the device; nothing is
    synchronised here."""
    R, row_stride = _strided_rows(x, "x")
    n, J, G = x.shape[-1], int(J), int(G)
    _psi_hat(psi_hat, J, n, x.device)
    L = load()
    ws = _workspace(L.psh_scattering_spectra_workspace_bytes, R, J, G, device=x.device)
    sums = torch.empty((G, scattering_nout(J)), dtype=torch.float64, device=x.device)
    rows_used = torch.empty((G,), dtype=torch.int64, device=x.device)
    status = torch.empty((1,), dtype=torch.int32, device=x.device)
    _check(L.psh_scattering_spectra(x.device.index, _stream_ptr(x.device), x.data_ptr(), R, row_stride, n, J,
                                    psi_hat.data_ptr(), G, sums.data_ptr(), rows_used.data_ptr(), status.data_ptr(),
                                    ws.data_ptr(), ws.numel() * 8), "psh_scattering_spectra")
    return sums, rows_used, status


def scattering_vjp(x: torch.Tensor, J: int, G: int, psi_hat: torch.Tensor, cot: torch.Tensor, out: torch.Tensor | None = None):
    """psh_scattering_vjp on the rows psh_scattering_spectra takes (same x, J, G, psi_hat) with the cotangent cot (G, NOUT)
    float64 of the group sums: (grad (R, n) float64, status (1,) int32) on the device, grad[r] the gradient of
    sum_o cot[group of r][o] out_o(x_r) with respect to row r.  out: a float64 (R, >= n) tensor whose rows lie a constant
    stride apart, written in place on its first n columns (the rest is left untouched).  Nothing is synchronised here."""
    R, row_stride = _strided_rows(x, "x")
    n, J, G = x.shape[-1], int(J), int(G)
    _psi_hat(psi_hat, J, n, x.device)
    nout = scattering_nout(J)
    if not (isinstance(cot, torch.Tensor) and cot.device == x.device and cot.dtype == torch.float64
            and cot.is_contiguous() and tuple(cot.shape) == (G, nout)):
        raise ValueError(f"cot must be a contiguous ({G}, {nout}) float64 tensor on {x.device}")
    if out is None:
        grad, grad_stride = torch.empty((R, n), dtype=torch.float64, device=x.device), n
    else:
        if not (isinstance(out, torch.Tensor) and out.device == x.device and out.dtype == torch.float64 and out.dim() == 2
                and out.shape[0] == R and out.shape[1] >= n and out.stride(1) == 1 and (R == 1 or out.stride(0) >= n)):
            raise ValueError(f"out must be a ({R}, >= {n}) float64 tensor on {x.device}, its last dimension contiguous")
        grad, grad_stride = out[:, :n], (out.stride(0) if R > 1 else max(out.shape[1], n))
    L = load()
    ws = _workspace(L.psh_scattering_vjp_workspace_bytes, R, n, J, G, device=x.device)
    status = torch.empty((1,), dtype=torch.int32, device=x.device)
    _check(L.psh_scattering_vjp(x.device.index, _stream_ptr(x.device), x.data_ptr(), R, row_stride, n, J,
                                psi_hat.data_ptr(), G, cot.data_ptr(), grad.data_ptr(), grad_stride, status.data_ptr(),
                                ws.data_ptr(), ws.numel() * 8), "psh_scattering_vjp")
    return grad, status


def _hmc_inputs(dlnx, weights, Ts, Ms, x_init, rate, degree, kind):
    """The checks hedged_mc and hedge_replay share: (x, Ts, Ms, the arguments both entry points begin with)."""
    x = dlnx
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise NativeLibraryError(f"dlnx must be a tensor on a HIP device (got {type(x).__name__}); there is no CPU path here")
    if x.dtype != torch.float32:
        raise TypeError(f"dlnx must be torch.float32, got {x.dtype}")
    if x.dim() != 3:
        raise ValueError("dlnx must be (B, k, L)")
    B, k, L = x.shape
    rows = _uniform_rows(x)
    if rows is None or rows[1] < L:
        x = x.contiguous()
        rows = _uniform_rows(x)
    w = None
    if weights is not None:
        w = _dev_tensor(weights, torch.float64, "weights")
        if tuple(w.shape) != (B, k):
            raise ValueError(f"weights must be (B, k) = ({B}, {k}), got {tuple(w.shape)}")
        if w.device != x.device:
            raise ValueError("weights and dlnx must be on the same device")
    Ts, Ms = [int(T) for T in Ts], [float(M) for M in Ms]
    nT, nM = len(Ts), len(Ms)
    return x, Ts, Ms, (x.device.index, _stream_ptr(x.device), x.data_ptr(), rows[1], B, k, L, _ptr(w), float(x_init), float(rate),
                       (C.c_int * max(nT, 1))(*Ts), nT, (C.c_double * max(nM, 1))(*Ms), nM, int(degree), int(kind))


def hedged_mc(dlnx: torch.Tensor, weights: torch.Tensor | None, Ts, Ms, x_init: float = 100.0, rate: float = 0.0,
              degree: int = 3, kind: int = PSH_HMC_OTM, policy: bool = False) -> dict:
    """psh_hedged_mc on a float32 HIP tensor of log-returns (B, k, L) whose rows lie a constant stride apart (contiguous,
    or the out-context view `paths[:, :, c, W:]` of gathered paths -- no copy); weights (B, k) float64 or None (uniform).
    Returns device tensors: price / iv / strike (B, nT, nM) float64, sigma (B, nT) float64, status (B,) int32.
    policy=True: psh_hedged_mc_policy, which adds "policy" (B, nT, nM, max Ts, 2 degree + 4) float64 (include/psh.h)."""
    x, Ts, Ms, head = _hmc_inputs(dlnx, weights, Ts, Ms, x_init, rate, degree, kind)
    B, nT, nM = x.shape[0], len(Ts), len(Ms)
    out = {name: torch.empty((B, nT, nM), dtype=torch.float64, device=x.device) for name in ("price", "iv", "strike")}
    out["sigma"] = torch.empty((B, nT), dtype=torch.float64, device=x.device)
    out["status"] = torch.empty((B,), dtype=torch.int32, device=x.device)
    args = head + tuple(out[name].data_ptr() for name in ("price", "iv", "strike", "sigma", "status"))
    if not policy:
        _check(load().psh_hedged_mc(*args), "psh_hedged_mc")
        return out
    n = _workspace_bytes(load().psh_hmc_policy_doubles, B, nT, nM, max(Ts, default=0), int(degree))
    out["policy"] = torch.empty((B, nT, nM, max(Ts), 2 * int(degree) + 4), dtype=torch.float64, device=x.device)
    assert out["policy"].numel() == n
    _check(load().psh_hedged_mc_policy(*args, out["policy"].data_ptr()), "psh_hedged_mc_policy")
    return out


def hedge_replay(dlnx: torch.Tensor, weights: torch.Tensor | None, Ts, Ms, policy: torch.Tensor, strike: torch.Tensor,
                 centre: torch.Tensor, x_init: float = 100.0, rate: float = 0.0, degree: int = 3, kind: int = PSH_HMC_OTM,
                 return_pnl: bool = False) -> dict:
    """psh_hedge_replay: the policy (B, nT, nM, max Ts, 2 degree + 4) of a fit, with the fit's strike and price
    (B, nT, nM) and its x_init, rate, Ts, Ms, degree, kind, replayed on float32 log-returns (B, k', L) (as hedged_mc's; any
    k').  Returns device tensors: sums (B, nT, nM, 9) float64, status (B,) int32, and pnl (B, nT, nM, k') when asked for."""
    x, Ts, Ms, head = _hmc_inputs(dlnx, weights, Ts, Ms, x_init, rate, degree, kind)
    (B, k), nT, nM = x.shape[:2], len(Ts), len(Ms)
    pol = _dev_tensor(policy, torch.float64, "policy").contiguous()
    if tuple(pol.shape) != (B, nT, nM, max(Ts, default=0), 2 * int(degree) + 4):
        raise ValueError(f"policy must be (B, nT, nM, max Ts, 2 degree + 4), got {tuple(pol.shape)}")
    ks = _dev_tensor(strike, torch.float64, "strike").contiguous()
    ce = _dev_tensor(centre, torch.float64, "centre").contiguous()
    if tuple(ks.shape) != (B, nT, nM) or tuple(ce.shape) != (B, nT, nM):
        raise ValueError(f"strike and centre must be (B, nT, nM) = ({B}, {nT}, {nM})")
    if any(t.device != x.device for t in (pol, ks, ce)):
        raise ValueError("policy, strike, centre and dlnx must be on the same device")
    out = {"sums": torch.empty((B, nT, nM, 9), dtype=torch.float64, device=x.device),
           "status": torch.empty((B,), dtype=torch.int32, device=x.device)}
    if return_pnl:
        out["pnl"] = torch.empty((B, nT, nM, k), dtype=torch.float64, device=x.device)
    ws = _workspace(load().psh_hedge_replay_workspace_bytes, B, k, nT, nM, device=x.device)
    _check(load().psh_hedge_replay(*head, pol.data_ptr(), ks.data_ptr(), ce.data_ptr(), out["sums"].data_ptr(), _ptr(out.get("pnl")),
                                   out["status"].data_ptr(), ws.data_ptr(), ws.numel() * 8), "psh_hedge_replay")
    return out


PSH_CAL_MAX_INSTRUMENTS = 32


def calibrate_weights(dlnx: torch.Tensor, prior: torch.Tensor | None, Ts, strike: torch.Tensor, target: torch.Tensor,
                      x_init: float = 100.0, rate: float = 0.0, kind: int = PSH_HMC_OTM, martingale: bool = True,
                      eps: float = 1e-6, tol: float = 1e-8, max_iter: int = 100) -> dict:
    """psh_calibrate_weights on float32 log-returns (B, k, L) (as hedged_mc's: any constant row stride), (B, k) float64 prior
    weights or None, and (B, nT, nM) float64 device strikes and quoted prices (NaN: not quoted).  Returns device tensors:
    weights (B, k), lam and model (B, J), info (B, 4) = [kl, n_eff, steps, max |grad|] float64, status (B,) int32; nothing
    is synchronised here."""
    x, Ts, _, head = _hmc_inputs(dlnx, prior, Ts, [0.0], x_init, rate, 1, kind)
    (B, k), nT = x.shape[:2], len(Ts)
    K = _dev_tensor(strike, torch.float64, "strike")
    c = _dev_tensor(target, torch.float64, "target")
    if K.dim() != 3 or tuple(K.shape[:2]) != (B, nT) or K.shape[2] < 1 or c.shape != K.shape:
        raise ValueError(f"strike and target must be (B, nT, nM) = ({B}, {nT}, nM), got {tuple(K.shape)} and {tuple(c.shape)}")
    if K.device != x.device or c.device != x.device:
        raise ValueError("strike, target and dlnx must be on the same device")
    nM = K.shape[2]
    J = nT * nM + (nT if martingale else 0)
    if k > PSH_MAX_K or J > PSH_CAL_MAX_INSTRUMENTS:
        raise NativeLibraryError(f"psh_calibrate_weights takes k <= {PSH_MAX_K} paths and at most {PSH_CAL_MAX_INSTRUMENTS} "
                                 f"instruments, got k = {k}, J = {J}")
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=x.device)   # noqa: E731
    out = {"weights": f64(B, k), "lam": f64(B, J), "model": f64(B, J), "info": f64(B, 4),
           "status": torch.empty((B,), dtype=torch.int32, device=x.device)}
    ws = _workspace(load().psh_calibrate_workspace_bytes, B, k, max(nT, 1), device=x.device)
    _check(load().psh_calibrate_weights(*head[:12], K.data_ptr(), c.data_ptr(), nM, int(kind), int(bool(martingale)), float(eps),
                                        float(tol), int(max_iter), *(out[n].data_ptr() for n in ("weights", "lam", "model", "info", "status")),
                                        ws.data_ptr(), ws.numel() * 8), "psh_calibrate_weights")
    return out


PDV_OUTPUTS = ("sigma", "St", "dlnx", "raw", "dw")


def pdv_generate(B: int, S: int, n_steps: int, lams1, lams2, decay1, decay2, thetas, betas, S0: float, sqrt_dt: float,
                 nu: float, R10, R20, *, draws: torch.Tensor | None = None, seed: int = 0, outputs=("sigma", "St"),
                 device: torch.device | None = None) -> dict:
    """psh_pdv_generate: S paths of n_steps steps for each of B dates of the discrete PDV model (shadowing_amd/pdv.py).
    lams1 .. thetas: 2 values each, betas: 3 or 4; R10, R20: (B, 2) initial factors (numpy or tensors); draws: (B*S,
    n_steps) float64 device tensor of raw draws, or None: the counter-based generator keyed by `seed`.  Returns a dict of
    the requested `outputs` (of PDV_OUTPUTS) as device tensors: (B*S, n_steps) float64, "dlnx" (B*S, n_steps - 1)
    float32.  Nothing is synchronised."""
    bad = [o for o in outputs if o not in PDV_OUTPUTS]
    if bad:
        raise ValueError(f"unknown outputs {bad}; choose from {PDV_OUTPUTS}")
    if draws is not None:
        draws = _dev_tensor(draws, torch.float64, "draws")
        if tuple(draws.shape) != (B * S, n_steps):
            raise ValueError(f"draws must be ({B * S}, {n_steps}), got {tuple(draws.shape)}")
    dev = draws.device if draws is not None else (device or torch.device("cuda", torch.cuda.current_device()))
    r10, r20 = (torch.as_tensor(R, dtype=torch.float64).to(dev).reshape(B, 2).contiguous() for R in (R10, R20))

    def host(v, n):
        v = [float(x) for x in v]
        if len(v) != n:
            raise ValueError(f"expected {n} values, got {len(v)}")
        return (C.c_double * n)(*v)

    nb = len(betas)
    if nb not in (3, 4):
        raise ValueError(f"betas must hold 3 or 4 values, got {nb}")
    out = {}
    for name in outputs:
        shape, dtype = ((B * S, n_steps - 1), torch.float32) if name == "dlnx" else ((B * S, n_steps), torch.float64)
        out[name] = torch.empty(shape, dtype=dtype, device=dev)
    ptr = lambda name: out[name].data_ptr() if name in out else None   # noqa: E731
    _check(load().psh_pdv_generate(dev.index, _stream_ptr(dev), int(B), int(S), int(n_steps), host(lams1, 2), host(lams2, 2),
                                   host(decay1, 2), host(decay2, 2), host(thetas, 2), host(betas, nb), nb, float(S0),
                                   float(sqrt_dt), float(nu), r10.data_ptr(), r20.data_ptr(),
                                   None if draws is None else draws.data_ptr(), int(seed), ptr("sigma"), ptr("St"),
                                   ptr("dlnx"), ptr("raw"), ptr("dw")), "psh_pdv_generate")
    return out


MRW_OUTPUTS = ("dlnx", "lnx", "omega")
PSH_MRW_MAX_N = 4096


def _dlnx_rows(R: int, n: int, dev, dlnx_out):
    """(tensor, row stride in floats) that takes R rows of n float32 returns: dlnx_out after its checks, or a fresh
    (R, 1, n) tensor."""
    if dlnx_out is None:
        return torch.empty((R, 1, n), dtype=torch.float32, device=dev), n
    if (not isinstance(dlnx_out, torch.Tensor) or dlnx_out.device != dev or dlnx_out.dtype != torch.float32 or
            dlnx_out.dim() < 2 or dlnx_out.shape[0] != R or dlnx_out.shape[-1] < n or dlnx_out.stride(-1) != 1 or
            (R > 1 and dlnx_out.stride(0) < n)):
        raise ValueError(f"dlnx_out must be a float32 tensor on {dev} with {R} rows of >= {n} contiguous floats")
    return dlnx_out, (dlnx_out.stride(0) if R > 1 else n)


def _mrw_generate(entry: str, names, R: int, n: int, tables, m, outputs, dlnx_out):
    """What mrw_generate and smrw_generate share: the output names, M, the tables' checks, the output tensors.  tables:
    (name, tensor, dtype) each, on the first one's device; m: the leverage kernel's lags, or None.  (device, out, row stride)."""
    bad = [o for o in outputs if o not in names]
    if bad:
        raise ValueError(f"unknown outputs {bad}; choose from {names}")
    if n > PSH_MRW_MAX_N:
        raise ValueError(f"{entry} makes paths of n <= {PSH_MRW_MAX_N} returns, got {n}")
    M = 4
    while M < 2 * n:
        M *= 2
    if m is not None and not 1 <= m <= M - n:
        raise ValueError(f"the memory must satisfy 1 <= m <= M - n = {M - n}, got {m}")
    for name, t, dtype in tables:
        _dev_tensor(t, dtype, name)
    dev = tables[0][1].device
    for name, t, _ in tables:
        if tuple(t.shape) != (M,) or t.device != dev:
            raise ValueError(f"{name} must hold M = {M} values on {dev}, got {tuple(t.shape)} on {t.device}")
    out = {}
    stride = n
    if "dlnx" in outputs:
        out["dlnx"], stride = _dlnx_rows(R, n, dev, dlnx_out)
    if "lnx" in outputs:
        out["lnx"] = torch.empty((R, n + 1), dtype=torch.float64, device=dev)
    if names[2] in outputs:
        out[names[2]] = torch.empty((R, n), dtype=torch.float64, device=dev)
    return dev, out, int(stride)


def mrw_generate(R: int, n: int, sigma: float, a_omega: torch.Tensor, a_eps: torch.Tensor | None, c0: float, *,
                 seed: int = 0, outputs=("dlnx",), dlnx_out: torch.Tensor | None = None) -> dict:
    """psh_mrw_generate: R multifractal random walks of n returns (shadowing_amd/mrw.py computes the tables).  a_omega,
    a_eps: (M,) float64 device tensors, M the smallest power of two >= 2n (a_eps None: H = 0.5).  Returns a dict of the
    requested `outputs` (of MRW_OUTPUTS) as device tensors: "dlnx" (R, 1, n) float32, "lnx" (R, n + 1) and "omega" (R, n)
    float64.  dlnx_out: a float32 device tensor (R, ..) whose rows (stride(0) >= n floats apart, unit stride inside) take
    the returns instead of a fresh tensor; whatever lies between the rows is left alone.  Nothing is synchronised."""
    tables = [("a_omega", a_omega, torch.float64)] + ([] if a_eps is None else [("a_eps", a_eps, torch.float64)])
    dev, out, stride = _mrw_generate("psh_mrw_generate", MRW_OUTPUTS, R, n, tables, None, outputs, dlnx_out)
    _check(load().psh_mrw_generate(dev.index, _stream_ptr(dev), int(R), int(n), float(sigma), a_omega.data_ptr(), _ptr(a_eps),
                                   float(c0), int(seed), _ptr(out.get("dlnx")), stride, _ptr(out.get("lnx")),
                                   _ptr(out.get("omega"))), "psh_mrw_generate")
    return out


SMRW_OUTPUTS = ("dlnx", "lnx", "logvol")


def smrw_generate(R: int, n: int, m: int, sigma: float, a_omega: torch.Tensor, k_hat: torch.Tensor, c0: float, v: float, *,
                  seed: int = 0, outputs=("dlnx",), dlnx_out: torch.Tensor | None = None) -> dict:
    """psh_smrw_generate: R skewed multifractal random walks of n returns, m lags of leverage kernel
    (shadowing_amd/mrw.py computes the tables).  a_omega: (M,) float64, k_hat: (M,) complex128 device tensors, M the
    smallest power of two >= 2n, 1 <= m <= M - n.  Returns a dict of the requested `outputs` (of SMRW_OUTPUTS) as device
    tensors: "dlnx" (R, 1, n) float32, "lnx" (R, n + 1) and "logvol" (R, n) float64.  dlnx_out: as mrw_generate.  Nothing
    is synchronised."""
    tables = [("a_omega", a_omega, torch.float64), ("k_hat", k_hat, torch.complex128)]
    dev, out, stride = _mrw_generate("psh_smrw_generate", SMRW_OUTPUTS, R, n, tables, m, outputs, dlnx_out)
    _check(load().psh_smrw_generate(dev.index, _stream_ptr(dev), int(R), int(n), int(m), float(sigma), a_omega.data_ptr(),
                                    k_hat.data_ptr(), float(c0), float(v), int(seed), _ptr(out.get("dlnx")), stride,
                                    _ptr(out.get("lnx")), _ptr(out.get("logvol"))), "psh_smrw_generate")
    return out


def count_nonfinite(x: torch.Tensor) -> int:
    """Number of NaN / +-inf samples of a float32 HIP tensor (one pass, one host synchronisation)."""
    t = _dev_tensor(x, torch.float32, "x")
    out = torch.empty((1,), dtype=torch.int64, device=t.device)
    _check(load().psh_count_nonfinite(t.device.index, _stream_ptr(t.device), t.data_ptr(), t.numel(), out.data_ptr()),
           "psh_count_nonfinite")
    return int(out.item())


def smear_nonfinite(dataset: torch.Tensor, back: int, fwd: int = 0) -> torch.Tensor:
    """(R, T) rows for the scan of an (R, C, T) ensemble that holds non-finite samples: NaN wherever any channel has one
    among the `fwd` samples before and the `back` samples after (the reference's zero-padded conv, see include/psh.h),
    channel 0 elsewhere."""
    ds = _dev_tensor(dataset, torch.float32, "dataset")
    if ds.dim() != 3:
        raise ValueError("dataset must be (R, C, T)")
    R, Cc, T = ds.shape
    out = torch.empty((R, T), dtype=torch.float32, device=ds.device)
    _check(load().psh_smear_nonfinite(ds.device.index, _stream_ptr(ds.device), ds.data_ptr(), R, Cc, T, int(back), int(fwd), out.data_ptr()),
           "psh_smear_nonfinite")
    return out


def rows_nonfinite(dataset: torch.Tensor) -> torch.Tensor:
    """(R,) int32 flags: 1 where a row of the (R, C, T) ensemble holds a NaN / +-inf sample in any channel."""
    ds = _dev_tensor(dataset, torch.float32, "dataset")
    if ds.dim() != 3:
        raise ValueError("dataset must be (R, C, T)")
    R, Cc, T = ds.shape
    out = torch.empty((R,), dtype=torch.int32, device=ds.device)
    _check(load().psh_rows_nonfinite(ds.device.index, _stream_ptr(ds.device), ds.data_ptr(), R, Cc, T, out.data_ptr()),
           "psh_rows_nonfinite")
    return out
