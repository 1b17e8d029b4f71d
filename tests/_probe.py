"""The probe library of the shared device primitives -- TEST INFRASTRUCTURE ONLY.

tests/csrc/psh_probe.hip wraps each primitive of psh_wave.h, psh_sort_lds.h and psh_long.h (and fast_div, unit_queue) in a thin
kernel; this module builds it with the product's flags into tests/csrc/lib/libpsh_probe.so and binds it with ctypes.
Nothing in shadowing_amd/ imports, links or loads it, and libpsh_hip.so exports none of its symbols
(tests/test_wave_twin_cpu.py holds both).  The same rules as the product's library: `build()` compiles when the
content hash of the sources differs, `load()` refuses a missing or stale library and never builds implicitly.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
if str(HERE.parent) not in sys.path:          # `python tests/_probe.py` from anywhere
    sys.path.insert(0, str(HERE.parent))

from shadowing_amd import _build  # noqa: E402

SOURCE = HERE / "csrc" / "psh_probe.hip"
LIBDIR = HERE / "csrc" / "lib"
LIB = LIBDIR / "libpsh_probe.so"
# what the probe is built from: its source and the five headers it includes by name (psh_kernels.h comes in through
# psh_device.h and holds argument blocks only)
HEADERS = [_build.CSRC / "psh_wave.h", _build.CSRC / "psh_sort_lds.h", _build.CSRC / "psh_device.h", _build.CSRC / "psh_segment.h", _build.CSRC / "psh_long.h"]
DEPS = [SOURCE] + HEADERS
PROBE_VERSION = 2

# wave / block_reduce operand types and operations (the enums of psh_probe.hip)
F32, F64, I32, U32 = 0, 1, 2, 3
SUM, MIN, MAX, OR, MINMAX, SCAN = 0, 1, 2, 3, 4, 5
DPP_MAX_NONNEG, DPP_SUM, DPP_SCAN, DPP_TOTAL = 0, 1, 2, 3
# psh_probe_long: the piece, and the ints of a case's parameter block
L_STAGE0, L_STAGE2, L_OPERAND_LO, L_OPERAND_HI, L_TILE_MIN, L_TABLES, L_EXACT_SCALAR, L_EXACT_VECTOR, L_BOUND, L_ZERO = range(10)
LONG_PARAMS = 136


class ProbeLibraryError(RuntimeError):
    """The probe library is missing, stale or failed."""


def _signatures() -> dict:
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    return {
        "psh_probe_version": [],
        "psh_probe_wave": [i32, i32, vp, vp, vp, vp, i64, vp],
        "psh_probe_dpp": [i32, vp, vp, i64, vp],
        "psh_probe_block_reduce": [i32, i32, i32, i32, vp, vp, vp, vp, i32, vp],
        "psh_probe_rank": [i32, vp, i32, vp, i32, i32, vp, vp],
        "psh_probe_bucket_edge": [vp, vp, vp, vp, vp, i64, vp],
        "psh_probe_key": [vp, vp, vp, i64, vp],
        "psh_probe_sort": [i32, vp, vp, i32, i32, vp],
        "psh_probe_scan": [i32, i32, vp, vp, vp, vp, vp, vp, i32, vp],
        "psh_probe_fast_div": [vp, vp, vp, vp, i64, vp],
        "psh_probe_unit_queue": [vp, i32, vp, vp, i32, vp],
        "psh_probe_long": [i32, vp, vp, vp, vp, i32, vp],
    }


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


def source_hash() -> str:
    """SHA-256 over the probe's source, the five headers and the flags (names + contents), as _build.source_hash."""
    h = hashlib.sha256()
    for p in DEPS:
        h.update(p.name.encode())
        h.update(p.read_bytes())
    h.update(" ".join(_build.HIPCC_FLAGS).encode())
    return h.hexdigest()


def _stamp(lib: Path) -> Path:
    return lib.with_suffix(lib.suffix + ".srchash")


def is_stale(lib: Path | None = None) -> bool:
    """True when `lib` is missing or was built from other bytes than the ones in the tree."""
    lib = lib or LIB
    stamp = _stamp(lib)
    if not lib.exists() or not stamp.exists():
        return True
    return stamp.read_text().strip() != source_hash()


def command(lib: Path) -> list[str]:
    """The one hipcc line: exactly _build.HIPCC_FLAGS, the product's include directories, nothing else."""
    return [_build.hipcc_path(), *_build.HIPCC_FLAGS, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", str(SOURCE), "-o", str(lib)]


def build(force: bool = False, lib: Path | None = None) -> Path:
    lib = lib or LIB
    if not force and not is_stale(lib):
        return lib
    lib.parent.mkdir(parents=True, exist_ok=True)
    res = subprocess.run(command(lib), capture_output=True, text=True)
    if res.returncode != 0:
        raise ProbeLibraryError(f"hipcc failed on {SOURCE.name}:\n{res.stdout}\n{res.stderr}")
    _stamp(lib).write_text(source_hash() + "\n")
    return lib


_lib = None


def load() -> C.CDLL:
    """dlopen tests/csrc/lib/libpsh_probe.so; a missing or stale library is an error, never a build."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB.exists():
        raise ProbeLibraryError(f"{LIB} is missing: build it with `python tests/_probe.py` (or __graft_entry__.build())")
    if is_stale():
        raise ProbeLibraryError(f"{LIB} was built from other sources than {SOURCE.name} and the headers in the tree "
                                "(content hash differs): rebuild it with `python tests/_probe.py`")
    try:
        L = C.CDLL(str(LIB))
    except OSError as e:  # pragma: no cover
        raise ProbeLibraryError(f"cannot load {LIB}: {e}") from e
    for name, argtypes in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = C.c_int, argtypes
    if L.psh_probe_version() != PROBE_VERSION:
        raise ProbeLibraryError(f"{LIB} is version {L.psh_probe_version()} of the probe, this binding {PROBE_VERSION}")
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise ProbeLibraryError(f"{what}: the probe returned {rc} (-1: a shape it does not take, else a hipError_t)")


# ---- plumbing of the GPU tests: device memory is torch's, words travel as int32 / int64 whatever they mean
def dev(a):
    """A device tensor holding the bytes of a numpy array of 4- or 8-byte words."""
    import numpy as np
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32 if a.dtype.itemsize == 4 else np.int64).copy()).cuda()


def words(n: int, itemsize: int = 4, fill: int = 0):
    """n device words of 4 or 8 bytes, every one `fill` (-1: all bits set)."""
    import torch
    return torch.full((int(n),), fill, dtype=torch.int32 if itemsize == 4 else torch.int64, device="cuda")


def host(t, dtype):
    """The words of a device tensor as a numpy array of `dtype`."""
    return t.cpu().numpy().view(dtype)


def stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


if __name__ == "__main__":
    print(build(force=True))
