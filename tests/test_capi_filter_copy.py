"""psh_filter_copy_bytes (host arithmetic) and the argument checks of psh_filter_copy_build: no device is touched."""
import ctypes as C

import pytest

PSH_ERR_ARG, PSH_ERR_UNSUPPORTED, PSH_ERR_WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from shadowing_amd import _build, _native
    _build.build()
    return _native.load()


def _bytes(lib, R, T):
    n, p = C.c_size_t(0), C.c_int64(0)
    rc = lib.psh_filter_copy_bytes(R, T, C.byref(n), C.byref(p))
    return rc, int(n.value), int(p.value)


@pytest.mark.parametrize("R,T", [(1, 1), (2048, 2048), (3072, 2300), (32768, 4096), (7, 1024), (5, 1025)])
def test_layout_arithmetic(lib, R, T):
    rc, nbytes, pitch = _bytes(lib, R, T)
    assert rc == 0
    # a 16-byte load of the 1024 + 32 halves behind every segment start below T stays inside the row
    last_start = (T - 1) // 1024 * 1024
    assert pitch >= T and pitch >= last_start + 1024 + 32 and pitch % 8 == 0
    assert pitch == (T + 1023) // 1024 * 1024 + 32
    assert nbytes == 64 + R * pitch * 2
    from shadowing_amd import _native
    assert _native.filter_copy_bytes(R, T) == (nbytes, pitch)


def test_bad_arguments(lib):
    n, p = C.c_size_t(0), C.c_int64(0)
    assert lib.psh_filter_copy_bytes(0, 8, C.byref(n), C.byref(p)) == PSH_ERR_ARG
    assert lib.psh_filter_copy_bytes(8, -1, C.byref(n), C.byref(p)) == PSH_ERR_ARG
    assert lib.psh_filter_copy_bytes(8, 8, None, C.byref(p)) == PSH_ERR_ARG
    assert lib.psh_filter_copy_bytes(8, 8, C.byref(n), None) == PSH_ERR_ARG
    assert lib.psh_filter_copy_bytes(8, 1 << 31, C.byref(n), C.byref(p)) == PSH_ERR_UNSUPPORTED
    rc, nbytes, _ = _bytes(lib, 16, 100)
    assert rc == 0
    from shadowing_amd import _native
    scratch = _native.PSH_FILTER_COPY_SCRATCH_BYTES
    ds, out, scr = 0x10000, 0x20000, 0x30000           # never dereferenced: every call below fails its checks first
    build = lib.psh_filter_copy_build
    assert build(0, None, None, 16, 100, out, nbytes, scr, scratch) == PSH_ERR_ARG
    assert build(0, None, ds, 16, 100, None, nbytes, scr, scratch) == PSH_ERR_ARG
    assert build(0, None, ds, 16, 100, out, nbytes, None, scratch) == PSH_ERR_ARG
    assert build(0, None, ds, 0, 100, out, nbytes, scr, scratch) == PSH_ERR_ARG
    assert build(0, None, ds, 16, 100, out, nbytes - 1, scr, scratch) == PSH_ERR_WORKSPACE
    assert build(0, None, ds, 16, 100, out, nbytes, scr, scratch - 1) == PSH_ERR_WORKSPACE
    assert build(0, None, ds, 16, 100, out + 8, nbytes, scr, scratch) == PSH_ERR_ARG      # the copy is read with 16-byte loads


def test_the_library_surface():
    from shadowing_amd import _build, _native
    for name in ("psh_filter_copy_bytes", "psh_filter_copy_build", "psh_scan_topk_copy"):
        assert name in _native.EXPORTS
    assert _build.CSRC / "psh_stream_copy.hip" in _build.SOURCES
    assert _native.PSH_VERSION == 3
