"""The host-only side of psh_scattering_spectra on the cross-compiled library (no GPU needed): the workspace size, and bad
arguments rejected before anything touches a device."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from shadowing_amd import _build, _native
    _build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _native.load()


def test_workspace_bytes(lib):
    from shadowing_amd import _native
    out = C.c_size_t(0)
    assert lib.psh_scattering_spectra_workspace_bytes(32768, 9, 64, C.byref(out)) == 0
    assert out.value == 64 * 16 * (438 * 8 + 8)              # 16 units per group, NOUT = 438 at J = 9
    assert lib.psh_scattering_spectra_workspace_bytes(9, 1, 2, C.byref(out)) == 0
    assert out.value == 2 * 5 * (6 * 8 + 8)                  # ceil(9 / 2) = 5 units per group, NOUT = 6 at J = 1
    assert lib.psh_scattering_spectra_workspace_bytes(1, 10, 1, C.byref(out)) == 0 and out.value == 570 * 8 + 8
    assert _native.scattering_spectra_workspace_bytes(32768, 9, 64) == 64 * 16 * (438 * 8 + 8)
    assert [_native.scattering_nout(J) for J in (1, 2, 9, 10)] == [6, 18, 438, 570]
    assert lib.psh_scattering_spectra_workspace_bytes(4, 3, 4, None) == -1              # PSH_ERR_ARG
    assert lib.psh_scattering_spectra_workspace_bytes(0, 3, 1, C.byref(out)) == -1
    assert lib.psh_scattering_spectra_workspace_bytes(4, 0, 4, C.byref(out)) == -1
    assert lib.psh_scattering_spectra_workspace_bytes(4, 3, 0, C.byref(out)) == -1
    assert lib.psh_scattering_spectra_workspace_bytes(4, 3, 5, C.byref(out)) == -1      # G > R
    assert lib.psh_scattering_spectra_workspace_bytes(4, 11, 4, C.byref(out)) == -2     # only n > 4096 admits J = 11
    assert lib.psh_scattering_spectra_workspace_bytes(1 << 31, 3, 4, C.byref(out)) == -2
    with pytest.raises(ValueError):
        _native.scattering_spectra_workspace_bytes(4, 3, 5)


def test_bad_arguments_are_rejected_before_the_device_is_touched(lib):
    """Every pointer here is a made-up address: a call that got past its checks would fault."""
    X, P, O, RW, W = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000

    def call(x=X, R=4, stride=256, n=256, J=6, psi=P, G=4, out=O, rows=RW, ws=W, nb=1 << 30):
        return lib.psh_scattering_spectra(0, None, x, R, stride, n, J, psi, G, out, rows, None, ws, nb)

    for name in ("x", "psi", "out", "rows", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(R=0, G=1) == -1
    for n in (0, 4, 7, 12, 255, 257, -256):
        assert call(n=n, stride=4096, J=1) == -1, n          # not a power of two, or below 8
    assert call(stride=255) == -1                            # row_stride < n
    assert call(J=0) == -1 and call(J=-1) == -1
    assert call(J=7) == -1                                   # J > log2(256) - 2
    assert call(n=8, stride=8, J=2) == -1
    assert call(G=0) == -1 and call(G=5) == -1
    assert call(n=8192, stride=8192, J=9) == -2              # PSH_ERR_UNSUPPORTED: the transforms leave LDS
    assert call(n=8192, stride=8192, J=11) == -2
    assert call(n=8192, stride=8192, J=12) == -1             # J > log2(8192) - 2
    assert call(R=1 << 31, G=4) == -2
    assert call(R=(1 << 31) - 1, stride=1 << 40, G=4) == -1  # R * row_stride past int64
    assert call(nb=4 * (146 * 8 + 8) - 1) == -3              # PSH_ERR_WORKSPACE: 4 units, NOUT = 146 at J = 6
    assert call(nb=0) == -3
