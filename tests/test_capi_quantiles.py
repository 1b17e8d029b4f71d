"""The host-only side of psh_weighted_quantiles on the cross-compiled library (no GPU needed): bad arguments are rejected
before anything touches a device."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from shadowing_amd import _build, _native
    _build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _native.load()


def test_bad_arguments_are_rejected_before_the_device_is_touched(lib):
    """Every device pointer here is a made-up address: a call that got past its checks would fault."""
    V, W, Q, LO, UP, ST = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    half = (C.c_double * 1)(0.5)
    keep = []

    def call(values=V, weights=W, B=2, k=64, m=3, levels=(0.05, 0.5, 0.95), n_levels=None, q=Q, lower=LO, upper=UP, status=ST):
        arr = None
        if levels is not None:
            arr = (C.c_double * max(len(levels), 1))(*levels)
            keep.append(arr)
        n = (len(levels) if levels is not None else 1) if n_levels is None else n_levels
        return lib.psh_weighted_quantiles(0, None, values, weights, B, k, m, arr, n, q, lower, upper, status)

    for name in ("values", "levels", "q", "lower", "upper"):
        assert call(**{name: None}) == -1, name                  # PSH_ERR_ARG (weights and status may be NULL)
    for name in ("B", "k", "m"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1, (name, bad)
    assert call(n_levels=0) == -1 and call(n_levels=-1) == -1
    assert call(levels=tuple(0.01 * (i + 1) for i in range(33))) == -1           # more than PSH_QUANTILE_MAX_LEVELS
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf"), -float("inf")):
        assert call(levels=(0.5, bad)) == -1, bad
        assert call(levels=(bad,)) == -1, bad
    assert call(k=16385) == -2                                   # PSH_ERR_UNSUPPORTED: k > PSH_MAX_K
    assert call(k=16385, weights=None, status=None) == -2
    assert call(B=1 << 16, m=1 << 15) == -2                      # one workgroup per column: B * m < 2^31
    assert call(k=16385, levels=(2.0,)) == -1                    # the argument errors come first
    assert lib.psh_weighted_quantiles(0, None, V, None, 1, 1, 1, half, 1, Q, LO, None, None) == -1


def test_the_binding_refuses_host_tensors_and_bad_levels():
    import torch
    from shadowing_amd import _native
    with pytest.raises(_native.NativeLibraryError):
        _native.weighted_quantiles(torch.zeros(1, 4, 1), None, [0.5])
    import shadowing_amd as sa
    if not torch.cuda.is_available():
        with pytest.raises(_native.NativeLibraryError):
            sa.weighted_quantiles(torch.zeros(1, 4, 1).numpy(), None, [0.5], cuda=True)
    with pytest.raises(_native.NativeLibraryError):
        sa.weighted_quantiles(torch.zeros(1, 16385, 1).numpy(), None, [0.5], cuda=True)      # k > PSH_MAX_K on the device
