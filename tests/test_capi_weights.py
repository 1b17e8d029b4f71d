"""The host-only side of psh_softmax_weights on the cross-compiled library (no GPU needed): bad arguments are rejected before
anything touches a device."""
import ctypes as C
import math

import pytest


@pytest.fixture(scope="module")
def lib():
    from shadowing_amd import _build, _native
    _build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _native.load()


def test_bad_arguments_are_rejected_before_the_device_is_touched(lib):
    """Every device pointer here is a made-up address: a call that got past its checks would fault."""
    D, OUT = 0x1000, 0x2000

    def call(distances=D, B=2, k=64, etas=(0.1, 0.2), n_etas=None, ks=(1, 64), n_ks=None, out=OUT):
        ea = None if etas is None else (C.c_double * max(len(etas), 1))(*etas)
        ka = None if ks is None else (C.c_int * max(len(ks), 1))(*ks)
        n_etas = (0 if etas is None else len(etas)) if n_etas is None else n_etas
        n_ks = (1 if ks is None else len(ks)) if n_ks is None else n_ks
        return lib.psh_softmax_weights(0, None, distances, B, k, ea, n_etas, ka, n_ks, out)

    assert call(distances=None) == -1 and call(out=None) == -1                # PSH_ERR_ARG
    assert call(etas=None, n_etas=2) == -1
    for name in ("B", "k", "n_etas", "n_ks"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1, (name, bad)
    assert call(etas=(0.1,) * 13, ks=(1, 2, 3, 4, 5)) == -1                  # 65 sets: more than PSH_SCORE_MAX_SETS
    assert call(etas=(0.1,) * 65, ks=None) == -1
    for bad in (0.0, -0.1, -math.inf, math.nan):
        assert call(etas=(0.1, bad)) == -1, bad                              # an eta that is NaN or not > 0
    for bad in (0, -1, 65):
        assert call(ks=(1, bad)) == -1, bad                                  # a k' outside 1 .. k
    assert call(ks=None, n_ks=2) == -1                                       # NULL ks is the ONE cut-off k
    assert call(k=16385, ks=(1, 16385)) == -2                                # PSH_ERR_UNSUPPORTED: k > PSH_MAX_K
    assert call(k=16385, ks=None) == -2
    assert call(k=16385, etas=(0.1, math.inf), ks=None) == -2                # +infinity is a width: the uniform weighting
    assert call(k=16385, ks=(1, 16386)) == -1                                # the argument errors come first
    assert call(k=16385, etas=(0.0,)) == -1
    assert call(k=16385, out=None) == -1


def test_the_binding_refuses_host_tensors():
    import torch
    from shadowing_amd import _native
    with pytest.raises(_native.NativeLibraryError):
        _native.softmax_weights(torch.zeros(2, 8), [0.1])
