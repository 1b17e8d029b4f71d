"""The host-only side of psh_separate_topk on the cross-compiled library (no GPU needed): bad arguments are rejected before
anything touches a device."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from shadowing_amd import _build, _native
    _build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _native.load()


def test_bad_arguments_are_rejected_before_the_device_is_touched(lib):
    """Every device pointer here is a made-up address: a call that got past its checks would fault."""
    ptrs = dict(d=0x1000, idx=0x2000, out_d=0x3000, out_idx=0x4000, out_pos=0x5000, out_count=0x6000, out_status=0x7000)

    def call(B=2, K=64, k=16, delta=3, **kw):
        p = {**ptrs, **kw}
        return lib.psh_separate_topk(0, None, p["d"], p["idx"], B, K, k, delta, p["out_d"], p["out_idx"], p["out_pos"],
                                     p["out_count"], p["out_status"])

    for name in ptrs:
        assert call(**{name: None}) == -1, name                                # PSH_ERR_ARG
    for name in ("B", "K", "k"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1, (name, bad)
    assert call(delta=-1) == -1
    assert call(K=64, k=65) == -1                                             # k > K
    assert call(K=16385, k=16) == -2                                          # PSH_ERR_UNSUPPORTED: K > PSH_MAX_K
    assert call(K=16385, k=16385) == -2
    assert call(K=16385, k=16386) == -1                                       # the argument errors come first
    assert call(K=16385, delta=-1) == -1
    assert call(K=16385, B=0) == -1
    assert call(K=16385, out_pos=None) == -1


def test_the_header_names_the_status_constant():
    from pathlib import Path
    import re
    from shadowing_amd import _native
    text = (Path(__file__).resolve().parent.parent / "include" / "psh.h").read_text()
    assert re.search(r"#define PSH_SEPARATE_STATUS_SHORT\s+1\b", text) and _native.PSH_SEPARATE_STATUS_SHORT == 1
    assert re.search(r"#define PSH_VERSION 3\b", text)


def test_the_binding_refuses_host_tensors():
    import torch
    from shadowing_amd import _native
    with pytest.raises(_native.NativeLibraryError):
        _native.separate_topk(torch.zeros(2, 8), torch.zeros(2, 8, 2, dtype=torch.int32), 4, 1)
