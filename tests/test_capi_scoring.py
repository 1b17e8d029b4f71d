"""The host-only side of psh_score_ensemble on the cross-compiled library (no GPU needed): bad arguments are rejected before
anything touches a device."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from shadowing_amd import _build, _native
    _build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _native.load()


def test_bad_arguments_are_rejected_before_the_device_is_touched(lib):
    """Every device pointer here is a made-up address: a call that got past its checks would fault."""
    V, W, Y, CR, LO, HI, MU, ST = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000

    def call(values=V, weights=W, obs=Y, B=2, k=64, m=3, n_sets=4, crps=CR, pit_lo=LO, pit_hi=HI, mean=MU, status=ST):
        return lib.psh_score_ensemble(0, None, values, weights, obs, B, k, m, n_sets, crps, pit_lo, pit_hi, mean, status)

    for name in ("values", "obs", "crps", "pit_lo", "pit_hi", "mean"):
        assert call(**{name: None}) == -1, name                  # PSH_ERR_ARG (status may be NULL)
    for name in ("B", "k", "m", "n_sets"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1, (name, bad)
    assert call(n_sets=65) == -1                                 # more than PSH_SCORE_MAX_SETS
    assert call(weights=None, n_sets=2) == -1 and call(weights=None, n_sets=64) == -1      # NULL weights are ONE set
    assert call(k=16385) == -2                                   # PSH_ERR_UNSUPPORTED: k > PSH_MAX_K
    assert call(k=16385, weights=None, n_sets=1, status=None) == -2
    assert call(B=1 << 16, m=1 << 15) == -2                      # one workgroup per column: B * m < 2^31
    assert call(k=16385, n_sets=65) == -1                        # the argument errors come first
    assert call(k=16385, weights=None, n_sets=2) == -1
    assert call(B=1 << 16, m=1 << 15, obs=None) == -1


def test_the_binding_refuses_host_tensors_and_cuda_true_has_no_fallback():
    import torch
    from shadowing_amd import _native
    with pytest.raises(_native.NativeLibraryError):
        _native.score_ensemble(torch.zeros(1, 4, 1), None, torch.zeros(1, 1))
    import shadowing_amd as sa
    if not torch.cuda.is_available():
        with pytest.raises(_native.NativeLibraryError):
            sa.score_ensemble(torch.zeros(1, 4, 1).numpy(), None, torch.zeros(1, 1).numpy(), cuda=True)
    with pytest.raises(_native.NativeLibraryError):
        sa.score_ensemble(torch.zeros(1, 16385, 1).numpy(), None, torch.zeros(1, 1).numpy(), cuda=True)   # k > PSH_MAX_K
