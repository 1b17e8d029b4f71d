"""Which error wins when two apply, for the entry points whose argument checks are shared helpers in psh_capi.hip (the
hedged Monte Carlo family, the two MRW generators, the scattering spectra and their gradient).  Every call fails in the
checks, before a device is touched: no GPU needed.  -1 PSH_ERR_ARG, -2 PSH_ERR_UNSUPPORTED, -3 PSH_ERR_WORKSPACE."""
import ctypes as C

import pytest

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from shadowing_amd import _build, _native
    _build.build()
    return _native.load()


BUF = (C.c_double * 64)()
P = C.addressof(BUF)                               # a non-null pointer no failing call reads


def hmc_head(B=1, k=8, L=30, stride=30, Ts=(5,), Ms=(0.1,), degree=3, kind=0, x_init=100.0, dlnx=P, nT=None, nM=None):
    return [0, None, dlnx, stride, B, k, L, None, x_init, 0.0, (C.c_int * 80)(*Ts), len(Ts) if nT is None else nT,
            (C.c_double * 80)(*Ms), len(Ms) if nM is None else nM, degree, kind]


@pytest.mark.parametrize("kw, want", [
    (dict(degree=6, dlnx=None), ARG),              # a null pointer before an unsupported degree
    (dict(degree=6, Ts=(0,)), UNSUPPORTED),        # the degree before a maturity outside the row
    (dict(k=16385, Ts=(31,)), UNSUPPORTED),        # k > PSH_MAX_K before the maturity
    (dict(nT=65, x_init=-1.0), ARG),
    (dict(B=1 << 10, k=16384, stride=1 << 20, Ms=(float("nan"),)), UNSUPPORTED),   # the size before a strike
    (dict(Ts=(31,)), ARG), (dict(Ms=(float("inf"),)), ARG),
])
def test_hedged_mc_and_policy(lib, kw, want):
    outs = [P] * 5
    assert lib.psh_hedged_mc(*hmc_head(**kw), *outs) == want
    assert lib.psh_hedged_mc_policy(*hmc_head(**kw), *outs, P) == want
    assert lib.psh_hedged_mc_policy(*hmc_head(**kw), *outs, None) == ARG


@pytest.mark.parametrize("kw, ws, want", [
    (dict(degree=6, dlnx=None), 1 << 30, ARG),
    (dict(degree=6, Ts=(0,)), 1 << 30, UNSUPPORTED),
    (dict(k=16385), 0, WORKSPACE),                 # no limit on k here: the replay takes any number of paths
    (dict(B=1 << 10, k=1 << 14, stride=1 << 20, Ts=(31,)), 1 << 30, UNSUPPORTED),
    (dict(Ts=(31,)), 0, ARG),                      # the maturity before the workspace
    (dict(Ts=(30000,), degree=5, L=30000, stride=30000), 0, UNSUPPORTED),   # the policy rows leave LDS, before the workspace
])
def test_hedge_replay(lib, kw, ws, want):
    tail = [P, P, P, P, None, None, P, ws]
    assert lib.psh_hedge_replay(*hmc_head(**kw), *tail) == want
    tail[0] = None
    assert lib.psh_hedge_replay(*hmc_head(**kw), *tail) == ARG


def test_mrw_generators(lib):
    def mrw(R=4, n=100, sigma=0.2, a_omega=P, c0=0.0, out=P, stride=100):
        return lib.psh_mrw_generate(0, None, R, n, sigma, a_omega, None, c0, 5, out, stride, None, None)

    def smrw(R=4, n=100, m=10, sigma=0.2, a_omega=P, k_hat=P, c0=0.0, v=0.0, out=P, stride=100):
        return lib.psh_smrw_generate(0, None, R, n, m, sigma, a_omega, k_hat, c0, v, 5, out, stride, None, None)

    for gen in (mrw, smrw):
        assert gen(n=4097, a_omega=None) == ARG
        assert gen(n=4097, sigma=-1.0) == ARG
        assert gen(n=4097, stride=4096) == ARG
        assert gen(n=4097, stride=4097) == UNSUPPORTED
        assert gen(R=1 << 32, stride=1 << 62) == UNSUPPORTED       # the row count before the overflow of R * stride
        assert gen(R=1 << 20, stride=1 << 62) == ARG
        assert gen(R=1 << 20, stride=1 << 62, out=None) not in (ARG, UNSUPPORTED)   # the stride is read with dlnx only
    assert smrw(n=4097, m=0) == ARG and smrw(n=4097, v=float("nan")) == ARG and smrw(n=4097, k_hat=None) == ARG
    assert smrw(n=4097, stride=4097, m=10 ** 6) == UNSUPPORTED                  # n before the wrap of the convolution
    assert smrw(m=157) == ARG and smrw(m=156) not in (ARG, UNSUPPORTED)             # M - n = 256 - 100


def test_scattering_spectra_and_gradient(lib):
    def spectra(R=8, stride=64, n=64, J=3, G=2, x=P, ws=1 << 30):
        return lib.psh_scattering_spectra(0, None, x, R, stride, n, J, P, G, P, P, None, P, ws)

    def vjp(R=8, stride=64, n=64, J=3, G=2, x=P, gstride=64, ws=1 << 30):
        return lib.psh_scattering_vjp(0, None, x, R, stride, n, J, P, G, P, P, gstride, None, P, ws)

    for fn in (spectra, vjp):
        assert fn(n=8192, stride=8192, x=None) == ARG
        assert fn(n=8192, stride=8191) == ARG
        assert fn(n=8192, stride=8192, J=12) == ARG                # J > log2(n) - 2 before n > the largest row
        assert fn(n=8192, stride=8192, J=11, **({"gstride": 8192} if fn is vjp else {})) == UNSUPPORTED
        assert fn(n=8192, stride=8192, G=9) == ARG
        assert fn(R=1 << 31, G=1 << 20, n=48, stride=48) == ARG    # n no power of two before R
        assert fn(R=1 << 31, G=1 << 20) == UNSUPPORTED
        assert fn(R=1 << 31, G=1 << 20, stride=1 << 62) == UNSUPPORTED              # R before the overflow of R * stride
        assert fn(R=1 << 20, G=2, stride=1 << 62) == ARG
        assert fn(ws=0) == WORKSPACE
    assert vjp(gstride=63, n=8192, stride=8192) == ARG
    out = C.c_size_t(7)
    assert lib.psh_scattering_vjp_workspace_bytes(8, 8192, 3, 2, C.byref(out)) == UNSUPPORTED and out.value == 7
    assert lib.psh_scattering_vjp_workspace_bytes(8, 64, 3, 2, None) == ARG
