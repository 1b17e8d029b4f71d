"""psh_lagged_moments on the MI355X: against the numpy twin at the bound two orderings of correctly rounded double terms
allow, the row stride and the (R, 1, n) view, bitwise repeatability, rows with NaN / inf, the error codes of the C ABI,
and end to end: an ensemble made on the device measured where it lies, against the closed forms, and fitted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import shadowing_amd as sa
from shadowing_amd import _native, mrw, stylized

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_device")]

LT = 2048                                            # PSH_MOM_TILE, the tile length Lt of psh_moments.hip
# (R, n, m, G): the smallest input; two rows' worth of groups; m = n - 1; the largest lag; one side of a tile boundary each;
# pairs that straddle tiles at every offset (three tiles, the last of 5 samples); more groups asked for than rows (clipped to
# R = 33); a market-length series (ten tiles, one workgroup); more rows than one pass of the grid, groups not dividing R.
# m = 17 and 20, 40 take one lag per lane, 252 and 1024 four (two per lane: m = 100 below, in the non-finite test).
SHAPES = [(1, 1, 0, 1), (3, 2, 1, 2), (5, 33, 32, 5), (7, 1025, 1024, 3), (3, LT - 1, 17, 1), (3, LT + 1, 17, 1),
          (2, 2 * LT + 5, min(1024, LT - 1), 2), (33, 64, 20, 64), (1, 20000, 252, 1), (4099, 96, 40, 64)]


def _ensemble(R, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, n)) * np.exp(0.5 * rng.standard_normal((R, n)))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _twin(R, n, m, G, seed):
    """(x, sums, rows, sums of the summands' absolute values): computed once per shape."""
    x = _ensemble(R, n, seed)
    sums, rows = stylized._host_sums(x, m, G)
    mag, _ = stylized._host_sums(np.abs(x), m, G)
    for a in (x, sums, rows, mag):
        a.setflags(write=False)
    return x, sums, rows, mag


def _check_against_twin(dev_sums, dev_rows, sums, rows, mag, n, what):
    """|dev - twin| <= 2 (N + 2) 2^-53 sum|summand| per element, N the pair count of that sum: the worst case for two
    orderings of N correctly rounded double terms, each carrying at most one product rounding."""
    assert np.array_equal(dev_rows, rows)
    N = rows[:, None, None] * (n - np.arange(sums.shape[2]))[None, None, :]
    bound = 2.0 * (N + 2) * 2.0 ** -53 * mag
    err = np.abs(dev_sums - sums)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))
    print(f"{what}: max |dev - twin| / bound = {ratio:.3e}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("R,n,m,G", SHAPES)
def test_device_matches_twin(R, n, m, G):
    G = min(G, R)
    x, sums, rows, mag = _twin(R, n, m, G, 100 + n)
    d_sums, d_rows, status = _native.lagged_moments(torch.tensor(x).cuda(), m, G)     # (x is read-only: a copy)
    assert d_sums.shape == (G, 4, m + 1) and d_sums.dtype == torch.float64 and d_rows.dtype == torch.int64
    assert int(status.item()) == 0
    _check_against_twin(d_sums.cpu().numpy(), d_rows.cpu().numpy(), sums, rows, mag, n, f"R={R} n={n} m={m} G={G}")
    assert np.array_equal(d_rows.cpu().numpy(), np.diff(stylized.group_bounds(R, G)))
    s = d_sums.cpu().numpy()
    assert np.array_equal(s[:, 1, 0], s[:, 2, 0])    # both are the third moment at lag 0


def test_row_stride_and_the_ensemble_view_give_the_bits_of_the_contiguous_call():
    R, n, m, G = 9, LT + 77, 130, 4
    wide = torch.from_numpy(_ensemble(R, n + 13, 5)).cuda()
    view = wide[:, :n]
    flat = view.contiguous()
    assert view.stride(0) == n + 13 and not view.is_contiguous()
    ref = _native.lagged_moments(flat, m, G)
    for other in (_native.lagged_moments(view, m, G), _native.lagged_moments(flat.reshape(R, 1, n), m, G),
                  _native.lagged_moments(flat, m, G)):                     # ... and two calls give identical bits
        assert torch.equal(other[0].view(torch.int64), ref[0].view(torch.int64))
        assert torch.equal(other[1], ref[1]) and int(other[2].item()) == 0
    mom = sa.lagged_moments(flat.reshape(R, 1, n), m, groups=G)
    assert np.array_equal(mom.group_sums, ref[0].cpu().numpy()) and mom.rows_used == R


def test_rows_with_nan_or_inf_are_left_out():
    """A NaN at the first sample, an inf at the last, a NaN in the first tile's halo (the samples the second tile owns):
    none of these rows adds anything, the status bit is set, and the result is the twin's."""
    R, n, m, G = 7, 2 * LT + 100, 100, 2
    x = _ensemble(R, n, 9)
    x[1, 0] = np.nan
    x[2, n - 1] = np.inf
    x[4, LT + 5] = np.nan
    x[5, LT - 1] = -np.inf
    sums, rows = stylized._host_sums(x, m, G)
    mag, _ = stylized._host_sums(np.abs(x), m, G)               # (|x| leaves the same rows out)
    d_sums, d_rows, status = _native.lagged_moments(torch.from_numpy(x).cuda(), m, G)
    assert int(status.item()) & _native.PSH_MOMENTS_STATUS_ROWS_EXCLUDED
    assert rows.tolist() == [1, 2] and np.isfinite(d_sums.cpu().numpy()).all()
    _check_against_twin(d_sums.cpu().numpy(), d_rows.cpu().numpy(), sums, rows, mag, n, "non-finite rows")
    # a group with no row left: sums 0, rows_used 0
    x[0, 7] = np.nan
    d_sums, d_rows, status = _native.lagged_moments(torch.from_numpy(x).cuda(), m, G)
    assert d_rows.tolist() == [0, 2] and torch.all(d_sums[0] == 0.0) and int(status.item()) == 1
    mom = sa.lagged_moments(torch.from_numpy(x).cuda(), m, groups=G)
    twin = sa.lagged_moments(x, m, groups=G, cuda=False)
    assert mom.rows_used == twin.rows_used == 2 and mom.rows_excluded == 5 and np.all(np.isnan(mom.xx_se))
    np.testing.assert_allclose(mom.xx2, twin.xx2, rtol=1e-12, atol=1e-300)


def test_the_error_codes_of_the_c_abi():
    L = _native.load()
    x = torch.zeros(4 * 2048, dtype=torch.float32, device="cuda")
    out = torch.zeros(4 * 4 * 1025, dtype=torch.float64, device="cuda")
    rows = torch.zeros(4, dtype=torch.int64, device="cuda")
    nbytes = C.c_size_t(0)
    assert L.psh_lagged_moments_workspace_bytes(4, 1024, 4, C.byref(nbytes)) == 0
    assert nbytes.value == 4 * (4 * 1025 * 8 + 8)
    ws = torch.zeros(nbytes.value // 8, dtype=torch.int64, device="cuda")
    X, O, RW, W = x.data_ptr(), out.data_ptr(), rows.data_ptr(), ws.data_ptr()
    call = lambda x_, R, stride, n, m, G, o=O, rw=RW, w=W, nb=nbytes.value: L.psh_lagged_moments(   # noqa: E731
        0, None, x_, R, stride, n, m, G, o, rw, None, w, nb)
    assert call(X, 4, 2048, 2048, 1024, 4) == 0
    assert call(X, 4, 2048, 2048, 1025, 4) == -2                 # m > 1024: PSH_ERR_UNSUPPORTED
    assert call(None, 4, 2048, 2048, 40, 4) == -1
    assert call(X, 4, 2048, 2048, 40, 4, o=None) == -1
    assert call(X, 4, 2048, 2048, 40, 4, rw=None) == -1
    assert call(X, 4, 2048, 2048, 40, 4, w=None) == -1
    assert call(X, 0, 2048, 2048, 40, 1) == -1
    assert call(X, 4, 2048, 0, 0, 4) == -1
    assert call(X, 4, 2047, 2048, 40, 4) == -1                   # row_stride < n
    assert call(X, 4, 2048, 2048, -1, 4) == -1
    assert call(X, 4, 2048, 41, 41, 4) == -1                     # m >= n
    assert call(X, 4, 2048, 2048, 40, 0) == -1
    assert call(X, 4, 2048, 2048, 40, 5) == -1                   # G > R
    assert call(X, 4, 2048, 2048, 1024, 4, nb=nbytes.value - 1) == -3
    assert L.psh_lagged_moments_workspace_bytes(4, 1025, 4, C.byref(nbytes)) == -2
    assert L.psh_lagged_moments_workspace_bytes(4, 40, 5, C.byref(nbytes)) == -1
    assert L.psh_lagged_moments_workspace_bytes(4, 40, 4, None) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="1024"):
        sa.lagged_moments(x.reshape(4, 2048), 1025)
    with pytest.raises(ValueError, match="groups"):
        sa.lagged_moments(x.reshape(4, 2048), 40, groups=5)


def test_an_ensemble_made_on_the_device_is_measured_where_it_lies_and_fitted(monkeypatch):
    R, n, K0, alpha, lam = 8192, 512, 0.1, 0.6, 0.2
    ens = sa.smrw_log_returns(R, n, K0, alpha, lam=lam, sigma=1.0, seed=11, cuda=True)
    assert isinstance(ens, torch.Tensor) and ens.is_cuda and ens.shape == (R, 1, n)
    copied = []
    to_host = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copied.append(self.numel()), to_host(self, *a, **k))[1])
    mom = sa.lagged_moments(ens, 40)
    fit = sa.fit_smrw(ens, max_lag=40)
    monkeypatch.undo()
    assert copied and max(copied) <= 64 * 4 * 41, copied     # only the (G, 4, m + 1) sums and the row counts cross
    assert mom.rows_used == R and mom.rows_excluded == 0 and abs(mom.variance - 1.0) < 0.05
    for tau in (1, 2, 5, 20):
        lev = mrw.smrw_leverage(tau, n, K0, alpha, lam=lam, sigma=1.0)
        sq = mrw.smrw_sq_moment(tau, n, K0, alpha, lam=lam, sigma=1.0)
        z1, z2 = (mom.xx2[tau] - lev) / mom.xx2_se[tau], (mom.x2x2[tau] - sq) / mom.x2x2_se[tau]
        print(f"tau={tau}: xx2 {mom.xx2[tau]:+.5f} closed form {lev:+.5f} z {z1:+.2f}; x2x2 {mom.x2x2[tau]:.4f} closed form "
              f"{sq:.4f} z {z2:+.2f}")
        assert abs(z1) <= 6.0 and abs(z2) <= 6.0
    host = sa.fit_smrw(ens.cpu().numpy(), max_lag=40, cuda=False)
    for name in ("sigma", "lam", "K0", "alpha"):
        print(f"{name}: device {fit[name]:.12g} host {host[name]:.12g} +- {fit['stderr'][name]:.3g}")
        assert fit[name] == pytest.approx(host[name], rel=1e-9)
    again = sa.smrw_log_returns(4, n, cuda=True, seed=3, **{k: fit["params"][k] for k in ("K0", "alpha", "lam", "sigma")})
    assert again.is_cuda and again.shape == (4, 1, n)


# ---- integer ensembles: the device equals an int64 reference exactly, on every plan of moments_lag_plan ----
import _moments_exact as mx                                                     # noqa: E402


def _device_sums(x, m, G):
    d_sums, d_rows, status = _native.lagged_moments(torch.from_numpy(np.ascontiguousarray(x)).cuda(), m, G)
    assert int(status.item()) == 0
    return d_sums.cpu().numpy(), d_rows.cpu().numpy()


@pytest.mark.parametrize("shape", mx.census_shapes(), ids=mx.census_id)
def test_device_equals_the_int64_reference_on_every_plan(shape):
    """The plan census of tests/_moments_exact.py: every (U, C, S), both sides of each boundary of m, a second tile of
    m + 3 samples behind a full one and a single tile of m + 1.  Integer samples: == , no tolerance."""
    R, n, m, G = shape
    x = mx.int_ensemble(R, n, 7)
    s, rows = _device_sums(x, m, G)
    assert s.shape == (G, 4, m + 1) and np.array_equal(s, mx.int_sums(x, m, G).astype(np.float64))
    assert np.array_equal(rows, np.diff(stylized.group_bounds(R, G))) and np.array_equal(s[:, 1, 0], s[:, 2, 0])


@pytest.mark.parametrize("m", mx.PLANT_M, ids=[f"m{m}-U{mx.lag_plan(m)[0]}C{mx.lag_plan(m)[1]}S{mx.lag_plan(m)[2]}" for m in mx.PLANT_M])
def test_device_finds_every_impulse_plant_exactly(m):
    """One pair a row (2 at t1, 3 at t1 + tau) at the row's ends, across the tile boundary from both sides, in the ragged
    last tile and on both sides of every slice boundary of the first tile: (6, 18, 12, 36) at lag tau, (13, 35, 35, 97) at
    lag 0 and 0 at every other lag.  A failure names the plants."""
    x, want = mx.plants(m)
    s, rows = _device_sums(x, m, len(x))
    bad = [mx.plant_positions(m)[i] for i in np.flatnonzero((s != want.astype(np.float64)).any(axis=(1, 2)))]
    assert not bad, f"plants (t1, tau) with wrong sums: {bad}"
    assert np.array_equal(rows, np.ones(len(x), np.int64))


def test_partition_invariance_is_exact_on_integers_on_the_device():
    """37 rows x 300 at m = 70: the sums added over the groups are bit-identical for 1, 2, 5 and 37 groups (2 and 5:
    groups of unequal size, and units that hold no row)."""
    x = mx.int_ensemble(37, 300, 11)
    total = mx.int_sums(x, 70, 1)[0].astype(np.float64)
    for G in (1, 2, 5, 37):
        s, rows = _device_sums(x, 70, G)
        assert np.array_equal(s, mx.int_sums(x, 70, G).astype(np.float64)), G
        assert np.array_equal(s.sum(axis=0), total) and np.array_equal(rows, np.diff(stylized.group_bounds(37, G)))
