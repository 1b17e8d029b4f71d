"""shadowing_amd.scattering without a GPU: the numpy twin on Gaussian rows (sparsity, power spectrum), on the twins' MRW and
skewed-MRW ensembles (the leverage effect in Im phi3), its time-domain sums against the Fourier-domain forms the kernel uses,
the group partition, the rows left out and the argument checks."""
import functools
import math

import numpy as np
import pytest

import shadowing_amd as sa
from shadowing_amd import scattering

R_ENS, N_ENS, J_ENS = 512, 256, 5


@functools.lru_cache(maxsize=None)
def _spectra(kind, seed):
    """The twin's spectra of a 512 x 256 ensemble at J = 5: computed once per ensemble, shared."""
    if kind == "gauss":
        x = np.random.default_rng(seed).standard_normal((R_ENS, N_ENS)).astype(np.float32)
    elif kind == "smrw":
        x = sa.smrw_log_returns(R_ENS, N_ENS, K0=0.1, alpha=0.6, lam=0.2, seed=seed)
    else:
        x = sa.mrw_log_returns(R_ENS, N_ENS, lam=0.2, seed=seed)
    return sa.scattering_spectra(x, J=J_ENS, cuda=False)


def test_bank_is_the_documented_one():
    bank = sa.scattering_bank(4096, 10)
    assert bank.shape == (10, 2048) and bank.dtype == np.float64
    bands = [(int(np.flatnonzero(row)[0]), int(np.flatnonzero(row)[-1])) for row in bank]
    assert bands == [(513, 2047), (257, 1023), (129, 511), (65, 255), (33, 127), (17, 63), (9, 31), (5, 15), (3, 7), (2, 3)]
    assert np.all(bank[:, 0] == 0.0) and np.all(bank >= 0.0)
    for j in range(1, 11):                                   # zero outside n / 2^(j+2) < k < n / 2^j, one at the centre
        k = np.arange(2048)
        assert np.all(bank[j - 1][(k <= 4096 >> (j + 2)) | (k >= 4096 >> j)] == 0.0)
        assert bank[j - 1][4096 >> (j + 1)] == 1.0
    for j in range(1, 10):                                   # adjacent bands tile the bins between their centres
        k = np.arange(4096 >> (j + 2), (4096 >> (j + 1)) + 1)
        np.testing.assert_allclose(bank[j - 1][k] ** 2 + bank[j][k] ** 2, 1.0, rtol=0, atol=1e-15)
    assert sa.scattering_bank(8, 1).tolist() == [[0.0, 0.0, 1.0, math.cos(0.5 * math.pi * math.log2(1.5))]]


def test_gaussian_rows_have_the_gaussian_sparsity_and_the_banks_power():
    s = _spectra("gauss", 0)
    bank = sa.scattering_bank(N_ENS, J_ENS)
    power = (bank ** 2).sum(axis=1) / N_ENS
    print("phi1 - sqrt(pi)/2:", s.phi1 - math.sqrt(math.pi) / 2, " phi2 / power - 1:", s.phi2 / power - 1.0)
    assert np.all(np.abs(s.phi1 - math.sqrt(math.pi) / 2) < 0.006)
    assert np.all(np.abs(s.phi2 / power - 1.0) < 0.03)
    assert s.n == N_ENS and s.J == J_ENS and s.rows_used == R_ENS and s.rows_excluded == 0
    assert s.phi3.shape == (5, 5) and s.phi4.shape == (5, 5, 5) and np.iscomplexobj(s.phi3) and np.iscomplexobj(s.phi4)
    for j1 in range(5):
        for j2 in range(5):
            assert np.isnan(s.phi3[j1, j2]) == (j1 > j2) and np.isnan(s.phi3_se[j1, j2]) == (j1 > j2)
            for j1p in range(5):
                assert np.isnan(s.phi4[j1, j1p, j2]) == (not j1 <= j1p <= j2)
    assert np.all(s.phi4[np.arange(5), np.arange(5), 4].imag == 0.0)         # C4 is real at j1 = j1'
    assert np.all(s.phi1_se > 0) and np.all(s.phi2_se > 0) and s.group_sums.shape == (64, scattering.n_outputs(5))


@pytest.mark.parametrize("seed", [1, 2])
def test_the_leverage_effect_shows_in_the_imaginary_part_of_phi3(seed):
    skew, sym = _spectra("smrw", seed), _spectra("mrw", seed)
    print(f"seed {seed}: smrw phi3[1,3] = {skew.phi3[0, 2]:.4f} +- {skew.phi3_se[0, 2]:.4f}, mrw {sym.phi3[0, 2]:.4f}, "
          f"mrw phi1 = {sym.phi1}")
    assert skew.phi3[0, 2].imag < -0.015
    assert abs(sym.phi3[0, 2]) < 0.015
    # sparser than a Gaussian (0.79 .. 0.85 measured): below the Gaussian value by more than the 0.006 Gaussian rows scatter
    assert np.all(sym.phi1 < math.sqrt(math.pi) / 2 - 0.006)


@pytest.mark.parametrize("n,J", [(8, 1), (16, 2), (64, 4), (4096, 10)])
def test_time_domain_sums_equal_the_fourier_domain_forms(n, J):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((2, n)) * np.exp(rng.standard_normal((2, n)))).astype(np.float32).astype(np.float64)
    bank = sa.scattering_bank(n, J)
    v = scattering._row_values(x, bank)
    P3, P4 = J * (J + 1) // 2, J * (J + 1) * (J + 2) // 6
    assert v.shape == (2, scattering.n_outputs(J)) and scattering.n_outputs(J) == 2 * J + 2 * P3 + 2 * P4
    psi = np.zeros((J, n))
    psi[:, :n // 2] = bank
    Fx = np.fft.fft(x, axis=-1)
    FU = np.fft.fft(np.abs(np.fft.ifft(Fx[:, None, :] * psi, axis=-1)), axis=-1)
    c3 = v[:, 2 * J:2 * J + P3] + 1j * v[:, 2 * J + P3:2 * J + 2 * P3]
    c4 = v[:, 2 * J + 2 * P3:2 * J + 2 * P3 + P4] + 1j * v[:, 2 * J + 2 * P3 + P4:]
    seen3, seen4, err3, err4 = set(), set(), 0.0, 0.0
    for j2 in range(1, J + 1):
        for j1 in range(1, j2 + 1):
            f3 = (Fx * np.conj(FU[:, j1 - 1]) * psi[j2 - 1] ** 2).sum(axis=-1) / n ** 2
            p3 = scattering.pair_index(j1, j2)
            seen3.add(p3)
            err3 = max(err3, float(np.abs(c3[:, p3] - f3).max()))
            for j1p in range(j1, j2 + 1):
                f4 = (FU[:, j1 - 1] * np.conj(FU[:, j1p - 1]) * psi[j2 - 1] ** 2).sum(axis=-1) / n ** 2
                p4 = scattering.triple_index(j1, j1p, j2)
                seen4.add(p4)
                err4 = max(err4, float(np.abs(c4[:, p4] - f4).max()))
    assert seen3 == set(range(P3)) and seen4 == set(range(P4))               # the index maps are bijections
    print(f"n={n} J={J}: C3 {err3 / np.abs(c3).max():.2e}  C4 {err4 / np.abs(c4).max():.2e} of the largest value")
    assert err3 <= 1e-12 * np.abs(c3).max() and err4 <= 1e-12 * np.abs(c4).max()


def test_group_sums_add_and_bad_rows_are_left_out():
    R, n, J = 23, 64, 3
    rng = np.random.default_rng(5)
    x = rng.standard_normal((R, n)).astype(np.float32)
    one = sa.scattering_spectra(x, J=J, groups=1, cuda=False)
    seven = sa.scattering_spectra(x, J=J, groups=7, cuda=False)
    assert one.group_sums.shape == (1, scattering.n_outputs(J)) and seven.group_sums.shape == (7, scattering.n_outputs(J))
    scale = np.abs(one.group_sums).max()
    np.testing.assert_allclose(seven.group_sums.sum(axis=0), one.group_sums[0], rtol=0, atol=1e-13 * scale)
    from shadowing_amd import stylized
    assert np.array_equal(seven.group_rows, np.diff(stylized.group_bounds(R, 7))) and one.group_rows.tolist() == [R]
    assert np.all(np.isnan(one.phi1_se)) and np.all(np.isfinite(seven.phi1_se))
    np.testing.assert_allclose(seven.phi2, one.phi2, rtol=1e-13)
    # a NaN row and an inf row: excluded and counted; the result is that of the ensemble without them
    bad = x.copy()
    bad[3, 10] = np.nan
    bad[20, 0] = -np.inf
    got = sa.scattering_spectra(bad, J=J, groups=1, cuda=False)
    ref = sa.scattering_spectra(np.delete(x, (3, 20), axis=0), J=J, groups=1, cuda=False)
    assert got.rows_used == R - 2 and got.rows_excluded == 2 and got.group_rows.tolist() == [R - 2]
    np.testing.assert_allclose(got.group_sums, ref.group_sums, rtol=0, atol=1e-13 * scale)
    # every layout, numpy or torch, float64 input rounded to float32 first
    import torch
    for other in (x[:, None, :], torch.from_numpy(x), x.astype(np.float64), torch.from_numpy(x)[:, None, :]):
        assert np.array_equal(sa.scattering_spectra(other, J=J, groups=7, cuda=False).group_sums, seven.group_sums)
    row = sa.scattering_spectra(x[0], J=J, cuda=False)
    assert row.rows_used == 1 and np.array_equal(row.group_sums[0], scattering._row_values(x[:1].astype(np.float64),
                                                                                         sa.scattering_bank(n, J))[0])
    # the caller's own bank
    own = sa.scattering_spectra(x, J=J, groups=7, cuda=False, bank=sa.scattering_bank(n, J))
    assert np.array_equal(own.group_sums, seven.group_sums)
    import shadowing
    assert shadowing.scattering_spectra is sa.scattering_spectra and shadowing.scattering_bank is sa.scattering_bank
    assert shadowing.ScatteringSpectra is sa.ScatteringSpectra


def test_argument_checks():
    x = np.zeros((4, 64), dtype=np.float32)
    assert sa.scattering_spectra(x, cuda=False).J == 4                        # min(log2(n) - 2, 9)
    assert sa.scattering_spectra(np.zeros((2, 4096), dtype=np.float32), cuda=False).J == 9
    assert sa.scattering_spectra(x, cuda=False).group_rows.size == 4          # min(R, 64)
    with pytest.raises(ValueError, match=r"x\[\.\.\., :4096\]"):
        sa.scattering_spectra(np.zeros((2, 5000), dtype=np.float32), cuda=False)
    with pytest.raises(ValueError, match=r"x\[\.\.\., :64\]"):
        sa.scattering_spectra(np.zeros((2, 100), dtype=np.float32), cuda=False)
    with pytest.raises(ValueError, match="at least 8"):
        sa.scattering_spectra(np.zeros((2, 4), dtype=np.float32), cuda=False)
    for J in (0, 5, -1, 2.5, True):
        with pytest.raises(ValueError, match="J must be"):
            sa.scattering_spectra(x, J=J, cuda=False)
    for G in (0, 5, 1.5, True):
        with pytest.raises(ValueError, match="groups"):
            sa.scattering_spectra(x, groups=G, cuda=False)
    with pytest.raises(ValueError, match="x must be"):
        sa.scattering_spectra(np.zeros((2, 2, 64), dtype=np.float32), cuda=False)
    with pytest.raises(ValueError, match="bank"):
        sa.scattering_spectra(x, J=3, bank=np.zeros((3, 64)), cuda=False)
    with pytest.raises(ValueError, match="J must be"):
        sa.scattering_bank(64, 5)
    import torch
    if not torch.cuda.is_available():
        from shadowing_amd import _native
        with pytest.raises(_native.NativeLibraryError):
            sa.scattering_spectra(x, cuda=True)                               # no host fallback
