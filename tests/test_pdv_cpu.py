"""The PDV model on the host (shadowing_amd.pdv; no GPU): against the reference's own outputs (tests/golden/pdv_*.npz,
tests/golden/make_golden_pdv.py), the Philox4x32-10 known answers, the predictor against sklearn, the deliberate
deviations (3-beta compute_factor), argument errors, the drop-in import path and psh_pdv_generate's argument checks."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from shadowing_amd import pdv

GOLDEN = Path(__file__).resolve().parent / "golden"
DT = 1 / 252
GEN_CASES = ["disc_b3_gauss_T75", "disc_b4_gauss_T1", "disc_b3_t3_T1", "disc_b4_t3_T75", "disc_clip", "disc_floor",
             "disc_nan", "cont_gauss"]
PRED_CASES = ["exp_plain", "exp_extra", "powerlaw_plain", "powerlaw_extra"]


def load(name):
    with np.load(GOLDEN / f"pdv_{name}.npz") as z:
        return {k: z[k] for k in z.files}


def model_of(g, cls=None):
    cls = cls or (pdv.PDVModel if bool(g.get("continuous", False)) else pdv.PDVModelDiscrete)
    nu = float(g.get("nu", 0.0))
    return cls(g["lams1"], g["lams2"], g["thetas"], g["betas"], nu=nu if nu > 0 else None)


def run(g, m, **kw):
    if isinstance(m, pdv.PDVModel):
        return m.gen(float(g["T"]), float(g["dt"]), float(g["S0"]), g["R10"], g["R20"])
    return m.gen(float(g["T"]), float(g["dt"]), float(g["S0"]), int(g["S"]), g["R10"], g["R20"], **kw)


@pytest.mark.parametrize("name", GEN_CASES)
def test_gen_matches_reference_under_the_global_seed(name):
    g = load(name)
    np.random.seed(int(g["seed"]))
    sigma, St = run(g, model_of(g))
    np.testing.assert_array_equal(sigma, g["sigma"])
    np.testing.assert_array_equal(St, g["St"])


@pytest.mark.parametrize("name", [c for c in GEN_CASES if c.startswith("disc")])
def test_gen_on_given_draws(name):
    g = load(name)
    sigma, St = run(g, model_of(g), draws=g["raw"])
    np.testing.assert_allclose(sigma, g["sigma"], rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(St, g["St"], rtol=1e-12, atol=0, equal_nan=True)


def test_goldens_exercise_the_edges():
    assert (load("disc_clip")["sigma"] == 1.5).any()
    St = load("disc_floor")["St"]
    assert np.isclose(St[:, 1:] / St[:, :-1], 1e-6, rtol=1e-6).any()           # rt floored at -0.999999
    g = load("disc_nan")
    assert np.isnan(g["sigma"]).all() and (g["St"][:, 0] == g["S0"]).all() and np.isnan(g["St"][:, 1:]).all()


def test_compute_factor_and_future_paths_match_reference():
    g = load("factor_b4")
    m = model_of(g, pdv.PDVModelDiscrete)
    R10, R20 = pdv.compute_factor(g["x_past"], m, int(g["w"]), DT)
    np.testing.assert_array_equal(R10, g["R10"])
    np.testing.assert_array_equal(R20, g["R20"])
    np.random.seed(int(g["seed"]))
    fut = pdv.future_pdv_model(g["x_past"], m, int(g["w"]), float(g["S0"]), int(g["S"]), float(g["T"]), DT)
    np.testing.assert_array_equal(fut, g["future"])
    # the batched entry point: each date its own factors; on the global stream it draws as gen does
    np.random.seed(int(g["seed"]))
    fut2 = pdv.pdv_future_paths(g["x_past"], m, int(g["w"]), float(g["S0"]), int(g["S"]), float(g["T"]), DT)
    np.testing.assert_array_equal(fut2[0], g["future"])


def test_compute_factor_accepts_three_betas():
    g = load("factor_b4")
    m4 = model_of(g, pdv.PDVModelDiscrete)
    m3 = pdv.PDVModelDiscrete(g["lams1"], g["lams2"], g["thetas"], g["betas"][:3])
    R10, R20 = pdv.compute_factor(g["x_past"], m3, int(g["w"]), DT)
    np.testing.assert_array_equal(R10, g["R10"])                 # the extra column never entered the factors
    np.testing.assert_array_equal(R20, g["R20"])


def test_pdv_future_paths_batches_dates():
    g = load("factor_b4")
    m = model_of(g, pdv.PDVModelDiscrete)
    x = np.concatenate([g["x_past"], g["x_past"][:, ::-1]], axis=0)
    out = pdv.pdv_future_paths(x, m, int(g["w"]), 100.0, 8, 20 / 252, DT, seed=5)
    assert out.shape == (2, 8, 20)
    for b in range(2):
        R10, R20 = pdv.compute_factor(x[b:b + 1], m, int(g["w"]), DT)
        raw = pdv.philox_draws(5, 8, 20, first_path=8 * b)
        _, St = m.gen(20 / 252, DT, 100.0, 8, R10, R20, draws=raw)
        np.testing.assert_array_equal(out[b], St)


@pytest.mark.parametrize("name", PRED_CASES)
def test_predictor_matches_reference(name):
    g = load(f"pred_{name}")
    p = pdv.AutoregressiveLinearPredictor(T=int(g["T"]), w=int(g["w"]), s=int(g["s"]), dt=float(g["dt"]),
                                          ktype=str(g["ktype"]), extra_term=bool(g["extra"]))
    np.testing.assert_array_equal(p.k1, g["k1"])
    np.testing.assert_array_equal(p.k2, g["k2"])
    idx_x, idx_y, x_train, y_train = p.separate(g["x"])
    for got, want in ((idx_x, "idx_x"), (idx_y, "idx_y"), (x_train, "x_train"), (y_train, "y_train")):
        np.testing.assert_array_equal(got, g[want])
    p.train(g["x"])
    np.testing.assert_allclose(p.linreg.coef_, g["coef"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(p.predict(g["x_test"]), g["y_pred"], rtol=1e-9, atol=1e-12)


def test_predictor_regression_is_least_squares():
    g = load("pred_exp_extra")
    p = pdv.AutoregressiveLinearPredictor(T=20, w=60, s=3, dt=DT, ktype="exp", extra_term=True)
    p.train(g["x"])
    _, _, dlnx, y = p.separate(g["x"])
    X = p.embedding(dlnx, p.k1, p.k2, True)
    try:
        from sklearn.linear_model import LinearRegression
        want = LinearRegression(fit_intercept=False).fit(X, y).coef_
    except ImportError:                                   # the normal equations, where sklearn is not installed
        want = np.linalg.solve(X.T @ X, X.T @ y)
    np.testing.assert_allclose(p.linreg.coef_, want, rtol=1e-9, atol=1e-12)


def test_windows():
    x = np.arange(10)
    np.testing.assert_array_equal(pdv.windows(x, 4, 3), [[0, 1, 2, 3], [3, 4, 5, 6], [6, 7, 8, 9]])
    np.testing.assert_array_equal(pdv.windows(x, 4, 3, offset=1), [[1, 2, 3, 4], [4, 5, 6, 7]])
    assert pdv.windows(x, 11, 1).shape == (0, 11)
    assert pdv.windows(np.zeros((2, 3, 10)), 5, 2).shape == (2, 3, 3, 5)


def test_errors():
    m = pdv.PDVModelDiscrete([60, 4], [40, 1.5], [0.6, 0.3], [0.04, -0.12, 0.6])
    with pytest.raises(ValueError):
        m.gen(1.0, 1 / 250, 100.0, 4, [0, 0], [0.04, 0.04])                 # dt must be one day
    with pytest.raises(ValueError):
        m.gen(1.0, DT, 100.0, 4, [0, 0], [0.04, 0.04], seed=-1)
    with pytest.raises(ValueError):
        m.gen(1.0, DT, 100.0, 4, [0, 0], [0.04, 0.04], draws=np.zeros((4, 3)))
    with pytest.raises(ValueError):
        m.gen(1.0, DT, 100.0, 4, [0, 0, 0], [0.04, 0.04])
    with pytest.raises(TypeError):
        pdv.pdv_future_paths(np.ones((1, 10)), pdv.PDVModel([60, 4], [40, 1.5], [0.6, 0.3], [0.04, -0.12, 0.6]), 10,
                             100.0, 4, 1.0, DT)


def test_drop_in_import_path():
    from shadowing.PDV.PDV import AutoregressiveLinearPredictor, PDVModelDiscrete, future_pdv_model
    import shadowing
    import shadowing_amd as sa
    assert PDVModelDiscrete is sa.PDVModelDiscrete is pdv.PDVModelDiscrete
    assert AutoregressiveLinearPredictor is sa.AutoregressiveLinearPredictor and future_pdv_model is pdv.future_pdv_model
    assert shadowing.PDVModel is pdv.PDVModel


def test_philox_known_answers():
    """Random123's Philox4x32-10 vectors (the first also what rocrand's philox4x32_10 engine gives for seed 0)."""
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        assert tuple(int(v) for v in pdv.philox4x32_10(ctr, key)) == want


def test_philox_draws_depend_only_on_seed_path_and_step():
    a = pdv.philox_draws(7, 40, 33)
    np.testing.assert_array_equal(pdv.philox_draws(7, 10, 33, first_path=30), a[30:])
    np.testing.assert_array_equal(pdv.philox_draws(7, 40, 20), a[:, :20])
    t = pdv.philox_draws(7, 40, 33, nu=3.0)
    np.testing.assert_array_equal(pdv.philox_draws(7, 5, 9, nu=3.0, first_path=35), t[35:, :9])
    assert not np.array_equal(a, pdv.philox_draws(8, 40, 33))
    big = pdv.philox_draws(1, 200, 1000)
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1) < 0.01


def test_seeded_host_twin_is_reproducible_and_normalised():
    m = pdv.PDVModelDiscrete([60, 4], [40, 1.5], [0.6, 0.3], [0.04, -0.12, 0.6, 0.5], nu=3.0)
    s1, S1 = m.gen(1.0, DT, 100.0, 16, [0, 0.01], [0.04, 0.03], seed=11)
    s2, S2 = m.gen(1.0, DT, 100.0, 16, [0, 0.01], [0.04, 0.03], seed=11)
    np.testing.assert_array_equal(S1, S2)
    np.testing.assert_array_equal(s1, s2)
    assert np.isfinite(S1).all() and (S1[:, 0] == 100.0).all()


def test_calibrate_needs_scipy_only_for_snp():
    class Prices:
        dlnx = np.random.default_rng(3).standard_t(4, size=(2, 500)) * 0.01
    try:
        import scipy  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="scipy"):
            pdv.PDVModelDiscrete([60, 4], [40, 1.5], [0.6, 0.3], [0.04, -0.12, 0.6], snp=Prices())
        return
    m = pdv.PDVModelDiscrete([60, 4], [40, 1.5], [0.6, 0.3], [0.04, -0.12, 0.6], snp=Prices())
    assert len(m.fit_params) == 3 and m._draw_nu() == m.fit_params[0]


@pytest.fixture(scope="module")
def lib():
    from shadowing_amd import _build, _native
    _build.build()
    return _native.load()


def test_capi_rejects_bad_arguments_before_the_device(lib):
    d2 = (C.c_double * 2)(1.0, 2.0)
    b3 = (C.c_double * 4)(0.04, -0.12, 0.6, 0.5)
    r = (C.c_double * 2)(0.0, 0.0)                         # (never read: every call below fails its argument checks)
    R = C.cast(r, C.c_void_p)

    def call(B=1, S=4, n=10, lams1=d2, betas=b3, nb=3, nu=0.0, R10=R):
        return lib.psh_pdv_generate(0, None, B, S, n, lams1, d2, d2, d2, d2, betas, nb, 100.0, 0.063, nu, R10, R, None, 0,
                                    None, None, None, None, None)
    assert call(n=0) == -1
    assert call(B=0) == -1
    assert call(S=0) == -1
    assert call(nu=-1.0) == -1
    assert call(nu=float("nan")) == -1
    assert call(nu=float("inf")) == -1
    assert call(nb=2) == -1 and call(nb=5) == -1
    assert call(lams1=None) == -1 and call(betas=None) == -1
    assert call(R10=None) == -1
    assert call(B=2, S=2 ** 62, n=4) == -1                 # B * S * n_steps past int64
    assert call(B=4, S=2 ** 40, n=1) == -2                 # a grid past what one launch takes
