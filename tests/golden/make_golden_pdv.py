#!/usr/bin/env python
"""Generate the pdv_*.npz golden vectors in this directory by running the READ-ONLY reference's PDV model
(shadowing/PDV/PDV.py of RudyMorel/shadowing) on CPU.

Run in the build container only (the reference does not travel):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pdv.py

`scatspectra` (un-vendored) is replaced by a names-only stub, as in make_golden.py, except that its `windows` is this
project's (shadowing_amd/pdv.py, loaded by path): the predictor's `separate` needs one.  Each generation case records the
raw draws too: seed numpy's global stream, draw with the reference's own call (randn, or its Student-t's rvs), seed
again and run gen.  Nothing but data is written: no reference source is copied.
"""
from __future__ import annotations

import importlib.util
import json
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.dont_write_bytecode = True
DT = 1 / 252


def load_ours():
    spec = importlib.util.spec_from_file_location("psh_pdv", REPO / "shadowing_amd" / "pdv.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(windows):
    stub = types.ModuleType("scatspectra")
    for name in ("TimeSeriesDataset", "Softmax", "Uniform", "DiscreteProba", "PriceData"):
        setattr(stub, name, type(name, (), {}))
    stub.windows = windows
    sys.modules["scatspectra"] = stub
    sys.path.insert(0, "/root/reference")
    import shadowing  # noqa: F401  (the reference)
    sys.path.pop(0)
    return sys.modules["shadowing.PDV.PDV"]


PARAMS = dict(lams1=[60.0, 4.0], lams2=[40.0, 1.5], thetas=[0.6, 0.3])
BETAS3, BETAS4 = [0.04, -0.12, 0.6], [0.04, -0.12, 0.6, 0.5]


def main():
    ours = load_ours()
    ref = load_reference(ours.windows)
    import scipy
    import sklearn
    versions = dict(numpy=np.__version__, scipy=scipy.__version__, sklearn=sklearn.__version__)

    def save(name, **arrays):
        np.savez_compressed(HERE / f"pdv_{name}.npz", meta=json.dumps(versions), **arrays)
        size = (HERE / f"pdv_{name}.npz").stat().st_size
        assert size < 1 << 20, (name, size)
        print(f"pdv_{name}: {size} bytes")

    def gen_case(name, betas, nu, T, S, R10, R20, seed, thetas=None, continuous=False, S0=100.0):
        params = dict(PARAMS, betas=betas)
        if thetas is not None:
            params["thetas"] = thetas
        cls = ref.PDVModel if continuous else ref.PDVModelDiscrete
        m = cls(**params, nu=nu)
        n = int(T / DT)
        size = (n - 1,) if continuous else (S, n)
        np.random.seed(seed)
        raw = m.dlnx_dist.rvs(size=size) if nu is not None else np.random.randn(*size)
        np.random.seed(seed)
        if continuous:
            sigma, St = m.gen(T=T, dt=DT, S0=S0, R10=np.array(R10), R20=np.array(R20))
        else:
            sigma, St = m.gen(T=T, dt=DT, S0=S0, S=S, R10=np.array(R10), R20=np.array(R20))
        save(name, lams1=params["lams1"], lams2=params["lams2"], thetas=params["thetas"], betas=betas,
             nu=0.0 if nu is None else nu, T=T, dt=DT, S0=S0, S=S, R10=R10, R20=R20, seed=seed, continuous=continuous,
             raw=raw, sigma=sigma, St=St)
        return sigma, St

    R10, R20 = [0.0, 0.01], [0.04, 0.03]
    gen_case("disc_b3_gauss_T75", BETAS3, None, 75 / 252, 32, R10, R20, 1)
    gen_case("disc_b4_gauss_T1", BETAS4, None, 1.0, 32, R10, R20, 2)
    gen_case("disc_b3_t3_T1", BETAS3, 3.0, 1.0, 32, R10, R20, 3)
    gen_case("disc_b4_t3_T75", BETAS4, 3.0, 75 / 252, 32, [0.05, -0.02], R20, 4)
    sig, _ = gen_case("disc_clip", [2.0, -0.12, 0.6], None, 75 / 252, 32, R10, R20, 5)
    assert (sig == 1.5).any()
    # a Student-t with nu = 0.5: one draw dominates a path, its normalised value nears -sqrt(n - 1), and 1.5 x that floors
    _, St = gen_case("disc_floor", [2.0, -0.12, 0.6], 0.5, 1.0, 32, R10, R20, 6)
    assert np.isclose(St[:, 1:] / St[:, :-1], 1e-6, rtol=1e-6).any()
    sig, _ = gen_case("disc_nan", BETAS3, None, 75 / 252, 32, R10, [0.04, 0.0], 7, thetas=[0.6, 2.0])
    assert np.isnan(sig).all()
    gen_case("cont_gauss", BETAS3, None, 75 / 252, 1, R10, R20, 8, continuous=True)

    # compute_factor and future_pdv_model (4 betas: the reference's only working case)
    g = np.random.default_rng(9)
    w = 100
    x_past = 100.0 * np.exp(np.cumsum(np.concatenate([[0.0], 0.012 * g.standard_normal(w - 1)])))[None, :]
    m = ref.PDVModelDiscrete(**PARAMS, betas=BETAS4)
    R10f, R20f = ref.compute_factor(x_past, m, w, DT)
    np.random.seed(10)
    raw = np.random.randn(16, 75)
    np.random.seed(10)
    future = ref.future_pdv_model(x_past, m, w, 100.0, 16, 75 / 252, DT)
    save("factor_b4", lams1=PARAMS["lams1"], lams2=PARAMS["lams2"], thetas=PARAMS["thetas"], betas=BETAS4, x_past=x_past,
         w=w, dt=DT, R10=R10f, R20=R20f, S0=100.0, S=16, T=75 / 252, seed=10, raw=raw, future=future)

    # the predictor: both kernel types, with and without the extra term
    x = 100.0 * np.exp(np.cumsum(0.01 * np.random.default_rng(11).standard_normal(1500)))
    x_test = 0.01 * np.random.default_rng(12).standard_normal((5, 60))
    for ktype in ("exp", "power-law"):
        for extra in (False, True):
            p = ref.AutoregressiveLinearPredictor(T=20, w=60, s=3, dt=DT, ktype=ktype, extra_term=extra)
            idx_x, idx_y, x_train, y_train = p.separate(x)
            p.train(x)
            save(f"pred_{ktype.replace('-', '')}_{'extra' if extra else 'plain'}", x=x, T=20, w=60, s=3, dt=DT,
                 ktype=ktype, extra=extra, k1=p.k1, k2=p.k2, idx_x=idx_x, idx_y=idx_y, x_train=x_train, y_train=y_train,
                 coef=p.linreg.coef_, x_test=x_test, y_pred=p.predict(x_test))


if __name__ == "__main__":
    main()
