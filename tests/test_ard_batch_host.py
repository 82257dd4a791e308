"""CPU tier of the per-feature (ARD) length scales in lockstep batches (include/sigp.h: sigp_batch_run_ard, sigp_nlml_grad_ard_batch): the ABI
is declared, exported and bound, the Python surface exists, and the lockstep BFGS of ``optim.py`` -- which the batch optimiser runs on
``GPR.nlml_ard_batch`` -- minimises d + 1 parameters per data set, pinned on the NumPy closed form of tests/test_ard_host.py against SciPy's
L-BFGS-B on the same function."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
from scipy.optimize import minimize

from test_ard_host import ard_closed_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARD_BATCH_SYMBOLS = {"sigp_batch_run_ard": 10, "sigp_nlml_grad_ard_batch": 11}
SEEDS = (20260100, 20260101, 20260102, 20260103)


def relevance_problem(seed, n=96, d=3):
    """y bends along x_1, leans on x_2 and ignores x_3 (the GPU tier optimises the same data sets)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    y = np.sin(1.5 * X[:, 0]) + 0.5 * X[:, 1] + 0.1 * rng.standard_normal(n)
    return X, y


def closed_form_objective(kind, X, y):
    d = X.shape[1]

    def f(th):
        try:
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                g, _, v = ard_closed_form(kind, X, y, np.exp(th[:d]), np.exp(th[d]))
        except np.linalg.LinAlgError:
            return np.inf, np.full(d + 1, np.inf)
        if not (np.isfinite(v) and np.all(np.isfinite(g))):
            return np.inf, np.full(d + 1, np.inf)
        return float(v), g
    return f


def bounded_reference(kind, X, y, th0):
    """SciPy's L-BFGS-B on the closed form with the bounds of test_hip_ard.test_optimize_ard_finds_the_irrelevant_feature"""
    d = X.shape[1]
    return minimize(closed_form_objective(kind, X, y), th0, jac=True, method="L-BFGS-B", bounds=[(-3.0, 5.0)] * d + [(-12.0, 3.0)])


def test_ard_batch_entry_points_declared_exported_and_bound():
    from seaiceextentforecasting_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "sigp.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name, nargs in ARD_BATCH_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, "%s is not declared in include/sigp.h" % name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(lib, name), "%s is not exported by libsigp.so" % name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
    assert L.load().sigp_version() >= 580


def test_ard_batch_null_handle_is_rejected_and_the_python_surface_exists():
    import seaiceextentforecasting_amd as S
    from seaiceextentforecasting_amd import _lib as L
    lib = L.load()
    a = np.ones(8)
    assert lib.sigp_batch_run_ard(None, 0, 1, 1, L.ptr(a), 3, L.ptr(a), L.ptr(a), None, None) == L.BAD_ARG
    assert lib.sigp_nlml_grad_ard_batch(None, 0, 1, 1, L.ptr(a), 4, 4, 2, L.ptr(a), L.ptr(a), 4) == L.BAD_ARG
    sig = inspect.signature(S.GPR.nlml_ard_batch).parameters
    assert list(sig)[1:] == ["theta", "first", "grad", "group"]
    assert sig["first"].default == 0 and sig["grad"].default == "exact" and sig["group"].default == 8
    assert inspect.signature(S.GPR.optimize_batch).parameters["ard"].default is False


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
def test_bfgs_lockstep_minimises_four_parameters_per_data_set(kind):
    """``bfgs_lockstep`` at p = d + 1 = 4 on the closed form: for every data set the value at the returned x is <= the bounded reference's
    + 1e-6 |reference| (the bound of test_optimize_ard_finds_the_irrelevant_feature).  The lockstep driver has no box: where l_3 runs past
    e^5 it ends below the reference."""
    from seaiceextentforecasting_amd.optim import bfgs_lockstep
    d = 3
    data = [relevance_problem(s) for s in SEEDS]
    fs = [closed_form_objective(kind, X, y) for X, y in data]
    th0 = np.log([np.sqrt(3.0)] * d + [1e-2])

    def evaluate(theta):
        assert theta.shape == (len(data), d + 1)
        out = [f(t) for f, t in zip(fs, theta)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])

    res = bfgs_lockstep(evaluate, np.tile(th0, (len(data), 1)), maxiter=50)
    assert res["x"].shape == (len(data), d + 1) and res["jac"].shape == (len(data), d + 1)
    for b, (X, y) in enumerate(data):
        ref = bounded_reference(kind, X, y, th0)
        at = fs[b](res["x"][b])[0]
        print("%s seed %d: reference %.12g, lockstep %.12g (reported %.12g) in %d steps, x = %s" % (kind, SEEDS[b], ref.fun, at, res["fun"][b], res["nit"][b], res["x"][b]))
        assert at == res["fun"][b]
        assert at <= ref.fun + 1e-6 * abs(ref.fun), (kind, SEEDS[b], at, ref.fun)
    assert np.all(res["converged"])


def test_bfgs_lockstep_with_two_parameters_is_what_it_was():
    """p = 2 on a quadratic whose BFGS iterates are easy to follow: the driver still returns [B, 2] arrays and finds both minima"""
    from seaiceextentforecasting_amd.optim import bfgs_lockstep
    A = np.array([[[3.0, 1.0], [1.0, 2.0]], [[1.0, 0.0], [0.0, 5.0]]])
    c = np.array([[1.0, -2.0], [0.5, 0.25]])

    def evaluate(theta):
        r = theta - c
        return 0.5 * np.einsum("bi,bij,bj->b", r, A, r), np.einsum("bij,bj->bi", A, r)

    res = bfgs_lockstep(evaluate, np.zeros((2, 2)), gtol=1e-9)
    assert res["x"].shape == (2, 2) and np.allclose(res["x"], c, atol=1e-7)
